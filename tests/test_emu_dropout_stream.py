"""The dropout stream on the CPU emulator against an independent Philox4x32-10 (tests/philox_ref.py; the cases and runners are in
tests/dropout_stream_util.py, shared with tests/test_gpu_dropout_stream.py):

  * the generator (``ops.dropout_mask`` = dropout_mask_kernel, the mask every stage test feeds its oracle) bit for bit over sizes, rates,
    seeds and positions with high words set, and in the device-counter form;
  * droprate outside [0, 1) refused by the mask entry point, the block descriptor and the head descriptor, NaN included;
  * WHERE each site of a model draws: eager, device counter, micro-batch chains, bf16, the counter on the weight-pack launch (the fold
    form of a captured step) and a tail batch in between -- the block patterns exactly;
  * the training step with dropout on against the float64 oracle fed with the reference's masks at those positions (which is what covers
    the head's mask and every backward consumer of a mask), at the bars of the droprate-0 trajectory.

Not covered: element indices above 2^34 (the counter's second word nonzero): a mask that large does not fit in a test.  Data-parallel
ranks: tests/test_dp_gloo.py builds its model with droprate 0.0 fixed inside ``_make`` and compares against a single process at the global
batch, which no longer holds once the ranks draw different masks; a rank case would need that harness restructured, so it is left out
(``init_distributed`` gives rank r the seed base + r, and ``test_rank_offset_survives_reseeding`` pins that part on the host).
"""
import pytest
import torch

from tests import dropout_stream_util as U
from tests.launch_log_util import run_child

DEV = "cpu"
THIS = "tests/test_emu_dropout_stream.py"


@pytest.mark.parametrize("n", U.GRID_N)
def test_generator_equals_reference(n):
    U.bind(DEV)
    U.check_generator_grid(DEV, n)


def test_device_counter_form_equals_host_offset_sum():
    U.bind(DEV)
    U.check_device_counter(DEV)


def test_droprate_outside_unit_interval_is_refused():
    U.bind(DEV)
    U.check_refusals(DEV)


def test_site_and_chain_limits_raise_on_the_host():
    from stgcn_amd import DropoutStream
    saved = DropoutStream._sites
    try:
        DropoutStream._sites = DropoutStream.CHAIN_STRIDE - 2
        assert DropoutStream.new_site() == DropoutStream.CHAIN_STRIDE - 1            # the last site that is chain 0's alone
        with pytest.raises(RuntimeError, match=str(DropoutStream.CHAIN_STRIDE - 1)):
            DropoutStream.new_site()
        assert DropoutStream._sites == DropoutStream.CHAIN_STRIDE - 1
    finally:
        DropoutStream._sites = saved
    top = DropoutStream.SITE_STRIDE // DropoutStream.CHAIN_STRIDE - 1
    assert DropoutStream.site_offset(3, 0) == 3 and DropoutStream.site_offset(3, top) == 3 + DropoutStream.CHAIN_STRIDE * top
    assert DropoutStream.site_offset(DropoutStream.CHAIN_STRIDE - 1, top) < DropoutStream.SITE_STRIDE
    for chain in (top + 1, -1):
        with pytest.raises(RuntimeError, match=str(top)):
            DropoutStream.site_offset(3, chain)


def test_rank_offset_survives_reseeding():
    from stgcn_amd import DropoutStream
    saved = (DropoutStream.seed, DropoutStream.rank_offset, DropoutStream._offset)
    try:
        DropoutStream.rank_offset = 1
        DropoutStream.manual_seed(41)
        assert DropoutStream.seed == 42 and DropoutStream._offset == 0
    finally:
        DropoutStream.seed, DropoutStream.rank_offset, DropoutStream._offset = saved


@pytest.mark.parametrize("p", [0.5, 0.3])
def test_eager_steps_draw_at_host_offsets_and_match_oracle(p):
    U.run_eager_trajectory(DEV, p)


@pytest.mark.parametrize("p", [0.5, 0.3])
@pytest.mark.parametrize("chains", [1, 2])
def test_counter_steps_draw_at_site_plus_counter_and_match_oracle(p, chains):
    U.run_counter_trajectory(DEV, p, chains)


@pytest.mark.parametrize("p", [0.5, 0.3])
def test_folded_counter_and_tail_batch_draw_at_distinct_positions_and_match_oracle(p):
    U.run_folded_trajectory(DEV, p)


def test_tail_batch_between_unfolded_steps():
    U.run_tail_unfolded(DEV, 0.5)


def test_chains_without_counter_take_consecutive_host_offsets():
    U.run_chains_without_counter(DEV, 0.5)


def test_bf16_patterns_sit_at_the_same_positions():
    U.run_positions_only(DEV, 0.5, torch.bfloat16)


def test_one_step_matches_oracle():
    """(also the body of the STGCN_HOOK_MASK=philox run below: the backward regenerating the LayerNorm hook's mask instead of reading it
    off the block output)"""
    U.run_eager_trajectory(DEV, 0.5, n_steps=1, name="eager, one step")


def test_one_step_matches_oracle_with_regenerated_hook_masks():
    out = run_child({"STGCN_HOOK_MASK": "philox"}, [THIS], "test_one_step_matches_oracle and not regenerated", marker="not gpu")
    assert "1 passed" in out
