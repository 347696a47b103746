"""-m gpu: the dropout stream on the MI355X against an independent Philox4x32-10 (tests/philox_ref.py).  The cases and runners are those
of tests/test_emu_dropout_stream.py (tests/dropout_stream_util.py; see there for what is and is not covered), plus what only the GPU has:
the hipGraph-captured step (``GraphedTrainStep``) -- fed batch by batch and in the shuffled resident-series form; the counter of both rides
on the weight-pack launch -- with a tail batch between its replays."""
import pytest
import torch

from tests import dropout_stream_util as U
from tests.launch_log_util import run_child

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THIS = "tests/test_gpu_dropout_stream.py"


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
    """(also the body of the STGCN_HOOK_MASK=philox run below)"""
    U.run_eager_trajectory(DEV, 0.5, n_steps=1, name="eager, one step")


def test_one_step_matches_oracle_with_regenerated_hook_masks():
    out = run_child({"STGCN_HOOK_MASK": "philox"}, [THIS], "test_one_step_matches_oracle and not regenerated")
    assert "1 passed" in out


@pytest.mark.parametrize("shuffle", [False, True], ids=["batches", "shuffled-series"])
def test_captured_step_draws_at_site_plus_counter_and_matches_oracle(shuffle):
    U.run_captured(DEV, shuffle=shuffle)
