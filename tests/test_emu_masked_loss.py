"""CPU emulator: the masked loss and metrics (train and score on observed readings only) through the stand-alone launch
(stgcn_loss_grad_masked), the fused head backward (stgcn_outblock_backward_loss_masked), the trainers, the evaluation launch
(stgcn_eval_accumulate_masked) and GraphedEvalPass(valid=, capture=False).  The cases, inputs and bars: tests/masked_loss_util.py."""
import pytest

from tests import masked_loss_util as U
from tests.masked_loss_util import BIG, KINDS, SINGLE

DEV = "cpu"


@pytest.mark.parametrize("kind", KINDS)
def test_standalone_masked_loss_matches_torch_float64(kind):
    U.check_standalone_matches_torch(DEV, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_all_ones_mask_is_bitwise_the_unmasked_entry_and_all_zero_gives_zero(kind):
    U.check_all_ones_is_the_unmasked_entry(DEV, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_labels_and_mask_from_a_resident_series_equal_the_gather(kind):
    U.check_resident_series_equals_gather(DEV, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_fused_masked_loss_equals_the_two_call_path(kind):
    U.check_fused_equals_two_call(DEV, kind)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("kind", ["mae", "huber"])
def test_masked_training_trajectory_matches_oracle(kind, fused):
    U.check_model_trajectory(DEV, kind, fused)


def test_tail_step_takes_the_mask_for_one_rank_only():
    U.check_tail_step(DEV, "mae")


@pytest.mark.parametrize("knob", [SINGLE, BIG], ids=["single_workgroup", "partial_slabs"])
def test_masked_evaluation_matches_the_float64_host_loop(knob, monkeypatch):
    U.check_eval_against_float64(DEV, knob, monkeypatch)
    U.check_eval_pos_walk(DEV, knob, monkeypatch)


@pytest.mark.parametrize("knob", [SINGLE, BIG], ids=["single_workgroup", "partial_slabs"])
def test_all_ones_mask_leaves_the_unmasked_kernels_words(knob, monkeypatch):
    U.check_eval_all_ones_is_the_unmasked_kernel(DEV, knob, monkeypatch)


def test_masked_eval_pass_matches_the_host_loop():
    from tests.optim_kinds_util import tiny_model
    U.bind(DEV)
    U.check_eval_pass(DEV, tiny_model(DEV, droprate=0.5)[0], 20, capture=False)


def test_refusals_and_the_abi():
    U.check_refusals(DEV)


def test_observed_mask_and_masked_host_metrics():
    U.check_data_helpers()
