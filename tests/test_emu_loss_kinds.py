"""CPU emulator: the loss kinds (MAE = nn.L1Loss, Huber = nn.HuberLoss) through the stand-alone launch (stgcn_loss_grad), the fused head
backward (stgcn_outblock_backward_loss, every fc_bwd_kernel instance) and the trainers.  The cases, inputs and bars: tests/loss_kinds_util.py."""
import pytest
import torch

from tests import loss_kinds_util as U
from tests.loss_kinds_util import KINDS, SHAPES

DEV = "cpu"


@pytest.mark.parametrize("kind", KINDS)
def test_standalone_loss_matches_torch(kind):
    for shape in SHAPES:
        U.check_standalone_matches_torch(DEV, kind, shape)


def test_standalone_mse_kind_is_bitwise_the_mse_entry():
    for shape in SHAPES:
        U.check_standalone_mse_is_bitwise_the_mse_entry(DEV, shape)


@pytest.mark.parametrize("kind", KINDS)
def test_standalone_nan_prediction_stays_visible(kind):
    U.check_standalone_nan(DEV, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_standalone_loss_reads_labels_through_index_and_table(kind):
    U.check_standalone_label_modes(DEV, kind)


def test_unknown_kind_and_bad_delta_are_refused():
    U.check_standalone_refusals(DEV)


def test_trainers_refuse_an_unknown_loss_up_front():
    from stgcn_amd import train
    for fn, nargs in ((train.fwd_loss_bwd, 3), (train.train_step, 4), (train.fused_train_step, 5), (train.tail_step, 4),
                      (train.chained_fwd_bwd, 4)):
        with pytest.raises(ValueError, match="unknown loss"):
            fn(*([None] * nargs), loss="l1")
    with pytest.raises(ValueError, match="unknown loss"):      # at construction: before anything touches the device
        train.GraphedTrainStep(None, None, torch.zeros(2, 1), torch.zeros(2, 1), loss="smooth_l1")
    with pytest.raises(ValueError, match="huber_delta"):
        train.GraphedTrainStep(None, None, torch.zeros(2, 1), torch.zeros(2, 1), loss="huber", huber_delta=0.0)


# fc_bwd_kernel<1,1> (h), <1,2> (a), T1 = 3 (b) -- and with 32-row tiles <2,1> (h), <2,2> (a): tests/test_gpu_head.py::CASES
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["h", "a", "b"])
def test_head_fused_loss_stages(name, kind):
    U.assert_head_loss_errors(U.run_head_loss_case(DEV, name, kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["h", "a"])
def test_head_fused_loss_stages_fc_tile_32(name, kind, monkeypatch):
    monkeypatch.setenv("STGCN_HEAD_FC_TILE", "32")
    U.assert_head_loss_errors(U.run_head_loss_case(DEV, name, kind))


@pytest.mark.parametrize("kind", KINDS)
def test_fused_loss_equals_the_two_call_path(kind):
    U.check_fused_equals_two_call(DEV, kind)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_training_trajectory_matches_oracle(kind, fused):
    U.check_model_trajectory(DEV, kind, fused)


@pytest.mark.parametrize("kind", KINDS)
def test_tail_step_shares_add_up_to_the_mean_gradient(kind, monkeypatch):
    U.check_tail_step_shares(DEV, kind, monkeypatch)


def test_chained_fwd_bwd_uses_the_loss_kind():
    """chained_fwd_bwd (torch.nn.functional.l1_loss / huber_loss in place of mse_loss): two chains give the gradient of the whole batch."""
    from stgcn_amd.train import chained_fwd_bwd, fwd_loss_bwd
    for kind in KINDS:
        m, x, y = U.fresh_tiny(DEV)
        if len(x) % 2:
            x, y = x[:len(x) - 1].contiguous(), y[:len(x) - 1].contiguous()
        l1 = float(fwd_loss_bwd(m, x, y, kind, U.DELTA))
        g1 = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
        m.zero_grad(set_to_none=True)
        l2 = float(chained_fwd_bwd(m, x, y, 2, loss=kind, huber_delta=U.DELTA))
        assert abs(l1 - l2) <= 1e-6 * abs(l1)
        for k, p in m.named_parameters():
            if p.grad is not None:
                assert float((p.grad - g1[k]).abs().max()) <= 1e-5 * float(g1[k].abs().max()) + 1e-12, k
