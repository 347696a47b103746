"""-m gpu: the loss kinds (MAE = nn.L1Loss, Huber = nn.HuberLoss) on the MI355X: the stand-alone launch (stgcn_loss_grad), the fused head
backward through every fc_bwd_kernel instance, the trainers, and the captured step on the resident series.  The cases, inputs and bars:
tests/loss_kinds_util.py."""
import numpy as np
import pytest
import torch

from tests import loss_kinds_util as U
from tests.loss_kinds_util import DELTA, KINDS, SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


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


@pytest.mark.parametrize("kind", KINDS)
def test_bf16_model_fused_loss_equals_the_two_call_path(kind):
    """One step of a bf16 model (the C2-shaped head of tests/test_gpu_graph.py: its bf16 backward is dense, not refused)."""
    from tests.test_gpu_graph import _make
    m = _make(0.0).set_compute_dtype(torch.bfloat16)
    m.train()
    x = torch.randn(4, 1, 12, 207, generator=torch.Generator().manual_seed(8)).to(DEV)
    U.check_fused_equals_two_call(DEV, kind, (m, x, U.target_from_own_prediction(m, x)))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_training_trajectory_matches_oracle(kind, fused):
    U.check_model_trajectory(DEV, kind, fused)


@pytest.mark.parametrize("kind", KINDS)
def test_tail_step_shares_add_up_to_the_mean_gradient(kind, monkeypatch):
    U.check_tail_step_shares(DEV, kind, monkeypatch)


# ---- the captured step on the resident series: a batch of 4 windows on the tiny fixture graph --------------------------------------
B, N_PRED, BATCHES, REPLAYS, WARMUP = 4, 3, 5, 4, 2
_counters = {}


def _captured(kind, shuffle):
    """(replay losses, state_dict, window tables of the steps, dropout counter, optimizer step count) of GraphedTrainStep(loss=kind)."""
    from stgcn_amd import DropoutStream
    from stgcn_amd.train import GraphedTrainStep, make_optimizer
    m, x = U.tiny_model(DEV)
    n_his, N = x.shape[2], x.shape[3]
    series = torch.randn(BATCHES * B + n_his + N_PRED, N, generator=torch.Generator().manual_seed(6)).to(DEV)
    DropoutStream.use_device_counter(torch.device(DEV))
    DropoutStream.manual_seed(3)
    try:
        o = make_optimizer(m, capturable=True)
        x0 = torch.stack([series[s:s + n_his] for s in range(B)]).unsqueeze(1).contiguous()
        y0 = series[n_his + N_PRED - 1:n_his + N_PRED - 1 + B].contiguous()
        gs = GraphedTrainStep(m, o, x0, y0, warmup=WARMUP, series=series, n_his=n_his, n_pred=N_PRED, shuffle=shuffle, shuffle_seed=5,
                              loss=kind, huber_delta=DELTA)
        assert gs.fused and gs.fold
        order = gs.order.cpu().tolist() if shuffle else list(range(BATCHES * B))
        losses = [float(gs().item()) for _ in range(REPLAYS)]
        torch.cuda.synchronize()
        counters = (int(DropoutStream.counter.item()), int(o.device_step_counter(torch.device(DEV)).item()))
        gs.close()
        return (losses, {k: v.clone() for k, v in m.state_dict().items()}, (series, order, n_his)) + counters
    finally:
        DropoutStream.disable_device_counter()


@pytest.mark.parametrize("shuffle", [False, True], ids=["in_order", "shuffled"])
@pytest.mark.parametrize("kind", KINDS)
def test_captured_step_equals_eager_fused_steps(kind, shuffle):
    """Four replays equal four eager fused_train_step calls on the same windows (the bars of tests/test_gpu_optim_kinds.py's replay
    against eager: losses rtol 1e-5, every state_dict entry within 2e-5); the dropout counter and the optimizer step count end where
    the MSE step's do."""
    from stgcn_amd.train import GradArena, fused_train_step, make_optimizer, train_step
    losses, sd, (series, order, n_his), drop, steps = _captured(kind, shuffle)
    if shuffle not in _counters:
        _counters[shuffle] = _captured("mse", shuffle)[3:]
    assert (drop, steps) == _counters[shuffle] and steps == WARMUP + 1 + REPLAYS

    def windows(k):
        starts = order[(k * B) % (BATCHES * B):(k * B) % (BATCHES * B) + B]
        x = torch.stack([series[s:s + n_his] for s in starts]).unsqueeze(1).contiguous()
        return x, torch.stack([series[s + n_his + N_PRED - 1] for s in starts]).contiguous()

    m2, _ = U.tiny_model(DEV)
    o2 = make_optimizer(m2)
    train_step(m2, o2, *windows(0), loss=kind, huber_delta=DELTA)
    arena = GradArena([p for p in m2.parameters() if p.grad is not None])
    ref = [float(fused_train_step(m2, o2, *windows(k), arena, loss=kind, huber_delta=DELTA)) for k in range(1, WARMUP + 1 + REPLAYS)]
    torch.cuda.synchronize()
    print(kind, shuffle, losses, ref[-REPLAYS:])
    assert np.allclose(losses, ref[-REPLAYS:], rtol=1e-5, atol=0), (losses, ref)
    for k, v in m2.state_dict().items():
        assert float((v - sd[k]).abs().max()) <= 2e-5, k
