"""-m gpu: gradient clipping by global norm inside the optimizer step (max_grad_norm) on the MI355X: the cases of
tests/test_emu_grad_clip.py (tests/grad_clip_util.py) on the HIP library, and the captured step -- the flush with the norm epilogue and the
clipping update inside the hipGraph -- against eager fused steps."""
import numpy as np
import pytest
import torch

from tests import grad_clip_util as U
from tests.launch_log_util import run_child

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bind():
    from tests.gpu_util import bind_hip
    return bind_hip()


@pytest.mark.parametrize("case", sorted(U.norm_tables()))
def test_norm_kernel(case):
    """|total - float64 norm| <= 2^-23 norm, coef is the fp32 expression on the returned total exactly, a second pass leaves bit-identical
    words, one NaN element gives a NaN total."""
    from stgcn_amd import _lib
    _bind()
    U.check_norm_case(_lib.lib(), DEV, case)


def test_c_abi_refuses_small_state_and_bad_max_norm():
    from stgcn_amd import _lib
    _bind()
    U.check_refusals(_lib.lib(), DEV)


@pytest.mark.parametrize("name", U.ALL_KINDS)
def test_optimizer_trajectory_matches_clip_grad_norm_and_reference(name):
    _bind()
    U.check_optimizer_trajectory(name, DEV)


def test_two_groups_share_one_norm():
    _bind()
    U.check_two_groups_share_one_norm(DEV)


@pytest.mark.parametrize("name", U.ALL_KINDS)
def test_infinite_max_norm_is_bitwise_the_unclipped_path(name):
    _bind()
    U.check_inf_is_bitwise_unclipped(name, DEV)


def test_two_producers_agree():
    _bind()
    U.check_two_producers_agree(DEV)


def test_two_producers_agree_big_table_forms():
    """the same in a fresh process with reduce_kernel's dvec and 4-slice job forms forced on the small model (STGCN_REDUCE_BIG)"""
    out = run_child({"STGCN_REDUCE_BIG": "1"}, ["tests/test_gpu_grad_clip.py"], "test_two_producers_agree and not big_table")
    assert "1 passed" in out, out[-2000:]


# ---- the captured step -------------------------------------------------------------------------------------------------------------------
REPLAYS, WARMUP = 8, 2


def _compare(m1, o1, norms1, losses1, m2, o2, norms2, losses2):
    """the bars of tests/test_gpu_optim_kinds.py's replay against eager: losses (and the norms) rtol 1e-5, every tensor within 2e-5"""
    print("replay norms", norms1, "eager norms", norms2)
    assert np.allclose(losses1, losses2, rtol=1e-5, atol=0), (losses1, losses2)
    assert np.allclose(norms1, norms2, rtol=1e-5, atol=0), (norms1, norms2)
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    for k in sd1:
        assert float((sd1[k] - sd2[k]).abs().max()) <= 2e-5, k
    live = 0
    for p1, p2 in zip(m1.parameters(), m2.parameters()):
        assert (p1 in o1.state and len(o1.state[p1]) > 0) == (p2 in o2.state and len(o2.state[p2]) > 0)
        if p2 in o2.state and o2.state[p2]:
            live += 1
            for key, v in o2.state[p2].items():
                assert float((o1.state[p1][key] - v).abs().max()) <= 2e-5, key
    assert live >= 20


@pytest.mark.parametrize("name", U.ALL_KINDS)
def test_graphed_clipping_step_equals_eager_fused_steps(name):
    """GraphedTrainStep with a capturable clipping optimizer: flush with the norm epilogue + the clipping update inside the graph.  8 replays
    (StepLR + sync_lr halving lr after 4) equal 8 eager fused steps in parameters, optimizer state and per-step last_grad_norm."""
    from stgcn_amd import DropoutStream
    from stgcn_amd.train import GradArena, GraphedTrainStep, check_in_launch_waits, fused_train_step, fwd_loss_bwd, make_optimizer, train_step
    from tests.test_gpu_optim_kinds import _make
    g = torch.Generator().manual_seed(4)
    xs = torch.randn(9, 8, 1, 12, 207, generator=g).to(DEV)
    ys = torch.randn(9, 8, 207, generator=g).to(DEV)
    m0 = _make()
    fwd_loss_bwd(m0, xs[0], ys[0])
    max_norm = 0.5 * U._grad_norm64([p.grad for p in m0.parameters() if p.grad is not None])
    DropoutStream.use_device_counter(torch.device(DEV))
    DropoutStream.manual_seed(3)
    try:
        m1 = _make()
        o1 = make_optimizer(m1, capturable=True, name=name, max_grad_norm=max_norm)
        s1 = torch.optim.lr_scheduler.StepLR(o1, step_size=4, gamma=0.5)
        gs = GraphedTrainStep(m1, o1, xs[0], ys[0], warmup=WARMUP)
        assert gs.fused
        l1, n1 = [], []
        for i in range(1, REPLAYS + 1):
            l1.append(float(gs(xs[i], ys[i]).item()))
            n1.append(float(o1.last_grad_norm.item()))
            s1.step()
            o1.sync_lr()
        torch.cuda.synchronize()
        check_in_launch_waits(m1)
        gs.close()
    finally:
        DropoutStream.disable_device_counter()
    # the twin: the constructor's 2 warm-up steps (plain, then fused) + its verification replay, all on batch 0, then the 8 batches
    m2 = _make()
    o2 = make_optimizer(m2, name=name, max_grad_norm=max_norm)
    s2 = torch.optim.lr_scheduler.StepLR(o2, step_size=4, gamma=0.5)
    train_step(m2, o2, xs[0], ys[0])
    assert abs(float(o2.last_clip_coef.item()) - 0.5) < 1e-3
    arena = GradArena([p for p in m2.parameters() if p.grad is not None])
    for _ in range(WARMUP):
        fused_train_step(m2, o2, xs[0], ys[0], arena)
    l2, n2 = [], []
    for i in range(1, REPLAYS + 1):
        l2.append(float(fused_train_step(m2, o2, xs[i], ys[i], arena).item()))
        n2.append(float(o2.last_grad_norm.item()))
        s2.step()
    assert o1.param_groups[0]["lr"] == o2.param_groups[0]["lr"]
    assert int(o1.device_step_counter(torch.device(DEV)).item()) == o2.param_groups[0]["_step"] == WARMUP + 1 + REPLAYS
    _compare(m1, o1, n1, l1, m2, o2, n2, l2)


def test_graphed_clipping_step_on_resident_series_with_dropout():
    """the same with the windows read from a resident series and dropout on: the twin runs eager fused steps in device-counter mode at the
    positions the captured step draws at (the constructor's plain step at 0, then one SITE_STRIDE per step from 2 on)."""
    from stgcn_amd import DropoutStream
    from stgcn_amd.train import GradArena, GraphedTrainStep, check_in_launch_waits, fused_train_step, fwd_loss_bwd, make_optimizer, train_step
    _bind()
    B, N_PRED, BATCHES, P = 4, 3, 5, 0.3

    def build():
        DropoutStream._sites = 0          # both runs build "the same" model: its blocks draw the same dropout sites
        return U.tiny_model(DEV, droprate=P)

    m0, x, _ = build()
    n_his, N = x.shape[2], x.shape[3]
    series = torch.randn(BATCHES * B + n_his + N_PRED, N, generator=torch.Generator().manual_seed(6)).to(DEV)

    def windows(k):
        starts = [(k * B) % (BATCHES * B) + b for b in range(B)]
        xw = torch.stack([series[s:s + n_his] for s in starts]).unsqueeze(1).contiguous()
        return xw, torch.stack([series[s + n_his + N_PRED - 1] for s in starts]).contiguous()

    fwd_loss_bwd(m0, *windows(0))
    max_norm = 0.5 * U._grad_norm64([p.grad for p in m0.parameters() if p.grad is not None])
    dev = torch.device(DEV)
    DropoutStream.use_device_counter(dev)
    DropoutStream.manual_seed(3)
    try:
        m1, _, _ = build()
        o1 = make_optimizer(m1, capturable=True, max_grad_norm=max_norm)
        s1 = torch.optim.lr_scheduler.StepLR(o1, step_size=4, gamma=0.5)
        gs = GraphedTrainStep(m1, o1, *windows(0), warmup=WARMUP, series=series, n_his=n_his, n_pred=N_PRED)
        assert gs.fused and gs.fold
        l1, n1 = [], []
        for _ in range(REPLAYS):
            l1.append(float(gs().item()))
            n1.append(float(o1.last_grad_norm.item()))
            s1.step()
            o1.sync_lr()
        torch.cuda.synchronize()
        check_in_launch_waits(m1)
        gs.close()
    finally:
        DropoutStream.disable_device_counter()
    DropoutStream.use_device_counter(dev)
    DropoutStream.manual_seed(3)
    try:
        m2, _, _ = build()
        o2 = make_optimizer(m2, max_grad_norm=max_norm)
        s2 = torch.optim.lr_scheduler.StepLR(o2, step_size=4, gamma=0.5)
        train_step(m2, o2, *windows(0))                       # draws at 0 and advances the counter to one SITE_STRIDE
        arena = GradArena([p for p in m2.parameters() if p.grad is not None])
        l2, n2 = [], []
        for k in range(1, WARMUP + 1 + REPLAYS):
            DropoutStream.advance()                           # (the captured step's pack launch bumps the counter in front of its sites)
            value = fused_train_step(m2, o2, *windows(k), arena)
            if k > WARMUP:
                l2.append(float(value.item()))
                n2.append(float(o2.last_grad_norm.item()))
                s2.step()
        torch.cuda.synchronize()
    finally:
        DropoutStream.disable_device_counter()
    _compare(m1, o1, n1, l1, m2, o2, n2, l2)
