"""-m gpu: NAdamW and Lion (the reference's --opt nadamw | lion) on the MI355X: the captured fused step (one stgcn_grad_flush_optim launch
inside the hipGraph, NAdamW's running product advanced on the device) against eager fused steps, the reference's trajectory, a capturable
state_dict round trip, and the launch count of a fused step."""
import copy
import ctypes as C
import json
import types

import numpy as np
import pytest
import torch

from tests.helpers import real_gso
from tests.optim_kinds_util import KINDS, check_trajectory, optim_fixture, tiny_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BLOCKS = [[1], [64, 16, 64], [64, 16, 64], [128, 128], [1]]


def _make():
    from stgcn_amd import models
    from tests.gpu_util import bind_hip
    bind_hip()
    gso = torch.from_numpy(real_gso("metr_la.cheb_sym_norm_lap")).to(DEV)
    args = types.SimpleNamespace(Kt=3, Ks=3, act_func="glu", graph_conv_type="cheb_graph_conv", gso=gso, enable_bias=True,
                                 droprate=0.0, n_his=12)
    torch.manual_seed(1)
    return models.STGCNChebGraphConv(args, BLOCKS, 207).to(DEV)


def _mu_product_f64(t, b1=0.9, md=4e-3):
    return float(np.prod([b1 * (1.0 - 0.5 * 0.96 ** (k * md)) for k in range(1, t + 1)]))


@pytest.mark.parametrize("name", KINDS)
def test_graphed_fused_step_equals_eager_fused_steps(name):
    """GraphedTrainStep with a capturable NAdamW / Lion takes the fused tail; 8 replays (StepLR + sync_lr halving lr after 4) equal 8 eager
    fused steps of a twin whose optimizer keeps step count and running product on the host; the device running product equals the fp64
    product of the mu_t."""
    from stgcn_amd import DropoutStream
    from stgcn_amd.train import GradArena, GraphedTrainStep, fused_train_step, make_optimizer, train_step
    g = torch.Generator().manual_seed(4)
    xs = torch.randn(9, 8, 1, 12, 207, generator=g).to(DEV)
    ys = torch.randn(9, 8, 207, generator=g).to(DEV)
    DropoutStream.use_device_counter(torch.device(DEV))
    DropoutStream.manual_seed(3)
    m1 = _make()
    o1 = make_optimizer(m1, capturable=True, name=name)
    s1 = torch.optim.lr_scheduler.StepLR(o1, step_size=4, gamma=0.5)
    gs = GraphedTrainStep(m1, o1, xs[0], ys[0], warmup=2)
    assert gs.fused
    l1 = []
    for i in range(1, 9):
        l1.append(float(gs(xs[i], ys[i]).item()))
        s1.step()
        o1.sync_lr()
    torch.cuda.synchronize()
    gs.close()
    DropoutStream.disable_device_counter()
    # the twin: the constructor's 2 warm-up steps (plain, then fused) + its verification replay, all on batch 0, then the 8 batches
    m2 = _make()
    o2 = make_optimizer(m2, name=name)
    s2 = torch.optim.lr_scheduler.StepLR(o2, step_size=4, gamma=0.5)
    train_step(m2, o2, xs[0], ys[0])
    arena = GradArena([p for p in m2.parameters() if p.grad is not None])
    for _ in range(2):
        fused_train_step(m2, o2, xs[0], ys[0], arena)
    l2 = []
    for i in range(1, 9):
        l2.append(float(fused_train_step(m2, o2, xs[i], ys[i], arena).item()))
        s2.step()
    assert o1.param_groups[0]["lr"] == o2.param_groups[0]["lr"] == 1e-3 * 0.25
    assert np.allclose(l1, l2, rtol=1e-5, atol=0), (l1, l2)
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    for k in sd1:
        d = float((sd1[k] - sd2[k]).abs().max())
        assert d <= 2e-5, (k, d)
    t = int(o1.device_step_counter(torch.device(DEV)).item())
    assert t == 11 and o2.param_groups[0]["_step"] == 11
    if name == "nadamw":
        mu = float(o1._mu[0][t & 1].item())
        assert abs(mu - _mu_product_f64(t)) <= 1e-6 * _mu_product_f64(t), (mu, _mu_product_f64(t))
        assert o1.state_dict()["param_groups"][0]["_mu_product"] == mu


@pytest.mark.parametrize("name", KINDS)
def test_training_trajectory_matches_reference(name):
    """3 steps (dropout 0) of the tiny_cheb_f32 model with make_optimizer(name=...) on the GPU path vs the reference's run."""
    from stgcn_amd.train import make_optimizer, train_step
    from tests.gpu_util import bind_hip
    bind_hip()
    fo = optim_fixture()
    m, x, y = tiny_model(DEV)
    opt = make_optimizer(m, lr=float(fo["train.lr"]), weight_decay=float(fo["train.wd"]), name=name)
    losses = [float(train_step(m, opt, x, y).item()) for _ in range(int(fo["train.steps"]))]
    check_trajectory(name, losses, m, fo)


@pytest.mark.parametrize("name", KINDS)
def test_capturable_state_dict_roundtrip(name):
    """model + capturable optimizer saved after 5 replays and loaded into a fresh pair: the device step count and NAdamW's device running
    product come back as saved, and one eager fused step on both pairs gives bitwise-equal parameters."""
    from stgcn_amd import DropoutStream
    from stgcn_amd.train import GradArena, GraphedTrainStep, fused_train_step, make_optimizer
    g = torch.Generator().manual_seed(7)
    xs = torch.randn(7, 8, 1, 12, 207, generator=g).to(DEV)
    ys = torch.randn(7, 8, 207, generator=g).to(DEV)
    DropoutStream.use_device_counter(torch.device(DEV))
    DropoutStream.manual_seed(3)
    m1 = _make()
    o1 = make_optimizer(m1, capturable=True, name=name)
    with GraphedTrainStep(m1, o1, xs[0], ys[0], warmup=2) as gs:
        for i in range(1, 6):
            gs(xs[i], ys[i])
        torch.cuda.synchronize()
    DropoutStream.disable_device_counter()
    sd_m, sd_o = copy.deepcopy(m1.state_dict()), copy.deepcopy(o1.state_dict())
    t = sd_o["param_groups"][0]["_step"]
    assert t == 8
    m2 = _make()
    o2 = make_optimizer(m2, capturable=True, name=name)
    m2.load_state_dict(sd_m)
    o2.load_state_dict(sd_o)
    assert int(o2.device_step_counter(torch.device(DEV)).item()) == t
    if name == "nadamw":
        assert float(o2._mu[0][t & 1].item()) == sd_o["param_groups"][0]["_mu_product"] == float(o1._mu[0][t & 1].item())
    live = [i for i, p in enumerate(m1.parameters()) if p.grad is not None]
    for m, o in ((m1, o1), (m2, o2)):
        ps = list(m.parameters())
        fused_train_step(m, o, xs[6], ys[6], GradArena([ps[i] for i in live]))
    torch.cuda.synchronize()
    for (k, a), b in zip(m1.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(a, b), k
    assert int(o1.device_step_counter(torch.device(DEV)).item()) == int(o2.device_step_counter(torch.device(DEV)).item()) == t + 1


def test_fused_step_launch_count_is_the_same_for_every_optimizer():
    """one eager fused step launches as many library kernels with NAdamW or Lion as with AdamW: the optimizer rides in the one gradient
    flush (labelled reduce_adamw / reduce_nadamw / reduce_lion)."""
    from stgcn_amd import _lib
    from stgcn_amd.train import GradArena, fused_train_step, make_optimizer, train_step
    g = torch.Generator().manual_seed(9)
    x, y = torch.randn(8, 1, 12, 207, generator=g).to(DEV), torch.randn(8, 207, generator=g).to(DEV)
    counts = {}
    for name in ("adamw",) + KINDS:
        m = _make()
        o = make_optimizer(m, name=name)
        train_step(m, o, x, y)
        arena = GradArena([p for p in m.parameters() if p.grad is not None])
        fused_train_step(m, o, x, y, arena)
        torch.cuda.synchronize()
        L = _lib.lib()
        buf = C.create_string_buffer(1 << 16)
        L.dll.stgcn_profile_enable(1)
        try:
            fused_train_step(m, o, x, y, arena)
            torch.cuda.synchronize()
            L.dll.stgcn_profile_collect(buf, len(buf))
        finally:
            L.dll.stgcn_profile_enable(0)
        launched = {}
        for k, v in json.loads(buf.value.decode()).items():         # "label@tag": {"calls": ..}
            launched[k.split("@")[0]] = launched.get(k.split("@")[0], 0) + v["calls"]
        assert launched.get("reduce_" + name) == 1, launched
        assert not any(k.startswith("reduce_") and k != "reduce_" + name for k in launched), launched
        counts[name] = sum(launched.values())
    assert counts["nadamw"] == counts["lion"] == counts["adamw"], counts
