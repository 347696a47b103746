"""NAdamW and Lion (the reference's --opt nadamw | lion, main.py:149-152) on the emulator: alone vs the reference's optimizers, the fused
step tail (stgcn_grad_flush_optim) vs the plain step (stgcn_optim_step), the data-parallel split, the reference's 3-step trajectory,
state_dict round trips and the C ABI's refusals."""
import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from stgcn_amd import _lib
from tests.emu_util import bind_emulator
from tests.optim_kinds_util import KINDS, check_trajectory, optim_fixture, tiny_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _make(name, params, lr, wd):
    from stgcn_amd.optim import Lion, NAdamW
    return NAdamW(params, lr=lr, weight_decay=wd) if name == "nadamw" else Lion(params, lr=lr, weight_decay=wd)


@pytest.mark.parametrize("name", KINDS)
def test_optimizer_alone_matches_reference(name):
    """6 steps on seeded tensors vs torch.optim.NAdam(decoupled_weight_decay=True) / the reference's Lion, StepLR halving lr after step 3;
    a parameter without a gradient is not touched (no decay, no state)."""
    bind_emulator()
    fo = optim_fixture()
    n, steps, lr, wd = int(fo["alone.n"]), int(fo["alone.steps"]), float(fo["alone.lr"]), float(fo["alone.wd"])
    ps = [torch.nn.Parameter(torch.from_numpy(fo[f"alone.init.{i}"].copy())) for i in range(n)]
    idle = torch.nn.Parameter(torch.ones(3))
    opt = _make(name, ps + [idle], lr, wd)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=3, gamma=0.5)       # main.py:156
    pre = f"alone.{name}."
    for k in range(steps):
        prev = [p.detach().clone() for p in ps]
        lr_k = opt.param_groups[0]["lr"]
        for i, p in enumerate(ps):
            p.grad = torch.from_numpy(fo[f"alone.grad.{i}"][k].copy())
        opt.step()
        sched.step()
        assert opt.param_groups[0]["lr"] == fo[pre + "lr"][k]
        for i, p in enumerate(ps):
            got, ref = p.detach().numpy(), fo[pre + f"param.{i}"][k]
            tol = (2e-6 if name == "nadamw" else 2e-7) * max(1.0, float(np.abs(ref).max()))
            assert float(np.abs(got - ref).max()) <= tol, (k, i, float(np.abs(got - ref).max()))
            m_ref = fo[pre + f"exp_avg.{i}"][k]
            assert float(np.abs(opt.state[p]["exp_avg"].numpy() - m_ref).max()) <= 1e-6 * max(1.0, float(np.abs(m_ref).max()))
            if name == "lion":
                # the sign the kernel applied, read off the update p' = p (1 - lr wd) - lr sign(c): every one equals the reference's sign(c)
                pd = prev[i].numpy() * np.float32(1.0 - lr_k * wd)
                applied = np.rint((pd - got) / np.float32(lr_k))
                assert np.array_equal(applied, np.sign(fo[pre + f"c.{i}"][k])), (k, i)
                assert "exp_avg_sq" not in opt.state[p]
            else:
                v_ref = fo[pre + f"exp_avg_sq.{i}"][k]
                assert float(np.abs(opt.state[p]["exp_avg_sq"].numpy() - v_ref).max()) <= 1e-6 * max(1.0, float(np.abs(v_ref).max()))
        if name == "nadamw":
            assert abs(opt.param_groups[0]["_mu_product"] - fo[pre + "mu_product"][k]) <= 1e-6 * fo[pre + "mu_product"][k]
    assert torch.equal(idle, torch.ones(3)) and idle not in opt.state


def _fused_vs_plain(name):
    from stgcn_amd.train import GradArena, fused_train_step, make_optimizer, train_step
    g = torch.Generator().manual_seed(5)
    m1, x0, _ = tiny_model()
    m2, _, _ = tiny_model()
    B, N = x0.shape[0], x0.shape[-1]
    xs = torch.randn(4, B, 1, x0.shape[2], N, generator=g)
    ys = torch.randn(4, B, N, generator=g)
    o1, o2 = make_optimizer(m1, lr=1e-2, weight_decay=1e-2, name=name), make_optimizer(m2, lr=1e-2, weight_decay=1e-2, name=name)
    l1 = [float(train_step(m1, o1, xs[i], ys[i])) for i in range(4)]
    l2 = [float(train_step(m2, o2, xs[0], ys[0]))]
    arena = GradArena([p for p in m2.parameters() if p.grad is not None])
    l2 += [float(fused_train_step(m2, o2, xs[i], ys[i], arena)) for i in range(1, 4)]
    assert l1 == l2, (l1, l2)
    for (k, a), b in zip(m1.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(a, b), k
    for p1, p2 in zip(m1.parameters(), m2.parameters()):
        if p1.grad is not None:
            assert torch.equal(o1.state[p1]["exp_avg"], o2.state[p2]["exp_avg"])
    if name == "nadamw":
        assert o1.param_groups[0]["_mu_product"] == o2.param_groups[0]["_mu_product"]


@pytest.mark.parametrize("name", KINDS)
def test_fused_tail_equals_plain_step(name):
    """fused_train_step (ONE stgcn_grad_flush_optim launch: reductions + the optimizer on each fresh gradient element) is bitwise the plain
    step (per-module reduce launches + stgcn_optim_step): same partials, same summation order, same element arithmetic."""
    bind_emulator()
    _fused_vs_plain(name)


@pytest.mark.parametrize("name", KINDS)
def test_world2_split_equals_fused_world1(name):
    """world > 1: reductions into the flat arena, the all-reduce (two identical ranks: x 2), then step() = stgcn_optim_step -- bitwise the
    world = 1 fused tail."""
    from stgcn_amd.train import GradArena, fused_train_step, make_optimizer, train_step
    bind_emulator()
    g = torch.Generator().manual_seed(6)
    ms = [tiny_model()[0] for _ in range(2)]
    x0 = tiny_model()[1]
    B, N = x0.shape[0], x0.shape[-1]
    xs, ys = torch.randn(3, B, 1, x0.shape[2], N, generator=g), torch.randn(3, B, N, generator=g)
    opts = [make_optimizer(m, lr=1e-2, weight_decay=1e-2, name=name) for m in ms]
    arenas = []
    for m, o in zip(ms, opts):
        train_step(m, o, xs[0], ys[0])
        arenas.append(GradArena([p for p in m.parameters() if p.grad is not None]))
    for i in (1, 2):
        fused_train_step(ms[0], opts[0], xs[i], ys[i], arenas[0])
        fused_train_step(ms[1], opts[1], xs[i], ys[i], arenas[1], world=2, all_reduce=lambda f: f.mul_(2))
    for (k, a), b in zip(ms[0].state_dict().items(), ms[1].state_dict().values()):
        assert torch.equal(a, b), k


def test_fused_tail_big_table_forms():
    """the same two bitwise checks with reduce_kernel's 16-byte state forms (dvec) forced on the small model (STGCN_REDUCE_BIG): Lion's
    form moves exp_avg only."""
    env = dict(os.environ, STGCN_REDUCE_BIG="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_emu_optim_kinds.py", "-x", "-q", "-p", "no:cacheprovider", "-k",
                        "fused_tail_equals_plain_step or world2_split"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "4 passed" in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("name", KINDS)
def test_training_trajectory_matches_reference(name):
    """3 steps of the reference model (tiny_cheb_f32 weights, dropout 0) with make_optimizer(name=...) vs the reference's run."""
    from stgcn_amd.train import make_optimizer, train_step
    bind_emulator()
    fo = optim_fixture()
    m, x, y = tiny_model()
    opt = make_optimizer(m, lr=float(fo["train.lr"]), weight_decay=float(fo["train.wd"]), name=name)
    losses = [float(train_step(m, opt, x, y)) for _ in range(int(fo["train.steps"]))]
    check_trajectory(name, losses, m, fo)


@pytest.mark.parametrize("name", KINDS)
def test_state_dict_roundtrip_continues_bitwise(name):
    """save the model and the optimizer mid-run, load both into a fresh pair: the next steps are bitwise those of the original pair (the
    step count and NAdamW's running product travel in the state_dict)."""
    from stgcn_amd.train import make_optimizer, train_step
    bind_emulator()
    g = torch.Generator().manual_seed(8)
    m1, x0, _ = tiny_model()
    B, N = x0.shape[0], x0.shape[-1]
    xs, ys = torch.randn(5, B, 1, x0.shape[2], N, generator=g), torch.randn(5, B, N, generator=g)
    o1 = make_optimizer(m1, lr=1e-2, weight_decay=1e-2, name=name)
    for i in range(3):
        train_step(m1, o1, xs[i], ys[i])
    sd_m, sd_o = copy.deepcopy(m1.state_dict()), copy.deepcopy(o1.state_dict())
    assert sd_o["param_groups"][0]["_step"] == 3
    if name == "nadamw":
        assert 0.0 < sd_o["param_groups"][0]["_mu_product"] < 0.5
    m2, _, _ = tiny_model()
    o2 = make_optimizer(m2, lr=1e-2, weight_decay=1e-2, name=name)
    m2.load_state_dict(sd_m)
    o2.load_state_dict(sd_o)
    for i in (3, 4):
        train_step(m1, o1, xs[i], ys[i])
        train_step(m2, o2, xs[i], ys[i])
    for (k, a), b in zip(m1.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(a, b), k


def test_c_abi_refuses_unknown_kind_and_missing_state():
    L = bind_emulator()
    p, gr, m, v = (torch.zeros(8) for _ in range(4))
    table = (_lib.AdamwTensor * 1)()
    table[0].param, table[0].grad, table[0].exp_avg, table[0].exp_avg_sq, table[0].numel = p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), 8

    def hyper(kind):
        h = _lib.OptimHyper()
        h.kind, h.lr, h.beta1, h.beta2, h.eps, h.weight_decay, h.momentum_decay, h.step, h.mu_product = kind, 1e-3, 0.9, 0.99, 1e-8, 0.0, 4e-3, 1, 1.0
        return h
    for kind in (3, -1, 99):
        assert L.dll.stgcn_optim_step(table, 1, C.byref(hyper(kind)), None) == 2
        assert b"unknown optimizer kind" in L.dll.stgcn_last_error()
        assert L.dll.stgcn_grad_flush_optim(0, None, None, None, None, table, 1, C.byref(hyper(kind)), None) == 2
    assert L.dll.stgcn_optim_step(table, 1, None, None) == 2
    table[0].exp_avg_sq = None
    assert L.dll.stgcn_optim_step(table, 1, C.byref(hyper(_lib.OPT_NADAMW)), None) == 2         # NAdamW needs exp_avg_sq
    assert L.dll.stgcn_optim_step(table, 1, C.byref(hyper(_lib.OPT_ADAMW)), None) == 2
    gr.fill_(1.0)
    assert L.dll.stgcn_optim_step(table, 1, C.byref(hyper(_lib.OPT_LION)), None) == 0           # Lion has none
    assert torch.equal(p, torch.full((8,), -1e-3)) and torch.equal(m, torch.full((8,), 1.0 - 0.99))     # sign(0.1) = 1; m = (1 - beta2) g
    table[0].exp_avg = None
    assert L.dll.stgcn_optim_step(table, 1, C.byref(hyper(_lib.OPT_LION)), None) == 2


def test_make_optimizer_kinds():
    from stgcn_amd.optim import AdamW, Lion, NAdamW
    from stgcn_amd.train import make_optimizer
    m = torch.nn.Linear(3, 2)
    assert type(make_optimizer(m, name="adamw")) is AdamW
    o = make_optimizer(m, name="nadamw", capturable=True, lr=2e-3, weight_decay=1e-3)
    assert type(o) is NAdamW and o.capturable and o.param_groups[0]["momentum_decay"] == 4e-3 and o.param_groups[0]["betas"] == (0.9, 0.999)
    o = make_optimizer(m, name="lion", capturable=True)
    assert type(o) is Lion and o.capturable and o.param_groups[0]["betas"] == (0.9, 0.99) and hasattr(o, "flush_with")
    with pytest.raises(ValueError, match="undefined"):
        make_optimizer(m, name="tiger")
