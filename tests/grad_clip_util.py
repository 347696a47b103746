"""Shared cases of the gradient-clipping tests (tests/test_emu_grad_clip.py on the emulator, tests/test_gpu_grad_clip.py on the GPU): the
norm kernel through the C ABI, optimizer trajectories against ``clip_grad_norm_`` + torch / the reference's Lion (tests/golden/optim_clip.npz,
made by make_golden_clip.py), max_grad_norm = inf against the unclipped unfused path, and the two norm producers on a model.  Every function
takes the device the bound library computes on ("cpu": the emulator)."""
import ctypes as C
import os
import re

import numpy as np
import torch

from stgcn_amd import _lib
from tests.helpers import load_fixture
from tests.optim_kinds_util import tiny_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_KINDS = ("adamw", "nadamw", "lion")
U23 = 2.0 ** -23


def multi_tensor_batch():
    """tensors one multi-tensor launch of stgcn_optim_step holds, read from the kernel source"""
    src = open(os.path.join(ROOT, "stgcn_amd", "csrc", "stgcn_kernels_head.hip.h")).read()
    return int(re.search(r"constexpr int kAdamwMaxTensors = (\d+);", src).group(1))


def norm_tables():
    """{case: [element counts]}; 'offset4': the tensor starts 4 bytes past a 16-byte boundary"""
    many = [1 + (7 * i) % 13 for i in range(2 * multi_tensor_batch() + 3)]
    return {"one": [1], "255_256_257": [255, 256, 257], "offset4": [1027], "70001": [70001], "many": many}


def _values(counts, seed):
    """seeded normals times magnitudes spread over 1e-18 .. 1e+15 (fp64 squares keep every element significant)"""
    rs = np.random.RandomState(seed)
    return [(rs.standard_normal(n) * 10.0 ** rs.uniform(-18, 15, n)).astype(np.float32) for n in counts]


def _table(tensors, with_state=None):
    t = (_lib.AdamwTensor * len(tensors))()
    for i, g in enumerate(tensors):
        t[i].grad, t[i].numel = g.data_ptr(), g.numel()
        if with_state is not None:
            p, m, v = with_state[i]
            t[i].param, t[i].exp_avg, t[i].exp_avg_sq = p.data_ptr(), m.data_ptr(), v.data_ptr()
    return t


def _sync(dev):
    if str(dev).startswith("cuda"):
        torch.cuda.synchronize()


def _device_tensors(arrays, dev, offset4):
    out = []
    for a in arrays:
        buf = torch.zeros(len(a) + 8, dtype=torch.float32, device=dev)
        lo = (-(buf.data_ptr() // 4)) % 4 + (1 if offset4 else 0)       # first element at a 16-byte boundary, or 4 bytes past one
        g = buf[lo:lo + len(a)]
        g.copy_(torch.from_numpy(a))
        assert g.data_ptr() % 16 == (4 if offset4 else 0)
        out.append(g)
    return out


def clip_words(L, table, count):
    w = C.c_int64(0)
    assert L.dll.stgcn_grad_clip_words(table, count, C.byref(w)) == 0
    return int(w.value)


def run_norm(L, dev, tensors, max_norm, state=None):
    """stgcn_grad_norm over device tensors; returns (state tensor, its words on the host after the launch)"""
    table = _table(tensors)
    if state is None:
        state = torch.zeros(clip_words(L, table, len(tensors)), dtype=torch.float64, device=dev)
    clip = _lib.GradClip()
    clip.state, clip.state_words, clip.max_norm = state.data_ptr(), state.numel(), max_norm
    L.check(L.dll.stgcn_grad_norm(table, len(tensors), C.byref(clip), None), "stgcn_grad_norm")
    _sync(dev)
    return state, state.cpu().numpy().copy()


def total_and_coef(words):
    f = words.view(np.float32)
    return f[2 * _lib.CLIP_TOTAL], f[2 * _lib.CLIP_COEF]


def expected_coef(total, max_norm):
    """min(1, max_norm / (total + 1e-6)) in fp32, as torch forms it (clamp: a NaN stays a NaN)"""
    with np.errstate(all="ignore"):
        q = np.float32(max_norm) / (np.float32(total) + np.float32(1e-6))
    return q if np.isnan(q) else min(np.float32(1.0), q)


def check_norm_case(L, dev, case, max_norm=1.0):
    counts = norm_tables()[case]
    arrays = _values(counts, seed=len(counts) + counts[0])
    tensors = _device_tensors(arrays, dev, offset4=case == "offset4")
    if case == "many":
        table = _table(tensors)
        assert len(tensors) > 2 * multi_tensor_batch() and clip_words(L, table, len(tensors)) >= _lib.CLIP_HDR_WORDS + 1
    state, w1 = run_norm(L, dev, tensors, max_norm)
    ref = float(np.sqrt(sum((a.astype(np.float64) ** 2).sum() for a in arrays)))
    total, coef = total_and_coef(w1)
    print(case, "total", total, "float64 norm", ref, "rel", abs(float(total) - ref) / ref, "coef", coef)
    assert abs(float(total) - ref) <= U23 * ref, (case, total, ref)
    assert coef.tobytes() == np.float32(expected_coef(total, max_norm)).tobytes(), (case, coef, expected_coef(total, max_norm))
    assert w1[3] == 0.0                                        # the ticket word is re-armed
    _, w2 = run_norm(L, dev, tensors, max_norm, state)         # a second pass over the same data: bit-identical words
    assert w1.tobytes() == w2.tobytes(), case
    # max_norm = inf: the norm is measured, coef is exactly 1
    _, w3 = run_norm(L, dev, tensors, float("inf"), state)
    t3, c3 = total_and_coef(w3)
    assert t3.tobytes() == total.tobytes() and c3 == np.float32(1.0)
    # one NaN element: a NaN total, and a NaN coef (torch: clamp keeps it)
    tensors[-1][counts[-1] // 2] = float("nan")
    _, w4 = run_norm(L, dev, tensors, max_norm, state)
    t4, c4 = total_and_coef(w4)
    assert np.isnan(t4) and np.isnan(c4), (case, t4, c4)


def check_refusals(L, dev):
    """a too-small state or a bad max_norm: STGCN_ERR_INVALID from every entry, nothing launched (state and parameters unchanged)"""
    g = torch.full((70001,), 0.5, device=dev)
    p, m, v = (torch.full((70001,), 1.0, device=dev) for _ in range(3))
    table = _table([g], [(p, m, v)])
    need = clip_words(L, table, 1)
    assert need > _lib.CLIP_HDR_WORDS + 1
    state = torch.full((need,), 7.0, dtype=torch.float64, device=dev)
    h = _lib.OptimHyper()
    h.kind, h.lr, h.beta1, h.beta2, h.eps, h.weight_decay, h.momentum_decay, h.step, h.mu_product = _lib.OPT_ADAMW, 1e-3, 0.9, 0.99, 1e-8, 0.0, 4e-3, 1, 1.0

    def clip(words, max_norm, ptr=state.data_ptr()):
        c = _lib.GradClip()
        c.state, c.state_words, c.max_norm = ptr, words, max_norm
        return c
    bad = [clip(need - 1, 1.0), clip(_lib.CLIP_HDR_WORDS, 1.0), clip(0, 1.0), clip(need, 0.0), clip(need, -1.0), clip(need, float("nan")),
           clip(need, float("-inf")), clip(need, 1.0, None)]
    for c in bad:
        for kind in (_lib.OPT_ADAMW, _lib.OPT_NADAMW, _lib.OPT_LION):
            h.kind = kind
            assert L.dll.stgcn_optim_step_clip(table, 1, C.byref(h), C.byref(c), None) == 2, (c.state_words, c.max_norm)
        assert L.dll.stgcn_grad_norm(table, 1, C.byref(c), None) == 2, (c.state_words, c.max_norm)
        assert L.dll.stgcn_grad_flush_clip(0, None, None, None, None, C.byref(c), None) == 2
    assert L.dll.stgcn_grad_norm(table, 1, None, None) == 2 and L.dll.stgcn_optim_step_clip(table, 1, C.byref(h), None, None) == 2
    _sync(dev)
    assert torch.equal(state.cpu(), torch.full((need,), 7.0, dtype=torch.float64))
    for t in (p, m, v):
        assert torch.equal(t.cpu(), torch.full((70001,), 1.0))
    # the same arguments with a good block run
    state.zero_()
    good = clip(need, float("inf"))
    assert L.dll.stgcn_grad_norm(table, 1, C.byref(good), None) == 0
    h.kind = _lib.OPT_LION
    assert L.dll.stgcn_optim_step_clip(table, 1, C.byref(h), C.byref(good), None) == 0
    _sync(dev)
    assert torch.equal(p.cpu(), torch.full((70001,), float(np.float32(1.0) - np.float32(1e-3))))      # sign(c) = 1, no decay


# ---- optimizer trajectories --------------------------------------------------------------------------------------------------------------
def _make_ours(name, params, lr, wd, **kw):
    from stgcn_amd.optim import AdamW, Lion, NAdamW
    return {"adamw": AdamW, "nadamw": NAdamW, "lion": Lion}[name](params, lr=lr, weight_decay=wd, **kw)


def _torch_reference(name, fo):
    """clip_grad_norm_ + torch.optim on the fixture's inputs, run inline: per step parameters, exp_avg, exp_avg_sq, torch's norm"""
    n, steps, lr, wd, max_norm = int(fo["n"]), int(fo["steps"]), float(fo["lr"]), float(fo["wd"]), float(fo["max_norm"])
    ps = [torch.nn.Parameter(torch.from_numpy(fo[f"init.{i}"].copy())) for i in range(n)]
    idle = torch.nn.Parameter(torch.ones(3))
    if name == "adamw":
        opt = torch.optim.AdamW(ps + [idle], lr=lr, weight_decay=wd)
    else:
        opt = torch.optim.NAdam(ps + [idle], lr=lr, weight_decay=wd, decoupled_weight_decay=True)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=3, gamma=0.5)
    rec = {"norm": []}
    for k in range(steps):
        for i, p in enumerate(ps):
            p.grad = torch.from_numpy(fo[f"grad.{i}"][k].copy())
        total = float(torch.nn.utils.clip_grad_norm_([p for p in ps + [idle] if p.grad is not None], max_norm))
        ratio = total / max_norm
        assert ratio >= 2.0 or ratio <= 0.5, (k, ratio)      # every step is clearly on one side of the threshold
        rec["norm"].append(total)
        opt.step()
        sched.step()
        for i, p in enumerate(ps):
            rec.setdefault(f"param.{i}", []).append(p.detach().numpy().copy())
            rec.setdefault(f"exp_avg.{i}", []).append(opt.state[p]["exp_avg"].numpy().copy())
            rec.setdefault(f"exp_avg_sq.{i}", []).append(opt.state[p]["exp_avg_sq"].numpy().copy())
    return rec


def check_optimizer_trajectory(name, dev):
    """6 steps on the fixture's tensors with max_grad_norm = the norm of the unscaled first gradient (steps 1, 2, 5 clip; 3, 4, 6 do not)
    against clip_grad_norm_ + the reference optimizer, at the bars of tests/test_emu_optim_kinds.py / tests/test_emu_optim.py."""
    fo = load_fixture("optim_clip")
    n, steps, lr, wd, max_norm = int(fo["n"]), int(fo["steps"]), float(fo["lr"]), float(fo["wd"]), float(fo["max_norm"])
    if name == "lion":
        ref = {k[len("lion."):]: fo[k] for k in fo if k.startswith("lion.")}
        for k in range(steps):
            ratio = float(ref["norm"][k]) / max_norm
            assert ratio >= 2.0 or ratio <= 0.5, (k, ratio)
    else:
        ref = _torch_reference(name, fo)
    assert [float(r) > max_norm for r in ref["norm"]] == [True, True, False, False, True, False]
    ps = [torch.nn.Parameter(torch.from_numpy(fo[f"init.{i}"].copy()).to(dev)) for i in range(n)]
    idle = torch.nn.Parameter(torch.ones(3, device=dev))
    opt = _make_ours(name, ps + [idle], lr, wd, max_grad_norm=max_norm)
    assert opt.state_dict()["param_groups"][0]["max_grad_norm"] == max_norm
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=3, gamma=0.5)
    b1 = opt.param_groups[0]["betas"][0]
    ptol = {"adamw": 2e-6, "nadamw": 2e-6, "lion": 2e-7}[name]
    for k in range(steps):
        grads = [torch.from_numpy(fo[f"grad.{i}"][k].copy()).to(dev) for i in range(n)]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt.step()
        sched.step()
        total, coef = float(opt.last_grad_norm.item()), float(opt.last_clip_coef.item())
        assert abs(total - float(ref["norm"][k])) <= 1e-6 * float(ref["norm"][k]), (k, total, ref["norm"][k])      # (torch sums in fp32)
        assert (coef < 1.0) == (float(ref["norm"][k]) > max_norm) and coef == float(expected_coef(np.float32(total), max_norm))
        for p, g in zip(ps, grads):
            assert torch.equal(p.grad, g)                    # .grad keeps the unclipped gradient (torch scales it in place)
        for i, p in enumerate(ps):
            got, want = p.detach().cpu().numpy(), ref[f"param.{i}"][k]
            if name == "lion":
                # where the reference's update direction is clear of zero (tests/optim_kinds_util.check_trajectory): elsewhere its sign is
                # not determined at fp32 accuracy of coef * g
                c = ref[f"c.{i}"][:k + 1]
                clear = np.all(np.abs(c) > 1e-5 * np.abs(c).reshape(len(c), -1).max(1).reshape((-1,) + (1,) * (c.ndim - 1)), axis=0)
                assert clear.mean() > 0.9, (k, i)
                got, want = got[clear], want[clear]
            if want.size:
                assert float(np.abs(got - want).max()) <= ptol * max(1.0, float(np.abs(want).max())), (name, k, i, float(np.abs(got - want).max()))
            m_got, m_ref = opt.state[p]["exp_avg"].cpu().numpy(), ref[f"exp_avg.{i}"][k]
            bar = 1e-6 * max(1.0, float(np.abs(m_ref).max()))
            assert float(np.abs(m_got - m_ref).max()) <= bar, (name, k, i)
            if name != "lion":
                v_ref = ref[f"exp_avg_sq.{i}"][k]
                assert float(np.abs(opt.state[p]["exp_avg_sq"].cpu().numpy() - v_ref).max()) <= 1e-6 * max(1.0, float(np.abs(v_ref).max())), (name, k, i)
            if k == 0:
                # the first moment after step 1 is (1 - beta) coef g -- and NOT the unclipped (1 - beta) g: the clip is no no-op (AdamW's
                # update alone is nearly scale-invariant and would hide one).  Lion keeps m = (1 - beta2) coef g.
                beta = opt.param_groups[0]["betas"][1] if name == "lion" else b1
                g_np = fo[f"grad.{i}"][0].astype(np.float64)
                assert float(np.abs(m_got - (1.0 - beta) * coef * g_np).max()) <= bar, (name, i)
                if i == n - 1:      # (the largest tensor: its largest gradient element is far above the bar)
                    assert float(np.abs(m_got - (1.0 - beta) * g_np).max()) > 100 * bar, (name, i)
    assert torch.equal(idle.detach().cpu(), torch.ones(3)) and idle not in opt.state


def check_two_groups_share_one_norm(dev):
    """two parameter groups with their own lr: ONE norm over the live gradients of both, as clip_grad_norm_ over all parameters"""
    from stgcn_amd.optim import AdamW
    g = torch.Generator().manual_seed(12)
    init = [torch.randn(300, generator=g), torch.randn(7, 9, generator=g), torch.randn(40, generator=g)]
    grads = [torch.randn(t.shape, generator=g) * 3 for t in init]
    a = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    b = [torch.nn.Parameter(t.clone()) for t in init]
    groups = lambda ps: [dict(params=ps[:2], lr=1e-2), dict(params=ps[2:], lr=3e-3)]
    o1 = AdamW(groups(a), weight_decay=1e-2, max_grad_norm=2.0)
    o2 = torch.optim.AdamW(groups(b), weight_decay=1e-2)
    for _ in range(2):
        for p, q, gr in zip(a, b, grads):
            p.grad, q.grad = gr.clone().to(dev), gr.clone()
        total = float(torch.nn.utils.clip_grad_norm_(b, 2.0))
        o1.step()
        o2.step()
        assert abs(float(o1.last_grad_norm.item()) - total) <= 1e-6 * total
    for p, q in zip(a, b):
        assert float((p.detach().cpu() - q.detach()).abs().max()) <= 2e-6 * max(1.0, float(q.detach().abs().max()))


# ---- on a model --------------------------------------------------------------------------------------------------------------------------
def _batches(x0, steps, seed):
    g = torch.Generator().manual_seed(seed)
    B, N = x0.shape[0], x0.shape[-1]
    return (torch.randn(steps, B, 1, x0.shape[2], N, generator=g).to(x0.device), torch.randn(steps, B, N, generator=g).to(x0.device))


def _unfused_step(model, optimizer, x, y, arena):
    """the existing unfused path on the arena: reduce-only ``sink.flush()``, then ``optimizer.step()``"""
    from stgcn_amd import ops
    arena.install()
    with ops.grad_sink_scope(arena.sink):
        pred = model(x).reshape(len(x), -1)
        value = ops.loss_backward(pred, y, "mse", 1.0, grad_scale=1.0)
    arena.sink.flush(stream=torch.cuda.current_stream(x.device).cuda_stream if x.is_cuda else None)
    optimizer.step()
    return value[0]


def check_inf_is_bitwise_unclipped(name, dev):
    """max_grad_norm = inf (norm measured, coef == 1, g * 1) over 3 steps of tiny_model: the plain step and the fused tail are bitwise the
    unclipped plain step and the unclipped unfused path ``sink.flush(); optimizer.step()``."""
    from stgcn_amd.train import GradArena, fused_train_step, make_optimizer, train_step
    m1, x0, _ = tiny_model(dev)
    m2, _, _ = tiny_model(dev)
    xs, ys = _batches(x0, 4, 5)
    o1 = make_optimizer(m1, lr=1e-2, weight_decay=1e-2, name=name, max_grad_norm=float("inf"))
    o2 = make_optimizer(m2, lr=1e-2, weight_decay=1e-2, name=name)
    l1, l2 = [float(train_step(m1, o1, xs[0], ys[0]))], [float(train_step(m2, o2, xs[0], ys[0]))]
    a1 = GradArena([p for p in m1.parameters() if p.grad is not None])
    a2 = GradArena([p for p in m2.parameters() if p.grad is not None])
    for i in range(1, 4):
        l1.append(float(fused_train_step(m1, o1, xs[i], ys[i], a1)))
        l2.append(float(_unfused_step(m2, o2, xs[i], ys[i], a2)))
        assert float(o1.last_clip_coef.item()) == 1.0 and float(o1.last_grad_norm.item()) > 0.0
    assert l1 == l2, (l1, l2)
    for (k, a), b in zip(m1.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(a, b), k
    for p1, p2 in zip(m1.parameters(), m2.parameters()):
        if p1.grad is not None:
            assert torch.equal(p1.grad, p2.grad)
            for key in o2.state[p2]:
                assert torch.equal(o1.state[p1][key], o2.state[p2][key]), key
    assert o2.last_grad_norm is None


def _grad_norm64(grads):
    return float(np.sqrt(sum((g.detach().cpu().numpy().astype(np.float64) ** 2).sum() for g in grads)))


def check_two_producers_agree(dev, name="adamw"):
    """tiny_model, max_grad_norm at half the first step's norm: ``train_step`` (stgcn_grad_norm) and ``fused_train_step`` (the flush
    epilogue) each report the float64 norm of their own fp32 gradients within 2^-23 relative, and their parameters agree bitwise (the bar
    of the existing fused-versus-plain tests)."""
    from stgcn_amd.train import GradArena, fused_train_step, fwd_loss_bwd, make_optimizer, train_step
    m0, x0, _ = tiny_model(dev)
    xs, ys = _batches(x0, 4, 5)
    fwd_loss_bwd(m0, xs[0], ys[0])
    max_norm = 0.5 * _grad_norm64([p.grad for p in m0.parameters() if p.grad is not None])
    m1, _, _ = tiny_model(dev)
    m2, _, _ = tiny_model(dev)
    o1 = make_optimizer(m1, lr=1e-2, weight_decay=1e-2, name=name, max_grad_norm=max_norm)
    o2 = make_optimizer(m2, lr=1e-2, weight_decay=1e-2, name=name, max_grad_norm=max_norm)
    train_step(m1, o1, xs[0], ys[0])
    train_step(m2, o2, xs[0], ys[0])
    assert abs(float(o1.last_clip_coef.item()) - 0.5) < 1e-3         # the first step clips to half
    arena = GradArena([p for p in m2.parameters() if p.grad is not None])
    clipped = 0
    for i in range(1, 4):
        train_step(m1, o1, xs[i], ys[i])
        fused_train_step(m2, o2, xs[i], ys[i], arena)
        for o, grads in ((o1, [p.grad for p in m1.parameters() if p.grad is not None]), (o2, list(arena.grads.values()))):
            ref = _grad_norm64(grads)
            got = float(o.last_grad_norm.item())
            print("producer", "norm" if o is o1 else "flush", i, got, ref, abs(got - ref) / ref)
            assert abs(got - ref) <= U23 * ref, (i, got, ref)
        assert float(o1.last_clip_coef.item()) == float(o2.last_clip_coef.item())
        clipped += float(o2.last_clip_coef.item()) < 1.0
    assert clipped >= 1
    for (k, a), b in zip(m1.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(a, b), k
