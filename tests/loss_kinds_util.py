"""Shared pieces of the loss-kind tests (tests/test_emu_loss_kinds.py on the emulator, tests/test_gpu_loss_kinds.py on the GPU): MAE
(nn.L1Loss) and Huber (nn.HuberLoss) through the stand-alone loss launch, the fused head backward and the trainers.

Inputs keep the non-smooth points out of the comparison.  sgn at 0 and Huber's switch at |d| = delta are discontinuities: an fp32
prediction that differs from the float64 oracle's by the forward tolerance could land on the other side.  So targets are never drawn at
random: target = (the oracle's float64 prediction) - off, |off| uniform in [0.05, 0.45] U [0.55, 2.0] with a random sign, delta = 0.5.
Every test asserts on the LIBRARY's own d = pred - target that min(|d|, ||d| - delta|) >= 0.04 for every element (none excluded): the
reference satisfies it by construction (0.05), so a failure is a forward error of 0.01 -- far outside FWD_TOL.
"""
import ctypes as C
import types

import numpy as np
import torch

from oracle import stblock_stages as st
from oracle import stgcn_oracle as orc
from stgcn_amd import _lib, ops
from tests.gpu_util import FWD_TOL
from tests.head_util import KEYS, NAMES, bind, grad_metrics, head_inputs, rel
from tests.helpers import cfg_from_fixture, fixture_gso, fixture_params, load_fixture

KINDS = ("mae", "huber")
DELTA = 0.5
MARGIN = 0.04
SHAPES = ((3, 5), (8, 207), (32, 325))      # test_emu_optim.py::test_mse_loss_and_grad_matches_torch


def offsets(rs, shape):
    """|off| uniform in [0.05, 0.45] U [0.55, 2.0] (the two intervals weighted by their lengths), random sign."""
    u = rs.uniform(0.0, 0.4 + 1.45, shape)
    mag = np.where(u < 0.4, 0.05 + u, 0.55 + (u - 0.4))
    return mag * rs.choice([-1.0, 1.0], shape)


def margin(d):
    """min over the elements of min(|d|, ||d| - delta|): the distance of the nearest element from a non-smooth point of either kind."""
    a = np.abs(np.asarray(d, np.float64))
    return float(np.minimum(a, np.abs(a - DELTA)).min())


def torch_loss(kind, delta=DELTA):
    return torch.nn.L1Loss() if kind == "mae" else torch.nn.HuberLoss(delta=delta) if kind == "huber" else torch.nn.MSELoss()


def loss_and_seed_np(kind, diff, scale, delta=DELTA):
    """(loss, d loss / d pred * scale) of the issue's table in diff's dtype (numpy); the loss value in float64."""
    dt, n, a = diff.dtype, diff.size, np.abs(diff)
    if kind == "mae":
        term, dterm = a, np.sign(diff)
    else:
        small = a < delta
        term, dterm = np.where(small, 0.5 * diff * diff, delta * (a - 0.5 * delta)), np.where(small, diff, delta * np.sign(diff))
    return float(term.astype(np.float64).mean()), (dterm * dt.type(scale / n)).astype(dt)


def standalone_case(dev, shape, seed=3):
    """pred / target of one stand-alone case (fp32 torch on dev) with the offsets above, two elements made bitwise equal."""
    rs = np.random.RandomState(seed)
    pred = rs.standard_normal(shape).astype(np.float32)
    target = (pred.astype(np.float64) - offsets(rs, shape)).astype(np.float32)
    target.reshape(-1)[[1, target.size - 2]] = pred.reshape(-1)[[1, pred.size - 2]]
    return torch.from_numpy(pred).to(dev), torch.from_numpy(target).to(dev)


# ---- stage level: the fused head backward (stgcn_outblock_backward_loss) -----------------------------------------------------------
# (param_seed, data_seed, offset seed) per row and kind, and next to it the worst oracle32.* metric measured on the CPU with those seeds
# (the stage oracle in np.float32 against its float64 run; bar head_util.ORACLE32_TOL = 2.5e-4).
HEAD_SEEDS = {
    ("h", "mae"): (5, 2, 0),        # oracle32 7.1e-7 (slice.tc_w.k1); the same with 32-row tiles (the oracle does not see the tile)
    ("h", "huber"): (5, 2, 0),      # oracle32 7.2e-7 (slice.tc_w.k1)
    ("a", "mae"): (5, 2, 0),        # oracle32 4.8e-7 (grad.fc2_w)
    ("a", "huber"): (5, 2, 0),      # oracle32 2.4e-6 (grad.ln_w)
    ("b", "mae"): (5, 2, 0),        # oracle32 8.9e-7 (slice.tc_w.k2)
    ("b", "huber"): (5, 2, 0),      # oracle32 8.2e-7 (slice.tc_w.k0)
}
# (head_util's own seeds served: no row's inputs nearly cancel a slice under either seed gradient, two orders below the bar.)


def run_head_loss_case(dev, name, kind, loss_scale=0.5, seed=77, offset=5, pdrop=0.5):
    """One row of tests/test_gpu_head.py::CASES through ops.loss_backward: the error keys of tests/head_util.py (loss.rel, bwd.dh1,
    bwd.dyln, bwd.dx, grad.*, slice.*, oracle32.*, kink.*), the oracle's backward fed with the oracle's own seed gradient, plus
    "margin" (see the module docstring) and "calls" (how often stgcn_outblock_backward_loss ran)."""
    from tests.test_gpu_head import CASES
    L = bind(dev)
    cuda = str(dev).startswith("cuda")
    c_in, channels, Ko, N, B, T, act, training, need_dx = CASES[name]
    param_seed, data_seed, off_seed = HEAD_SEEDS[(name, kind)]
    c0, c1 = channels
    T1 = T - Ko + 1
    p, x_np, _, _ = head_inputs(c_in, channels, Ko, N, B, T, act, pdrop, param_seed, data_seed)
    hcfg = ops.HeadConfig(Ko=Ko, n_vertex=N, c_in=c_in, channels=(c0, c1), end_channel=1, act_func=act, droprate=pdrop)
    params = [p["output." + n].clone().to(dev).requires_grad_(True) for n in NAMES]
    x = torch.from_numpy(x_np).to(dev).requires_grad_(bool(need_dx))
    wsc = ops.WorkspaceCache()
    out = ops.output_block(x, hcfg, params, training, seed, offset, wsc)

    # the oracle forward first, on the library's own dropout mask; the target from ITS prediction
    cl = lambda a: np.ascontiguousarray(a.transpose(0, 2, 3, 1))
    keep = None
    if training:
        keep = (ops.dropout_mask(B * T1 * N * c1, pdrop, seed, offset, dev).cpu().numpy().reshape(B, T1, N, c1) > 0)

    def oracle_fwd(dt):
        hp = st.head_params_np(p, dt)
        o, sv = st.outblock_fwd(cl(x_np).astype(dt), hp, Ko, c_in, channels, act, None if keep is None else keep.astype(dt), pdrop)
        return hp, o, sv

    hp64, out_ref, sv = oracle_fwd(np.float64)
    hp32, out32, sv32 = oracle_fwd(np.float32)
    target_np = (out_ref - offsets(np.random.RandomState(off_seed), out_ref.shape)).astype(np.float32)      # (B, T1, N)
    out_lib = out.detach().cpu().numpy()[:, 0]
    err = {"margin": margin(out_lib.astype(np.float64) - target_np), "fwd.out": float(np.abs(out_lib - out_ref).max())}

    calls = []
    real = L.dll.stgcn_outblock_backward_loss
    L.dll.stgcn_outblock_backward_loss = lambda *a: (calls.append(1), real(*a))[1]
    try:
        assert ops._head_node_of(out) is not None
        loss = ops.loss_backward(out, torch.from_numpy(target_np[:, None]).to(dev), kind, DELTA, grad_scale=loss_scale)
    finally:
        L.dll.stgcn_outblock_backward_loss = real
    if cuda:
        torch.cuda.synchronize()
    err["calls"] = float(len(calls))

    # the saved hidden units through a second forward into buffers of our own (head_util.run_head_case: units at the ReLU kink take the
    # library's side, and both of their counts are bounded)
    desc = ops.make_head_desc(hcfg, B, T, training, bool(need_dx))
    plan = ops.query_head_plan(desc)
    saved = torch.empty(plan.saved_floats, device=dev)
    ws2 = ops.WorkspaceCache().get(plan.ws_floats, torch.device(dev))
    out2 = torch.empty(B, T1, N, device=dev)
    pst = ops._head_struct(_lib.OutblockParams, [t.detach() for t in params])
    x_cl = x.detach().permute(0, 2, 3, 1).contiguous()
    L.check(L.dll.stgcn_outblock_forward(C.byref(desc), C.byref(pst), x_cl.data_ptr(), out2.data_ptr(), saved.data_ptr(), ws2.data_ptr(),
                                         seed, offset, None, torch.cuda.current_stream().cuda_stream if cuda else None),
            "stgcn_outblock_forward")
    svn = saved.cpu().numpy()
    rows = B * T1 * N
    h1 = sv["yln"] @ hp64["fc1_w"].T + (0.0 if hp64["fc1_b"] is None else hp64["fc1_b"])
    kink = np.abs(h1) < FWD_TOL
    if keep is not None:
        kink &= keep
    hd_lib = svn[plan.sv_hd:plan.sv_hd + rows * c1].reshape(B, T1, N, c1).astype(np.float64)
    n_kink, n_flip = float(kink.sum()), float((kink & ((hd_lib != 0) != (sv["hd"] != 0))).sum())
    eligible = float(h1.size if keep is None else keep.sum())
    err["kink.window_over_bar"] = max(0.0, n_kink - (2.0 * eligible * 2.0 * FWD_TOL / (float(h1.std()) * np.sqrt(2.0 * np.pi)) + 5.0))
    err["kink.flips_over_bar"] = max(0.0, n_flip - (0.25 * n_kink + 1.0))
    sv["hd"] = np.where(kink, hd_lib, sv["hd"])
    sv32["hd"] = np.where(kink, hd_lib.astype(np.float32), sv32["hd"])

    def oracle_bwd(dt, hp, o, s):
        lv, d = loss_and_seed_np(kind, o - target_np.astype(dt), loss_scale)
        stages = {}
        dx, g = st.outblock_bwd(d.astype(dt), s, hp, Ko, c_in, channels, act, pdrop, bool(need_dx), stages=stages)
        return dx, g, stages, lv

    dx_ref, g_ref, stages, loss_ref = oracle_bwd(np.float64, hp64, out_ref, sv)
    _, g32, _, _ = oracle_bwd(np.float32, hp32, out32, sv32)
    ws = wsc.buf.cpu().numpy()
    seg = lambda off, ref: rel(ws[off:off + ref.size].reshape(ref.shape), ref)
    err["bwd.dh1"] = seg(plan.ws_dh1, stages["dh1"])
    err["bwd.dyln"] = seg(plan.ws_dyln, stages["dyln"])
    if need_dx:
        err["bwd.dx"] = rel(cl(x.grad.cpu().numpy()), dx_ref)
    got = {}
    for k, prm in zip(KEYS, params):
        if g_ref[k] is None:
            err["grad_none_ok." + k] = 0.0 if prm.grad is None else 1.0
            got[k] = None
        else:
            got[k] = None if prm.grad is None else prm.grad.cpu().numpy().astype(np.float64)
            g_ref[k] = np.asarray(g_ref[k]).reshape(prm.shape)
            g32[k] = np.asarray(g32[k]).reshape(prm.shape)
    err.update(grad_metrics(got, g_ref, Ko, N))
    err.update(grad_metrics(g32, g_ref, Ko, N, prefix="oracle32."))
    err["loss.rel"] = abs(float(loss.item()) - loss_ref) / abs(loss_ref)
    return err


def assert_head_loss_errors(err):
    from tests.head_util import assert_head_errors
    err = dict(err)
    print(err)
    assert err.pop("margin") >= MARGIN, err
    assert err.pop("calls") == 1.0
    assert_head_errors(err)


# ---- model level: the tiny_cheb_f32 model, droprate 0 ----------------------------------------------------------------------------
def tiny_model(dev):
    from tests.optim_kinds_util import tiny_model as make
    m, x, _ = make(dev)
    return m, x


def oracle_trajectory(kind, steps=3, lr=1e-3, wd=1e-3, seed=17):
    """`steps` AdamW steps of the float64 oracle (oracle.stgcn_oracle.stgcn_forward, torch's own loss module, autograd) on the
    tiny_cheb_f32 fixture.  The target of each step is built from the oracle's prediction AT that step (module docstring).
    Returns (targets [fp32 torch, (B, N)], losses, final parameters {name: float64 torch})."""
    fx = load_fixture("tiny_cheb_f32")
    cfg = cfg_from_fixture(fx)
    p = {k: v.clone() for k, v in fixture_params(fx, cfg, torch.float64).items()}
    gso = torch.from_numpy(fixture_gso("tiny_cheb_f32", fx)).double()
    rs = np.random.RandomState(int(fx["seed"]) + 1)
    B, N = int(fx["B"]), int(fx["n_vertex"])
    x = torch.from_numpy(rs.standard_normal((B, 1, cfg.n_his, N))).float().double()      # (tests/optim_kinds_util.tiny_model's batch)
    ro = np.random.RandomState(seed)
    fn, state, targets, losses = torch_loss(kind), {}, [], []
    for _ in range(steps):
        leaves = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
        pred = orc.stgcn_forward(x, gso, leaves, cfg).reshape(B, -1)
        y = (pred.detach() - torch.from_numpy(offsets(ro, (B, N)))).float()
        loss = fn(pred, y.double())
        names = list(leaves)
        grads = dict(zip(names, torch.autograd.grad(loss, [leaves[n] for n in names], allow_unused=True)))
        orc.adamw_step(p, grads, state, lr=lr, weight_decay=wd)
        targets.append(y)
        losses.append(float(loss))
    return targets, losses, p


def check_model_trajectory(dev, kind, fused):
    """Three AdamW steps through train_step / fused_train_step against the oracle's: the bars of
    tests/test_gpu_model.py::test_training_trajectory_matches_oracle (losses 1e-4 relative, every parameter 1e-4 absolute and its
    sum of magnitudes 1e-4 relative)."""
    from stgcn_amd.train import GradArena, fused_train_step, make_optimizer, train_step
    bind(dev)
    targets, ref_losses, ref_p = oracle_trajectory(kind)
    m, x = tiny_model(dev)
    opt = make_optimizer(m)
    losses, arena = [], None
    for i, y in enumerate(targets):
        y = y.to(dev)
        with torch.no_grad():
            d = m(x).reshape(len(x), -1) - y
        assert margin(d.cpu().numpy()) >= MARGIN, (i, margin(d.cpu().numpy()))
        if fused and i > 0:      # (the first step is plain: it shows which parameters are live, as GraphedTrainStep does it)
            if arena is None:
                arena = GradArena([q for q in m.parameters() if q.grad is not None])
            losses.append(float(fused_train_step(m, opt, x, y, arena, loss=kind, huber_delta=DELTA)))
        else:
            losses.append(float(train_step(m, opt, x, y, loss=kind, huber_delta=DELTA)))
    print(kind, fused, losses, ref_losses)
    assert np.allclose(losses, ref_losses, rtol=1e-4), (losses, ref_losses)
    for k, v in m.state_dict().items():
        r = ref_p[k]
        s = float(r.abs().sum())
        assert abs(float(v.double().abs().sum()) - s) <= 1e-4 * s + 1e-9, k
        assert float((v.double().cpu() - r).abs().max()) <= 1e-4, k


def check_tail_step_shares(dev, kind, monkeypatch, n=5):
    """tail_step with a ragged batch of n windows split over world = 2 shares (3 + 2): the sum of the two ranks' gradients and losses
    equals the single-rank gradient of the mean.  One process: the all-reduce is stubbed to the identity and the shares are added here."""
    from stgcn_amd import train
    bind(dev)
    targets, _, _ = oracle_trajectory(kind, steps=1)
    x = tiny_model(dev)[1][:n].contiguous()
    y = targets[0][:n].contiguous().to(dev)
    monkeypatch.setattr(train.dist, "all_reduce", lambda t, op=None: None)

    def run(world, rank):
        m, _ = tiny_model(dev)
        loss = train.tail_step(m, torch.optim.SGD(m.parameters(), lr=0.0), x, y, world=world, rank=rank, loss=kind, huber_delta=DELTA)
        return float(loss), {k: q.grad.detach().double().cpu() for k, q in m.named_parameters() if q.grad is not None}

    l1, g1 = run(1, 0)
    la, ga = run(2, 0)
    lb, gb = run(2, 1)
    assert set(g1) == set(ga) == set(gb)
    assert abs(la + lb - l1) <= 1e-6 * abs(l1), (la, lb, l1)
    for k, g in g1.items():
        assert float((ga[k] + gb[k] - g).abs().max()) <= 1e-5 * float(g.abs().max()) + 1e-12, k


def target_from_own_prediction(m, x, seed=23):
    """A target built from the model's own fp32 prediction and the offsets above (for comparisons of two library paths)."""
    with torch.no_grad():
        pred = m(x).reshape(len(x), -1).float()
    return (pred.double().cpu() - torch.from_numpy(offsets(np.random.RandomState(seed), tuple(pred.shape)))).float().to(x.device)


def fresh_tiny(dev):
    m, x = tiny_model(dev)
    return m, x, target_from_own_prediction(m, x)


# ---- the stand-alone launch (stgcn_loss_grad) --------------------------------------------------------------------------------------
def check_standalone_matches_torch(dev, kind, shape):
    """Against torch's own module in float64: test_mse_loss_and_grad_matches_torch's bars (loss 1e-6 relative, gradient 1e-7 of its
    max); elements with pred == target bitwise get a gradient of exactly 0."""
    bind(dev)
    pred, y = standalone_case(dev, shape)
    d = (pred - y).cpu().numpy()
    same = d == 0
    assert same.sum() == 2 and margin(d[~same]) >= MARGIN
    loss, dpred = ops.loss_and_grad(pred, y, kind, DELTA, grad_scale=0.5)
    p = pred.double().cpu().requires_grad_(True)
    ref = torch_loss(kind)(p, y.double().cpu())
    ref.backward()
    g = 0.5 * p.grad
    assert abs(float(loss[0]) - float(ref)) <= 1e-6 * abs(float(ref))
    assert float((dpred.double().cpu() - g).abs().max()) <= 1e-7 * float(g.abs().max()) + 1e-12
    assert bool((dpred.cpu()[torch.from_numpy(same)] == 0).all())


def check_standalone_mse_is_bitwise_the_mse_entry(dev, shape):
    L = bind(dev)
    pred, y = standalone_case(dev, shape)
    loss_a, d_a = torch.empty(1, device=dev), torch.empty_like(pred)
    stream = torch.cuda.current_stream().cuda_stream if str(dev).startswith("cuda") else None
    L.check(L.dll.stgcn_mse_loss_grad(pred.data_ptr(), y.data_ptr(), pred.numel(), 0.3, loss_a.data_ptr(), d_a.data_ptr(), None, 0, stream),
            "stgcn_mse_loss_grad")
    loss_b, d_b = ops.loss_and_grad(pred, y, "mse", grad_scale=0.3)
    loss_c, d_c = ops.mse_loss_and_grad(pred, y, grad_scale=0.3)
    assert torch.equal(loss_a, loss_b) and torch.equal(d_a, d_b) and torch.equal(loss_a, loss_c) and torch.equal(d_a, d_c)
    p = pred.double().cpu().requires_grad_(True)      # (and it is still nn.MSELoss())
    ref = torch.nn.MSELoss()(p, y.double().cpu())
    assert abs(float(loss_b[0]) - float(ref)) <= 1e-6 * abs(float(ref))


def check_standalone_nan(dev, kind, shape=(8, 207)):
    """One NaN prediction: NaN loss, NaN gradient there (torch's L1 backward would give 0), every other element unaffected."""
    bind(dev)
    pred, y = standalone_case(dev, shape)
    _, clean = ops.loss_and_grad(pred, y, kind, DELTA)
    bad = pred.clone()
    bad[3, 11] = float("nan")
    loss, dpred = ops.loss_and_grad(bad, y, kind, DELTA)
    assert bool(torch.isnan(loss[0])) and bool(torch.isnan(dpred[3, 11]))
    mask = torch.ones_like(pred, dtype=torch.bool)
    mask[3, 11] = False
    assert torch.equal(dpred[mask], clean[mask])


def check_standalone_label_modes(dev, kind):
    """Index mode and window-table mode equal the same call on the gathered label rows (tests/test_emu_shuffle.py's table test)."""
    bind(dev)
    B, N, n_his, n_pred, pos = 4, 20, 12, 3, 2
    table = [7, 0, 3, 9, 1, 5, 8, 2]
    rs = np.random.RandomState(1)
    series = torch.from_numpy(rs.standard_normal((max(table) + n_his + n_pred + B + 2, N)).astype(np.float32)).to(dev)
    shift = n_his + n_pred - 1
    yv = series[shift:shift + B]                                     # label rows of windows 0 .. B-1, moved by the index / the table
    for tab in (None, table):
        starts = list(range(pos, pos + B)) if tab is None else tab[pos:pos + B]
        y = torch.stack([series[s + shift] for s in starts]).contiguous()
        pred = (y.double().cpu() + torch.from_numpy(offsets(rs, (B, N)))).float().to(dev)
        l_ref, d_ref = ops.loss_and_grad(pred, y, kind, DELTA)
        idx = torch.tensor([pos], dtype=torch.int64, device=dev)
        ops.bind_input_index(yv, idx, N, table=None if tab is None else torch.tensor(tab, dtype=torch.int64, device=dev))
        try:
            l_got, d_got = ops.loss_and_grad(pred, yv, kind, DELTA)
        finally:
            ops.unbind_input_index(yv)
        assert float(l_ref) == float(l_got) and torch.equal(d_ref, d_got)


def check_standalone_refusals(dev):
    import pytest
    L = bind(dev)
    pred, y = standalone_case(dev, (3, 5))
    before = L.dll.stgcn_version()
    with pytest.raises(ValueError, match="kind 7"):
        ops.loss_and_grad(pred, y, 7)
    for delta in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="delta"):
            ops.loss_and_grad(pred, y, "huber", delta)
    with pytest.raises(ValueError, match="unknown loss"):
        ops.loss_and_grad(pred, y, "l1")
    assert before == _lib.ABI_VERSION == 10
    ops.loss_and_grad(pred, y, "mae", float("nan"))      # delta is Huber's alone


def check_fused_equals_two_call(dev, kind, model_xy=None):
    """ops.loss_backward on the head's own prediction (fused: stgcn_outblock_backward_loss, once) against the one-launch loss +
    pred.backward(dpred), and a prediction with arithmetic behind the head (two-call path): test_mse_loss_fused_into_the_head_backward's
    1e-6.  model_xy: (model, x, y) in place of the tiny_cheb_f32 model (a bf16 model: the seed is formed from the same fp32 predictions
    either way)."""
    L = bind(dev)
    m, x, y = fresh_tiny(dev) if model_xy is None else model_xy
    B = len(x)
    pred = m(x).reshape(B, -1)
    assert margin((pred.detach().float() - y).cpu().numpy()) >= MARGIN
    assert ops._head_node_of(pred) is not None and ops._head_node_of(pred * 1.0) is None
    loss_a, dpred = ops.loss_and_grad(pred, y, kind, DELTA, grad_scale=0.5)
    pred.backward(dpred)
    ga = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    calls = []
    real = L.dll.stgcn_outblock_backward_loss
    L.dll.stgcn_outblock_backward_loss = lambda *a: (calls.append(1), real(*a))[1]
    try:
        m.zero_grad(set_to_none=True)
        loss_b = ops.loss_backward(m(x).reshape(B, -1), y, kind, DELTA, grad_scale=0.5)
        assert calls == [1]
        assert abs(float(loss_a) - float(loss_b)) <= 1e-6 * abs(float(loss_a))
        for k, p in m.named_parameters():
            if p.grad is not None:
                assert float((p.grad - ga[k]).abs().max()) <= 1e-6 * float(ga[k].abs().max()) + 1e-12, k
        m.zero_grad(set_to_none=True)
        loss_c = ops.loss_backward(m(x).reshape(B, -1) * 1.0, y, kind, DELTA, grad_scale=0.5)
        assert calls == [1] and abs(float(loss_a) - float(loss_c)) <= 1e-6 * abs(float(loss_a))
    finally:
        L.dll.stgcn_outblock_backward_loss = real
