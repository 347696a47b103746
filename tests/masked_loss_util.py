"""Shared pieces of the masked-loss tests (tests/test_emu_masked_loss.py on the emulator, tests/test_gpu_masked_loss.py on the GPU): the
loss and the metrics over observed labels only, through the stand-alone launch (stgcn_loss_grad_masked), the fused head backward
(stgcn_outblock_backward_loss_masked), the trainers and the evaluation launch (stgcn_eval_accumulate_masked).

The reference everywhere is torch (or numpy) on the CPU in float64: (term * m).sum() / m.sum() and its autograd gradient.  Inputs keep
the non-smooth points of MAE and Huber out of the comparison as tests/loss_kinds_util.py does (its offsets, DELTA and MARGIN), for the
OBSERVED elements; masked elements hold anything -- in half of the stand-alone cases a NaN label and an inf prediction.
"""
import numpy as np
import torch

from oracle import stgcn_oracle as orc
from stgcn_amd import _lib, data, ops
from tests import loss_kinds_util as LK
from tests.head_util import bind
from tests.helpers import cfg_from_fixture, fixture_gso, fixture_params, load_fixture
from tests.loss_kinds_util import DELTA, MARGIN, margin, offsets

KINDS = ("mse", "mae", "huber")
SHAPES = ((3, 5), (9, 207))      # 1863 elements: the 1024-thread walk wraps
PATTERNS = ("random30", "row", "first", "last")


def mask_pattern(pattern, shape, seed=11):
    m = np.ones(shape, dtype=bool)
    if pattern == "random30":
        m = np.random.RandomState(seed).uniform(size=shape) >= 0.3
    elif pattern == "row":
        m[shape[0] // 2] = False
    elif pattern == "first":
        m.reshape(-1)[0] = False
    elif pattern == "last":
        m.reshape(-1)[-1] = False
    return m


def term64(kind, d, delta=DELTA):
    """the per-element term of the header's loss table, float64 torch (differentiable)"""
    F = torch.nn.functional
    z = torch.zeros_like(d)
    if kind == "mse":
        return F.mse_loss(d, z, reduction="none")
    if kind == "mae":
        return F.l1_loss(d, z, reduction="none")
    return F.huber_loss(d, z, reduction="none", delta=delta)


def masked_ref(kind, pred, y, m, scale=1.0):
    """(loss, d loss / d pred * scale) in float64: (term * m).sum() / m.sum() and autograd; masked inputs are replaced by zeros first (a
    masked element is selected out, whatever it holds)."""
    mt = torch.from_numpy(np.asarray(m, dtype=bool))
    p = torch.where(mt, pred.double().cpu(), torch.zeros((), dtype=torch.float64)).requires_grad_(True)
    t = torch.where(mt, y.double().cpu(), torch.zeros((), dtype=torch.float64))
    md = mt.double()
    loss = (term64(kind, p - t) * md).sum() / md.sum()
    loss.backward()
    return float(loss), scale * p.grad


def check_standalone_matches_torch(dev, kind):
    """Every shape and mask pattern; the bars of loss_kinds_util's unmasked comparison (loss 1e-6 relative, gradient 1e-7 of its largest
    magnitude + 1e-12); the gradient of a masked element is +0.0 exactly; poisoned masked elements (every other case) change nothing.

    (The bars hold for every kind because a gradient element under a partial mask carries ONE fp32 rounding: with three -- the difference,
    1 / n_valid, the product -- MSE's elements of largest |d| came out up to 1.04e-7 of the largest magnitude off at (9, 207).)"""
    bind(dev)
    case, over = 0, []
    for shape in SHAPES:
        for pattern in PATTERNS:
            pred, y = LK.standalone_case(dev, shape)
            m = mask_pattern(pattern, shape)
            mt = torch.from_numpy(m).to(dev)
            d = (pred - y).cpu().numpy()
            obs = d[m]
            assert margin(obs[obs != 0]) >= MARGIN      # (standalone_case makes two elements bitwise equal: sgn(0) = 0)
            loss_ref, g_ref = masked_ref(kind, pred, y, m, 0.5)
            poison = case % 2 == 1
            case += 1
            if poison:
                pred = torch.where(mt, pred, torch.full_like(pred, float("inf")))
                y = torch.where(mt, y, torch.full_like(y, float("nan")))
            loss, dpred = ops.loss_and_grad(pred, y, kind, DELTA, grad_scale=0.5, valid=mt)
            got = dpred.double().cpu()
            print(kind, shape, pattern, poison, float(loss), loss_ref, float((got - g_ref).abs().max()))
            assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dpred).all())
            masked = dpred.cpu()[torch.from_numpy(~m)]
            assert bool((masked == 0).all()) and not bool(torch.signbit(masked).any())
            assert abs(float(loss[0]) - loss_ref) <= 1e-6 * abs(loss_ref)
            err, bar = float((got - g_ref).abs().max()), 1e-7 * float(g_ref.abs().max()) + 1e-12
            if err > bar:
                over.append((shape, pattern, err, bar))
    assert not over, over


# ---- labels and mask from a resident series: plain, index and table addressing ------------------------------------------------------
N_HIS, N_PRED, SN, SB = 12, 3, 7, 3
SHIFT = N_HIS + N_PRED - 1


def series_case(dev, seed=1):
    """A resident (rows, 7) series with a random mask, a non-monotone table whose middle entry is the last usable window, the position
    words and predictions off the gathered labels by loss_kinds_util's offsets."""
    rs = np.random.RandomState(seed)
    rows = 12 + N_HIS + N_PRED
    num = rows - N_HIS - N_PRED
    table = [7, 0, num - 1, 9, 1, 5, 8, 2]
    series = torch.from_numpy(rs.standard_normal((rows, SN)).astype(np.float32)).to(dev)
    valid = torch.from_numpy(rs.uniform(size=(rows, SN)) >= 0.3).to(dev)
    return series, valid, table, 2, rs


def addressing_modes(dev, series, valid, table, pos, all_ones=False):
    """yields (mode, explicit labels, explicit mask, bound label view, bound LossMask view, unbind): the batch of SB windows at `pos`
    gathered by hand, and the same labels / mask read in place through an index word (and a table)."""
    if all_ones:
        valid = torch.ones_like(valid)
    whole = ops.LossMask(valid)
    for mode in ("plain", "index", "table"):
        starts = list(range(SB)) if mode == "plain" else list(range(pos, pos + SB)) if mode == "index" else table[pos:pos + SB]
        y = torch.stack([series[s + SHIFT] for s in starts]).contiguous()
        v = torch.stack([valid[s + SHIFT] for s in starts]).contiguous()
        yv, mv = series[SHIFT:SHIFT + SB], whole.rows(SHIFT, SB)
        if mode != "plain":
            idx = torch.tensor([pos], dtype=torch.int64, device=dev)
            tab = None if mode == "index" else torch.tensor(table, dtype=torch.int64, device=dev)
            ops.bind_input_index(yv, idx, SN, table=tab)
            mv.bind(idx, SN, table=tab)
        try:
            yield mode, y, v, yv, mv
        finally:
            ops.unbind_input_index(yv)
            mv.unbind()


def check_resident_series_equals_gather(dev, kind):
    """Index mode and table mode (non-monotone, one entry at the last usable window) equal the explicit gather bit for bit: the check of
    loss_kinds_util.check_standalone_label_modes with the mask read in place beside the labels."""
    bind(dev)
    series, valid, table, pos, rs = series_case(dev)
    for mode, y, v, yv, mv in addressing_modes(dev, series, valid, table, pos):
        pred = (y.double().cpu() + torch.from_numpy(offsets(rs, (SB, SN)))).float().to(dev)
        l_ref, d_ref = ops.loss_and_grad(pred, y, kind, DELTA, valid=v)
        l_got, d_got = ops.loss_and_grad(pred, yv, kind, DELTA, valid=mv)
        assert int(v.sum()) not in (0, SB * SN)
        assert torch.equal(l_ref, l_got) and torch.equal(d_ref, d_got), mode
        loss_ref, g_ref = masked_ref(kind, pred, y, v.cpu().numpy())
        assert abs(float(l_got) - loss_ref) <= 1e-6 * abs(loss_ref), mode


def check_all_ones_is_the_unmasked_entry(dev, kind):
    """An all-ones mask gives the unmasked entry's loss and gradient bit for bit on the plain, index and table addressing; an all-zero
    mask gives loss 0.0 and a zero gradient."""
    bind(dev)
    series, valid, table, pos, rs = series_case(dev)
    for mode, y, v, yv, mv in addressing_modes(dev, series, valid, table, pos, all_ones=True):
        pred = (y.double().cpu() + torch.from_numpy(offsets(rs, (SB, SN)))).float().to(dev)
        l_ref, d_ref = ops.loss_and_grad(pred, yv, kind, DELTA, grad_scale=0.3)
        l_got, d_got = ops.loss_and_grad(pred, yv, kind, DELTA, grad_scale=0.3, valid=mv)
        assert torch.equal(l_ref, l_got) and torch.equal(d_ref, d_got), mode
    for shape in SHAPES:
        pred, y = LK.standalone_case(dev, shape)
        l_ref, d_ref = ops.loss_and_grad(pred, y, kind, DELTA, grad_scale=0.3)
        l_got, d_got = ops.loss_and_grad(pred, y, kind, DELTA, grad_scale=0.3, valid=torch.ones(shape, dtype=torch.bool, device=dev))
        assert torch.equal(l_ref, l_got) and torch.equal(d_ref, d_got), shape
        l0, d0 = ops.loss_and_grad(pred, y, kind, DELTA, valid=torch.zeros(shape, dtype=torch.uint8, device=dev))
        assert float(l0) == 0.0 and bool((d0 == 0).all()) and not bool(torch.signbit(d0).any())


# ---- model level --------------------------------------------------------------------------------------------------------------------
def batch_mask(shape, seed, dev):
    return torch.from_numpy(np.random.RandomState(seed).uniform(size=tuple(shape)) >= 0.3).to(dev)


def check_fused_equals_two_call(dev, kind, model_xy=None):
    """loss_kinds_util.check_fused_equals_two_call under a mask: ops.loss_backward on the head's own prediction (fused:
    stgcn_outblock_backward_loss_masked, exactly once) against the one-launch masked loss + pred.backward(dpred), its 1e-6 bars."""
    L = bind(dev)
    m, x, y = LK.fresh_tiny(dev) if model_xy is None else model_xy
    B = len(x)
    valid = batch_mask(y.shape, 31, dev)
    pred = m(x).reshape(B, -1)
    assert margin((pred.detach().float() - y).cpu().numpy()) >= MARGIN
    assert ops._head_node_of(pred) is not None
    loss_a, dpred = ops.loss_and_grad(pred, y, kind, DELTA, grad_scale=0.5, valid=valid)
    assert bool((dpred[~valid] == 0).all())
    pred.backward(dpred)
    ga = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    calls, plain = [], []
    real, real_plain = L.dll.stgcn_outblock_backward_loss_masked, L.dll.stgcn_outblock_backward_loss
    L.dll.stgcn_outblock_backward_loss_masked = lambda *a: (calls.append(1), real(*a))[1]
    L.dll.stgcn_outblock_backward_loss = lambda *a: (plain.append(1), real_plain(*a))[1]
    try:
        m.zero_grad(set_to_none=True)
        loss_b = ops.loss_backward(m(x).reshape(B, -1), y, kind, DELTA, grad_scale=0.5, valid=valid)
        assert calls == [1] and plain == []
        assert abs(float(loss_a) - float(loss_b)) <= 1e-6 * abs(float(loss_a))
        for k, p in m.named_parameters():
            if p.grad is not None:
                assert float((p.grad - ga[k]).abs().max()) <= 1e-6 * float(ga[k].abs().max()) + 1e-12, k
        m.zero_grad(set_to_none=True)      # arithmetic behind the head: the two-call path takes the mask too
        loss_c = ops.loss_backward(m(x).reshape(B, -1) * 1.0, y, kind, DELTA, grad_scale=0.5, valid=valid)
        assert calls == [1] and plain == [] and abs(float(loss_a) - float(loss_c)) <= 1e-6 * abs(float(loss_a))
    finally:
        L.dll.stgcn_outblock_backward_loss_masked, L.dll.stgcn_outblock_backward_loss = real, real_plain


_traj = {}


def oracle_trajectory(kind, steps=3, lr=1e-3, wd=1e-3, seed=17):
    """loss_kinds_util.oracle_trajectory with the torch masked loss: `steps` AdamW steps of the float64 oracle model on the tiny_cheb_f32
    fixture, a fresh 30 % mask every step.  Computed once per kind.  Returns (targets, masks, losses, final parameters)."""
    if kind in _traj:
        return _traj[kind]
    fx = load_fixture("tiny_cheb_f32")
    cfg = cfg_from_fixture(fx)
    p = {k: v.clone() for k, v in fixture_params(fx, cfg, torch.float64).items()}
    gso = torch.from_numpy(fixture_gso("tiny_cheb_f32", fx)).double()
    rs = np.random.RandomState(int(fx["seed"]) + 1)
    B, N = int(fx["B"]), int(fx["n_vertex"])
    x = torch.from_numpy(rs.standard_normal((B, 1, cfg.n_his, N))).float().double()
    ro = np.random.RandomState(seed)
    state, targets, masks, losses = {}, [], [], []
    for i in range(steps):
        leaves = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
        pred = orc.stgcn_forward(x, gso, leaves, cfg).reshape(B, -1)
        y = (pred.detach() - torch.from_numpy(offsets(ro, (B, N)))).float()
        mk = torch.from_numpy(ro.uniform(size=(B, N)) >= 0.3)
        md = mk.double()
        loss = (term64(kind, pred - y.double()) * md).sum() / md.sum()
        names = list(leaves)
        grads = dict(zip(names, torch.autograd.grad(loss, [leaves[n] for n in names], allow_unused=True)))
        orc.adamw_step(p, grads, state, lr=lr, weight_decay=wd)
        targets.append(y)
        masks.append(mk)
        losses.append(float(loss))
    _traj[kind] = (targets, masks, losses, p)
    return _traj[kind]


def check_model_trajectory(dev, kind, fused):
    """Three AdamW steps through train_step / fused_train_step with valid= against the oracle's: loss_kinds_util.check_model_trajectory's
    bars (losses 1e-4 relative, every parameter 1e-4 absolute and its sum of magnitudes 1e-4 relative)."""
    from stgcn_amd.train import GradArena, fused_train_step, make_optimizer, train_step
    bind(dev)
    targets, masks, ref_losses, ref_p = oracle_trajectory(kind)
    m, x = LK.tiny_model(dev)
    opt = make_optimizer(m)
    losses, arena = [], None
    for i, (y, mk) in enumerate(zip(targets, masks)):
        y, mk = y.to(dev), mk.to(dev)
        with torch.no_grad():
            d = m(x).reshape(len(x), -1) - y
        assert margin(d[mk].cpu().numpy()) >= MARGIN, (i, margin(d[mk].cpu().numpy()))
        if fused and i > 0:
            if arena is None:
                arena = GradArena([q for q in m.parameters() if q.grad is not None])
            losses.append(float(fused_train_step(m, opt, x, y, arena, loss=kind, huber_delta=DELTA, valid=mk)))
        else:
            losses.append(float(train_step(m, opt, x, y, loss=kind, huber_delta=DELTA, valid=mk)))
    print(kind, fused, losses, ref_losses)
    assert np.allclose(losses, ref_losses, rtol=1e-4), (losses, ref_losses)
    for k, v in m.state_dict().items():
        r = ref_p[k]
        s = float(r.abs().sum())
        assert abs(float(v.double().abs().sum()) - s) <= 1e-4 * s + 1e-9, k
        assert float((v.double().cpu() - r).abs().max()) <= 1e-4, k


def check_tail_step(dev, kind):
    """tail_step(valid=) for world == 1 equals train_step's masked loss; world > 1 names why it is not served."""
    import pytest
    from stgcn_amd import train
    bind(dev)
    m, x, y = LK.fresh_tiny(dev)
    valid = batch_mask(y.shape, 5, dev)
    la = float(train.tail_step(m, torch.optim.SGD(m.parameters(), lr=0.0), x, y, loss=kind, huber_delta=DELTA, valid=valid))
    lb = float(train.train_step(m, torch.optim.SGD(m.parameters(), lr=0.0), x, y, loss=kind, huber_delta=DELTA, valid=valid))
    assert la == lb
    with pytest.raises(NotImplementedError, match="observed count"):
        train.tail_step(m, None, x, y, world=2, loss=kind, huber_delta=DELTA, valid=valid)


# ---- evaluation ---------------------------------------------------------------------------------------------------------------------
BIG, SINGLE = "0", str(1 << 40)      # STGCN_EVAL_BIG: every batch takes the partial slabs / the single workgroup


def eval_case(B, N, seed, rows=None):
    """z-scored labels whose raw values are at least 10 (MAPE is then of WMAPE's size), predictions near them, a 30 % mask, and NaN at
    the masked labels."""
    rs = np.random.RandomState(seed)
    rows = B if rows is None else rows
    scale, mean = rs.uniform(5.0, 25.0, N).astype(np.float32), rs.uniform(40.0, 70.0, N).astype(np.float32)
    raw = rs.uniform(10.0, 90.0, (rows, N))
    y = ((raw - mean) / scale).astype(np.float32)
    pred = (y + 0.3 * rs.standard_normal((rows, N))).astype(np.float32)
    valid = rs.uniform(size=(rows, N)) >= 0.3
    y[~valid] = np.nan
    return pred, y, valid, scale, mean


def metrics64(pred, y, valid, scale, mean):
    """the float64 host loop: MSE in z-scored units, MAE / RMSE / WMAPE / MAPE after the inverse transform, over observed labels"""
    ok = valid.reshape(-1)
    p, t = pred.astype(np.float64), np.where(valid, y, 0.0).astype(np.float64)
    sc, mu = scale.astype(np.float64), mean.astype(np.float64)
    mse = float((((p - t) ** 2).reshape(-1)[ok]).mean())
    mae, rmse, wmape, mape = data.masked_metrics_from_arrays(t * sc + mu, p * sc + mu, ok)
    return {"mse": mse, "mae": mae, "rmse": rmse, "wmape": wmape, "mape": mape, "elements": int(ok.sum())}


def mape32(pred, y, valid, scale, mean):
    """the device's MAPE formula restated in numpy float32 (terms fp32, the sum float64)"""
    t = np.where(valid, y, np.float32(0)).astype(np.float32)
    d = np.abs((t - pred) * scale)
    term = d / np.abs(t * scale + mean)
    return float(term.astype(np.float64)[valid].sum() / valid.sum())


def assert_metrics(got, ref, what=""):
    """Bars of tests/test_gpu_eval_pass.py: 1e-4 absolute on MSE, MAE, RMSE; 1e-5 on WMAPE; MAPE takes WMAPE's 1e-5 (raw labels >= 10)."""
    print(what, "device", got, "float64", ref)
    for k in ("mse", "mae", "rmse"):
        assert abs(got[k] - ref[k]) <= 1e-4, (k, got, ref)
    assert abs(got["wmape"] - ref["wmape"]) <= 1e-5 and abs(got["mape"] - ref["mape"]) <= 1e-5, (got, ref)
    assert got["elements"] == ref["elements"]


def run_eval(dev, batches, scale, mean, masked=True, pos_num=None):
    """batches: (pred, y, valid, first_valid) numpy; returns the state after all of them.  pos_num: read through position words over a
    resident label / mask buffer of that many windows (y / valid of the first batch are then the whole buffers)."""
    state, pos = ops.eval_state(dev, masked=masked)
    state.fill_(float("nan"))
    state[8:] = 7.0
    ops.eval_arm(state, pos)
    sc, mu = torch.from_numpy(scale).to(dev), torch.from_numpy(mean).to(dev)
    for pred, y, valid, fv in batches:
        p, t = torch.from_numpy(pred).to(dev).contiguous(), torch.from_numpy(y).to(dev).contiguous()
        v = None if not masked else torch.from_numpy(valid).to(dev).contiguous()
        if pos_num is None:
            ops.eval_accumulate(p, t, state, sc, mu, first_valid=fv, valid=v)
        else:
            B = len(pred)
            ops.eval_accumulate(p, t[:B], state, sc, mu, pos=pos, num_windows=pos_num, valid=None if v is None else v[:B])
    return state, pos


def check_eval_against_float64(dev, knob, monkeypatch):
    """(B, N) = (4, 7) with first_valid = 2, through the single workgroup or the partial slabs (STGCN_EVAL_BIG), then one more batch."""
    bind(dev)
    monkeypatch.setenv("STGCN_EVAL_BIG", knob)
    B, N = 4, 7
    pred, y, valid, scale, mean = eval_case(B, N, 21)
    pred2, y2, valid2, _, _ = eval_case(B, N, 22)
    state, _ = run_eval(dev, [(pred, y, valid, 2), (pred2, y2, valid2, 0)], scale, mean)
    again, _ = run_eval(dev, [(pred, y, valid, 2), (pred2, y2, valid2, 0)], scale, mean)
    assert torch.equal(state[:8], again[:8]), "the summation order must not depend on the run"
    P, Y, V = np.concatenate([pred[2:], pred2]), np.concatenate([y[2:], y2]), np.concatenate([valid[2:], valid2])
    ref = metrics64(P, Y, V, scale, mean)
    restated = abs(mape32(P, Y, V, scale, mean) - ref["mape"])
    print("MAPE restated in numpy float32 against float64:", restated)
    assert restated <= 1e-5      # (the issue's condition for taking WMAPE's bar as it is)
    assert_metrics(ops.eval_metrics(state[:6].tolist()), ref, knob)
    assert int(state[6:7].cpu().view(torch.int64).item()) == 0, "the ticket word is re-armed"
    slabs = state[8:].cpu().numpy()
    assert np.all(slabs == 7.0) if knob == SINGLE else not np.all(slabs[:12] == 7.0)


def check_eval_pos_walk(dev, knob, monkeypatch):
    """48 windows at batch 32 over resident labels and mask: the second batch starts at window 16 and counts from its window 16 on."""
    bind(dev)
    monkeypatch.setenv("STGCN_EVAL_BIG", knob)
    num, B, N = 48, 32, 7
    pred, y, valid, scale, mean = eval_case(num, N, 23)
    state, pos = run_eval(dev, [(pred[:B], y, valid, 0), (pred[16:48], y, valid, 0)], scale, mean, pos_num=num)
    assert pos.tolist()[:3] == [16, 32, 2]
    assert_metrics(ops.eval_metrics(state[:6].tolist()), metrics64(pred, y, valid, scale, mean), "pos walk " + knob)


def check_eval_all_ones_is_the_unmasked_kernel(dev, knob, monkeypatch):
    bind(dev)
    monkeypatch.setenv("STGCN_EVAL_BIG", knob)
    B, N = 4, 7
    pred, y, valid, scale, mean = eval_case(B, N, 24)
    y = np.where(valid, y, np.float32(0.25)).astype(np.float32)
    ones = np.ones_like(valid)
    batches = [(pred, y, ones, 2), (pred[::-1].copy(), y[::-1].copy(), ones, 0)]
    a, _ = run_eval(dev, batches, scale, mean, masked=True)
    b, _ = run_eval(dev, batches, scale, mean, masked=False)
    assert torch.equal(a[:5], b[:5]) and float(a[4]) == (2 * B - 2) * N


def host_pass_metrics(model, zs, valid, z, n_his, n_pred, B, dev):
    """float64 metrics of the model's predictions over every window of the split (data.WindowSampler batches)"""
    sampler = data.WindowSampler(zs, n_his, n_pred, dev)      # (the inputs are what the series holds, missing readings included)
    ys, ps = [], []
    model.eval()
    with torch.no_grad():
        for x, y in sampler.batches(B):
            ys.append(y.cpu().numpy())
            ps.append(model(x).view(len(x), -1).float().cpu().numpy())
    shift = n_his + n_pred - 1
    return metrics64(np.concatenate(ps), np.concatenate(ys), valid[shift:shift + len(sampler)].astype(bool),
                     np.asarray(z.scale_, np.float32).reshape(-1), np.asarray(z.mean_, np.float32).reshape(-1)), len(sampler)


def pass_series(rows, N, seed):
    """a raw series of readings >= 10 with 20 % failed detectors (reported as 0), its mask and its z-score"""
    rs = np.random.RandomState(seed)
    raw = np.clip(55.0 + 12.0 * rs.standard_normal((rows, N)), 10.0, None)
    raw[rs.uniform(size=raw.shape) < 0.2] = 0.0
    valid = data.observed_mask(raw, 0.0)
    z = data.ZScore().fit(raw)
    return z.transform(raw).astype(np.float32), valid, z


def check_eval_pass(dev, model, N, capture, num=11, B=4):
    """GraphedEvalPass(valid=) over a ragged split against the float64 host loop; capture=True (GPU): the replayed graph equals the eager
    launches bit for bit."""
    from stgcn_amd.train import GraphedEvalPass
    n_his, n_pred = 12, 3
    bound = set(ops._input_index)
    zs, valid, z = pass_series(num + n_his + n_pred, N, 3)
    with GraphedEvalPass(model, zs, n_his, n_pred, B, scaler=z, capture=capture, valid=valid) as ev:
        assert (ev.graph is not None) == bool(capture)
        got = ev.run()
        assert ev.run() == got
    if capture:
        with GraphedEvalPass(model, zs, n_his, n_pred, B, scaler=z, capture=False, valid=valid) as ev:
            assert ev.run() == got
    ref, windows = host_pass_metrics(model, zs, valid, z, n_his, n_pred, B, dev)
    assert got.pop("windows") == windows == num
    assert_metrics(got, ref, "pass")
    assert set(ops._input_index) == bound, "a closed pass leaves no index binding behind"


# ---- refusals and the ABI -------------------------------------------------------------------------------------------------------------
def check_refusals(dev):
    import pytest
    from stgcn_amd import train
    L = bind(dev)
    bound = set(ops._input_index)
    pred, y = LK.standalone_case(dev, (3, 5))
    ok = torch.ones(3, 5, dtype=torch.bool, device=dev)
    assert L.dll.stgcn_version() == _lib.ABI_VERSION == 10
    with pytest.raises(ValueError, match="shape"):
        ops.loss_and_grad(pred, y, "mae", valid=ok[:2])
    with pytest.raises(ValueError, match="bool or uint8"):
        ops.loss_and_grad(pred, y, "mae", valid=ok.float())
    with pytest.raises(ValueError, match="bool or uint8"):
        ops.loss_backward(pred, y, "mae", valid=ok.to(torch.int32))
    with pytest.raises(ValueError, match="unknown loss"):
        ops.loss_and_grad(pred, y, "l1", valid=ok)
    with pytest.raises(ValueError, match="delta"):
        ops.loss_and_grad(pred, y, "huber", 0.0, valid=ok)
    # a stride that is not a multiple of row_elems: refused by the library before any launch
    series = torch.zeros(8, 5, device=dev)
    whole = ops.LossMask(torch.ones(8, 5, dtype=torch.bool, device=dev))
    yv, mv = series[1:4], whole.rows(1, 3)
    idx = torch.zeros(1, dtype=torch.int64, device=dev)
    ops.bind_input_index(yv, idx, 6)
    mv.bind(idx, 6)
    try:
        with pytest.raises(ValueError, match="not a multiple of row_elems"):
            ops.loss_and_grad(pred, yv, "mae", valid=mv)
    finally:
        ops.unbind_input_index(yv)
        mv.unbind()
    with pytest.raises(ValueError, match="same index word"):      # a bound label view needs the mask bound beside it
        ops.bind_input_index(yv, idx, 5)
        try:
            ops.loss_and_grad(pred, yv, "mae", valid=mv)
        finally:
            ops.unbind_input_index(yv)
    # the C ABI: NULL mask parts, row_elems <= 0, labels that are not whole rows
    mk = _lib.LossMask()
    loss, dp = torch.empty(1, device=dev), torch.empty_like(pred)
    vb, rv = torch.ones(15, dtype=torch.uint8, device=dev), torch.full((3,), 5, dtype=torch.int32, device=dev)

    def call(valid, row_valid, row_elems):
        import ctypes as C
        mk.valid, mk.row_valid, mk.row_elems = valid, row_valid, row_elems
        return L.dll.stgcn_loss_grad_masked(1, 1.0, pred.data_ptr(), y.data_ptr(), 15, 1.0, loss.data_ptr(), dp.data_ptr(), None, 0, None, 0,
                                            C.byref(mk), None if str(dev) == "cpu" else torch.cuda.current_stream().cuda_stream)

    assert call(vb.data_ptr(), rv.data_ptr(), 5) == 0
    for bad in ((None, rv.data_ptr(), 5), (vb.data_ptr(), None, 5), (vb.data_ptr(), rv.data_ptr(), 0), (vb.data_ptr(), rv.data_ptr(), 4)):
        assert call(*bad) == 2, bad      # STGCN_ERR_INVALID
    # the evaluation launch: wrong shape / dtype, and a state of the unmasked size
    st_small, _ = ops.eval_state(dev)
    st, _ = ops.eval_state(dev, masked=True)
    assert st.numel() == _lib.EVAL_MASKED_STATE_WORDS == 8 + 64 * 6
    with pytest.raises(ValueError, match="mask"):
        ops.eval_accumulate(pred, y, st, valid=ok[:2])
    with pytest.raises(ValueError, match="mask"):
        ops.eval_accumulate(pred, y, st, valid=ok.float())
    with pytest.raises(ValueError, match="392"):
        ops.eval_accumulate(pred, y, st_small, valid=ok)
    # the captured step's constructor, before anything touches the device
    x0, y0 = torch.zeros(2, 1), torch.zeros(2, 1)
    with pytest.raises(ValueError, match="needs the resident series"):
        train.GraphedTrainStep(None, None, x0, y0, valid=torch.ones(4, 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="chains > 1"):
        train.GraphedTrainStep(None, None, x0, y0, series=torch.zeros(4, 1), chains=2, valid=torch.ones(4, 1, dtype=torch.bool))
    assert set(ops._input_index) == bound, "refused calls leave no index binding behind"


def check_data_helpers():
    raw = np.array([[0.0, 3.0, np.nan], [5.0, 0.0, 7.0]])
    assert data.observed_mask(raw).tolist() == [[0, 1, 0], [1, 0, 1]] and data.observed_mask(raw).dtype == np.uint8
    assert data.observed_mask(raw, float("nan")).tolist() == [[1, 1, 0], [1, 1, 1]]
    assert data.observed_mask(raw, 3.0).tolist() == [[1, 0, 0], [1, 1, 1]]
    y, p, v = np.array([10.0, np.nan, 20.0, 40.0]), np.array([12.0, np.inf, 19.0, 44.0]), np.array([1, 0, 1, 1])
    mae, rmse, wmape, mape = data.masked_metrics_from_arrays(y, p, v)
    assert abs(mae - 7.0 / 3) < 1e-12 and abs(rmse - np.sqrt(21.0 / 3)) < 1e-12 and abs(wmape - 0.1) < 1e-12
    assert abs(mape - (0.2 + 0.05 + 0.1) / 3) < 1e-12
    assert data.masked_metrics_from_arrays(y[[0, 2, 3]], p[[0, 2, 3]], np.ones(3))[:3] == data.metrics_from_arrays(y[[0, 2, 3]], p[[0, 2, 3]])
