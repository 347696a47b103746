"""Shuffled epochs on the CPU emulator: a device table of window starts (``ops.bind_input_index(..., table=...)``, ``x_window_dev`` /
``target_window_dev`` of the C ABI) places window b of a step at series row ``table[pos + b]``.  Only addresses change, so every
comparison with the same windows gathered into contiguous tensors is bitwise."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from stgcn_amd import _lib, models, ops
from stgcn_amd.train import GradArena, WindowOrder, fused_train_step, fwd_loss_bwd, make_optimizer, train_step
from tests.emu_util import bind_emulator, block_case, nonsym_gso, params_in_field_order
from tests.helpers import cfg_from_fixture, fixture_gso, fixture_params, load_fixture

N_PRED = 3
# non-monotonic, with a repeated entry (2) and the first window of the series (0)
TABLE = [7, 2, 2, 11, 0, 5, 9, 3, 12, 1, 6, 4, 10, 8]
POS, B = 2, 6          # the step reads TABLE[2:8] = [2, 11, 0, 5, 9, 3]


def _fixture_model(dtype=torch.float32):
    bind_emulator()
    fx = load_fixture("tiny_cheb_f32")
    cfg = cfg_from_fixture(fx)
    N = int(fx["n_vertex"])
    args = types.SimpleNamespace(Kt=cfg.Kt, Ks=cfg.Ks, act_func=cfg.act_func, graph_conv_type=cfg.graph_conv_type,
                                 gso=torch.from_numpy(fixture_gso("tiny_cheb_f32", fx)), enable_bias=True, droprate=cfg.droprate, n_his=cfg.n_his)
    m = models.STGCNChebGraphConv(args, cfg.blocks, N)
    m.load_state_dict(fixture_params(fx, cfg, torch.float32), strict=True)
    m.set_compute_dtype(dtype)
    m.train()
    return m, cfg.n_his, N


def _random_model(N, n_his=12):
    """The fixture's architecture on another graph size (random parameters: the comparison is gathered vs materialised, not vs a golden)."""
    bind_emulator()
    torch.manual_seed(11)
    args = types.SimpleNamespace(Kt=3, Ks=3, act_func="glu", graph_conv_type="cheb_graph_conv", gso=torch.from_numpy(nonsym_gso(N, 4)),
                                 enable_bias=True, droprate=0.0, n_his=n_his)
    m = models.STGCNChebGraphConv(args, [[1], [64, 16, 64], [64, 16, 64], [128, 128], [1]], N)
    m.train()
    return m, n_his, N


def _series(rows, N, seed=9):
    return torch.randn(rows, N, generator=torch.Generator().manual_seed(seed))


def _gather(series, series_x, starts, n_his):
    """The windows of ``starts`` materialised the reference's way (script/dataloader.py:32-47): (B, 1, n_his, N) inputs, (B, N) labels."""
    x = torch.stack([series_x[s:s + n_his] for s in starts]).unsqueeze(1).contiguous()
    y = torch.stack([series[s + n_his + N_PRED - 1] for s in starts]).contiguous()
    return x, y


def _views(series, series_x, n_his, N, batch=B):
    xv = torch.as_strided(series_x, (batch, 1, n_his, N), (N, n_his * N, N, 1))
    yv = series[n_his + N_PRED - 1:n_his + N_PRED - 1 + batch]
    return xv, yv


def _grads(model):
    return [None if p.grad is None else p.grad.clone() for p in model.parameters()]


def _assert_same(ref, got):
    (l_ref, g_ref), (l_got, g_got) = ref, got
    assert float(l_ref) == float(l_got)
    for r, g in zip(g_ref, g_got):
        assert (r is None) == (g is None)
        if r is not None:
            assert torch.equal(r, g)


def _run(model, x, y):
    model.zero_grad(set_to_none=True)
    loss = fwd_loss_bwd(model, x, y)
    return loss, _grads(model)


def _run_bound(model, xv, yv, idx, stride, table):
    ops.bind_input_index(xv, idx, stride, table=table)
    ops.bind_input_index(yv, idx, stride, table=table)
    try:
        return _run(model, xv, yv)
    finally:
        ops.unbind_input_index(xv)
        ops.unbind_input_index(yv)


@pytest.mark.parametrize("case", ["f32", "bf16", "straddle"])
def test_gathered_windows_equal_materialised_tensor(case):
    """A non-monotonic table with a repeated entry, read at a position that is not 0, against the same windows stacked into contiguous
    tensors: loss and every gradient bitwise.  f32 / bf16: the tiny_cheb_f32 model (N = 20: a window is 10 x 20 = 200 output rows of the
    thin first layer, 12.5 of its 16-row tiles, so tiles straddle two unrelated windows already).  straddle: N = 21, where n_his * N = 252
    is no multiple of 16 either (and 10 x 21 = 210 rows per window)."""
    if case == "straddle":
        model, n_his, N = _random_model(21)
    else:
        model, n_his, N = _fixture_model(torch.bfloat16 if case == "bf16" else torch.float32)
    assert case != "straddle" or (n_his * N) % 16 != 0
    assert ((n_his - 2) * N) % 16 != 0
    series = _series(max(TABLE) + n_his + N_PRED + 2, N)
    series_x = series.to(torch.bfloat16) if case == "bf16" else series      # (both sides round the fp32 series to bf16 once)
    ref = _run(model, *_gather(series, series_x, TABLE[POS:POS + B], n_his))
    table = torch.tensor(TABLE, dtype=torch.int64)
    idx = torch.tensor([POS], dtype=torch.int64)
    got = _run_bound(model, *_views(series, series_x, n_his, N), idx, N, table)
    _assert_same(ref, got)


def test_identity_table_equals_index_mode():
    model, n_his, N = _fixture_model()
    series = _series(POS + B + n_his + N_PRED + 4, N)
    xv, yv = _views(series, series, n_his, N)
    idx = torch.tensor([POS], dtype=torch.int64)
    ref = _run_bound(model, xv, yv, idx, N, None)
    got = _run_bound(model, xv, yv, idx, N, torch.arange(POS + B + 2, dtype=torch.int64))
    _assert_same(ref, got)


def test_standalone_loss_reads_labels_through_the_table():
    """``mse_loss_and_grad`` (stgcn_mse_loss_grad_windows) with a table equals the same call on the gathered label rows."""
    bind_emulator()
    n_his, N = 12, 20
    series = _series(max(TABLE) + n_his + N_PRED + 2, N)
    pred = torch.randn(B, N, generator=torch.Generator().manual_seed(1))
    _, y = _gather(series, series, TABLE[POS:POS + B], n_his)
    l_ref, d_ref = ops.mse_loss_and_grad(pred, y)
    _, yv = _views(series, series, n_his, N)
    ops.bind_input_index(yv, torch.tensor([POS], dtype=torch.int64), N, table=torch.tensor(TABLE, dtype=torch.int64))
    try:
        l_got, d_got = ops.mse_loss_and_grad(pred, yv)
    finally:
        ops.unbind_input_index(yv)
    assert float(l_ref) == float(l_got) and torch.equal(d_ref, d_got)


def test_general_first_layer_reads_a_multi_feature_series_through_the_table():
    """One STConvBlock with c_in = 4 (K = Kt * c_in = 12: the row-tile kernels, not the thin layer) on a strided view of a resident
    (time, N, 4) series: forward output and every parameter gradient bitwise those of the materialised (B, 4, T, N) tensor."""
    bind_emulator()
    c_in, channels, Kt, Ks, N, T = 4, (64, 16, 64), 3, 3, 21, 8
    cfg, p = block_case(c_in, channels, Kt, Ks, "cheb_graph_conv", "glu", N, B, T)
    bcfg = ops.BlockConfig(Kt=Kt, Ks=Ks, n_vertex=N, c_in=c_in, channels=channels, act_func="glu", graph_conv_type="cheb_graph_conv", droprate=0.0)
    gp, gt = ops.gso_prepare(torch.from_numpy(nonsym_gso(N, 2)), ops.graph_terms(bcfg))
    g = torch.Generator().manual_seed(3)
    series = torch.randn(max(TABLE) + T + 2, N, c_in, generator=g)
    dy = torch.randn(B, channels[2], T - 2 * (Kt - 1), N, generator=g)

    def run(x):
        params = [None if t is None else t.clone().requires_grad_(True) for t in params_in_field_order(p, "st_blocks.0.", "cheb_graph_conv")]
        y = ops.st_conv_block(x, gp, gt, bcfg, params, True, 1, 0, ops.WorkspaceCache())
        y.backward(dy)
        return y.detach().clone(), [None if t is None or t.grad is None else t.grad.clone() for t in params]

    starts = TABLE[POS:POS + B]
    x_mat = torch.stack([series[s:s + T] for s in starts]).permute(0, 3, 1, 2)      # logical (B, c_in, T, N), channels-last storage
    y_ref, g_ref = run(x_mat)
    xv = torch.as_strided(series, (B, c_in, T, N), (N * c_in, 1, N * c_in, c_in))     # window b = rows [b, b + T) of the series
    assert ops.window_strided_rows(xv.permute(0, 2, 3, 1)) == N
    ops.bind_input_index(xv, torch.tensor([POS], dtype=torch.int64), N * c_in, table=torch.tensor(TABLE, dtype=torch.int64))
    try:
        y_got, g_got = run(xv)
    finally:
        ops.unbind_input_index(xv)
    assert torch.equal(y_ref, y_got)
    assert any(r is not None for r in g_ref)
    for r, q in zip(g_ref, g_got):
        assert (r is None) == (q is None) and (r is None or torch.equal(r, q))


def test_eager_fused_steps_walk_the_table_across_a_wrap_and_a_new_order():
    """``fused_train_step`` with the position word on the model's weight-pack launch (the launch fused with the thin first layer forms
    (old + inc) % mod itself): two "epochs" of three minibatches with ``set_order`` in between and one step past the second wrap train
    to bitwise the parameters of the same sequence fed as explicit gathered batches."""
    num, batch = 17, 5
    usable = num // batch * batch
    results = []
    for mode in ("table", "explicit"):
        model, n_his, N = _fixture_model()
        series = _series(num + n_his + N_PRED, N)
        opt = make_optimizer(model, lr=1e-2, weight_decay=1e-2)
        order = WindowOrder(num, usable, "cpu", seed=4)
        order.reshuffle()
        first = order.order.tolist()
        assert sorted(first) != first and len(set(first)) == usable and max(first) <= num - 1
        second = [16, 3, 3, 0, 9, 14, 1, 7, 12, 5, 2, 11, 8, 6, 10]      # any table: a repeat, the last window of the series
        seq = [first[k * batch:(k + 1) * batch] for k in range(3)] + [second[k * batch:(k + 1) * batch] for k in (0, 1, 2, 0)]
        train_step(model, opt, *_gather(series, series, seq[0], n_his))      # plain step: shows which parameters are live
        arena = GradArena([q for q in model.parameters() if q.grad is not None])
        losses = []
        if mode == "explicit":
            for starts in seq[1:]:
                losses.append(float(fused_train_step(model, opt, *_gather(series, series, starts, n_his), arena)))
        else:
            xv, yv = _views(series, series, n_his, N, batch)
            idx = torch.tensor([0], dtype=torch.int64)      # the pack launch advances BEFORE the step: the next one reads position `batch`
            model._step_counters = [(idx, batch, usable)]
            ops.bind_input_index(xv, idx, N, table=order.order)
            ops.bind_input_index(yv, idx, N, table=order.order)
            try:
                for k in range(1, len(seq)):
                    if k == 3:
                        assert int(idx) == 2 * batch      # the epoch is over: the next bump wraps to 0
                        order.set_order(second)
                    losses.append(float(fused_train_step(model, opt, xv, yv, arena)))
                assert int(idx) == 0
            finally:
                ops.unbind_input_index(xv)
                ops.unbind_input_index(yv)
                model._step_counters = None
        results.append((losses, {k: v.clone() for k, v in model.state_dict().items()}))
    (l_tab, sd_tab), (l_exp, sd_exp) = results
    assert l_tab == l_exp, (l_tab, l_exp)
    for k in sd_tab:
        assert torch.equal(sd_tab[k], sd_exp[k]), k


def test_set_order_validates_on_the_host():
    order = WindowOrder(17, 15, "cpu", seed=0)
    before = order.order.clone()
    ptr = order.order.data_ptr()
    good = list(range(15))
    for bad in (good[:-1], good + [0], torch.tensor(good, dtype=torch.int32), np.asarray(good, dtype=np.float64),
                [-1] + good[1:], good[:-1] + [17]):
        with pytest.raises(ValueError):
            order.set_order(bad)
        assert torch.equal(order.order, before)          # nothing was uploaded
    order.set_order(good[:-1] + [16])                    # num - 1 is the last window
    order.set_order(np.asarray(good[::-1], dtype=np.int64))
    order.set_order(torch.tensor(good, dtype=torch.int64))
    assert order.order.data_ptr() == ptr                 # written in place: a captured graph holds this address
    a = WindowOrder(17, 15, "cpu", seed=3)
    b = WindowOrder(17, 15, "cpu", seed=3)
    a.reshuffle(), b.reshuffle()
    assert torch.equal(a.order, b.order)                 # same seed, same table (data-parallel ranks draw it independently)
    e1 = a.order.clone()
    a.reshuffle()
    assert not torch.equal(e1, a.order) and sorted(set(a.order.tolist())) == sorted(a.order.tolist())


def test_c_abi_refuses_a_table_without_index_or_with_input_gradient():
    L = bind_emulator()
    bcfg = ops.BlockConfig(Kt=3, Ks=3, n_vertex=20, c_in=1, channels=(64, 16, 64), act_func="glu", graph_conv_type="cheb_graph_conv", droprate=0.0)
    idx = torch.zeros(1, dtype=torch.int64)
    tab = torch.arange(8, dtype=torch.int64)
    plan = _lib.StblockPlan()

    def query(**kw):
        need_dx = kw.pop("need_dx", False)
        d = ops.make_desc(bcfg, 2, 12, True, need_dx, **kw)
        return L.dll.stgcn_stblock_plan_query(C.byref(d), C.byref(plan))

    assert query(x_index=idx.data_ptr(), x_index_stride=20, x_window=tab.data_ptr()) == _lib.STGCN_OK
    assert query(x_window=tab.data_ptr(), x_index_stride=20) == 2            # STGCN_ERR_INVALID: no x_index_dev
    assert "x_window_dev" in L.dll.stgcn_last_error().decode()
    assert query(x_index=idx.data_ptr(), x_index_stride=20, x_window=tab.data_ptr(), need_dx=True) == 2
    assert "x_window_dev" in L.dll.stgcn_last_error().decode()
    assert query(x_index=idx.data_ptr(), x_index_stride=0, x_window=tab.data_ptr()) == 2      # windows must start on whole rows
    # the stand-alone loss: a table needs the position word
    pred, y, loss, dpred = torch.zeros(4, 20), torch.zeros(4, 20), torch.zeros(1), torch.zeros(4, 20)
    rc = L.dll.stgcn_mse_loss_grad_windows(pred.data_ptr(), y.data_ptr(), 80, 1.0, loss.data_ptr(), dpred.data_ptr(), None, 20, tab.data_ptr(), 20, None)
    assert rc == 2 and "target_window_dev" in L.dll.stgcn_last_error().decode()
