"""CPU emulator: the device-side evaluation metrics (``stgcn_eval_accumulate`` / ``stgcn_eval_arm``) against the reference's own recorded
numbers and a float64 numpy evaluation, in both reduction forms, and ``train.GraphedEvalPass(capture=False)`` against the host loop
(``data.evaluate_model`` / ``data.evaluate_metric``) it replaces."""
import math

import numpy as np
import pytest
import torch

from tests.emu_util import bind_emulator
from tests.helpers import load_fixture

BIG, SINGLE = "0", str(1 << 40)      # STGCN_EVAL_BIG: every batch takes the partial slabs / the single workgroup


def _numpy_sums(pred, y, scale, mean, first_valid=0):
    """float64 evaluation of one batch (the terms' definitions of script/utility.py:90-121)."""
    p, t = pred[first_valid:].astype(np.float64), y[first_valid:].astype(np.float64)
    sc = np.ones(p.shape[1]) if scale is None else scale.astype(np.float64)
    mu = np.zeros(p.shape[1]) if mean is None else mean.astype(np.float64)
    d = (t - p) * sc
    return np.array([((p - t) ** 2).sum(), np.abs(d).sum(), (d ** 2).sum(), (t * sc + mu).sum(), p.size]), np.abs(t * sc + mu).sum()


def _accumulate(batches, scale, mean, monkeypatch, knob=None):
    """``batches``: (pred, y, first_valid); returns the first five words of the state after all of them."""
    from stgcn_amd import ops
    if knob is None:
        monkeypatch.delenv("STGCN_EVAL_BIG", raising=False)
    else:
        monkeypatch.setenv("STGCN_EVAL_BIG", knob)
    state, _ = ops.eval_state("cpu")
    state.fill_(float("nan"))            # arm, not the allocation, is what zeroes the words a pass reads
    state[8:] = 7.0                      # (stale partial slabs must not matter)
    ops.eval_arm(state)
    sc = None if scale is None else torch.from_numpy(scale.astype(np.float32))
    mu = None if mean is None else torch.from_numpy(mean.astype(np.float32))
    for pred, y, fv in batches:
        ops.eval_accumulate(torch.from_numpy(pred).contiguous(), torch.from_numpy(y).contiguous(), state, sc, mu, first_valid=fv)
    return state[:5].numpy().copy(), state


def test_kernel_reproduces_the_reference_metrics_of_the_fixture(monkeypatch):
    """pred_test / y_test / z-score of pipeline_metr_la.npz are the reference's fp32 arrays bit for bit (48 windows at batch size 32: one
    full batch, then the batch that starts at window 16 and counts from its window 16 on).  MAE, RMSE, WMAPE within 1e-6 relative of the
    reference's: a term carries at most four fp32 roundings (<= 2.4e-7 relative), the sums of |d| and d^2 have non-negative terms and
    are carried in fp64, and the reference forms the three in float64 numpy.  The MSE is different: the reference's evaluate_model
    averages FLOAT32 per-batch losses (``l.item() * n``), so its recorded value carries fp32 summation error of its own -- the device MSE
    is held to 1e-6 relative of a float64 numpy evaluation of the same arrays and to the project's 1e-4 absolute of the recorded value."""
    from stgcn_amd import ops
    bind_emulator()
    fx = load_fixture("pipeline_metr_la")
    pred, y, bs = fx["pred_test"], fx["y_test"], int(fx["batch_size"])
    num, N = pred.shape
    assert (num, bs) == (48, 32)
    scale, mean = fx["zscore_scale"], fx["zscore_mean"]
    # the labels as rows of one resident buffer: batch k reads them at target + index * stride, index moved by the launch itself
    state, pos = ops.eval_state("cpu")
    ops.eval_arm(state, pos)
    target = torch.from_numpy(y).contiguous()
    sc, mu = torch.from_numpy(scale.astype(np.float32)), torch.from_numpy(mean.astype(np.float32))
    want_pos = [(0, 0), (16, 16)]
    for k in range(2):
        s, fv = int(pos[0]), int(pos[1])
        assert (s, fv) == want_pos[k]
        ops.eval_accumulate(torch.from_numpy(pred[s:s + bs]).contiguous(), target[:bs], state, sc, mu, pos=pos, num_windows=num)
    assert int(pos[2]) == 2
    m = ops.eval_metrics(state[:5].tolist())
    assert m["elements"] == num * N
    mse_ref, mae_ref, rmse_ref, wmape_ref = (float(v) for v in fx["metrics"])
    print("device", m, "reference", fx["metrics"])
    assert abs(m["mae"] - mae_ref) <= 1e-6 * mae_ref
    assert abs(m["rmse"] - rmse_ref) <= 1e-6 * rmse_ref
    assert abs(m["wmape"] - wmape_ref) <= 1e-6 * wmape_ref
    mse64 = float(((pred.astype(np.float64) - y.astype(np.float64)) ** 2).mean())
    assert abs(m["mse"] - mse64) <= 1e-6 * mse64
    assert abs(m["mse"] - mse_ref) <= 1e-4
    # the same two batches with explicit arguments instead of position words
    got, _ = _accumulate([(pred[:32], y[:32], 0), (pred[16:48], y[16:48], 16)], scale, mean, monkeypatch)
    assert np.array_equal(got, state[:5].numpy())


@pytest.mark.parametrize("knob", [SINGLE, BIG], ids=["single_workgroup", "partial_slabs"])
@pytest.mark.parametrize("first_valid", [0, 1, 31])
@pytest.mark.parametrize("scaler", ["none", "positive", "negative_means"])
def test_both_reduction_forms_match_float64_numpy_and_repeat_bitwise(knob, first_valid, scaler, monkeypatch):
    bind_emulator()
    rs = np.random.RandomState(17 + first_valid)
    B, N = 32, 207
    pred = rs.standard_normal((B, N)).astype(np.float32)
    y = rs.standard_normal((B, N)).astype(np.float32)
    scale = mean = None
    if scaler != "none":
        scale = rs.uniform(5.0, 25.0, N)
        mean = rs.uniform(40.0, 70.0, N) if scaler == "positive" else rs.uniform(-30.0, 10.0, N)   # mixed-sign labels after the inverse
    batches = [(pred, y, first_valid), (pred[::-1].copy(), y[::-1].copy(), 0)]
    got, state = _accumulate(batches, scale, mean, monkeypatch, knob)
    again, _ = _accumulate(batches, scale, mean, monkeypatch, knob)
    assert np.array_equal(got, again), "the summation order must not depend on the run"
    want, sum_abs_y = np.zeros(5), 0.0
    for p, t, fv in batches:
        w, a = _numpy_sums(p, t, None if scale is None else scale.astype(np.float32), None if mean is None else mean.astype(np.float32), fv)
        want += w
        sum_abs_y += a
    print(knob, first_valid, scaler, got, want)
    for i in range(3):
        assert abs(got[i] - want[i]) <= 1e-6 * want[i], i
    assert abs(got[3] - want[3]) <= 1e-6 * sum_abs_y
    assert got[4] == want[4] == (2 * B - first_valid) * N
    assert int(state[6:7].view(torch.int64).item()) == 0, "the ticket word is re-armed by the last arriver"


def test_forms_are_chosen_by_size_and_slabs_fold_in_index_order(monkeypatch):
    """Without the knob a 6 624-element batch is one workgroup and a 131 072-element batch (C5) takes 64; the two forms agree to
    fp64 rounding on the same data."""
    bind_emulator()
    rs = np.random.RandomState(5)
    B, N = 16, 8192
    pred, y = rs.standard_normal((B, N)).astype(np.float32), rs.standard_normal((B, N)).astype(np.float32)
    big, state = _accumulate([(pred, y, 3)], None, None, monkeypatch)
    assert not np.all(state[8:8 + 4 * 64].numpy() == 7.0), "a 131 072-element batch writes partial slabs"
    one, state1 = _accumulate([(pred, y, 3)], None, None, monkeypatch, SINGLE)
    assert np.all(state1[8:].numpy() == 7.0)
    small, state2 = _accumulate([(pred[:, :207].copy(), y[:, :207].copy(), 0)], None, None, monkeypatch)
    assert np.all(state2[8:].numpy() == 7.0), "a C2-sized batch is one workgroup"
    want, _ = _numpy_sums(pred, y, None, None, 3)
    for i in range(3):
        assert abs(big[i] - want[i]) <= 1e-6 * want[i] and abs(one[i] - big[i]) <= 1e-12 * want[i]
    assert big[4] == one[4] == 13 * N


def test_c_abi_refuses_bad_arguments():
    from stgcn_amd import _lib
    L = bind_emulator()
    d = L.dll
    state = torch.zeros(_lib.EVAL_STATE_WORDS, dtype=torch.float64)
    pos = torch.zeros(_lib.EVAL_POS_WORDS, dtype=torch.int64)
    p, t = torch.zeros(4, 5), torch.zeros(4, 5)
    sc = torch.ones(5)

    def call(pred=p.data_ptr(), target=t.data_ptr(), B=4, N=5, scale=None, mean=None, fv=0, pos_=None, stride=5, num=0, st=state.data_ptr()):
        return d.stgcn_eval_accumulate(pred, target, B, N, scale, mean, fv, pos_, stride, num, st, None)

    def refused(rc, text):
        assert rc == 2, rc                                       # STGCN_ERR_INVALID
        assert text in d.stgcn_last_error().decode(), d.stgcn_last_error().decode()

    assert call() == 0
    refused(call(st=None), "state is NULL")
    refused(d.stgcn_eval_arm(None, None, None), "state is NULL")
    refused(call(pred=None), "NULL pred / target")
    refused(call(B=0), "must be positive")
    refused(call(N=-1), "must be positive")
    refused(call(fv=-1), "first_valid=-1 outside [0, B=4)")
    refused(call(fv=4), "first_valid=4 outside [0, B=4)")
    refused(call(scale=sc.data_ptr()), "scale and mean come together")
    refused(call(pos_=pos.data_ptr(), num=3), "fewer than one batch")
    refused(call(pos_=pos.data_ptr(), num=8, fv=1), "first_valid is read from them")
    assert call(pos_=pos.data_ptr(), num=8) == 0 and pos.tolist()[:3] == [4, 0, 1]
    with pytest.raises(ValueError):
        from stgcn_amd import ops
        ops.eval_accumulate(p, t, state, first_valid=9)


# ------------------------------------------------------------------------------------------------ the pass
def _tiny(droprate=0.5, batch=False):
    from tests.optim_kinds_util import tiny_model
    bind_emulator()
    model, x, y = tiny_model("cpu", droprate=droprate)
    return (model, x, y) if batch else model


def _series(rows, N, seed):
    rs = np.random.RandomState(seed)
    raw = 55.0 + 12.0 * rs.standard_normal((rows, N)) + 6.0 * np.sin(np.arange(rows))[:, None]
    from stgcn_amd import data
    z = data.ZScore().fit(raw)
    return z.transform(raw).astype(np.float32), z


@pytest.mark.parametrize("num", [11, 12], ids=["ragged_tail", "whole_batches"])
def test_pass_equals_the_host_loop(num):
    """GraphedEvalPass(capture=False) against data.evaluate_model / evaluate_metric on WindowSampler.batches(B) of the same model, at the
    project's bars (1e-4 absolute; WMAPE 1e-5), with a window count that is / is not a multiple of the batch size."""
    from stgcn_amd import data
    from stgcn_amd.layers import DropoutStream
    from stgcn_amd.train import GraphedEvalPass, make_optimizer, train_step
    model, x1, y1 = _tiny(batch=True)
    n_his, n_pred, B, N = 12, 3, 4, 20
    zs, z = _series(num + n_his + n_pred, N, 3)
    sampler = data.WindowSampler(zs, n_his, n_pred, "cpu")
    assert len(sampler) == num
    opt = make_optimizer(model)
    model.train()
    # one real step at the pass's batch size: the dropout stream and the optimizer have positions to keep, the workspaces exist
    train_step(model, opt, torch.cat([x1, x1]), torch.cat([y1, y1]))
    offset_before, steps_before = DropoutStream._offset, opt.param_groups[0]["_step"]
    assert offset_before > 0 and steps_before == 1
    with GraphedEvalPass(model, zs, n_his, n_pred, B, scaler=z, capture=False) as ev:
        assert model.training, "the constructor restores the mode it found"
        got = ev.run()
        assert model.training
        assert ev.run() == got, "two passes return identical dicts"
        model.eval()
        assert ev.run() == got and not model.training
    assert DropoutStream._offset == offset_before and DropoutStream.counter is None, "an evaluation pass draws no dropout positions"
    assert opt.param_groups[0]["_step"] == steps_before and getattr(model, "_step_counters", None) is None
    mse = data.evaluate_model(model, torch.nn.MSELoss(), sampler.batches(B))
    mae, rmse, wmape = data.evaluate_metric(model, sampler.batches(B), z)
    print("pass", got, "host", (mse, mae, rmse, wmape))
    assert got["windows"] == len(sampler) == num
    assert abs(got["mse"] - mse) <= 1e-4 and abs(got["mae"] - mae) <= 1e-4 and abs(got["rmse"] - rmse) <= 1e-4
    assert abs(got["wmape"] - wmape) <= 1e-5
    assert all(isinstance(got[k], float) for k in ("mse", "mae", "rmse", "wmape")) and isinstance(got["windows"], int)


def test_pass_without_scaler_reports_z_scored_metrics_and_refuses_short_splits():
    from stgcn_amd import data
    from stgcn_amd.train import GraphedEvalPass
    model = _tiny()
    n_his, n_pred, B, N = 12, 3, 4, 20
    zs, _ = _series(6 + n_his + n_pred, N, 4)
    with GraphedEvalPass(model, torch.from_numpy(zs), n_his, n_pred, B, capture=False) as ev:
        got = ev.run()
    assert got["windows"] == 6 and abs(got["rmse"] - math.sqrt(got["mse"])) <= 1e-12
    sampler = data.WindowSampler(zs, n_his, n_pred, "cpu")
    assert abs(got["mse"] - data.evaluate_model(model, torch.nn.MSELoss(), sampler.batches(B))) <= 1e-4
    with pytest.raises(ValueError, match=r"3 windows.*batch of 4"):
        GraphedEvalPass(model, zs[:3 + n_his + n_pred], n_his, n_pred, B, capture=False)
    from stgcn_amd import ops
    assert not ops._input_index, "a refused or closed pass leaves no index binding behind"


def test_pass_refuses_to_grow_a_live_workspace():
    """A module whose workspace already exists (a captured training step would hold its address) must not see it reallocated: the pass
    raises before it moves anything, and names the module."""
    from stgcn_amd.train import GraphedEvalPass
    model = _tiny()
    n_his, n_pred, N = 12, 3, 20
    zs, _ = _series(40, N, 5)
    with GraphedEvalPass(model, zs, n_his, n_pred, 2, capture=False) as ev:      # workspaces now sized for batch size 2
        ev.run()
    ptrs = {n: m._ws.buf.data_ptr() for n, m in model.named_modules() if hasattr(m, "_ws")}
    with pytest.raises(RuntimeError, match=r"st_blocks\.0.*Build the evaluation pass before the training step"):
        GraphedEvalPass(model, zs, n_his, n_pred, 8, capture=False)
    assert ptrs == {n: m._ws.buf.data_ptr() for n, m in model.named_modules() if hasattr(m, "_ws")}, "nothing moved"
    with GraphedEvalPass(model, zs, n_his, n_pred, 2, capture=False) as ev:      # an equal batch size fits
        ev.run()
