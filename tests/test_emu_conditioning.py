"""The ST block's kernels on ill-conditioned inputs, on the CPU emulator: every row of tests/conditioning_util.py under every condition, each
key relative to its own stage and at most R = 16 times what the float32 stage oracle loses on the same inputs; the rows with two product
forms under both; every block row once as production launches it; the non-finite contract; and tanh_f on its own against float64.
tests/test_gpu_conditioning.py runs the same table on the MI355X (the hardware's v_exp_f32 / v_rcp_f32 and MFMA summation order)."""
import ctypes as C

import numpy as np
import pytest

from tests import conditioning_util as cu
from tests.block_util import bind

DEV = "cpu"


@pytest.mark.parametrize("cond", list(cu.CONDITIONS))
@pytest.mark.parametrize("row,x6", cu.RUNS, ids=cu.RUN_IDS)
def test_condition(row, x6, cond):
    bind(DEV)
    err = cu.run_condition(DEV, row, cond, x6=x6)
    print(row, x6, cond, "worst ratio %.2f at %s" % cu.worst_ratio(err), err)
    cu.report(err, row, cond, x6, "debug", "emu")
    assert "fwd.y" in err and "oracle32.fwd.G" in err and "oracle32.bwd.dA" in err and "kink.window_over_bar" in err
    cu.assert_condition(err, f"{row} {cond} x6={x6}")


@pytest.mark.parametrize("cond", cu.PROD_CONDITIONS)
@pytest.mark.parametrize("row", list(cu.ROWS))
def test_condition_as_production_launches_it(row, cond):
    """debug_stages off, the partial arena poisoned with NaN between forward and backward: the fused backward kernels see the condition."""
    bind(DEV)
    err = cu.run_condition(DEV, row, cond, debug_stages=False)
    print(row, cond, "prod: worst ratio %.2f at %s" % cu.worst_ratio(err), err)
    cu.report(err, row, cond, None, "prod", "emu")
    cu.assert_condition(err, f"{row} {cond} production")


@pytest.mark.parametrize("cond", list(cu.CONDITIONS))
def test_sparse_operator_condition(cond):
    bind(DEV)
    err = cu.run_sparse_condition(DEV, cond)
    print("sparse", cond, "worst ratio %.2f at %s" % cu.worst_ratio(err), err)
    cu.report(err, "sparse-" + cu.SPARSE_ROW, cond, None, "debug", "emu")
    cu.assert_condition(err, f"sparse {cond}")


@pytest.mark.parametrize("cond", ["small-10", "small-14", "small-40", "small-60"])
def test_relative_kink_window_holds_tens_of_units(cond):
    """Under small-* every pre-activation is below the absolute window FWD_TOL: it would hold every unit, and the backward oracle would
    take the library's ReLU side for all of them.  The relative window holds what it holds at unit scale."""
    from tests.block_util import BlockOracle
    held = {}
    for relative in (True, False):      # (oracles of their own: the window depends on the pre-activations alone, not on the dropout mask)
        O = BlockOracle(*cu.ROWS["kipfgtu"][:9], kink_rel=relative, oracle32=False)
        cu.CONDITIONS[cond](O)
        O.forward(None)
        held[relative] = int(O.kink.sum())
        if relative:
            assert held[True] <= O.window_bar < 100, (held, O.window_bar)
    assert held[False] > (100 if cond == "small-10" else 1000), held      # the absolute window: hundreds at 2^-10, then nearly all 1680


# ------------------------------------------------------------------------------------------------------------------------- tanh_f
def probe():
    from tests.emu.build_emu import build_probe
    dll = C.CDLL(build_probe())
    fp = np.ctypeslib.ndpointer(np.float32, flags="C")
    dll.probe_tanh.argtypes = [fp, fp, C.c_int]
    dll.probe_relu.argtypes = [fp, fp, C.c_int]
    dll.probe_gate_bwd.argtypes = [fp, fp, fp, C.c_int, fp, fp, C.c_int]
    return dll


def sweep_points():
    x = np.exp(np.linspace(np.log(2.0 ** -40), np.log(16.0), 1_000_001)).astype(np.float32)
    edge = np.float32(0.625)      # where tanh_f changes form
    x = np.concatenate([x, [np.nextafter(edge, np.float32(0)), edge, np.nextafter(edge, np.float32(1))], 2.0 ** np.arange(-40, 5, dtype=np.float32)])
    return np.concatenate([x, -x]).astype(np.float32)


def test_tanh_relative_error():
    """4 ulp = 4 * 2^-24 relative, from the two 1-ulp instructions tanh_f is built on, over 2^-40 <= |x| <= 16 (2 000 000 points, both
    signs, the crossover and its neighbours).  The former 2 sigmoid(2x) - 1 had an absolute error of 2^-24: relative 7e-4 at 2^-14."""
    dll = probe()
    x = sweep_points()
    t = np.empty_like(x)
    dll.probe_tanh(x, t, x.size)
    ref = np.tanh(x.astype(np.float64))
    e = np.abs(t.astype(np.float64) - ref) / np.abs(ref)
    i = int(e.argmax())
    print("tanh_f: max relative error %.3g (%.2f x 2^-24) at x = %r" % (e[i], e[i] / 2.0 ** -24, float(x[i])))
    assert e[i] <= 4 * 2.0 ** -24
    assert np.array_equal(np.signbit(t), np.signbit(x)) and np.all(np.abs(t) <= 1)
    sp = np.array([np.nan, np.inf, -np.inf, 0.0, 100.0, -100.0], np.float32)
    o = np.empty_like(sp)
    dll.probe_tanh(sp, o, sp.size)
    assert np.isnan(o[0]) and np.array_equal(o[1:], np.array([1, -1, 0, 1, -1], np.float32))


def test_gate_bwd_gtu_forms_its_derivative_from_the_same_tanh():
    """du = dh s (1 - t^2) and dq = dh t s (1 - s) with t = tanh_f(u), the value the forward gated with: against float64 within the 4 ulp of
    t and the roundings of the products (8 * 2^-24 of the result), at |u| from 2^-40 up to where 1 - t^2 is still a normal number."""
    dll = probe()
    rs = np.random.RandomState(4)
    n = 200_000
    u = (np.exp(rs.uniform(np.log(2.0 ** -40), np.log(8.0), n)) * rs.choice([-1.0, 1.0], n)).astype(np.float32)
    dh = rs.standard_normal(n).astype(np.float32)
    s = rs.uniform(0.01, 0.99, n).astype(np.float32)
    du, dq, t = np.empty_like(u), np.empty_like(u), np.empty_like(u)
    dll.probe_gate_bwd(dh, u, s, 1, du, dq, n)
    dll.probe_tanh(u, t, n)
    t64, dh64, s64 = t.astype(np.float64), dh.astype(np.float64), s.astype(np.float64)
    # (1) the same t: the factors are fp32 roundings of exact functions of the probe's own t
    d = (1.0 - t64 * t64).astype(np.float32)      # one rounding: the fma
    assert np.array_equal(du, (dh * s) * d)
    # (2) against float64 tanh
    th = np.tanh(u.astype(np.float64))
    ref_du, ref_dq = dh64 * s64 * (1 - th * th), dh64 * th * s64 * (1 - s64)
    # 1 - t^2 amplifies t's relative error by 2 t^2 / (1 - t^2)
    amp = 1 + 2 * th * th / (1 - th * th)
    assert np.all(np.abs(du - ref_du) <= 8 * 2.0 ** -24 * amp * np.abs(ref_du))
    assert np.all(np.abs(dq - ref_dq) <= 8 * 2.0 ** -24 * np.abs(ref_dq))


def test_relu_hands_nan_on():
    dll = probe()
    x = np.array([np.nan, -np.inf, np.inf, -1.0, -0.0, 0.0, 2.5], np.float32)
    y = np.empty_like(x)
    dll.probe_relu(x, y, x.size)
    assert np.isnan(y[0]) and np.array_equal(y[1:], np.array([0, np.inf, 0, 0, 0, 2.5], np.float32))


# --------------------------------------------------------------------------------------------------------------- non-finite inputs
@pytest.mark.parametrize("what", list(cu.NONFINITE))
@pytest.mark.parametrize("row,x6", cu.NF_RUNS, ids=cu.NF_IDS)
def test_nonfinite_input(row, x6, what):
    bind(DEV)
    cu.assert_nonfinite(cu.run_nonfinite(DEV, row, what, x6=x6), row, what, x6)


@pytest.mark.parametrize("what", ["nan", "inf"])
@pytest.mark.parametrize("row", list(cu.HEAD_ROWS))
def test_head_hands_nonfinite_input_on(row, what):
    """The same contract for the output head's two forward forms, whose ReLU sits behind the LayerNorm that spreads the element over the
    item: every prediction of item 0 non-finite, item 1 bitwise that of the clean run."""
    got = cu.run_head_nonfinite(DEV, row, what)
    assert ("head.fc_fwd@0" if row == "fc_fwd" else "head.fwd@0") in got["kernels"], got      # the form the row is in the table for
    assert got["clean_nonfinite"] == 0 and got["chain_words"] == 0 and got["other_item_differs"] == 0, got
    assert got["oracle_nonfinite"] > 0 and got["finite_where_oracle_is_not"] == 0, got
