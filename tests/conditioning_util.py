"""Ill-conditioned inputs for the ST block's kernels, shared by tests/test_emu_conditioning.py and tests/test_gpu_conditioning.py.

Every other numerical test of the suite draws x ~ N(0, 1) beside default-init parameters and holds the forward to an ABSOLUTE 1e-4.  Here
the same harness (tests/block_util.py: BlockOracle, run_block_case) runs a block under a CONDITION -- a transformation of a fresh
BlockOracle's inputs, applied before its first forward -- and every key is measured relative to its own stage and set against what fp32
rounding alone does on the same inputs: the stage oracle run in np.float32 against its float64 run (the oracle32.* idea).

Conditions (the names are the test ids):
  x2^-40, x2^3, x2^6        x *= 2^k (at 2^6 the gates saturate)
  off20                     x += 20
  n0x100, nlastx100         node 0 / the last node (the ragged 16-node tile) times 100: an outlying row for both LayerNorm statistic forms
                            (n0x10, the 600-node row only: times 10, see BIG_CONDITIONS)
  small-10 .. small-60      x and every bias outside the LayerNorm times 2^-k: every stage up to the LayerNorm scales by 2^-k
  dead0                     node 0 constant over time (a failed detector)

Metrics:
  fwd.U1, S1, A, X<k>, G, U2, S2     max |err| / max |float64 stage|, with no clamp at 1
  fwd.mean                           max |err| * rstd (in units of the slab's standard deviation);  fwd.rstd_rel: relative
  fwd.y, slice.y.tail                absolute: y is normalised
  bwd.*, grad.*, slice.*             max |err| / max |ref| as tests/block_util.py forms them (kink window: FWD_TOL of the largest pre-activation)
  oracle32.<key>                     the same metric of the float32 stage oracle: every key above has this twin

Criterion, the same for every key k, on the emulator and on the GPU:
      err_k <= max(R * oracle32.err_k, floor_k)          and      err_k <= GRAD_TOL for bwd.*, grad.* and slice.* keys (the project's bar)
  R = 16 is fixed from the reference side: the healthy block kernels measured at most 7.3 on the emulator when it was set (8.9 with the
  sparse row, 5.4 on the MI355X: profiles/conditioning_errors.md), and a factor of two covers what the emulator cannot show (1-ulp
  v_exp_f32 / v_rcp_f32, the MFMA summation order); the defect this harness was written against (tanh as 2 sigmoid(2x) - 1) sat at 126
  and above.  A healthy kernel over R is a finding to explain there, not a reason to raise R.  floor_k = 1e-5 (1 % of GRAD_TOL) for gradient keys, FWD_TOL / 10 for forward keys: below it
  ratios are rounding noise.  All other keys (chain words, bitwise counts, kink.*) keep the bars of tests/block_util.py.
Cap, a condition on the INPUTS: a (row, condition) pair is in the table only if the float32 oracle alone stays within ORACLE32_TOL on every
  gradient key and within FWD_TOL on every forward key -- asserted per run, so that no effective bar exceeds 16 times those values and a
  later seed change cannot pass by making the reference bad.

Non-finite inputs (run_nonfinite): the contract of DESIGN.md section 5.
"""
import ctypes as C
import json
import os

import numpy as np
import torch

from stgcn_amd import _lib, ops
from tests import sparse_gc_util as sg
from tests.block_util import FWD_TOL, GRAD_TOL, ORACLE32_TOL, BlockOracle, bar, bind, cl, rel, run_block_case, slice_metrics
from tests.emu_util import big_gso, params_in_field_order

R = 16.0
FLOOR_GRAD = 1e-5
FLOOR_FWD = FWD_TOL / 10
CHEB, KIPF = "cheb_graph_conv", "graph_conv"

# row: (c_in, channels, Kt, Ks, graph conv, act, N, B, T, training)
ROWS = {
    "t64glu": (64, (64, 16, 64), 3, 3, CHEB, "glu", 21, 2, 7, True),       # time-stepping kernels, default product form
    "r128glu": (16, (64, 16, 128), 3, 3, CHEB, "glu", 21, 2, 7, False),    # row-tile conv + ln_norm with slab_stats_from_rows
    "thin1": (1, (64, 16, 64), 3, 3, CHEB, "glu", 21, 2, 7, True),         # thin first layer
    "t64gtu": (64, (64, 16, 64), 3, 3, CHEB, "gtu", 21, 2, 7, True),       # as t64glu, GTU
    "kipfgtu": (64, (64, 16, 64), 3, 1, KIPF, "gtu", 35, 1, 5, True),
}
BIG_ROW = (64, (64, 16, 64), 3, 3, CHEB, "glu", 600, 1, 5, True)           # GPU only: tiled graph conv, a 600-row slab_stats_from_rows
X6_ROWS = ("t64glu", "t64gtu")                                              # also run with STGCN_MFMA_X6=0 (the fp32-MFMA form)
SPARSE_ROW = "n21"                                                          # tests/sparse_gc_util.py CASES
PROD_CONDITIONS = ("n0x100", "small-14")                                    # every block row once as production launches it
RUNS = [(row, None) for row in ROWS] + [(row, "0") for row in X6_ROWS]      # (row, STGCN_MFMA_X6): None = default
RUN_IDS = [row + ("" if x6 is None else "-x6=" + x6) for row, x6 in RUNS]
# the 600-node row: its outlying first row is 10 times the others, not 100 -- under n0x100 the float32 oracle ALONE is at 1.7e-4 on y (the
# outlying node's normalised values reach 70 where 600 nodes share one LayerNorm slab), outside the cap; at 10 they reach 28 and it holds 7e-5
BIG_CONDITIONS = ("n0x10", "dead0")
NF_RUNS = [("t64glu", None), ("t64glu", "0"), ("r128glu", None), ("r128glu", "0")]
NF_IDS = [row + ("" if x6 is None else "-x6=" + x6) for row, x6 in NF_RUNS]


def _scale_x(k):
    def f(O):
        O.x_np *= np.float32(2.0 ** k)
    return f


def _offset(O):
    O.x_np += np.float32(20.0)


def _node(idx, factor=100.0):
    def f(O):
        O.x_np[..., idx] *= np.float32(factor)
    return f


def _small(k):
    def f(O):
        O.x_np *= np.float32(2.0 ** k)
        for name in list(O.p):
            if name.endswith(".bias") and "tc2_ln" not in name:
                O.p[name] = O.p[name] * (2.0 ** k)
    return f


def _dead0(O):
    O.x_np[:, :, :, 0] = O.x_np[:, :, :1, 0]


CONDITIONS = {"x2^-40": _scale_x(-40), "x2^3": _scale_x(3), "x2^6": _scale_x(6), "off20": _offset, "n0x100": _node(0), "nlastx100": _node(-1),
              "small-10": _small(-10), "small-14": _small(-14), "small-40": _small(-40), "small-60": _small(-60), "dead0": _dead0}
BIG_ONLY = {"n0x10": _node(0, 10.0)}      # (not a condition of the table's other rows)

_oracles = {}


def oracle(row, cond):
    """The BlockOracle of (row, condition), made once and shared by the runs of the pair (both product forms, the production run).
    row: a key of ROWS, "big", or "sparse"."""
    if (row, cond) not in _oracles:
        if row == "sparse":
            dense, _ = sg.case_operator(SPARSE_ROW)
            O = BlockOracle(*sg.CASES[SPARSE_ROW][:9], gso=dense, kink_rel=True)
        elif row == "big":
            O = BlockOracle(*BIG_ROW[:9], gso=big_gso(BIG_ROW[6], 5), kink_rel=True)
        else:
            O = BlockOracle(*ROWS[row][:9], kink_rel=True)
        if cond is not None:
            (CONDITIONS.get(cond) or BIG_ONLY[cond])(O)
        _oracles[(row, cond)] = O
    return _oracles[(row, cond)]


class x6_env:
    """STGCN_MFMA_X6 for the calls inside (the library reads it per call): None = default (on), "0" = fp32 MFMAs."""

    def __init__(self, x6):
        self.x6 = x6

    def __enter__(self):
        self.prev = os.environ.get("STGCN_MFMA_X6")
        if self.x6 is None:
            os.environ.pop("STGCN_MFMA_X6", None)
        else:
            os.environ["STGCN_MFMA_X6"] = self.x6

    def __exit__(self, *exc):
        if self.prev is None:
            os.environ.pop("STGCN_MFMA_X6", None)
        else:
            os.environ["STGCN_MFMA_X6"] = self.prev


def is_forward(key):
    return key.startswith("fwd.") or key == "slice.y.tail"


def is_measured(key):
    """Keys under the criterion (all others keep tests/block_util.py's bar)."""
    return key.startswith(("fwd.", "bwd.", "grad.", "slice.")) and not key.endswith("bitwise")


def forward_metrics(got, sv, y, y_ref, prefix=""):
    """got: {stage: array} as the library (or the float32 oracle) holds them; sv / y_ref: the float64 oracle's."""
    err = {}
    for name, a in got.items():
        if name == "mean":
            err[prefix + "fwd.mean"] = float((np.abs(a.astype(np.float64) - sv["mean"]) * sv["rstd"]).max())
        elif name == "rstd":
            err[prefix + "fwd.rstd_rel"] = float(np.abs(a.astype(np.float64) / sv["rstd"] - 1).max())
        else:
            ref = sv["Xs"][int(name[1:])] if name.startswith("X") else sv[name]
            err[prefix + "fwd." + name] = float(np.abs(a.astype(np.float64) - ref).max() / np.abs(ref).max())
    err[prefix + "fwd.y"] = float(np.abs(y.astype(np.float64) - y_ref).max())
    return err


def oracle32_stages(O, names):
    sv32 = O.fwd[np.float32][2]
    return {n: (sv32["Xs"][int(n[1:])] if n.startswith("X") else sv32[n]) for n in names}


def backward_stage_twins(O, G_lib, names):
    """oracle32.bwd.<stage> for the materialised intermediate gradients (tests/block_util.py compares them with the float64 oracle only)."""
    side = (G_lib > 0) & O.kink
    _, _, st64, _, _, st32 = O.bwd[side.tobytes()]
    return {"oracle32.bwd." + n: rel(st32[n], st64[n]) for n in names}


def run_condition(dev, row, cond, x6=None, debug_stages=True):
    """One (row, condition) run: {key: error}, the forward keys relative, every measured key with its oracle32 twin."""
    O = oracle(row, cond)
    case = BIG_ROW if row == "big" else ROWS[row]
    got = {}
    outs = {}
    with x6_env(x6):
        err = run_block_case(dev, *case, oracle=O, debug_stages=debug_stages, stages_out=got, outputs=outs)
    _, y_ref, sv = O.fwd[np.float64]
    err = {k: v for k, v in err.items() if not (k.startswith("fwd.") and not k.endswith("bitwise")) and not k.startswith("oracle32.fwd.")}
    err.update(forward_metrics(got, sv, outs["y"], y_ref))
    err.update(forward_metrics(oracle32_stages(O, [n for n in got if n not in ("mean", "rstd")]) | {"mean": O.fwd[np.float32][2]["mean"],
                                                                                                   "rstd": O.fwd[np.float32][2]["rstd"]},
                               sv, O.fwd[np.float32][1], y_ref, prefix="oracle32."))
    err.update(backward_stage_twins(O, got["G"], [k[4:] for k in err if k.startswith("bwd.") and k != "bwd.dx"]))
    return err


def run_sparse_condition(dev, cond):
    """The sparse-operator row (tests/sparse_gc_util.py n21) under a condition: the stages its runner reads back, same metrics."""
    O = oracle("sparse", cond)
    c_in, channels, Kt, Ks, gct, act, N, B, T = O.args
    _, out = sg.run_case(dev, SPARSE_ROW, sparse=True, oracle=O)
    _, y_ref, sv = O.fwd[np.float64]
    G_lib = out["G"].astype(np.float32)
    dx_ref, g_ref, stages, dx32, g32, info = O.backward(G_lib)
    names = ["A", "G"] + [k for k in out if k.startswith("X")]
    err = dict(info)
    err.update(forward_metrics({n: out[n] for n in names}, sv, out["y"], y_ref))
    err.update(forward_metrics(oracle32_stages(O, names), sv, O.fwd[np.float32][1], y_ref, prefix="oracle32."))
    err["fwd.y_repeat_bitwise"] = out["y2_differs"]
    err["bwd.dA"] = rel(out["dA"], stages["dA"])
    err.update(backward_stage_twins(O, G_lib, ["dA"]))
    got = {nm: out.get("grad." + nm) for nm in _lib.PARAM_FIELDS}
    shaped = lambda g: {k: (None if (v is None or got[k] is None) else np.asarray(v).reshape(got[k].shape)) for k, v in g.items()}
    r64 = shaped(g_ref)
    err.update(slice_metrics(got, r64, out["dx"], dx_ref, out["y"], y_ref, Kt, N, gct))
    err.update(slice_metrics(shaped(g32), r64, dx32, dx_ref, O.fwd[np.float32][1], y_ref, Kt, N, gct, prefix="oracle32."))
    for nm in _lib.PARAM_FIELDS:
        if (got[nm] is None) != (g_ref[nm] is None):
            err["grad_none_ok." + nm] = 1.0
    return err


def cap_violations(err):
    """Keys on which the float32 oracle ALONE is outside the cap: the pair does not belong in the table."""
    bad = {}
    for k, v in err.items():
        if k.startswith("oracle32.") and is_measured(k[9:]):
            limit = FWD_TOL if is_forward(k[9:]) else ORACLE32_TOL
            if not (v <= limit):
                bad[k] = v
    return bad


def effective_bar(key, err):
    if not is_measured(key):
        return bar(key)
    twin = err["oracle32." + key]
    if is_forward(key):
        return max(R * twin, FLOOR_FWD)
    return min(max(R * twin, FLOOR_GRAD), GRAD_TOL)


def violations(err):
    return {k: (v, effective_bar(k, err)) for k, v in err.items() if not k.startswith("oracle32.") and not (v <= effective_bar(k, err))}


def worst_ratio(err):
    """(ratio, key) of the measured key furthest up its bar's scale: err / max(oracle32 err, floor / R)."""
    best = (0.0, None)
    for k, v in err.items():
        if not k.startswith("oracle32.") and is_measured(k):
            floor = FLOOR_FWD if is_forward(k) else FLOOR_GRAD
            r = v / max(err["oracle32." + k], floor / R)
            if r > best[0]:
                best = (r, k)
    return best


def assert_condition(err, label):
    cap = cap_violations(err)
    assert not cap, f"{label}: the float32 oracle alone is outside the cap (not a pair for this table): {cap}"
    bad = violations(err)
    ratio, key = worst_ratio(err)
    assert not bad, f"{label}: over the criterion (error, bar): {bad}\nworst ratio {ratio:.1f} at {key}\nall: {err}"


def report(err, row, cond, x6, mode, backend):
    """STGCN_COND_REPORT=<file>: one JSON line per run (how profiles/conditioning_errors.md is made: tools/conditioning_report.py)."""
    path = os.environ.get("STGCN_COND_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps({"row": row, "condition": cond, "x6": "default" if x6 is None else x6, "mode": mode, "backend": backend, **err}) + "\n")


# ---------------------------------------------------------------------------------------------------------------- non-finite inputs
BF16X6_RANGE = 2.0 ** 127 * (2.0 - 2.0 ** -8)      # |x| at and above it rounds to an infinite bf16 h plane (split3): 3.3962e38 < FLT_MAX
NONFINITE = {"nan": float("nan"), "inf": float("inf"), "3.3e38": 3.3e38, "3.4e38": 3.4e38}      # the last: finite in fp32, beyond the x6 range
INJECT_AT = (0, 5, 3, 7)      # (batch item, channel, step, node) -- channel 0 for a one-channel row


def forward_only(dev, case, O, seed=99, offset=3):
    """An eval forward through the C entry, into buffers of the caller's own: (y channels-last, U1 or None where the plan does not store it,
    the three chain words of the workspace)."""
    c_in, channels, Kt, Ks, gct, act, N, B, T, _ = case
    L = bind(dev)
    cuda = str(dev).startswith("cuda")
    bcfg = ops.BlockConfig(Kt=Kt, Ks=Ks, n_vertex=N, c_in=c_in, channels=tuple(channels), act_func=act, graph_conv_type=gct, droprate=O.pdrop)
    gp, gt = ops.gso_prepare(torch.from_numpy(O.gso).to(dev), ops.graph_terms(bcfg))
    params = [None if t is None else t.clone().to(dev) for t in params_in_field_order(O.p, "st_blocks.0.", gct)]
    desc = ops.make_desc(bcfg, B, T, False, False)
    plan = ops.query_plan(desc)
    x_cl = torch.from_numpy(cl(O.x_np)).to(dev)
    y = torch.empty(B, plan.T2, N, channels[2], device=dev)
    saved = torch.empty(plan.saved_floats, device=dev)
    ws = torch.zeros(plan.ws_floats, device=dev)
    pst = ops._param_struct(_lib.StblockParams, params)
    stream = torch.cuda.current_stream().cuda_stream if cuda else None
    L.check(L.dll.stgcn_stblock_forward(C.byref(desc), C.byref(pst), x_cl.data_ptr(), gp.data_ptr(), y.data_ptr(), saved.data_ptr(), ws.data_ptr(),
                                        seed, offset, None, stream), "fwd")
    if cuda:
        torch.cuda.synchronize()
    words = ws[plan.ws_chain:plan.ws_chain + 4].view(torch.int32).cpu().numpy()[:3]
    U1 = None
    if not plan.recompute_tc1:
        U1 = saved[plan.sv_U1:plan.sv_U1 + B * plan.T1 * N * channels[0]].cpu().numpy().reshape(B, plan.T1, N, channels[0])
    return y.cpu().numpy(), U1, words


FLT_MAX = float(np.finfo(np.float32).max)


def run_nonfinite(dev, row, what, x6=None):
    """One element of x[0] replaced by NONFINITE[what]; eval forward of the row beside the clean forward.  Returns counts:
      oracle_nonfinite             y elements of batch item 0 the float64 oracle leaves non-finite
      finite_where_oracle_is_not   ... of those, finite in the library (contract: 0)
      lib_nonfinite                y elements of batch item 0 non-finite in the library
      other_item_differs           elements of batch item 1 that differ bitwise from the clean run (contract: 0)
      chain_words                  |sticky / ticket words| of both runs (contract: 0)
      u1_representable, u1_lost    elements of the first conv's U1 (batch item 0; rows that store it) whose float64 value an fp32 number can
                                   hold (|v| <= 0.99 FLT_MAX), and those of them the library holds as inf / NaN
      u1_rel                       max |library - float64| / max |float64| over the representable elements the library holds finite"""
    case = ROWS[row]
    clean = oracle(row, None)
    O = BlockOracle(*case[:9], oracle32=False)
    b, c, t, n = INJECT_AT
    O.x_np[b, min(c, case[0] - 1), t, n] = np.float32(NONFINITE[what])
    with np.errstate(all="ignore"):
        O.forward(None)
    _, y_ref, sv = O.fwd[np.float64]
    with x6_env(x6):
        y0, _, w0 = forward_only(dev, case, clean)
        y1, U1, w1 = forward_only(dev, case, O)
    bad_ref = ~np.isfinite(y_ref[0])
    bad_lib = ~np.isfinite(y1[0])
    out = {"oracle_nonfinite": int(bad_ref.sum()), "finite_where_oracle_is_not": int((bad_ref & ~bad_lib).sum()), "lib_nonfinite": int(bad_lib.sum()),
           "other_item_differs": int((y1[1:].view(np.uint32) != y0[1:].view(np.uint32)).sum()), "chain_words": int(np.abs(w0).sum() + np.abs(w1).sum()),
           "clean_nonfinite": int((~np.isfinite(y0)).sum()), "y_elements_per_item": int(y_ref[0].size)}
    if U1 is not None:
        ref = sv["U1"][0]
        ok = np.isfinite(ref) & (np.abs(np.where(np.isfinite(ref), ref, 0.0)) <= 0.99 * FLT_MAX)
        held = ok & np.isfinite(U1[0])
        out.update(u1_representable=int(ok.sum()), u1_lost=int((ok & ~held).sum()),
                   u1_rel=float(np.abs(U1[0][held].astype(np.float64) - ref[held]).max() / np.abs(ref[held]).max()))
    return out


def assert_nonfinite(got, row, what, x6):
    """The contract of DESIGN.md section 5 (non-finite inputs)."""
    label = f"{row} {what} x6={x6}: {got}"
    assert got["clean_nonfinite"] == 0 and got["chain_words"] == 0 and got["other_item_differs"] == 0, label
    assert got["finite_where_oracle_is_not"] == 0, label
    if what in ("nan", "inf"):
        assert got["oracle_nonfinite"] > 0 and got["lib_nonfinite"] >= got["oracle_nonfinite"], label
    if "u1_lost" in got:
        beyond_x6 = x6 is None and abs(NONFINITE[what]) >= BF16X6_RANGE and np.isfinite(NONFINITE[what])
        if beyond_x6:
            # pinned, not wished for: the bf16 h plane of split3 is infinite from 2^127 (2 - 2^-8) on, the m plane -inf, and every product the
            # element enters is NaN -- including those an fp32 number holds.  A non-finite result, never a wrong finite one.
            assert got["u1_lost"] > 0, label
        else:
            assert got["u1_lost"] == 0 and got["u1_rel"] <= 1e-6, label


# (c_in, channels, Ko, N, B, T, act): the head's two forward forms -- tconv_fwd4 + fc_fwd_kernel (N < 32) and the one-launch head_fwd_kernel
HEAD_ROWS = {"fc_fwd": (64, (128, 128), 4, 21, 2, 4, "glu"), "head_fwd": (64, (128, 128), 4, 37, 2, 4, "glu")}


def run_head_nonfinite(dev, row, what):
    """The output head's eval forward with one element of x[0] replaced by NONFINITE[what], beside the clean forward: the counts of
    run_nonfinite for the prediction, and the kernels the forward launched."""
    from oracle import stblock_stages as st
    from tests import head_util as hu
    c_in, channels, Ko, N, B, T, act = HEAD_ROWS[row]
    L = hu.bind(dev)
    p, x_np, _, _ = hu.head_inputs(c_in, channels, Ko, N, B, T, act)
    hcfg = ops.HeadConfig(Ko=Ko, n_vertex=N, c_in=c_in, channels=channels, end_channel=1, act_func=act, droprate=0.5)
    params = [p["output." + n].clone().to(dev) for n in hu.NAMES]
    bad = x_np.copy()
    b, c, t, n = INJECT_AT
    bad[b, c, min(t, T - 1), n] = np.float32(NONFINITE[what])
    outs, launched = [], {}
    for x in (x_np, bad):
        L.dll.stgcn_profile_enable(1)
        try:
            with torch.no_grad():
                wsc = ops.WorkspaceCache()
                o = ops.output_block(torch.from_numpy(x).to(dev), hcfg, params, False, 77, 5, wsc)
            chain = ops.head_chain_status(hcfg, B, T, wsc)
        finally:
            buf = C.create_string_buffer(1 << 16)
            L.dll.stgcn_profile_collect(buf, len(buf))
            L.dll.stgcn_profile_enable(0)
        launched.update(json.loads(buf.value.decode()))
        outs.append((o.cpu().numpy(), chain))
    with np.errstate(all="ignore"):
        ref, _ = st.outblock_fwd(cl(bad).astype(np.float64), st.head_params_np(p, np.float64), Ko, c_in, channels, act)
    (y0, w0), (y1, w1) = outs
    bad_ref, bad_lib = ~np.isfinite(ref[0]), ~np.isfinite(y1[0, 0])
    return {"oracle_nonfinite": int(bad_ref.sum()), "finite_where_oracle_is_not": int((bad_ref & ~bad_lib).sum()), "lib_nonfinite": int(bad_lib.sum()),
            "other_item_differs": int((y1[1:].view(np.uint32) != y0[1:].view(np.uint32)).sum()), "chain_words": int(abs(w0) + abs(w1)),
            "clean_nonfinite": int((~np.isfinite(y0)).sum()), "kernels": sorted(launched)}
