"""Stage-level harness of the fused ST-Conv block, shared by the -m gpu tests and the emulator tests: run one block through the bound
library -- the CPU emulator for "cpu", the HIP library for "cuda:0" -- and compare every saved tensor, every materialised intermediate
gradient, dx and the parameter gradients with the float64 stage oracle (oracle/stblock_stages.py: stblock_fwd / stblock_bwd).

debug_stages=True is the launch sequence of the stage tests (ops.set_debug_stages: two extra launches per fp32 backward,
ln_gate_bwd_kernel in front of tc2_bwd_kernel and align_gate_bwd_kernel<1> in front of tc1_bwd_kernel, which materialise dZ2 / dZ1 --
and write the same LayerNorm-parameter partials the fused kernel then overwrites).  debug_stages=False is the sequence every training
step launches; there the partial-sum arena is filled with NaN between forward and backward, so that a partial block the fused kernels
do not write (and the reduction reads) reaches a gradient as NaN instead of as whatever the previous call left.  The flag is restored
on return: what runs after a case launches the production sequence.

Error keys, in the order a fault would propagate (the first key out of tolerance names the stage to look at):
  grad_none_ok.chain_words_*                          sticky / ticket words of both workspaces: bar 0 (grad_none_ok.<param>: no gradient where
                                                      the reference leaves .grad None)
  fwd.U1 .. fwd.y, fwd.rstd_rel                       absolute (rstd: relative), bar FWD_TOL
  fwd.y_repeat_bitwise                                a second forward into the harness's own buffers: bar 0
  slice.y.tail                                        |y - oracle| over the last ragged 16-node tile (N % 16 != 0), bar FWD_TOL
  bwd.dZ2, bwd.dYg, bwd.dA, bwd.dZ1, bwd.dx           max error / max |ref|, bar GRAD_TOL; dZ2 / dZ1 only where they are materialised
  grad.<param>                                        max error / max |ref| of the whole tensor, bar GRAD_TOL
  slice.tc1_w.k<k>, slice.tc2_w.k<k>, slice.gc_w.k<k> the same over tap / Chebyshev term k alone, normalised by THAT slice's max
  slice.ln_w.tail, slice.ln_b.tail                    over the last ragged 16-node tile
  slice.dx.t0, slice.dx.tlast                         the edge steps of the transposed conv (one tap each)
  info.relu_units_*, kink.*                           graph-conv outputs at the ReLU kink (see BlockOracle.forward): counts, and by how much they
                                                      exceed their bounds (bar 0)
  oracle32.<grad / slice key>                         the SAME metric for the stage oracle run in np.float32 against its float64 run: what
                                                      fp32 rounding alone does on these inputs.  Bar ORACLE32_TOL = GRAD_TOL / 4 -- inputs
                                                      that nearly cancel a slice get another seed, never another bar.
run_block_pair adds, for the production run, every key above as prod.<key> and
  prod.bitwise_vs_debug                               elements of y, dx and all parameter gradients that differ between the two runs: bar 0
  prod.nan_elements                                   NaN elements among them in the production run: bar 0
"""
import ctypes as C
import json

import numpy as np
import torch

from oracle import stblock_stages as st
from stgcn_amd import _lib, ops
from tests.emu_util import block_case, nonsym_gso, params_in_field_order

FWD_TOL = 1e-4     # north star: activations within 1e-4 abs of the reference CPU path
GRAD_TOL = 1e-3    # north star / SURVEY.md 8d: gradients rtol 1e-3
ORACLE32_TOL = GRAD_TOL / 4      # tests/head_util.py


def bind(dev):
    if str(dev) == "cpu":
        from tests.emu_util import bind_emulator
        return bind_emulator()
    L = _lib.use_library(_lib.DEFAULT_LIB)
    assert L.backend == "hip-gfx950", "GPU tests must run on the HIP library, not the emulator"
    return L


def rel(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(1e-30, float(np.abs(ref).max())))


def cl(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1))


def param_slices(ref, Kt, N, gct):
    """(key, parameter name, index) of every parameter-gradient slice the harnesses measure on its own (tests/bf16_util.py shares it):
    tap k of the two temporal convs, Chebyshev term k of the graph conv, the LayerNorm rows of the last ragged 16-node tile."""
    for name in ("tc1_w", "tc2_w"):
        for k in range(Kt):
            yield f"slice.{name}.k{k}", name, (slice(None), slice(None), k)
    if gct == "cheb_graph_conv":
        for k in range(ref["gc_w"].shape[0]):
            yield f"slice.gc_w.k{k}", "gc_w", (k,)
    if N % 16:
        for k in ("ln_w", "ln_b"):
            yield f"slice.{k}.tail", k, (slice(N - N % 16, None),)


def slice_metrics(got, ref, dx, dx_ref, y, y_ref, Kt, N, gct, prefix=""):
    """{key: error} of the gradients `got` against `ref` (dicts keyed like st.block_params_np, arrays shaped like the parameters; None =
    no gradient), dx and y (channels-last; None = absent): per tensor, per tap, per Chebyshev term, over the ragged node tile and over
    the edge steps of the transposed conv."""
    err = {}
    for k, r in ref.items():
        if r is not None and got.get(k) is not None:
            err[f"{prefix}grad.{k}"] = rel(got[k], r)
    for key, name, idx in param_slices(ref, Kt, N, gct):
        err[prefix + key] = rel(got[name][idx], ref[name][idx])
    tail = N - N % 16
    if N % 16:
        if y is not None:
            err[f"{prefix}slice.y.tail"] = float(np.abs(y[:, :, tail:].astype(np.float64) - y_ref[:, :, tail:]).max())
    if dx_ref is not None and dx is not None:
        err[f"{prefix}bwd.dx"] = rel(dx, dx_ref)
        err[f"{prefix}slice.dx.t0"] = rel(dx[:, 0], dx_ref[:, 0])
        err[f"{prefix}slice.dx.tlast"] = rel(dx[:, -1], dx_ref[:, -1])
    return err


class BlockOracle:
    """The inputs of one case and its float64 / float32 oracle.  The forward is computed once and never changed; the backward is
    computed once per ReLU side pattern (see backward)."""

    def __init__(self, c_in, channels, Kt, Ks, gct, act, N, B, T, gso=None, pdrop=0.5, param_seed=3, data_seed=11, oracle32=True, kink=True):
        self.dtypes = (np.float64, np.float32) if oracle32 else (np.float64,)
        self.kink_on = kink      # False: the oracle keeps its own ReLU mask everywhere (the whole-tensor stage tests of tests/gpu_util.py)
        self.args = (c_in, tuple(channels), Kt, Ks, gct, act, N, B, T)
        self.pdrop = pdrop
        _, self.p = block_case(c_in, channels, Kt, Ks, gct, act, N, B, T, seed=param_seed)
        self.gso = nonsym_gso(N, 5) if gso is None else gso
        rs = np.random.RandomState(data_seed)
        self.x_np = rs.standard_normal((B, c_in, T, N)).astype(np.float32)
        self.T2 = T - 2 * (Kt - 1)
        self.dy_np = rs.standard_normal((B, channels[2], self.T2, N)).astype(np.float32)
        self.fwd = {}
        self.bwd = {}
        self.keep = "unset"

    def forward(self, keep):
        """keep: the library's dropout mask (bool, channels-last) or None; the same for every run of the case (seed and offset are)."""
        if self.fwd:
            assert (keep is None) == (self.keep is None) and (keep is None or np.array_equal(keep, self.keep))
            return
        c_in, channels, Kt, Ks, gct, act, N, B, T = self.args
        self.keep = keep
        for dt in self.dtypes:
            bp = st.block_params_np(self.p, "st_blocks.0.", gct, dt)
            y, sv = st.stblock_fwd(cl(self.x_np).astype(dt), self.gso.astype(dt), bp, Kt, c_in, channels, gct, act,
                                   None if keep is None else keep.astype(dt), self.pdrop)
            self.fwd[dt] = (bp, y, sv)
        # ReLU is not differentiable at 0: a graph-conv output whose float64 pre-activation lies within FWD_TOL of zero -- closer than
        # the forward is held to -- may come out on either side in fp32, and dYg = dG * (G > 0) differs by the whole of dG there
        # (tests/head_util.py records the same for the head's hidden units).  The window and the flips are counted and bounded exactly as
        # there; the backward oracle takes the library's side for the units of the window ONLY, so a wrong mask anywhere else still shows.
        bp, _, sv = self.fwd[np.float64]
        Wk = sv["Wk"]
        pre = sum(sv["Xs"][k] @ Wk[k] for k in range(Wk.shape[0])) + (0.0 if bp["gc_b"] is None else bp["gc_b"]) + sv["A"]
        assert np.array_equal(np.maximum(pre, 0.0) > 0, sv["G"] > 0)
        self.kink = (np.abs(pre) < FWD_TOL) & bool(self.kink_on)
        self.window_bar = 2.0 * pre.size * 2.0 * FWD_TOL / (float(pre.std()) * np.sqrt(2.0 * np.pi)) + 5.0

    def backward(self, G_lib):
        """(dx64, g64, stages64, dx32, g32, kink metrics) with the units of the kink window on the side the library's saved G took."""
        c_in, channels, Kt, Ks, gct, act, N, B, T = self.args
        side = (G_lib > 0) & self.kink
        key = side.tobytes()
        if key not in self.bwd:
            out = []
            for dt in self.dtypes:
                bp, _, sv = self.fwd[dt]
                sv = dict(sv)
                sv["G"] = np.where(self.kink, G_lib.astype(dt), sv["G"])
                stages = {}
                dx, g = st.stblock_bwd(cl(self.dy_np).astype(dt), sv, self.gso.astype(dt), bp, Kt, c_in, channels, gct, act, self.pdrop,
                                       need_dx=c_in > 1, stages=stages)
                # the stages the harness compares beyond dYg / dA
                dH2, _, _ = st.ln_dropout_bwd(cl(self.dy_np).astype(dt), sv["H2"], bp["ln_w"], sv["mean"], sv["rstd"], sv["keep"], self.pdrop)
                stages["dZ2"] = st.gate_bwd(dH2, sv["U2"], sv["S2"], act)
                stages["dZ1"] = st.gate_bwd(stages["dA"] @ sv["Wa"].T, sv["U1"], sv["S1"], act)
                out += [dx, g, stages]
            self.bwd[key] = out
        dx64, g64, stages, dx32, g32, _ = (self.bwd[key] + [None, None, None])[:6]
        G64 = self.fwd[np.float64][2]["G"]
        window = float(self.kink.sum())
        flips = float((self.kink & ((G_lib > 0) != (G64 > 0))).sum())
        info = {"info.relu_units_within_fwd_tol_of_zero": window, "info.relu_units_on_the_other_side": flips,
                "kink.window_over_bar": max(0.0, window - self.window_bar), "kink.flips_over_bar": max(0.0, flips - (0.25 * window + 1.0))}
        if not self.kink_on:
            info = {}
        return dx64, g64, stages, dx32, g32, info


def run_block_case(dev, c_in, channels, Kt, Ks, gct, act, N, B, T, training, gso=None, seed=99, offset=3, pdrop=0.5, debug_stages=True,
                   oracle=None, oracle32=True, kink=True, outputs=None):
    """Returns the dict of errors described in the module docstring.  oracle: a BlockOracle of the same case to share between runs;
    outputs: a dict that receives y, dx and the parameter gradients (numpy) for bitwise comparisons between runs."""
    L = bind(dev)
    cuda = str(dev).startswith("cuda")
    prev_debug = ops.set_debug_stages(bool(debug_stages))
    try:
        O = oracle if oracle is not None else BlockOracle(c_in, channels, Kt, Ks, gct, act, N, B, T, gso=gso, pdrop=pdrop, oracle32=oracle32, kink=kink)
        assert O.args == (c_in, tuple(channels), Kt, Ks, gct, act, N, B, T) and O.pdrop == pdrop
        T2 = O.T2
        c0, c1, c2 = channels
        bcfg = ops.BlockConfig(Kt=Kt, Ks=Ks, n_vertex=N, c_in=c_in, channels=tuple(channels), act_func=act, graph_conv_type=gct, droprate=pdrop)
        gp, gt = ops.gso_prepare(torch.from_numpy(O.gso).to(dev), ops.graph_terms(bcfg))
        params = [None if t is None else t.clone().to(dev).requires_grad_(True) for t in params_in_field_order(O.p, "st_blocks.0.", gct)]
        x = torch.from_numpy(O.x_np).to(dev).requires_grad_(c_in > 1)
        desc = ops.make_desc(bcfg, B, T, training, c_in > 1)
        plan = ops.query_plan(desc)
        wsc = ops.WorkspaceCache()
        y = ops.st_conv_block(x, gp, gt, bcfg, params, training, seed, offset, wsc)
        assert y.shape == (B, c2, T2, N)
        if not debug_stages:
            # the arena of per-workgroup gradient partials ONLY: the packed weights and the chain words live in the same buffer
            assert wsc.buf.numel() >= plan.ws_part + plan.part_floats
            wsc.buf[plan.ws_part:plan.ws_part + plan.part_floats].fill_(float("nan"))
        y.backward(torch.from_numpy(O.dy_np).to(dev))
        if cuda:
            torch.cuda.synchronize()

        keep = None
        if training:
            keep = ops.dropout_mask(B * T2 * N * c2, pdrop, seed, offset, dev).cpu().numpy().reshape(B, T2, N, c2) > 0
        O.forward(keep)
        bp, y_ref, sv = O.fwd[np.float64]
        y32 = O.fwd[np.float32][1] if oracle32 else None

        # the autograd ctx keeps `saved`; fetch it again through a second forward into our own buffers
        ws = wsc.buf.cpu().numpy()
        saved = torch.empty(plan.saved_floats, device=dev)
        y2 = torch.empty_like(y.permute(0, 2, 3, 1).contiguous())
        pst = ops._param_struct(_lib.StblockParams, [None if t is None else t.detach() for t in params])
        x_cl = x.detach().permute(0, 2, 3, 1).contiguous()
        ws2 = torch.empty(plan.ws_floats, device=dev)
        stream = torch.cuda.current_stream().cuda_stream if cuda else None
        L.check(L.dll.stgcn_stblock_forward(C.byref(desc), C.byref(pst), x_cl.data_ptr(), gp.data_ptr(), y2.data_ptr(), saved.data_ptr(),
                                            ws2.data_ptr(), seed, offset, None, stream), "fwd")
        if cuda:
            torch.cuda.synchronize()
        svn = saved.cpu().numpy()
        T1 = plan.T1
        terms = 2 if gct == "graph_conv" else Ks

        def seg(buf, off, ref):
            return float(np.abs(buf[off:off + ref.size].reshape(ref.shape) - ref).max())

        err = {}
        # chained launches: the sticky error word (a bounded wait gave up) of both workspaces, and ticket / finished-workgroup words re-armed
        for nm, buf in (("autograd", wsc.buf), ("direct", ws2)):
            cw = buf[plan.ws_chain:plan.ws_chain + 4].view(torch.int32).cpu().numpy()
            err[f"grad_none_ok.chain_words_{nm}"] = float(abs(cw[:3]).sum())
        if not plan.recompute_tc1:
            err["fwd.U1"] = seg(svn, plan.sv_U1, sv["U1"])
            err["fwd.S1"] = seg(svn, plan.sv_S1, sv["S1"])
        err["fwd.A"] = seg(svn, plan.sv_A, sv["A"])
        for k in range(1, terms):
            err[f"fwd.X{k}"] = seg(svn, plan.sv_Xk + (k - 1) * B * T1 * N * c1, sv["Xs"][k])
        err["fwd.G"] = seg(svn, plan.sv_G, sv["G"])
        if plan.stored_US2:
            err["fwd.U2"] = seg(svn, plan.sv_U2, sv["U2"])
            err["fwd.S2"] = seg(svn, plan.sv_S2, sv["S2"])
        err["fwd.mean"] = seg(svn, plan.sv_mean, sv["mean"])
        err["fwd.rstd_rel"] = float(np.abs(svn[plan.sv_rstd:plan.sv_rstd + B * T2].reshape(B, T2) / sv["rstd"] - 1).max())
        y_cl = cl(y.detach().cpu().numpy())
        err["fwd.y"] = float(np.abs(y_cl.astype(np.float64) - y_ref).max())
        err["fwd.y_repeat_bitwise"] = float((y2 != y.detach().permute(0, 2, 3, 1)).sum().item())

        G_lib = svn[plan.sv_G:plan.sv_G + sv["G"].size].reshape(sv["G"].shape)
        dx_ref, g_ref, stages, dx32, g32, info = O.backward(G_lib)
        err.update(info)

        def stage(name, off):
            ref = stages[name]
            err["bwd." + name] = rel(ws[off:off + ref.size].reshape(ref.shape), ref)

        if debug_stages or not plan.fused_tc2_bwd:      # tc2_bwd_kernel keeps dZ2 on chip
            stage("dZ2", plan.ws_dZ2)
        stage("dYg", plan.ws_dYg)
        stage("dA", plan.ws_dA)
        # tc1_bwd_kernel keeps dZ1 on chip; the thin first layer does unless dx is needed
        if not (plan.thin_tc1 and c_in == 1) and (debug_stages or not plan.fused_tc1_bwd):
            stage("dZ1", plan.ws_dZ1)

        got = {}
        for name, prm in zip(_lib.PARAM_FIELDS, params):
            ref = g_ref[name]
            got[name] = None
            if prm is None:
                continue
            if ref is None:
                err["grad_none_ok." + name] = 0.0 if prm.grad is None else 1.0
                continue
            if prm.grad is None:
                err["grad." + name] = float("inf")
                continue
            got[name] = prm.grad.cpu().numpy()
        shaped = lambda g: {k: (None if (v is None or got[k] is None) else np.asarray(v).reshape(got[k].shape)) for k, v in g.items()}
        r64 = shaped(g_ref)
        dx = None
        if c_in > 1:
            dx = cl(x.grad.cpu().numpy())
        else:
            err["grad_none_ok.dx"] = 0.0 if x.grad is None else 1.0
        err.update(slice_metrics(got, r64, dx, dx_ref, y_cl, y_ref, Kt, N, gct))
        if oracle32:
            err.update(slice_metrics(shaped(g32), r64, dx32, dx_ref, y32, y_ref, Kt, N, gct, prefix="oracle32."))
        if outputs is not None:
            outputs["y"] = y_cl
            if dx is not None:
                outputs["dx"] = dx
            outputs.update({"grad." + k: v for k, v in got.items() if v is not None})
        return err
    finally:
        ops.set_debug_stages(prev_debug)


def run_block_pair(dev, *case, on_half=None, **kw):
    """One case as the stage tests launch it (debug_stages=True) and as production does (False, partial arena poisoned): the first
    run's keys, the second's as prod.<key>, and prod.bitwise_vs_debug."""
    O = BlockOracle(*case[:9], gso=kw.get("gso"), pdrop=kw.get("pdrop", 0.5))
    out_d, out_p = {}, {}
    on_half = on_half or (lambda half, edge: None)      # (the launch-log test marks where each half's launches begin and end)
    on_half("debug", "begin")
    err = run_block_case(dev, *case, debug_stages=True, oracle=O, outputs=out_d, **kw)
    on_half("debug", "end")
    on_half("prod", "begin")
    prod = run_block_case(dev, *case, debug_stages=False, oracle=O, outputs=out_p, **kw)
    on_half("prod", "end")
    err.update({"prod." + k: v for k, v in prod.items() if not k.startswith("oracle32.")})
    assert out_d.keys() == out_p.keys()
    err["prod.nan_elements"] = float(sum(int(np.isnan(v).sum()) for v in out_p.values()))
    err["prod.bitwise_vs_debug"] = float(sum(int((out_d[k].view(np.uint32) != out_p[k].view(np.uint32)).sum()) for k in out_d))
    return err


def bar(key):
    """The bar a key is held to."""
    if key.startswith("prod."):
        key = key[5:]
    if key.startswith(("grad_none_ok", "chain.", "kink.")) or key.endswith("bitwise") or key in ("bitwise_vs_debug", "nan_elements"):
        return 0.0
    if key.startswith("info."):
        return float("inf")
    if key.startswith("oracle32."):
        return ORACLE32_TOL
    if key.startswith("fwd.") or key == "slice.y.tail":
        return FWD_TOL
    return GRAD_TOL      # bwd.*, grad.*, slice.*


def assert_errors(err):
    bad = {k: v for k, v in err.items() if not (v <= bar(k))}
    assert not bad, f"out of tolerance: {bad}\nall: {err}"


def worst_oracle32(err):
    return max(v for k, v in err.items() if k.startswith("oracle32."))


def report_block_errors(err, label, path):
    """Appends one JSON line per case to `path` (how profiles/block_stage_errors.md is made: tools/block_stage_report.py)."""
    with open(path, "a") as fh:
        fh.write(json.dumps({"case": label, **err}) + "\n")
