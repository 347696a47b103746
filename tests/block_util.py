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

Consumer mode (run_block_case(consumer="block" | "head"), tests/test_gpu_block_hooks.py): the block P feeds a second fused module Q, whose
backward writes P's LayerNorm-backward row partials (stgcn_ln_hook); P then runs with dy_rowstats_ready.  Every key above is computed for P
with dy = y.grad; the partials are read from P's workspace, wsc.buf[plan.ws_rowstat_b : + 2 * B * T2 * N] as [B, T2, N, 2].  Added keys:
  hook.rowstat_g, hook.rowstat_gx                     the partials against the float64 sums sum_c g, sum_c g * xhat (g = keep * dy * gamma / (1 - p);
                                                      oracle/stblock_stages.py ln_rowstats): max error / max |ref| per component, bar GRAD_TOL
  oracle32.hook.rowstat_g, oracle32.hook.rowstat_gx   the same sums formed in np.float32 the way the kernels form them -- sum_kept dy * (y -
                                                      keep_scale * beta), y rounded to fp32 -- against the float64 sums: bar ORACLE32_TOL
  hook.rowstat_nan                                    the region is filled with NaN after both forwards: NaN left after the backward, bar 0
  hook.dy_bitwise_vs_unhooked                         Q alone on a copy of y (no hook offered): elements of its input gradient that differ, bar 0
  hook.rowstat_vs_own_pass_g, _gx                     against the partials of P's own ln_bwd_rowstats pass over the same dy (another summation
                                                      order: not bitwise), bar GRAD_TOL
  grad_none_ok.hook_launches                          |observed - expected| ln_bwd_rowstats launches of the backward, bar 0
and the hooked partials and dy count among the outputs of prod.bitwise_vs_debug / prod.nan_elements.
"""
import ctypes as C
import hashlib
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

    def __init__(self, c_in, channels, Kt, Ks, gct, act, N, B, T, gso=None, pdrop=0.5, param_seed=3, data_seed=11, oracle32=True, kink=True,
                 ln_scale=None, kink_rel=False):
        """kink_rel: the ReLU kink window is FWD_TOL of the LARGEST pre-activation instead of FWD_TOL itself (tests/conditioning_util.py: inputs
        away from unit scale, where an absolute window holds every unit or none).  The default is the absolute window."""
        self.kink_rel = bool(kink_rel)
        self.dtypes = (np.float64, np.float32) if oracle32 else (np.float64,)
        self.kink_on = kink      # False: the oracle keeps its own ReLU mask everywhere (the whole-tensor stage tests of tests/gpu_util.py)
        self.args = (c_in, tuple(channels), Kt, Ks, gct, act, N, B, T)
        self.pdrop = pdrop
        _, self.p = block_case(c_in, channels, Kt, Ks, gct, act, N, B, T, seed=param_seed)
        self.ln_scale = ln_scale
        if ln_scale is not None:      # gamma = g * U(-1, 1), beta = b * U(-1, 1), drawn as tests/bf16_util.py draws them
            rl = np.random.RandomState(77)
            shp = tuple(self.p["st_blocks.0.tc2_ln.weight"].shape)
            self.p["st_blocks.0.tc2_ln.weight"] = torch.from_numpy((ln_scale[0] * rl.uniform(-1, 1, shp)).astype(np.float32))
            self.p["st_blocks.0.tc2_ln.bias"] = torch.from_numpy((ln_scale[1] * rl.uniform(-1, 1, shp)).astype(np.float32))
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
        width, sigma = FWD_TOL, float(pre.std())
        if self.kink_rel:
            # rounding errors scale with the largest magnitude; the count is bounded through the density at zero of a normal distribution
            # as before, with the scale of the BULK of the units (median |pre| / 0.6745, the same sigma on normal data) where one outlying
            # node inflates the standard deviation
            width = FWD_TOL * float(np.abs(pre).max())
            sigma = min(sigma, float(np.median(np.abs(pre))) / 0.6745)
        self.kink = (np.abs(pre) < width) & bool(self.kink_on)
        self.window_bar = 2.0 * pre.size * 2.0 * width / (sigma * np.sqrt(2.0 * np.pi)) + 5.0

    def backward(self, G_lib, dy=None):
        """(dx64, g64, stages64, dx32, g32, kink metrics) with the units of the kink window on the side the library's saved G took.
        dy (NCHW float32): the output gradient the block actually received (consumer mode); None: the case's own external dy."""
        c_in, channels, Kt, Ks, gct, act, N, B, T = self.args
        side = (G_lib > 0) & self.kink
        dy_np = self.dy_np if dy is None else np.ascontiguousarray(dy, dtype=np.float32)
        key = side.tobytes() + (b"" if dy is None else hashlib.sha1(dy_np.tobytes()).digest())
        if key not in self.bwd:
            out = []
            for dt in self.dtypes:
                bp, _, sv = self.fwd[dt]
                sv = dict(sv)
                sv["G"] = np.where(self.kink, G_lib.astype(dt), sv["G"])
                stages = {}
                dx, g = st.stblock_bwd(cl(dy_np).astype(dt), sv, self.gso.astype(dt), bp, Kt, c_in, channels, gct, act, self.pdrop,
                                       need_dx=c_in > 1, stages=stages)
                # the stages the harness compares beyond dYg / dA
                dH2, _, _ = st.ln_dropout_bwd(cl(dy_np).astype(dt), sv["H2"], bp["ln_w"], sv["mean"], sv["rstd"], sv["keep"], self.pdrop)
                # the LayerNorm-backward row partials: float64 from xhat; np.float32 the way the kernels form them, from y rounded to fp32
                if dt == np.float64:
                    stages["rowstat_g"], stages["rowstat_gx"] = st.ln_rowstats(cl(dy_np).astype(dt), sv["H2"], bp["ln_w"], sv["mean"], sv["rstd"],
                                                                               sv["keep"], self.pdrop)
                else:
                    y32 = self.fwd[np.float64][1].astype(np.float32)
                    stages["rowstat_g"], stages["rowstat_gx"] = st.ln_rowstats(cl(dy_np), None, bp["ln_w"], None, None, sv["keep"], self.pdrop,
                                                                               y_stored=y32, beta=bp["ln_b"])
                stages["dZ2"] = st.gate_bwd(dH2, sv["U2"], sv["S2"], act)
                stages["dZ1"] = st.gate_bwd(stages["dA"] @ sv["Wa"].T, sv["U1"], sv["S1"], act)
                out += [dx, g, stages]
            self.bwd[key] = out
        dx64, g64, stages, dx32, g32, stages32 = (self.bwd[key] + [None, None, None])[:6]
        if stages32 is not None:
            stages = dict(stages, rowstat32_g=stages32["rowstat_g"], rowstat32_gx=stages32["rowstat_gx"])
        G64 = self.fwd[np.float64][2]["G"]
        window = float(self.kink.sum())
        flips = float((self.kink & ((G_lib > 0) != (G64 > 0))).sum())
        info = {"info.relu_units_within_fwd_tol_of_zero": window, "info.relu_units_on_the_other_side": flips,
                "kink.window_over_bar": max(0.0, window - self.window_bar), "kink.flips_over_bar": max(0.0, flips - (0.25 * window + 1.0))}
        if not self.kink_on:
            info = {}
        return dx64, g64, stages, dx32, g32, info


def rowstats_launched(L, fn):
    """Runs fn() with the library's launch profile on; returns the number of ln_bwd_rowstats launches (a block's own pass or the pass behind
    a consumer kernel that has no epilogue: the same kernel, the same grid -- only the launch log's order tells them apart)."""
    L.dll.stgcn_profile_enable(1)
    try:
        fn()
    finally:
        buf = C.create_string_buffer(1 << 16)
        L.dll.stgcn_profile_collect(buf, len(buf))
        L.dll.stgcn_profile_enable(0)
    launched = json.loads(buf.value.decode())
    return sum(v["calls"] for k, v in launched.items() if k.startswith("ln_bwd_rowstats"))


def run_block_case(dev, c_in, channels, Kt, Ks, gct, act, N, B, T, training, gso=None, seed=99, offset=3, pdrop=0.5, debug_stages=True,
                   oracle=None, oracle32=True, kink=True, outputs=None, consumer=None, consumer_shape=None, ln_scale=None, expect_rowstats=None,
                   tamper=None, caches=None, data_seed=11, on_span=None, stages_out=None):
    """Returns the dict of errors described in the module docstring.  oracle: a BlockOracle of the same case to share between runs;
    outputs: a dict that receives y, dx and the parameter gradients (numpy) for bitwise comparisons between runs.
    consumer = "block" / "head" (consumer_shape: see make_consumer): the block's output goes straight into a second fused module Q, the
    backward starts at Q's output with a seeded gradient, and dy of the block's oracle is y.grad -- the LayerNorm-backward row partials come
    out of Q's epilogue (or of the pass behind a Q kernel without one) and the block runs with dy_rowstats_ready.  expect_rowstats: the
    ln_bwd_rowstats launches that backward must contain.  ln_scale = (g, b): gamma = g * U(-1, 1), beta = b * U(-1, 1).
    tamper: see run_consumer.  caches: a dict that keeps the workspace caches of P and Q between calls (successive steps of one model);
    data_seed: seed of x and of the external dy.  on_span(name, "begin" / "end"): see run_consumer.
    stages_out: a dict that receives the library's saved forward stages as arrays (U1, S1, A, X<k>, G, U2, S2, mean, rstd -- those the plan
    stores), for metrics of the caller's own (tests/conditioning_util.py)."""
    L = bind(dev)
    cuda = str(dev).startswith("cuda")
    prev_debug = ops.set_debug_stages(bool(debug_stages))
    try:
        O = oracle if oracle is not None else BlockOracle(c_in, channels, Kt, Ks, gct, act, N, B, T, gso=gso, pdrop=pdrop, oracle32=oracle32, kink=kink,
                                                          ln_scale=ln_scale, data_seed=data_seed)
        assert O.args == (c_in, tuple(channels), Kt, Ks, gct, act, N, B, T) and O.pdrop == pdrop and O.ln_scale == ln_scale
        T2 = O.T2
        c0, c1, c2 = channels
        bcfg = ops.BlockConfig(Kt=Kt, Ks=Ks, n_vertex=N, c_in=c_in, channels=tuple(channels), act_func=act, graph_conv_type=gct, droprate=pdrop)
        gp, gt = ops.gso_prepare(torch.from_numpy(O.gso).to(dev), ops.graph_terms(bcfg))
        params = [None if t is None else t.clone().to(dev).requires_grad_(True) for t in params_in_field_order(O.p, "st_blocks.0.", gct)]
        x = torch.from_numpy(O.x_np).to(dev).requires_grad_(c_in > 1)
        desc = ops.make_desc(bcfg, B, T, training, c_in > 1)
        plan = ops.query_plan(desc)
        caches = {} if caches is None else caches
        wsc = caches.setdefault("p", ops.WorkspaceCache())
        y = ops.st_conv_block(x, gp, gt, bcfg, params, training, seed, offset, wsc)
        assert y.shape == (B, c2, T2, N)
        if not debug_stages:
            # the arena of per-workgroup gradient partials ONLY: the packed weights and the chain words live in the same buffer
            assert wsc.buf.numel() >= plan.ws_part + plan.part_floats
            wsc.buf[plan.ws_part:plan.ws_part + plan.part_floats].fill_(float("nan"))
        hook, dy_got = {}, None
        if consumer is None:
            y.backward(torch.from_numpy(O.dy_np).to(dev))
        else:
            dy_got = run_consumer(L, dev, consumer, consumer_shape, O, y, x, params, gp, gt, bcfg, plan, wsc, training, seed, offset, expect_rowstats, hook,
                                  tamper=tamper, q_wsc=caches.setdefault("q", ops.WorkspaceCache()), on_span=on_span)
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

        def seg(buf, off, ref, name=None):
            got = buf[off:off + ref.size].reshape(ref.shape)
            if stages_out is not None and name is not None:
                stages_out[name] = got
            return float(np.abs(got - ref).max())

        err = {}
        # chained launches: the sticky error word (a bounded wait gave up) of both workspaces, and ticket / finished-workgroup words re-armed
        for nm, buf in (("autograd", wsc.buf), ("direct", ws2)):
            cw = buf[plan.ws_chain:plan.ws_chain + 4].view(torch.int32).cpu().numpy()
            err[f"grad_none_ok.chain_words_{nm}"] = float(abs(cw[:3]).sum())
        if not plan.recompute_tc1:
            err["fwd.U1"] = seg(svn, plan.sv_U1, sv["U1"], "U1")
            err["fwd.S1"] = seg(svn, plan.sv_S1, sv["S1"], "S1")
        err["fwd.A"] = seg(svn, plan.sv_A, sv["A"], "A")
        for k in range(1, terms):
            err[f"fwd.X{k}"] = seg(svn, plan.sv_Xk + (k - 1) * B * T1 * N * c1, sv["Xs"][k], f"X{k}")
        err["fwd.G"] = seg(svn, plan.sv_G, sv["G"], "G")
        if plan.stored_US2:
            err["fwd.U2"] = seg(svn, plan.sv_U2, sv["U2"], "U2")
            err["fwd.S2"] = seg(svn, plan.sv_S2, sv["S2"], "S2")
        err["fwd.mean"] = seg(svn, plan.sv_mean, sv["mean"], "mean")
        err["fwd.rstd_rel"] = float(np.abs(svn[plan.sv_rstd:plan.sv_rstd + B * T2].reshape(B, T2) / sv["rstd"] - 1).max())
        if stages_out is not None:
            stages_out["rstd"] = svn[plan.sv_rstd:plan.sv_rstd + B * T2].reshape(B, T2)
        y_cl = cl(y.detach().cpu().numpy())
        err["fwd.y"] = float(np.abs(y_cl.astype(np.float64) - y_ref).max())
        err["fwd.y_repeat_bitwise"] = float((y2 != y.detach().permute(0, 2, 3, 1)).sum().item())

        G_lib = svn[plan.sv_G:plan.sv_G + sv["G"].size].reshape(sv["G"].shape)
        dx_ref, g_ref, stages, dx32, g32, info = O.backward(G_lib, dy_got)
        err.update(info)
        if consumer is not None:
            for c, nm in enumerate(("g", "gx")):
                ref = stages["rowstat_" + nm]
                err["hook.rowstat_" + nm] = rel(hook["rowstat"][..., c], ref)
                if hook["rowstat_own"] is not None:
                    err["hook.rowstat_vs_own_pass_" + nm] = rel(hook["rowstat"][..., c], hook["rowstat_own"][..., c].astype(np.float64))
                if oracle32:
                    err["oracle32.hook.rowstat_" + nm] = rel(stages["rowstat32_" + nm], ref)
            err.update(hook["err"])

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
            if consumer is not None:
                outputs["hook.rowstat"], outputs["dy"] = hook["rowstat"], dy_got
        return err
    finally:
        ops.set_debug_stages(prev_debug)


def make_consumer(dev, kind, shape, c_in, Kt, Ks, gct, act, N, T_in, pdrop, gp, gt):
    """The fused module Q that consumes a block's output (B, c_in, T_in, N): kind "block" (shape: channels, Kt -- defaults (64, 16, 64) and the
    producer's Kt; graph conv, activation and operator as the producer's) or "head" (shape: channels, default (128, 128); Ko = T_in, the head
    consumes the whole remaining axis).  Returns make(wsc=None) -> run: fresh parameter leaves holding the same values on every call, and
    run(x, training, seed, offset) -> Q(x) on the workspace cache given (None: one of its own)."""
    shape = dict(shape or {})
    if kind == "block":
        qch, qKt = tuple(shape.get("channels", (64, 16, 64))), shape.get("Kt", Kt)
        _, pc = block_case(c_in, qch, qKt, Ks, gct, act, N, 1, T_in, seed=8)
        cfg = ops.BlockConfig(Kt=qKt, Ks=Ks, n_vertex=N, c_in=c_in, channels=qch, act_func=act, graph_conv_type=gct, droprate=pdrop)
        values = params_in_field_order(pc, "st_blocks.0.", gct)

        def make(wsc=None):
            params = [None if t is None else t.clone().to(dev).requires_grad_(True) for t in values]
            wsc = wsc or ops.WorkspaceCache()
            return lambda x, training, seed, offset: ops.st_conv_block(x, gp, gt, cfg, params, training, seed, offset, wsc)
        return make
    assert kind == "head", kind
    from oracle import stgcn_oracle as orc
    hch = tuple(shape.get("channels", (128, 128)))
    hc = orc.OracleConfig(Kt=Kt, Ks=Ks, n_his=T_in + 4 * (Kt - 1), act_func=act, graph_conv_type=gct, droprate=pdrop,
                          blocks=[[1], [64, 16, 64], [64, 16, c_in], list(hch), [1]])
    hp = orc.random_params(hc, N, seed=3, dtype=torch.float32)
    names = ["tmp_conv1.causal_conv.weight", "tmp_conv1.causal_conv.bias", "tmp_conv1.align.align_conv.weight", "tmp_conv1.align.align_conv.bias",
             "tc1_ln.weight", "tc1_ln.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]
    assert tuple(hp["output.tmp_conv1.causal_conv.weight"].shape)[2] == T_in
    cfg = ops.HeadConfig(Ko=T_in, n_vertex=N, c_in=c_in, channels=hch, end_channel=1, act_func=act, droprate=pdrop)

    def make(wsc=None):
        params = [hp["output." + n].clone().to(dev).requires_grad_(True) for n in names]
        wsc = wsc or ops.WorkspaceCache()
        return lambda x, training, seed, offset: ops.output_block(x, cfg, params, training, seed, offset, wsc)
    return make


# What may come between the consumer Q and the producer P (tests/hook_trust_util.py): in each of them the buffer P receives is not, or no
# longer, the one Q's epilogue summed over, and P must form the row partials in a pass of its own
TAMPERS = ("inplace", "second_consumer", "batch_slice", "clone")


def run_consumer(L, dev, kind, shape, O, y, x, params, gp, gt, bcfg, plan, wsc, training, seed, offset, expect_rowstats, hook, tamper=None,
                 q_wsc=None, on_span=None):
    """The consumer half of run_block_case: Q(y) forward, the row-partial region of the producer's workspace filled with NaN, the backward
    from Q's output under the launch profile (on_span("hooked", "begin" / "end") around it); then -- unless a tamper is set -- Q alone on a
    copy of y (no hook offered) and the producer alone on the dy it received (its own ln_bwd_rowstats pass).  Fills hook["rowstat"],
    hook["rowstat_own"] ([B, T2, N, 2]; None with a tamper) and hook["err"]; returns dy (NCHW numpy), the gradient P received.
    tamper: "inplace" a tensor hook doubles the gradient in place between Q and P; "second_consumer" the loss adds (y * w).sum(); "batch_slice"
    Q consumes y[:1] (same address, another shape); "clone" Q consumes y.clone()."""
    c_in, channels, Kt, Ks, gct, act, N, B, T = O.args
    c2, T2 = channels[2], O.T2
    assert tamper is None or tamper in TAMPERS, tamper
    make = make_consumer(dev, kind, shape, c2, Kt, Ks, gct, act, N, T2, O.pdrop, gp, gt)
    region = lambda buf: buf[plan.ws_rowstat_b:plan.ws_rowstat_b + 2 * B * T2 * N]
    assert plan.ws_rowstat_b + 2 * B * T2 * N <= plan.ws_part      # (in front of the partial arena: the poisoning above does not reach it)
    on_span = on_span or (lambda name, edge: None)
    y.retain_grad()
    if tamper == "inplace":
        y.register_hook(lambda g: g.mul_(2))
    q_in = {"batch_slice": lambda: y[:1], "clone": lambda: y.clone()}.get(tamper, lambda: y)()
    out = make(q_wsc)(q_in, training, seed + 1, offset)
    rs = np.random.RandomState(23)
    dout = torch.from_numpy(rs.standard_normal(tuple(out.shape)).astype(np.float32)).to(dev)
    roots, seeds = [out], [dout]
    if tamper == "second_consumer":
        w = torch.from_numpy(rs.standard_normal(tuple(y.shape)).astype(np.float32)).to(dev)
        roots, seeds = [out, (y * w).sum()], [dout, None]
    # stgcn_stblock_ln_hook only describes the region and no forward kernel is handed ws_rowstat_b: whatever is not NaN afterwards, the
    # backward wrote
    region(wsc.buf).fill_(float("nan"))
    on_span("hooked", "begin")
    n_rs = rowstats_launched(L, lambda: torch.autograd.backward(roots, seeds))
    on_span("hooked", "end")
    rowstat = region(wsc.buf).cpu().numpy().reshape(B, T2, N, 2).copy()
    dy = y.grad.detach()
    err = {"hook.rowstat_nan": float(np.isnan(rowstat).sum())}
    if expect_rowstats is not None:
        err["grad_none_ok.hook_launches"] = float(abs(n_rs - expect_rowstats))
    hook["rowstat"], hook["rowstat_own"], hook["err"] = rowstat, None, err
    if tamper is not None:
        return dy.cpu().numpy()
    # Q alone on a leaf holding a copy of y (another address: nothing is offered, nothing taken): the epilogue must not change dx
    y_leaf = y.detach().clone().requires_grad_(True)
    assert y_leaf.stride() == y.stride() and y_leaf.data_ptr() != y.data_ptr()
    make()(y_leaf, training, seed + 1, offset).backward(dout)
    err["hook.dy_bitwise_vs_unhooked"] = float((y_leaf.grad.contiguous().view(torch.int32) != dy.contiguous().view(torch.int32)).sum().item())
    # the producer alone, the same dy as an external gradient: the partials of its own ln_bwd_rowstats pass
    prm3 = [None if t is None else t.detach().clone().requires_grad_(True) for t in params]
    x3 = x.detach().clone().requires_grad_(x.requires_grad)
    wsc3 = ops.WorkspaceCache()
    y3 = ops.st_conv_block(x3, gp, gt, bcfg, prm3, training, seed, offset, wsc3)
    region(wsc3.buf).fill_(float("nan"))
    n_own = rowstats_launched(L, lambda: y3.backward(dy.clone()))
    assert n_own == 1, n_own
    hook["rowstat_own"] = region(wsc3.buf).cpu().numpy().reshape(B, T2, N, 2).copy()
    return dy.cpu().numpy()


def run_block_pair(dev, *case, on_half=None, **kw):
    """One case as the stage tests launch it (debug_stages=True) and as production does (False, partial arena poisoned): the first
    run's keys, the second's as prod.<key>, and prod.bitwise_vs_debug (with a consumer: the hooked row partials count among the outputs)."""
    O = BlockOracle(*case[:9], gso=kw.get("gso"), pdrop=kw.get("pdrop", 0.5), ln_scale=kw.get("ln_scale"), data_seed=kw.get("data_seed", 11))
    out_d, out_p = {}, {}
    on_half = on_half or (lambda half, edge: None)      # (the launch-log test marks where each half's launches begin and end)
    span = lambda half: (lambda name, edge: on_half(half + "." + name, edge))      # (spans inside a half: the hooked backward of a consumer row)
    on_half("debug", "begin")
    err = run_block_case(dev, *case, debug_stages=True, oracle=O, outputs=out_d, on_span=span("debug"), **kw)
    on_half("debug", "end")
    on_half("prod", "begin")
    prod = run_block_case(dev, *case, debug_stages=False, oracle=O, outputs=out_p, on_span=span("prod"), **kw)
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
    if (key.startswith(("grad_none_ok", "chain.", "kink.")) or key.endswith("bitwise") or key in ("bitwise_vs_debug", "nan_elements")
            or key in ("hook.rowstat_nan", "hook.dy_bitwise_vs_unhooked")):
        return 0.0
    if key.startswith("info."):
        return float("inf")
    if key.startswith("oracle32."):
        return ORACLE32_TOL
    if key.startswith("fwd.") or key == "slice.y.tail":
        return FWD_TOL
    return GRAD_TOL      # bwd.*, grad.*, slice.*, hook.rowstat_*


def assert_errors(err):
    bad = {k: v for k, v in err.items() if not (v <= bar(k))}
    assert not bad, f"out of tolerance: {bad}\nall: {err}"


def worst_oracle32(err):
    return max(v for k, v in err.items() if k.startswith("oracle32."))


def report_block_errors(err, label, path):
    """Appends one JSON line per case to `path` (how profiles/block_stage_errors.md is made: tools/block_stage_report.py)."""
    with open(path, "a") as fh:
        fh.write(json.dumps({"case": label, **err}) + "\n")
