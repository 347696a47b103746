"""bf16 configurations (BASELINE.json configs[2], [4]): run one ST block with bfloat16 activations through the bound library (the CPU
emulator or the HIP library, same host code) and compare every stored tensor and every gradient with the bf16 statement of the stage
oracle (oracle/stblock_stages.py, QuantBf16: same rounding points, float64 accumulation).

Tolerances (stated here, asserted by `assert_bf16_errors`):
  * stored bf16 tensors: the HIP value and the oracle value are both bf16 numbers formed from sums that differ only in accumulation
    order / precision (fp32 vs float64), so they are EQUAL except where the sum sits on a rounding boundary (one bf16 ulp apart), and a
    flipped value then perturbs what is computed from it.  Bars: relative rms error <= 2^-9 (0.2 %: well below the bf16 quantisation
    noise of 2^-9 / sqrt(3) per element that the fp32 -> bf16 statement itself introduces) and max |diff| <= 2^-5 of the tensor's max.
  * fp32 outputs (LayerNorm statistics, parameter gradients): relative-to-max error <= 1e-2 (parameter gradients are sums over
    10^4 - 10^5 products of bf16 numbers: flips average out; measured values are ~1e-3).
"""
import ctypes as C

import numpy as np
import torch

from oracle import stblock_stages as st
from stgcn_amd import _lib, ops
from tests.block_util import param_slices
from tests.emu_util import block_case, nonsym_gso, params_in_field_order

Q = st.QuantBf16()
RMS_TOL = 2.0 ** -9
MAX_TOL = 2.0 ** -5
F32_TOL = 1e-2


def bf16_tensor(a: np.ndarray, dev) -> torch.Tensor:
    """float array -> torch.bfloat16 tensor holding RNE-rounded values."""
    bits = st.to_bf16_bits(a).astype(np.int16)
    return torch.from_numpy(bits).view(torch.bfloat16).to(dev)


def bf16_numpy(t: torch.Tensor) -> np.ndarray:
    return st.from_bf16_bits(t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16))


def seg_bf16(buf_f32: np.ndarray, off_floats: int, shape) -> np.ndarray:
    """A bf16 tensor stored inside a float32 plan buffer (offsets count 4-byte units)."""
    n = int(np.prod(shape))
    bits = buf_f32.view(np.uint16)[2 * off_floats:2 * off_floats + n]
    return st.from_bf16_bits(bits).reshape(shape)


def err_stored(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    rms_ref = max(1e-30, float(np.sqrt((ref ** 2).mean())))
    return dict(rms=float(np.sqrt((d ** 2).mean())) / rms_ref, max=float(d.max()) / max(1e-30, float(np.abs(ref).max())),
                mismatch=float((d > 0).mean()))


def _bits(a):
    """The bit patterns of an array of float32 / float64 values, for bitwise comparisons."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def run_block_case_bf16(dev, c_in, channels, Kt, Ks, gct, act, N, B, T, training, gso=None, seed=99, offset=3, pdrop=0.5, gc_form=None,
                        ln_scale=None, consumer=None, poison=True, need_dx=None, data_seed=11, oracle=None, outputs=None):
    """Returns ({name: stored-tensor error dict}, {name: relative-to-max error of an fp32 output}).
    poison: the arena of per-workgroup gradient partials is filled with NaN between forward and backward (as tests/block_util.py does for the
    fp32 production sequence -- bf16 always runs that sequence): a partial block a bf16 kernel fails to write reaches a gradient as NaN
    instead of as whatever the previous call left.  Keys prod.nan_elements (NaN among y, dx and the parameter gradients) and
    grad_none_ok.chain_words_* (sticky / ticket words of both workspaces), bar 0.
    need_dx: whether x requires grad (None: c_in > 1, what a model's first / later blocks do).  data_seed: seed of x and dy.
    oracle: a dict shared between runs of one case (run_block_pair_bf16): the oracle's forward and both backwards are computed once;
    outputs: a dict that receives y, dx and the parameter gradients (numpy) for bitwise comparisons between runs.
    Slice keys (module docstring of tests/test_gpu_bf16_paths.py): slice.tc1_w.k<k>, slice.tc2_w.k<k>, slice.gc_w.k<k>, slice.ln_w.tail,
    slice.ln_b.tail among the fp32 outputs (each normalised by THAT slice's max, bar F32_TOL), slice.y.tail, slice.dx.t0, slice.dx.tlast
    among the stored tensors (err_stored over the slice, bars RMS_TOL / MAX_TOL); info.slice_ratio.<slice>: max |slice| / max |whole
    tensor| of the PURE oracle (its own saved tensors), a condition on the inputs alone (assert_slice_ratios).
    gc_form: "poly" (slab-resident graph conv) / "recursion" (tiled path); None = whichever the plan selects.
    ln_scale = (g, b): the block's LayerNorm parameters are drawn as gamma = g * U(-1, 1), beta = b * U(-1, 1) (the
    backward rebuilds sum g * xhat from dy * (y - keep_scale * beta) with y in bf16, which amplifies y's rounding by |beta| / |gamma xhat|).
    consumer = "block" / "head": the block's output feeds a second fused module and dy is what THAT module's backward produces, so the
    LayerNorm-backward row partials come out of the consumer's hook epilogue (tc1_bwd_kernel / the head's transposed conv) instead of
    ln_bwd_rowstats_kernel; everything is then checked as for an external dy."""
    L = _lib.lib()
    cfg, p = block_case(c_in, channels, Kt, Ks, gct, act, N, B, T)
    if ln_scale is not None:
        rl = np.random.RandomState(77)
        shp = tuple(p["st_blocks.0.tc2_ln.weight"].shape)
        p["st_blocks.0.tc2_ln.weight"] = torch.from_numpy((ln_scale[0] * rl.uniform(-1, 1, shp)).astype(np.float32))
        p["st_blocks.0.tc2_ln.bias"] = torch.from_numpy((ln_scale[1] * rl.uniform(-1, 1, shp)).astype(np.float32))
    if gso is None:
        gso = nonsym_gso(N, 5)
    need_dx = c_in > 1 if need_dx is None else bool(need_dx)
    oracle = {} if oracle is None else oracle
    rs = np.random.RandomState(data_seed)
    x_np = Q(rs.standard_normal((B, c_in, T, N)))                     # bf16 values, logical NCHW
    T2 = T - 2 * (Kt - 1)
    dy_np = Q(rs.standard_normal((B, channels[2], T2, N)))
    bcfg = ops.BlockConfig(Kt=Kt, Ks=Ks, n_vertex=N, c_in=c_in, channels=tuple(channels), act_func=act, graph_conv_type=gct, droprate=pdrop)
    gp, gt = ops.gso_prepare(torch.from_numpy(gso).to(dev), ops.graph_terms(bcfg))
    params = [None if t is None else t.clone().to(dev).requires_grad_(True) for t in params_in_field_order(p, "st_blocks.0.", gct)]
    x = bf16_tensor(x_np, dev).requires_grad_(need_dx)
    desc = ops.make_desc(bcfg, B, T, training, need_dx, dtype=torch.bfloat16)
    plan = ops.query_plan(desc)
    wsc = ops.WorkspaceCache()
    y = ops.st_conv_block(x, gp, gt, bcfg, params, training, seed, offset, wsc)
    assert y.dtype == torch.bfloat16
    if poison:
        # the arena of per-workgroup gradient partials ONLY: the packed weights, the chain words and the row partials of a hooked
        # LayerNorm live in front of it in the same buffer (tests/test_emu_bf16_paths.py checks that for the bf16 plans)
        assert wsc.buf.numel() >= plan.ws_part + plan.part_floats
        wsc.buf[plan.ws_part:plan.ws_part + plan.part_floats].fill_(float("nan"))
    hooked = None
    if consumer is None:
        y.backward(bf16_tensor(dy_np, dev))
    else:
        y.retain_grad()
        L.dll.stgcn_profile_enable(1)
        if consumer == "block":
            _, pc = block_case(channels[2], channels, Kt, Ks, gct, act, N, B, T2, seed=8)
            ccfg = ops.BlockConfig(Kt=Kt, Ks=Ks, n_vertex=N, c_in=channels[2], channels=tuple(channels), act_func=act, graph_conv_type=gct, droprate=pdrop)
            cparams = [None if t is None else t.clone().to(dev).requires_grad_(True) for t in params_in_field_order(pc, "st_blocks.0.", gct)]
            out = ops.st_conv_block(y, gp, gt, ccfg, cparams, training, seed + 1, offset, ops.WorkspaceCache())
            out.backward(bf16_tensor(Q(rs.standard_normal(tuple(out.shape))), dev))
        else:
            from oracle import stgcn_oracle as orc
            hc = orc.OracleConfig(Kt=Kt, Ks=Ks, n_his=12, act_func=act, graph_conv_type=gct, droprate=pdrop,
                                  blocks=[[1], [64, 16, 64], [64, 16, channels[2]], [128, 128], [1]])
            hp_ = {k: v for k, v in orc.random_params(hc, N, seed=3, dtype=torch.float32).items() if k.startswith("output.")}
            hn = ["tmp_conv1.causal_conv.weight", "tmp_conv1.causal_conv.bias", "tmp_conv1.align.align_conv.weight", "tmp_conv1.align.align_conv.bias",
                  "tc1_ln.weight", "tc1_ln.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]
            assert tuple(hp_["output.tmp_conv1.causal_conv.weight"].shape)[2] >= 1
            hparams = [hp_["output." + n].clone().to(dev).requires_grad_(True) for n in hn]
            Ko = tuple(hp_["output.tmp_conv1.causal_conv.weight"].shape)[2]
            assert Ko == T2, (Ko, T2)       # (the head consumes the whole remaining time axis: T - 2 (Kt - 1) must be the fixture's Ko)
            hcfg = ops.HeadConfig(Ko=Ko, n_vertex=N, c_in=channels[2], channels=(128, 128), end_channel=1, act_func=act, droprate=pdrop)
            out = ops.output_block(y, hcfg, hparams, training, seed + 1, offset, ops.WorkspaceCache())
            out.backward(torch.from_numpy(rs.standard_normal(tuple(out.shape)).astype(np.float32)).to(dev))
        buf = C.create_string_buffer(1 << 16)
        L.dll.stgcn_profile_collect(buf, len(buf))
        L.dll.stgcn_profile_enable(0)
        import json
        launched = json.loads(buf.value.decode())
        n_rs = sum(v["calls"] for k, v in launched.items() if k.startswith("ln_bwd_rowstats"))
        hooked = n_rs == (1 if consumer == "block" else 0)      # (a consumer BLOCK runs the pass for its own LayerNorm: its dy came from outside)
        dy_np = bf16_numpy(y.grad)
    if str(dev).startswith("cuda"):
        torch.cuda.synchronize()

    cl = lambda a: np.ascontiguousarray(a.transpose(0, 2, 3, 1)).astype(np.float64)
    keep = None
    if training:
        ks = ops.dropout_mask(B * T2 * N * channels[2], pdrop, seed, offset, dev).cpu().numpy().reshape(B, T2, N, channels[2])
        keep = (ks > 0).astype(np.float64)
    g64 = gso.astype(np.float64)
    bp = st.block_params_np(p, "st_blocks.0.", gct, np.float64)
    if gc_form is None:
        gc_form = "recursion" if plan.tiled_gc else "poly"
    if "fwd" not in oracle:
        y_ref, sv = st.stblock_fwd(cl(x_np), g64, bp, Kt, c_in, channels, gct, act, keep, pdrop, q=Q, gc_form=gc_form, ln_from_stored=N > 448)
        # the same block in the fp64 statement: how far the bf16 configuration is from the reference arithmetic (reported, loosely bounded)
        y64, _ = st.stblock_fwd(cl(x_np), g64, bp, Kt, c_in, channels, gct, act, keep, pdrop)
        oracle["fwd"] = (y_ref, sv, y64, None if keep is None else keep.copy())
    y_ref, sv, y64, keep0 = oracle["fwd"]
    assert (keep is None) == (keep0 is None) and (keep is None or np.array_equal(keep, keep0))      # (a shared oracle: the same mask in every run)

    ws = wsc.buf.cpu().numpy()
    saved = torch.empty(plan.saved_floats, device=dev)
    y2 = torch.empty(B, T2, N, channels[2], dtype=torch.bfloat16, device=dev)
    pst = ops._param_struct(_lib.StblockParams, [None if t is None else t.detach() for t in params])
    x_cl = x.detach().permute(0, 2, 3, 1).contiguous()
    ws2 = torch.empty(plan.ws_floats, device=dev)
    stream = torch.cuda.current_stream().cuda_stream if str(dev).startswith("cuda") else None
    L.check(L.dll.stgcn_stblock_forward(C.byref(desc), C.byref(pst), x_cl.data_ptr(), gp.data_ptr(), y2.data_ptr(), saved.data_ptr(),
                                        ws2.data_ptr(), seed, offset, None, stream), "fwd")
    if str(dev).startswith("cuda"):
        torch.cuda.synchronize()
    svn = saved.cpu().numpy()
    T1 = plan.T1
    c0, c1, c2 = channels
    terms = 2 if gct == "graph_conv" else Ks
    stored, f32 = {}, {}
    # chained launches: the sticky error word (a bounded wait gave up) of both workspaces, and ticket / finished-workgroup words re-armed
    for nm, buf in (("autograd", wsc.buf), ("direct", ws2)):
        cw = buf[plan.ws_chain:plan.ws_chain + 4].view(torch.int32).cpu().numpy()
        f32[f"grad_none_ok.chain_words_{nm}"] = float(abs(cw[:3]).sum())
    if hooked is not None:
        f32["grad_none_ok.hook_epilogue_used"] = 0.0 if hooked else 1.0      # (tolerance 0: the consumer's epilogue wrote the row partials, no ln_bwd_rowstats launch)
    if not plan.recompute_tc1:
        stored["fwd.U1"] = err_stored(seg_bf16(svn, plan.sv_U1, (B, T1, N, c0)), sv["U1"])
        stored["fwd.S1"] = err_stored(seg_bf16(svn, plan.sv_S1, (B, T1, N, c0)), sv["S1"])
    stored["fwd.A"] = err_stored(seg_bf16(svn, plan.sv_A, (B, T1, N, c1)), sv["A"])
    per = B * T1 * N * c1 // 2      # 4-byte units per term: the X_k follow each other without padding (c1 = 16 elements per row)
    for k in range(1, terms):
        stored[f"fwd.X{k}"] = err_stored(seg_bf16(svn, plan.sv_Xk + (k - 1) * per, (B, T1, N, c1)), sv["Xs"][k])
    stored["fwd.G"] = err_stored(seg_bf16(svn, plan.sv_G, (B, T1, N, c1)), sv["G"])
    if plan.stored_US2:      # (only when LayerNorm runs as a separate pass over the stored gate inputs: more than 448 nodes)
        stored["fwd.U2"] = err_stored(seg_bf16(svn, plan.sv_U2, (B, T2, N, c2)), Q(sv["U2"]))
        stored["fwd.S2"] = err_stored(seg_bf16(svn, plan.sv_S2, (B, T2, N, c2)), Q(sv["S2"]))
    stored["fwd.y"] = err_stored(cl(bf16_numpy(y)), y_ref)
    stored["fwd.y_vs_fp64"] = err_stored(cl(bf16_numpy(y)), y64)          # (reported; bounded loosely below)
    f32["fwd.mean"] = float(np.abs(svn[plan.sv_mean:plan.sv_mean + B * T2].reshape(B, T2) - sv["mean"]).max() / max(1e-30, np.abs(sv["mean"]).max() + 1e-3))
    # the same error in units of the slab's standard deviation: a slab whose mean happens to lie near zero does not inflate it (bar: fwd.rstd's)
    f32["fwd.mean_over_std"] = float((np.abs(svn[plan.sv_mean:plan.sv_mean + B * T2].reshape(B, T2) - sv["mean"]) * sv["rstd"]).max())
    f32["info.ref_abs_mean_max"], f32["info.ref_std_min"] = float(np.abs(sv["mean"]).max()), float((1.0 / sv["rstd"]).min())
    f32["fwd.rstd"] = float(np.abs(svn[plan.sv_rstd:plan.sv_rstd + B * T2].reshape(B, T2) / sv["rstd"] - 1).max())
    f32["fwd.y_repeat_bitwise"] = float((y2.view(torch.int16) != y.detach().permute(0, 2, 3, 1).contiguous().view(torch.int16)).sum().item())
    # Backward: checked on the HIP path's OWN saved tensors ("teacher forcing").  ReLU is discontinuous: where a stored G sits on the
    # rounding boundary next to zero the two forwards may disagree about the mask, and a flipped mask changes the gradient entering the
    # graph conv by O(1) in that element -- a property of the forward's rounding, not of the backward kernels under test.
    svh = dict(sv)
    if not plan.recompute_tc1:
        svh["U1"], svh["S1"] = seg_bf16(svn, plan.sv_U1, (B, T1, N, c0)), seg_bf16(svn, plan.sv_S1, (B, T1, N, c0))
        svh["H1"] = st._gate(svh["U1"], svh["S1"], act)
    svh["A"] = seg_bf16(svn, plan.sv_A, (B, T1, N, c1))
    svh["Xs"] = [svh["A"]] + [seg_bf16(svn, plan.sv_Xk + (k - 1) * per, (B, T1, N, c1)) for k in range(1, terms)]
    svh["G"] = seg_bf16(svn, plan.sv_G, (B, T1, N, c1))
    svh["U2"], svh["S2"], svh["H2"] = st.tconv_fwd(svh["G"], sv["W2"], st.fold_tconv(bp["tc2_w"], bp["tc2_b"], bp["tc2_aw"], bp["tc2_ab"], c1, c2, Kt)[1],
                                                   Kt, c2, act, Q)      # what tc2_bwd_kernel recomputes from the stored G
    svh["y"] = cl(bf16_numpy(y))
    svh["mean"] = svn[plan.sv_mean:plan.sv_mean + B * T2].reshape(B, T2).astype(np.float64)
    svh["rstd"] = svn[plan.sv_rstd:plan.sv_rstd + B * T2].reshape(B, T2).astype(np.float64)
    import hashlib
    digest = lambda *arrs: hashlib.sha1(b"".join(np.ascontiguousarray(a).tobytes() for a in arrs)).hexdigest()
    fkey = ("forced", digest(svh["U1"], svh["S1"], *svh["Xs"], svh["G"], svh["mean"], svh["rstd"], svh["y"], dy_np))      # (the forced oracle depends on what the library saved)
    if fkey not in oracle:
        stages = {}
        dx_ref, g_ref = st.stblock_bwd(cl(dy_np), svh, g64, bp, Kt, c_in, channels, gct, act, pdrop, need_dx=need_dx, q=Q, gc_form=gc_form,
                                       stages=stages)
        oracle[fkey] = (dx_ref, g_ref, stages)
    dx_ref, g_ref, stages = oracle[fkey]
    # How much of the backward the teacher forcing hides: the ReLU-mask flip rate between the two forwards, and the
    # gradients against the PURE oracle (its own saved tensors, no forcing), bounded in rms: a flipped mask element changes the gradient
    # entering the graph conv by O(1) there, so the un-forced error is ~sqrt(flip rate) in rms, not a kernel defect.
    flip = float(((svh["G"] > 0) != (np.asarray(sv["G"]) > 0)).mean())
    f32["relu_flip_rate"] = flip
    ukey = ("unforced", digest(dy_np))
    if ukey not in oracle:
        oracle[ukey] = st.stblock_bwd(cl(dy_np), sv, g64, bp, Kt, c_in, channels, gct, act, pdrop, need_dx=need_dx, q=Q, gc_form=gc_form)
    dx_u, g_u = oracle[ukey]
    rms = lambda a: float(np.sqrt((np.asarray(a, np.float64) ** 2).mean()))
    if need_dx:
        f32["unforced_rms.dx"] = rms(cl(bf16_numpy(x.grad)) - dx_u) / max(1e-30, rms(dx_u))
    worst = 0.0
    for name, prm in zip(_lib.PARAM_FIELDS, params):
        if prm is not None and prm.grad is not None and g_u.get(name) is not None:
            worst = max(worst, rms(prm.grad.cpu().numpy().astype(np.float64) - g_u[name].reshape(prm.shape)) / max(1e-30, rms(g_u[name])))
    f32["unforced_rms.param_grads_worst"] = worst
    stored["bwd.dYg"] = err_stored(seg_bf16(ws, plan.ws_dYg, (B, T1, N, c1)), stages["dYg"])
    stored["bwd.dA"] = err_stored(seg_bf16(ws, plan.ws_dA, (B, T1, N, c1)), stages["dA"])
    dx = cl(bf16_numpy(x.grad)) if need_dx else None
    if need_dx:
        stored["bwd.dx"] = err_stored(dx, dx_ref)
    else:
        f32["grad_none_ok.dx"] = 0.0 if x.grad is None else 1.0
    rel = lambda got, ref: float(np.abs(got - ref).max() / max(1e-30, np.abs(ref).max()))
    got, shaped, shaped_u = {}, {}, {}
    for name, prm in zip(_lib.PARAM_FIELDS, params):
        ref = g_ref[name]
        if prm is None:
            continue
        if ref is None:
            f32["grad_none_ok." + name] = 0.0 if prm.grad is None else 1.0
            continue
        f32["grad." + name] = rel(prm.grad.cpu().numpy().astype(np.float64), ref.reshape(prm.shape)) if prm.grad is not None else float("inf")
        if prm.grad is not None:
            got[name], shaped[name], shaped_u[name] = prm.grad.cpu().numpy(), ref.reshape(prm.shape), g_u[name].reshape(prm.shape)
    # ---- slices: a whole-tensor maximum hides a wrong tap / term / ragged tile / edge step.  Every element of a tap or term slice sums over the
    # same rows as the whole tensor, every ln_w element over the same B * T2 slabs, tail or not: the per-element statistics are those the
    # whole-tensor bars were stated for, only the normaliser shrinks -- and info.slice_ratio.* bounds by how much (assert_slice_ratios)
    amax = lambda a: float(np.abs(a).max())
    y_cl = svh["y"]
    for key, name, idx in param_slices(shaped, Kt, N, gct):
        f32[key] = rel(got[name][idx].astype(np.float64), shaped[name][idx]) if name in got else float("inf")
        if name in got:
            f32["info.slice_ratio." + key[len("slice."):]] = amax(shaped_u[name][idx]) / max(1e-30, amax(shaped_u[name]))
    tail = N - N % 16
    if N % 16:
        stored["slice.y.tail"] = err_stored(y_cl[:, :, tail:], y_ref[:, :, tail:])
        f32["info.slice_ratio.y.tail"] = amax(y_ref[:, :, tail:]) / max(1e-30, amax(y_ref))
    if need_dx:
        for nm, t in (("t0", 0), ("tlast", T - 1)):
            stored[f"slice.dx.{nm}"] = err_stored(dx[:, t], dx_ref[:, t])
            f32[f"info.slice_ratio.dx.{nm}"] = amax(dx_u[:, t]) / max(1e-30, amax(dx_u))
    outs = {"y": y_cl.astype(np.float32), **({"dx": dx.astype(np.float32)} if need_dx else {}), **{"grad." + k: v for k, v in got.items()}}
    if poison:
        f32["prod.nan_elements"] = float(sum(int(np.isnan(v).sum()) for v in outs.values()))
    if outputs is not None:
        outputs.update(outs)
    return stored, f32


def run_block_pair_bf16(dev, *case, on_half=None, **kw):
    """One case twice with a shared oracle: the partial-sum arena as the forward left it ("clean"), then filled with NaN ("poisoned").  Returns
    the poisoned run's keys, the clean run's as clean.<key>, and prod.bitwise_clean_vs_poisoned: elements of y, dx and all parameter
    gradients whose bits differ between the two runs (bar 0: the bf16 counterpart of block_util's prod.bitwise_vs_debug)."""
    oracle, out_c, out_p = {}, {}, {}
    on_half = on_half or (lambda half, edge: None)      # (the launch-log test marks where each half's launches begin and end)
    on_half("clean", "begin")
    stored_c, f32_c = run_block_case_bf16(dev, *case, poison=False, oracle=oracle, outputs=out_c, **kw)
    on_half("clean", "end")
    on_half("poisoned", "begin")
    stored, f32 = run_block_case_bf16(dev, *case, poison=True, oracle=oracle, outputs=out_p, **kw)
    on_half("poisoned", "end")
    stored.update({"clean." + k: v for k, v in stored_c.items()})
    f32.update({"clean." + k: v for k, v in f32_c.items() if not k.startswith("info.")})
    assert out_c.keys() == out_p.keys()
    f32["prod.bitwise_clean_vs_poisoned"] = float(sum(int((_bits(out_c[k]) != _bits(out_p[k])).sum()) for k in out_c))
    return stored, f32


def slice_ratios(f32):
    return {k[len("info.slice_ratio."):]: v for k, v in f32.items() if k.startswith("info.slice_ratio.")}


def assert_slice_ratios(f32, floor=0.25):
    """The condition under which the slice keys may share the whole-tensor bars: every slice's max |ref| is at least `floor` of its whole
    tensor's (the oracle alone, on the case's inputs).  A row that misses it gets another data seed, never another bar."""
    r = slice_ratios(f32)
    assert r and min(r.values()) >= floor, {k: v for k, v in r.items() if v < floor} or "no slice keys"


def bf16_bar(k):
    """The bar an fp32-output key is held to."""
    if k.startswith("clean."):
        k = k[len("clean."):]
    # (LayerNorm statistics are fp32 sums, but of values downstream of bf16 tensors in which a few elements differ by one ulp)
    # relu_flip_rate: measured 0 - 3e-4 (elements of G within one bf16 ulp of zero); un-forced gradients: rms error <= 5 % (measured ~1 %)
    if k.startswith("grad_none_ok") or k.endswith("bitwise") or k in ("prod.nan_elements", "prod.bitwise_clean_vs_poisoned"):
        return 0.0
    if k.startswith("info."):
        return float("inf")
    return (1e-3 if k in ("fwd.mean", "fwd.rstd", "fwd.mean_over_std") else 2e-3 if k == "relu_flip_rate" else
            5e-2 if k.startswith("unforced_rms") else F32_TOL)


def report_bf16_paths(stored, f32, label, path):
    """Appends one JSON line per row with every key to `path` (how profiles/bf16_block_stage_errors.md is made: tools/bf16_stage_report.py)."""
    import json
    with open(path, "a") as fh:
        fh.write(json.dumps({"case": label, "f32": f32, "stored": stored}) + "\n")


def assert_bf16_errors(stored, f32, report_only=()):
    """report_only: keys that are reported but not held to their bar (fwd.mean of a row with fewer than 4 (b, t2) slabs, whose normaliser
    is a maximum over that few |mean|: such a row is held to fwd.mean_over_std, tests/test_gpu_bf16_paths.py)."""
    import json, os
    if os.environ.get("STGCN_BF16_REPORT"):      # (GPU passes: the measured flip rates / un-forced errors go into profiles/)
        with open(os.environ["STGCN_BF16_REPORT"], "a") as fh:
            fh.write(json.dumps({"f32": {k: v for k, v in f32.items() if "flip" in k or "unforced" in k},
                                 "stored_rms": {k: round(v["rms"], 6) for k, v in stored.items()}}) + "\n")
    bad = {}
    for k, e in stored.items():
        if k.endswith("_vs_fp64"):      # (clean.* keys: the same bars)
            if not (e["rms"] <= 3e-2):          # bf16 storage + bf16 operands vs exact arithmetic: ~1 % rms on unit-variance outputs
                bad[k] = e
            continue
        if not (e["rms"] <= RMS_TOL and e["max"] <= MAX_TOL):
            bad[k] = e
    for k, v in f32.items():
        if k in report_only or (k.startswith("clean.") and k[len("clean."):] in report_only):
            continue
        if not (v <= bf16_bar(k)):
            bad[k] = v
    assert not bad, f"out of tolerance: {bad}\nstored: {stored}\nf32: {f32}"


def run_head_case_bf16(dev, N, B, c_in=64, channels=(128, 128), Ko=4, act="glu", training=True, seed=5, offset=9, pdrop=0.5, T=None, need_dx=True):
    """The output head with bf16 activations against outblock_fwd / outblock_bwd of the stage oracle (q = QuantBf16).
    T: length of the input's time axis (None: Ko, one output step); need_dx = False: x does not require grad, no input gradient is formed."""
    T = Ko if T is None else T
    T1 = T - Ko + 1
    from oracle import stgcn_oracle as orc
    cfg = orc.OracleConfig(Kt=3, Ks=3, n_his=12, act_func=act, graph_conv_type="cheb_graph_conv", droprate=pdrop,
                           blocks=[[1], [64, 16, 64], [64, 16, c_in], list(channels), [1]])
    full = orc.random_params(cfg, N, seed=3, dtype=torch.float32)
    p = {k: v for k, v in full.items() if k.startswith("output.")}
    names = ["tmp_conv1.causal_conv.weight", "tmp_conv1.causal_conv.bias", "tmp_conv1.align.align_conv.weight", "tmp_conv1.align.align_conv.bias",
             "tc1_ln.weight", "tc1_ln.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]
    params = [p["output." + n].clone().to(dev).requires_grad_(True) for n in names]
    rs = np.random.RandomState(4)
    x_np = Q(rs.standard_normal((B, c_in, T, N)))
    dout_np = rs.standard_normal((B, 1, T1, N)).astype(np.float32)
    hcfg = ops.HeadConfig(Ko=Ko, n_vertex=N, c_in=c_in, channels=tuple(channels), end_channel=1, act_func=act, droprate=pdrop)
    x = bf16_tensor(x_np, dev).requires_grad_(bool(need_dx))
    wsc = ops.WorkspaceCache()
    out = ops.output_block(x, hcfg, params, training, seed, offset, wsc)
    assert out.dtype == torch.float32 and out.shape == (B, 1, T1, N)
    out.backward(torch.from_numpy(dout_np).to(dev))
    if str(dev).startswith("cuda"):
        torch.cuda.synchronize()
    cl = lambda a: np.ascontiguousarray(a.transpose(0, 2, 3, 1)).astype(np.float64)
    keep = None
    c0, c1 = channels
    if training:
        ks = ops.dropout_mask(B * T1 * N * c1, pdrop, seed, offset, dev).cpu().numpy().reshape(B, T1, N, c1)
        keep = (ks > 0).astype(np.float64)
    hp = st.head_params_np(p, np.float64)
    out_ref, sv = st.outblock_fwd(cl(x_np), hp, Ko, c_in, channels, act, keep, pdrop, q=Q)
    dx_ref, g_ref = st.outblock_bwd(dout_np[:, 0].astype(np.float64), sv, hp, Ko, c_in, channels, act, pdrop, bool(need_dx), q=Q)
    rel = lambda got, ref: float(np.abs(got - ref).max() / max(1e-30, np.abs(ref).max()))
    stored = {"head.dx": err_stored(cl(bf16_numpy(x.grad)), dx_ref)} if need_dx else {}
    f32 = {"head.out": rel(out.detach().cpu().numpy()[:, 0].astype(np.float64), out_ref)}
    if not need_dx:
        f32["grad_none_ok.head.dx"] = 0.0 if x.grad is None else 1.0
    keys = ["tc_w", "tc_b", "tc_aw", "tc_ab", "ln_w", "ln_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b"]
    for k, prm in zip(keys, params):
        ref = g_ref[k]
        if ref is None:
            f32["grad_none_ok.head." + k] = 0.0 if prm.grad is None else 1.0
        else:
            f32["grad.head." + k] = rel(prm.grad.cpu().numpy().astype(np.float64), np.asarray(ref).reshape(prm.shape)) if prm.grad is not None else float("inf")
    return stored, f32
