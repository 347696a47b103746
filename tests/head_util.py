"""Stage-level harness of the fused output head (the head's twin of tests/gpu_util.py::run_block_case): run one head through the bound
library -- the CPU emulator for "cpu", the HIP library for "cuda:0" -- and compare every saved tensor, every intermediate gradient, dx
and the ten parameter gradients with the float64 stage oracle (oracle/stblock_stages.py: outblock_fwd / outblock_bwd).

Error keys, in the order a fault would propagate (the first key out of tolerance names the stage to look at):
  fwd.U, fwd.S, fwd.mean, fwd.rstd_rel, fwd.yln, fwd.hd, fwd.out   absolute (rstd: relative), bar FWD_TOL; fwd.out also OUT_TIGHT
  fwd.out_repeat_bitwise, chain.*                                  a second forward into the harness's own buffers: bar 0
  bwd.dh1, bwd.dyln, bwd.dZ, bwd.dx                                max error / max |ref|, bar GRAD_TOL; bwd.dx also GRAD_TIGHT
  grad.<param>                                                     max error / max |ref| of the whole tensor, bars GRAD_TOL and GRAD_TIGHT
  slice.tc_w.k<k>                                                  the same over tap k alone (tc_w[:, :, k]), normalised by THAT slice's max
  slice.ln_w.tail / slice.ln_b.tail                                over the last ragged 16-node tile (N - N % 16 .. N), when N % 16 != 0
  loss.rel                                                         fused MSE loss (ops.mse_backward) against the oracle's, relative
  info.relu_units_*, kink.*                                        hidden units at the ReLU kink (see run_head_case): the counts, and by how
                                                                   much they exceed their bounds (bar 0)
  oracle32.<grad / slice key>                                      the SAME metric for the stage oracle run in np.float32 against its float64
                                                                   run: what fp32 rounding alone does to it.  Bar GRAD_TOL / 4 -- a case whose
                                                                   inputs nearly cancel a slice gets another seed, never another bar.
(tc_aw / tc_ab, the folded align conv, are tensors of their own among the ten: grad.tc_aw / grad.tc_ab.)
"""
import ctypes as C
import json

import numpy as np
import torch

from oracle import stblock_stages as st
from oracle import stgcn_oracle as orc
from stgcn_amd import _lib, ops
from tests.gpu_util import FWD_TOL, GRAD_TOL

OUT_TIGHT = 5e-5      # tests/test_emu_head.py: |out - oracle|
GRAD_TIGHT = 2e-4     # tests/test_emu_head.py: dx and the parameter gradients, relative to the tensor's max
ORACLE32_TOL = GRAD_TOL / 4

NAMES = ["tmp_conv1.causal_conv.weight", "tmp_conv1.causal_conv.bias", "tmp_conv1.align.align_conv.weight", "tmp_conv1.align.align_conv.bias",
         "tc1_ln.weight", "tc1_ln.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]
KEYS = ["tc_w", "tc_b", "tc_aw", "tc_ab", "ln_w", "ln_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b"]


def bind(dev):
    if str(dev) == "cpu":
        from tests.emu_util import bind_emulator
        return bind_emulator()
    from tests.gpu_util import bind_hip
    return bind_hip()


def rel(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(1e-30, float(np.abs(ref).max())))


def head_inputs(c_in, channels, Ko, N, B, T, act, pdrop=0.5, param_seed=5, data_seed=2):
    """Parameters (reference state_dict names, fp32 torch; tc1_ln.bias of the size of the normalised values so that dbeta / dgamma and the
    forward's beta are exercised), x and dout (standard normal, logical NCHW) and a target for the fused-loss form."""
    cfg = orc.OracleConfig(Kt=3, Ks=3, n_his=Ko, act_func=act, droprate=pdrop, blocks=[[c_in], list(channels), [1]])
    assert cfg.n_st_blocks == 0 and cfg.Ko == Ko
    p = {k: v for k, v in orc.random_params(cfg, N, seed=param_seed, dtype=torch.float32).items() if k.startswith("output.")}
    rs = np.random.RandomState(data_seed)
    T1 = T - Ko + 1
    x_np = rs.standard_normal((B, c_in, T, N)).astype(np.float32)
    dout_np = rs.standard_normal((B, 1, T1, N)).astype(np.float32)
    p["output.tc1_ln.bias"] = torch.from_numpy(rs.uniform(-0.5, 0.5, (N, channels[0])).astype(np.float32))
    target_np = rs.standard_normal((B, 1, T1, N)).astype(np.float32)
    return p, x_np, dout_np, target_np


def grad_metrics(got, ref, Ko, N, prefix=""):
    """{key: error} of the parameter gradients `got` against `ref` (dicts keyed like head_params_np; numpy arrays shaped like `ref`):
    per tensor, per tap of tc_w, and over the last ragged 16-node tile of the LayerNorm parameters."""
    err = {}
    for k in KEYS:
        if ref[k] is None:
            continue
        err[f"{prefix}grad.{k}"] = rel(got[k], ref[k]) if got[k] is not None else float("inf")
    if got["tc_w"] is not None:
        for k in range(Ko):
            err[f"{prefix}slice.tc_w.k{k}"] = rel(got["tc_w"][:, :, k], ref["tc_w"][:, :, k])
    if N % 16:
        for k in ("ln_w", "ln_b"):
            if got[k] is not None:
                err[f"{prefix}slice.{k}.tail"] = rel(got[k][N - N % 16:], ref[k][N - N % 16:])
    return err


def run_head_case(dev, c_in, channels, Ko, N, B, T, act, training, need_dx=True, seed=77, offset=5, pdrop=0.5, loss_scale=None,
                  param_seed=5, data_seed=2):
    """Returns the dict of errors described in the module docstring.  loss_scale: run the backward through ops.mse_backward (the fused
    MSE loss of stgcn_outblock_backward_loss) with that grad_scale instead of an external dout."""
    L = bind(dev)
    cuda = str(dev).startswith("cuda")
    c0, c1 = channels
    T1 = T - Ko + 1
    p, x_np, dout_np, target_np = head_inputs(c_in, channels, Ko, N, B, T, act, pdrop, param_seed, data_seed)
    hcfg = ops.HeadConfig(Ko=Ko, n_vertex=N, c_in=c_in, channels=(c0, c1), end_channel=1, act_func=act, droprate=pdrop)
    assert ops.head_supported(hcfg)
    params = [p["output." + n].clone().to(dev).requires_grad_(True) for n in NAMES]
    x = torch.from_numpy(x_np).to(dev).requires_grad_(bool(need_dx))
    wsc = ops.WorkspaceCache()
    out = ops.output_block(x, hcfg, params, training, seed, offset, wsc)
    assert out.shape == (B, 1, T1, N) and out.dtype == torch.float32
    err = {"chain.autograd": float(ops.head_chain_status(hcfg, B, T, wsc))}
    loss = None
    if loss_scale is None:
        out.backward(torch.from_numpy(dout_np).to(dev))
    else:
        assert ops._head_node_of(out) is not None
        loss = ops.mse_backward(out, torch.from_numpy(target_np).to(dev), grad_scale=loss_scale)
    if cuda:
        torch.cuda.synchronize()

    # ---- the oracle, float64 and float32, on the library's own dropout mask
    cl = lambda a: np.ascontiguousarray(a.transpose(0, 2, 3, 1))
    keep = None
    if training:
        keep = (ops.dropout_mask(B * T1 * N * c1, pdrop, seed, offset, dev).cpu().numpy().reshape(B, T1, N, c1) > 0)

    def oracle_fwd(dt):
        hp = st.head_params_np(p, dt)
        o, sv = st.outblock_fwd(cl(x_np).astype(dt), hp, Ko, c_in, channels, act, None if keep is None else keep.astype(dt), pdrop)
        return hp, o, sv

    def oracle_bwd(dt, hp, o, sv):
        if loss_scale is None:
            d, lv = dout_np[:, 0].astype(dt), None
        else:      # nn.MSELoss() (mean over every prediction) scaled by grad_scale in the gradient only
            diff = o - target_np[:, 0].astype(dt)
            d, lv = (2.0 * loss_scale / diff.size) * diff, float((diff.astype(np.float64) ** 2).mean())
        stages = {}
        dx, g = st.outblock_bwd(d.astype(dt), sv, hp, Ko, c_in, channels, act, pdrop, bool(need_dx), stages=stages)
        return dx, g, stages, lv

    hp64, out_ref, sv = oracle_fwd(np.float64)
    hp32, out32, sv32 = oracle_fwd(np.float32)

    # ---- the saved tensors: the autograd ctx keeps `saved`; fetch it again through a second forward into our own buffers
    desc = ops.make_head_desc(hcfg, B, T, training, bool(need_dx))
    plan = ops.query_head_plan(desc)
    assert plan.T1 == T1 and plan.rows == B * T1 * N
    saved = torch.empty(plan.saved_floats, device=dev)
    wsc2 = ops.WorkspaceCache()
    ws2 = wsc2.get(plan.ws_floats, torch.device(dev))
    out2 = torch.empty(B, T1, N, device=dev)
    pst = ops._head_struct(_lib.OutblockParams, [t.detach() for t in params])
    x_cl = x.detach().permute(0, 2, 3, 1).contiguous()
    stream = torch.cuda.current_stream().cuda_stream if cuda else None
    L.check(L.dll.stgcn_outblock_forward(C.byref(desc), C.byref(pst), x_cl.data_ptr(), out2.data_ptr(), saved.data_ptr(), ws2.data_ptr(),
                                         seed, offset, None, stream), "stgcn_outblock_forward")
    err["chain.direct"] = float(ops.head_chain_status(hcfg, B, T, wsc2))
    svn = saved.cpu().numpy()
    rows = B * T1 * N

    def seg(buf, off, ref, norm=False):
        d = float(np.abs(buf[off:off + ref.size].reshape(ref.shape) - ref).max())
        return d / max(1e-30, float(np.abs(ref).max())) if norm else d

    err["fwd.U"] = seg(svn, plan.sv_U, sv["U"])
    err["fwd.S"] = seg(svn, plan.sv_S, sv["S"])
    err["fwd.mean"] = seg(svn, plan.sv_mean, sv["mean"])
    err["fwd.rstd_rel"] = float(np.abs(svn[plan.sv_rstd:plan.sv_rstd + B * T1].reshape(B, T1) / sv["rstd"] - 1).max())
    err["fwd.yln"] = seg(svn, plan.sv_yln, sv["yln"])
    err["fwd.hd"] = seg(svn, plan.sv_hd, sv["hd"])      # (before the kink units below take the library's side)
    err["fwd.out"] = float(np.abs(out.detach().cpu().numpy()[:, 0].astype(np.float64) - out_ref).max())
    err["fwd.out_repeat_bitwise"] = float((out2 != out.detach()[:, 0]).sum().item())

    # ---- ReLU is not differentiable at 0: a hidden unit whose float64 pre-activation lies within FWD_TOL of zero -- closer than the
    #      forward is held to -- may come out on either side in fp32 (which side is a matter of summation order: the emulator and the MI355X
    #      differ), and the two one-sided derivatives differ by the whole of dout * fc2_w there (measured: one unit at 2.2e-7 among the
    #      266 240 of case l moved bwd.dh1 by 5.4 % of its max).  For THOSE units the backward oracle takes the side the library's saved
    #      hd took; every other unit keeps the oracle's own mask, so a wrong mask anywhere else still shows in bwd.dh1.
    h1 = sv["yln"] @ hp64["fc1_w"].T + (0.0 if hp64["fc1_b"] is None else hp64["fc1_b"])
    kink = np.abs(h1) < FWD_TOL
    if keep is not None:
        kink &= keep
    hd_lib = svn[plan.sv_hd:plan.sv_hd + rows * c1].reshape(B, T1, N, c1).astype(np.float64)
    err["info.relu_units_within_fwd_tol_of_zero"] = float(kink.sum())
    err["info.relu_units_on_the_other_side"] = float((kink & ((hd_lib != 0) != (sv["hd"] != 0))).sum())
    # Both counts are bounded, so that neither the inputs nor the library can hide a wrong mask in this window.  The window: at most twice
    # what a normal distribution of h1's own spread puts within FWD_TOL of zero (units * 2 FWD_TOL / (sigma sqrt(2 pi))), + 5 -- inputs
    # that pile units up at the kink get another seed.  The flips: a unit changes side only if the library's own h1 is wrong by more than
    # |h1|; its forward error is two orders below FWD_TOL (fwd.hd), so flips belong to the innermost part of the window -- at most a
    # quarter of it, + 1.
    eligible = float(h1.size if keep is None else keep.sum())
    window_bar = 2.0 * eligible * 2.0 * FWD_TOL / (float(h1.std()) * np.sqrt(2.0 * np.pi)) + 5.0
    err["kink.window_over_bar"] = max(0.0, err["info.relu_units_within_fwd_tol_of_zero"] - window_bar)
    err["kink.flips_over_bar"] = max(0.0, err["info.relu_units_on_the_other_side"] - (0.25 * err["info.relu_units_within_fwd_tol_of_zero"] + 1.0))
    sv["hd"] = np.where(kink, hd_lib, sv["hd"])
    sv32["hd"] = np.where(kink, hd_lib.astype(np.float32), sv32["hd"])
    dx_ref, g_ref, stages, loss_ref = oracle_bwd(np.float64, hp64, out_ref, sv)
    _, g32, _, _ = oracle_bwd(np.float32, hp32, out32, sv32)

    # ---- backward stages out of the autograd workspace (every launch path materialises all three: the fc1 weight gradient reads dh1,
    #      LayerNorm backward reads dyln, the conv weight gradient reads dZ -- also where the dense transposed conv forms dZ in its staging)
    ws = wsc.buf.cpu().numpy()
    assert rows * c1 == stages["dh1"].size and rows * 2 * c0 == stages["dZ"].size
    err["bwd.dh1"] = seg(ws, plan.ws_dh1, stages["dh1"], norm=True)
    err["bwd.dyln"] = seg(ws, plan.ws_dyln, stages["dyln"], norm=True)
    err["bwd.dZ"] = seg(ws, plan.ws_dZ, stages["dZ"], norm=True)
    if need_dx:
        err["bwd.dx"] = rel(cl(x.grad.cpu().numpy()), dx_ref)
    else:
        err["grad_none_ok.dx"] = 0.0 if x.grad is None else 1.0
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
    if loss is not None:
        err["loss.rel"] = abs(float(loss.item()) - loss_ref) / abs(loss_ref)
    return err


def bars(key):
    """The bars a key is held to (all of them)."""
    if key.startswith(("grad_none_ok", "chain.", "kink.")) or key.endswith("bitwise"):
        return (0.0,)
    if key.startswith("info."):
        return (float("inf"),)
    if key.startswith("oracle32."):
        return (ORACLE32_TOL,)
    if key == "fwd.out":
        return (FWD_TOL, OUT_TIGHT)
    if key.startswith("fwd."):
        return (FWD_TOL,)
    if key == "bwd.dx" or key.startswith("grad."):
        return (GRAD_TOL, GRAD_TIGHT)
    if key == "loss.rel":
        return (1e-5,)      # an fp32 mean of squares (test_mse_loss_fused_into_the_head_backward holds the two fp32 forms to 1e-6 of each other)
    return (GRAD_TOL,)      # bwd.* stages, slice.*


def report_head_errors(err, label, path):
    """Appends one JSON line per case to `path` (how profiles/head_stage_errors.md is made: tools/head_stage_report.py)."""
    with open(path, "a") as fh:
        fh.write(json.dumps({"case": label, **err}) + "\n")


def assert_head_errors(err):
    bad = {k: v for k, v in err.items() if not (v <= min(bars(k)))}
    assert not bad, f"out of tolerance: {bad}\nall: {err}"
