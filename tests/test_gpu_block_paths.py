"""-m gpu: the ST block's launch paths, stage by stage, on the MI355X against the float64 stage oracle (tests/block_util.py), every row
once as the stage tests launch it (debug_stages on) and once as a training step does (off, partial-sum arena poisoned with NaN), the
two runs bitwise equal in y, dx and every parameter gradient.

Branches of route_block (stgcn_amd/csrc/stgcn_route.h) and of the launchers that read it (stgcn_capi.hip, stgcn_capi_bwd.inc).  "old": taken by
tests/test_gpu_block.py (debug_stages on only); a letter: the row of CASES that takes it.

stgcn_stblock_forward
  [F1] tmp_conv1 on the time-stepping kernels (c0 64, Kt 3, c_in 16 / 32 / 64): tc1_fwd_x6_kernel / tc1_fwd_kernel (STGCN_MFMA_X6=0), GLU / GTU
         c_in 64 GLU x6: old.  c_in 32 GLU x6: old.  c_in 16 GLU: g (x6), g0 (fp32 MFMA).  c_in 32 GTU: h, h0.  c_in 16 GTU: f.  c_in 64 GTU: b, p4
       grid = min(max(items, items * T1 / 2), CUs): ranges cut inside items: old;  more items than CUs (260 on 256): a
  [F2] thin first layer (Kt * c_in <= 4): old
  [F3] launch_tconv_fwd -> launch_tconv_fwd_nt (c0 128, Kt != 3, Kt * c_in <= 16): old for <2> and <4>; Kt 4: c, c2; its tile rows are chosen
       by occupancy (16 rows at these sizes) -- 32 / 48 / 64 rows: tests/test_gpu_block_variants.py (STGCN_TCONV_TR is read once)
  [F4] launch_gconv_fwd: slab-resident, one tile per wave by default (maxq 1): old; 2 .. 4 tiles per wave only under STGCN_GC_PARTS
       (variants); 28 node tiles in 7 parts: b; tiled: tests/test_gpu_gctile.py
  [F5] tc2_ln_fwd (c2 64, N <= 448), by N, slabs2 <= 2 CUs, peers, Kt, STGCN_MFMA_X6:
         x6 <.., 4, 4, 1> (wide): old          x6 <.., 2, 4, 2>: p2 (old at C2 size)      x6 <.., 1, 4, 4>: p4 (old at C2 size)
         fp32 <.., 2, 4, 2> N <= 256: p2f, d (Kt 2), c2 (Kt 4)     fp32 <.., 1, 4, 4> N <= 256: p4f
         fp32 <.., 3, 4, 2> / <.., 2, 4, 4> N > 256: old           fp32 <.., 4, 4, 1>: c (Kt 4: the only Kt that leaves the x6 forms)
         <.., 7, 2, 1> (slabs2 > 2 CUs, N <= 224): a                <.., 14, 2, 1>: b (384 < N <= 448), old at the C3 size (N 325)
  [F6] c2 128 or N > 448: tconv_fwd.tc2 + ln_fwd: old (GLU), f (GTU); ln_slab_stats: variants (STGCN_LN_STATS_MIN_CHUNKS is read once)
stgcn_stblock_backward_hook
  [B1] tc2_bwd_kernel<C2, KT, training, act>: <64, 3, *, GLU / GTU> old; <64, 2>: old (x6 forward), d; <64, 4>: c, c2.  One item per
       workgroup: old; items above 2 CUs (520 on 512: eight workgroups walk two items into one partial block): e.
       There is no <128, ..> instance: tc2_bwd_fused_ok bounds tc2_bwd_lds_bytes(c2, Kt, T1, T2) -- with the recompute staging counted,
       as for bf16 -- by 81 920 bytes, and c2 = 128 needs 113 936 at the shortest T (80 656 without the staging), so the predicate admits
       c2 = 64 only.  Every c2 = 128 block takes [B2]; row f pins that through the launch log, so that a change of the bound shows up here.
  [B2] tc2 backward not fused (c2 128: old (GLU), f (GTU); T1 > 32 steps do not fit the kernel's LDS ring: m): ln_gate_bwd + tconv_bwd_weight.tc2 + tconv_bwd_data.tc2 in
       PRODUCTION
  [B3] launch_gconv_bwd: gconv_bwd2 by occupancy: old; STGCN_GCBWD2_PARTS: variants
  [B4] tc1_bwd_x6_kernel / tc1_bwd_kernel<64, c_in, 3, act>: as [F1]
  [B5] tc1 backward not fused: thin: old; align_gate_bwd<1> / <2> + tconv_bwd_weight.tc1 + launch_bwd_data with 1 / 2 / 8 channel tiles:
       old (1, 8), c (2); 4 channel tiles (c_in 64 beside c0 128: the 8- or 4-wave kernel by occupancy; forced: variants): k

Every bar is tests/block_util.py's: FWD_TOL / GRAD_TOL as tests/test_gpu_block.py, 0 for the bitwise and NaN counts, GRAD_TOL / 4 for
the oracle's own fp32 run.  tests/test_emu_block_paths.py runs the rows that are small enough on the CPU emulator.
"""
import os

import pytest

from tests.block_util import assert_errors, report_block_errors, run_block_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHEB, KIPF = "cheb_graph_conv", "graph_conv"

# name: case = (c_in, (c0, c1, c2), Kt, Ks, graph conv, act, N, B, T, training); x6: STGCN_MFMA_X6 (None = default, on);
#       log: (kernel text, workgroups or None) that must appear in STGCN_LAUNCH_LOG for this row (tests/test_gpu_block_variants.py);
#       fused: which of the two debug launches the row's production half must NOT contain ("ln_gate_bwd" / "align_gate_bwd");
#       emu: (pretended CU count, B) for the emulator run (None: as is; False: too big for the CPU)
# oracle32: the worst gradient / slice metric of the stage oracle run in np.float32 against its float64 run, on these inputs (bar
#           GRAD_TOL / 4 = 2.5e-4): a condition on the inputs alone, measured on the CPU (the worst key is slice.y.tail, absolute, on every row)
CASES = {
    # [F5] two-group small form at 520 slabs > 2 * 256 CUs; [F1] 260 items on 256 workgroups      oracle32 6.0e-6
    "a": dict(case=(64, (64, 16, 64), 3, 3, CHEB, "glu", 17, 130, 8, True), log=[("7, 2, 1", 520), ("tc1_fwd_x6_kernel<64, 64, 3, 0>", 256)],
              fused=("ln_gate_bwd", "align_gate_bwd"), emu=(2, 2)),
    # [F5] <.., 14, 2, 1> at 28 node tiles, one slab; [F4] 7 parts      oracle32 2.1e-6
    "b": dict(case=(64, (64, 16, 64), 3, 3, CHEB, "gtu", 440, 1, 5, False), log=[("14, 2, 1", 1)], fused=("ln_gate_bwd", "align_gate_bwd")),
    # Kt = 4: [F5] fp32 wide form, [B1] tc2_bwd<64, 4>, [F3] / [B5] row-tile tmp_conv1 with 2 channel tiles      oracle32 2.5e-6
    "c": dict(case=(32, (64, 16, 64), 4, 2, CHEB, "glu", 35, 2, 8, True), log=[("tc2_ln_fwd_kernel<64, 4, 4, 4, 1", 4), ("tc2_bwd_kernel<64, 4, true, 0", 6)],
              fused=("ln_gate_bwd",)),
    # Kt = 4 with two workgroups per slab (4 node tiles), GTU, eval, T2 = 1      oracle32 1.0e-6
    "c2": dict(case=(16, (64, 16, 64), 4, 3, CHEB, "gtu", 50, 1, 7, False), log=[("tc2_ln_fwd_kernel<64, 4, 2, 4, 2", 2), ("tc2_bwd_kernel<64, 4, false, 1", 4)],
               fused=("ln_gate_bwd",)),
    # Kt = 2 on the fp32-MFMA peer form      oracle32 1.3e-6
    "d": dict(case=(64, (64, 16, 64), 2, 3, CHEB, "gtu", 50, 1, 4, False), x6="0", log=[("tc2_ln_fwd_kernel<64, 2, 2, 4, 2", 4), ("tc2_bwd_kernel<64, 2, false, 1", 4)],
              fused=("ln_gate_bwd",)),
    # [B1] 520 items on the 512 workgroups the cap leaves      oracle32 4.0e-6
    "e": dict(case=(64, (64, 16, 64), 3, 2, CHEB, "glu", 17, 260, 5, True), log=[("tc2_bwd_kernel<64, 3, true, 0", 512)], fused=("ln_gate_bwd", "align_gate_bwd"),
              emu=(2, 3)),
    # c2 = 128 with GTU, eval: [F6] GTU, [B2] (tc2_bwd_kernel has no c2 = 128 instance, see [B1]); [F1] / [B4] c_in 16 GTU      oracle32 1.4e-6
    "f": dict(case=(16, (64, 16, 128), 3, 2, CHEB, "gtu", 21, 2, 6, False),
              log=[("ln_gate_bwd_kernel<float>", None), ("tconv_bwd_weight_kernel<", None), ("tconv_bwd_data_kernel<1, 1, 1>", None),
                   ("tc1_fwd_x6_kernel<64, 16, 3, 1>", None), ("tc1_bwd_x6_kernel<64, 16, 3, 1>", None)],
              fused=("align_gate_bwd",)),
    # [F1] / [B4] c_in 16, GLU, training: x6 and fp32-MFMA forms      oracle32 2.5e-6
    "g": dict(case=(16, (64, 16, 64), 3, 3, CHEB, "glu", 19, 2, 6, True), log=[("tc1_fwd_x6_kernel<64, 16, 3, 0>", None), ("tc1_bwd_x6_kernel<64, 16, 3, 0>", None)],
              fused=("ln_gate_bwd", "align_gate_bwd")),
    "g0": dict(case=(16, (64, 16, 64), 3, 3, CHEB, "glu", 19, 2, 6, True), x6="0",
               log=[("tc1_fwd_kernel<64, 16, 3, 0, ET>", None), ("tc1_bwd_kernel<64, 16, 3, 0, ET>", None)], fused=("ln_gate_bwd", "align_gate_bwd")),
    # [F1] / [B4] c_in 32, GTU, training, Kipf graph conv: x6 and fp32-MFMA forms      oracle32 1.6e-6
    "h": dict(case=(32, (64, 16, 64), 3, 3, KIPF, "gtu", 33, 2, 7, True), log=[("tc1_fwd_x6_kernel<64, 32, 3, 1>", None), ("tc1_bwd_x6_kernel<64, 32, 3, 1>", None)],
              fused=("ln_gate_bwd", "align_gate_bwd")),
    "h0": dict(case=(32, (64, 16, 64), 3, 3, KIPF, "gtu", 33, 2, 7, True), x6="0",
               log=[("tc1_fwd_kernel<64, 32, 3, 1, ET>", None), ("tc1_bwd_kernel<64, 32, 3, 1, ET>", None)], fused=("ln_gate_bwd", "align_gate_bwd")),
    # [F5] two workgroups per slab at N <= 256 (4 node tiles, ragged): x6 and fp32 MFMA      oracle32 2.4e-6
    "p2": dict(case=(64, (64, 16, 64), 3, 3, CHEB, "glu", 50, 2, 6, True), log=[("tc2_ln_fwd_x6_kernel<64, (3 <= 3 ? 3 : 3), 2, 4, 2>", 8)], fused=("ln_gate_bwd", "align_gate_bwd")),
    "p2f": dict(case=(64, (64, 16, 64), 3, 3, CHEB, "glu", 50, 2, 6, True), x6="0", log=[("tc2_ln_fwd_kernel<64, 3, 2, 4, 2, ET>", 8)],
                fused=("ln_gate_bwd", "align_gate_bwd")),
    # [F5] four workgroups per slab at N <= 256 (8 node tiles, ragged): x6 and fp32 MFMA      oracle32 1.1e-6
    "p4": dict(case=(64, (64, 16, 64), 3, 2, CHEB, "gtu", 114, 1, 6, False), log=[("tc2_ln_fwd_x6_kernel<64, (3 <= 3 ? 3 : 3), 1, 4, 4>", 8)], fused=("ln_gate_bwd", "align_gate_bwd")),
    "p4f": dict(case=(64, (64, 16, 64), 3, 2, CHEB, "gtu", 114, 1, 6, False), x6="0", log=[("tc2_ln_fwd_kernel<64, 3, 1, 4, 4, ET>", 8)],
                fused=("ln_gate_bwd", "align_gate_bwd")),
    # [B5] transposed conv of tmp_conv1 with 4 input-channel tiles, align_gate_bwd<2> (c0 128)      oracle32 2.8e-6
    "k": dict(case=(64, (128, 16, 64), 2, 2, CHEB, "glu", 20, 2, 5, True), log=[("tconv_bwd_data_kernel<", None), ("align_gate_bwd_kernel<2>", None)],
              fused=("ln_gate_bwd",)),
    # [B2] T1 = 34 > 32: tmp_conv2 / LayerNorm backward on the stage-per-launch kernels in production      oracle32 1.2e-6
    "m": dict(case=(16, (64, 16, 64), 3, 2, CHEB, "glu", 17, 1, 36, False), log=[("tconv_bwd_weight_kernel<", None), ("ln_gate_bwd_kernel<float>", None)],
              fused=("align_gate_bwd",)),
}


def run(name, dev=DEV, label=None, case=None, on_half=None):
    row = CASES[name]
    x6 = row.get("x6")
    prev = os.environ.get("STGCN_MFMA_X6")      # (read per call by the library)
    if x6 is not None:
        os.environ["STGCN_MFMA_X6"] = x6
    else:
        os.environ.pop("STGCN_MFMA_X6", None)
    try:
        err = run_block_pair(dev, *(case or row["case"]), on_half=on_half)
    finally:
        if prev is None:
            os.environ.pop("STGCN_MFMA_X6", None)
        else:
            os.environ["STGCN_MFMA_X6"] = prev
    print(label or name, err)
    if os.environ.get("STGCN_BLOCK_REPORT"):
        report_block_errors(err, label or name, os.environ["STGCN_BLOCK_REPORT"])
    return err


def log_spans(name):
    """STGCN_BLOCK_LOG_SPANS=<file> (set by tests/test_gpu_block_variants.py beside STGCN_LAUNCH_LOG): the byte range of the launch log
    each half of each row wrote, one JSON line per half (tests/launch_log_util.py)."""
    from tests.launch_log_util import span_recorder
    return span_recorder(name, "STGCN_BLOCK_LOG_SPANS")


@pytest.mark.parametrize("name", list(CASES))
def test_block_paths(name):
    err = run(name, on_half=log_spans(name))
    assert "prod.bitwise_vs_debug" in err and "prod.grad.ln_w" in err and "oracle32.grad.tc1_w" in err
    assert_errors(err)
