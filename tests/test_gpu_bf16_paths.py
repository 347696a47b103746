"""-m gpu: the bf16 launch paths of the ST block (BASELINE.json configs[2] C3 and configs[4] C5 are bf16), stage by stage, on the MI355X
against the bf16 statement of the stage oracle (tests/bf16_util.py: run_block_pair_bf16).  bf16 always runs the launch sequence of a
training step (g_debug_stages && !g_bf16 skips the debug launches), so every row runs that sequence twice with a shared oracle: the
partial-sum arena as the forward left it, then filled with NaN between forward and backward -- y, dx and every parameter gradient bitwise
equal between the two (prod.bitwise_clean_vs_poisoned), no NaN among them (prod.nan_elements), chain words 0.

Every row has channels (64, 16, 64): stgcn_stblock_backward refuses bf16 with any other width (bf16_backward_ok, stgcn_route.h;
test_bf16_blocks_the_backward_cannot_run_are_refused).  The launch log prints ET for both activation types: what places a row in the bf16
lane is y.dtype == torch.bfloat16 and plan.stored_US2 == False (the forward stores no gate inputs of tmp_conv2, so tc2_bwd_kernel runs
its RECOMP = true instance behind the RC_ of the log text).

Branches of route_block (stgcn_amd/csrc/stgcn_route.h) and of the launchers that read it, bf16 lane.  "old": taken by tests/test_gpu_bf16.py
(whole-tensor keys, one run); a name: the row of CASES that takes it.
  [F1] tc1_fwd_kernel<64, c_in, 3, act, bf16> on two workgroups per CU: c_in 64 GLU old; c_in 64 GTU eval old, training: b (eval), e4 is c_in 32
       GTU training, h32 c_in 32 GTU Kipf training; c_in 16 GLU / GTU: h16 / h16t.  Grid 2 x CUs with ranges cut inside items: a
  [F2] thin first layer (c_in 1): old (Kt 3); Kt 2: f2; Kt 4: f4, f4p
  [F4] gconv_fwd_b16p_kernel<1, 16>: old, b (28 node tiles), k5 (Ks 5); <2, 8> and the non-plane kernel with 3 tiles per wave: variants
       (STGCN_GC_PARTS); Ks 1 -> b16p is off, gconv_fwd_kernel<.., bf16, 1> / gconv_bwd2_kernel<1, bf16>: k1
  [F5] tc2_ln_fwd_kernel<64, Kt, tiles per wave, groups, peers, bf16>:
         <3, 4, 4, 1> old   <3, 6, 4, 1> (bf16 only; 256 < N <= 384): c, old at the C3 size   <3, 7, 2, 1> (slabs > 2 CUs, N <= 224): a
         <3, 14, 2, 1>: b (384 < N <= 448, one slab), b2 (224 < N <= 384 with slabs > 2 CUs: C3 above bs 64)
         <3, 2, 4, 2> / <3, 1, 4, 4> (N <= 256): d2 / d4       <3, 2, 4, 4> / <3, 3, 4, 2> (N > 256, default rule): e4 / e2
         <2, 4, 4, 1>: f2      <4, 4, 4, 1>: f4      <4, 2, 4, 2>: f4p
  [B1] tc2_bwd_kernel<64, Kt, training, act, RECOMP = true, bf16>: <3, *> old; <2, true, GLU>: f2; <4, true, GTU>: f4; <4, false, GTU>: f4p;
       GTU with dropout on: e4, h16t, h32, f4; grid at its cap (520 items on 2 x 256 workgroups): g; mask regenerated: variants (STGCN_HOOK_MASK)
  [B3] gconv_bwd2_kernel<1, bf16, true>: old; more parts / tiles per wave: variants (STGCN_GC_PARTS, STGCN_GCBWD2_PARTS)
  [B4] tc1_bwd_kernel<64, c_in, 3, act, bf16>: as [F1]
  reduction of big tables (STGCN_REDUCE_BIG=1) on g's 512 partial blocks: variants

Keys and bars: tests/bf16_util.py (every bar is the one tests/test_gpu_bf16.py is held to; the slice keys share them because a slice's
elements sum over the same rows as the whole tensor's, under the condition assert_slice_ratios checks on the oracle alone).  Rows with
fewer than 4 (b, t2) slabs (b, d4, e4, f4p) are held to fwd.mean_over_std and only report fwd.mean, whose normaliser is then a maximum
over one or two |mean|.  tests/test_emu_bf16_paths.py runs the rows that are small enough on the CPU emulator.
"""
import os

import pytest
import torch

from tests.bf16_util import assert_bf16_errors, assert_slice_ratios, report_bf16_paths, run_block_case_bf16, run_block_pair_bf16
from tests.launch_log_util import check_rows_take_their_branch, passed, read_launches, run_child, span_recorder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHEB, KIPF = "cheb_graph_conv", "graph_conv"
C = (64, 16, 64)
THIS = "tests/test_gpu_bf16_paths.py"

# name: case = (c_in, (c0, c1, c2), Kt, Ks, graph conv, act, N, B, T, training);
#       seed / emu_seed: data seed of x and dy (default 11) -- the first seed from 11 upwards at which every slice's max |ref| is at least 0.25
#           of its whole tensor's (assert_slice_ratios; the oracle alone, measured on the CPU).  The slice that decides is dx.t0 on every row
#           that forms dx: the first input step receives ONE tap of the transposed conv, from a dA whose first step received one tap itself
#           (0.25 - 0.35 of the whole tensor's max; seed 11 gives 0.16 - 0.24 on rows a, c, d4, e2, h32).  The bars never move;
#       gso_sym: the operator is tests/emu_util.sym_gso(N, gso_sym) instead of the non-symmetric default, under which T_4 of the Ks = 5 row
#           dwarfs the low terms (gc_w.k0 0.09 of the whole gradient's max; 0.35 is then the row's smallest ratio, dx.t0);
#       log: (kernel text, workgroups or None) that must appear in STGCN_LAUNCH_LOG in both runs of the row (256 CUs);
#       emu: (pretended CU count, B) for the emulator run (None: as is; False: too big for the CPU), emu_log: its log texts
CASES = {
    # [F5] two-group small form at 520 slabs > 2 x 256 CUs; [F1] 260 items on 2 x 256 workgroups: ranges cut inside items
    "a": dict(case=(64, C, 3, 3, CHEB, "glu", 17, 130, 8, True), log=[("tc2_ln_fwd_kernel<64, 3, 7, 2, 1, ET>", 520), ("tc1_fwd_kernel<64, 64, 3, 0, ET>", 512)],
              seed=17, emu=(2, 2), emu_seed=27, emu_log=[("tc2_ln_fwd_kernel<64, 3, 7, 2, 1, ET>", 8), ("tc1_fwd_kernel<64, 64, 3, 0, ET>", 4)]),
    # [F5] <.., 14, 2, 1> at 28 node tiles, one slab, GTU eval; [F4] 28 node tiles in 7 parts through the bf16-plane kernel
    "b": dict(case=(64, C, 3, 3, CHEB, "gtu", 440, 1, 5, False), log=[("tc2_ln_fwd_kernel<64, 3, 14, 2, 1, ET>", 1), ("gconv_fwd_b16p_kernel<1, 16>", 21)]),
    # [F5] <.., 14, 2, 1> at 516 slabs > 2 x 256 CUs, 224 < N <= 384 (C3's block 1 above bs 64)
    "b2": dict(case=(64, C, 3, 3, CHEB, "glu", 230, 129, 8, True), log=[("tc2_ln_fwd_kernel<64, 3, 14, 2, 1, ET>", 516)], emu=False),
    # [F5] the 6-tile form, which has no fp32 instance; 300 % 16 = 12
    "c": dict(case=(64, C, 3, 3, CHEB, "glu", 300, 33, 8, True), log=[("tc2_ln_fwd_kernel<64, 3, 6, 4, 1, bf16>", 132)], seed=15, emu=False),
    # [F5] peer forms at N <= 256, ragged
    "d2": dict(case=(64, C, 3, 3, CHEB, "glu", 50, 2, 6, True), log=[("tc2_ln_fwd_kernel<64, 3, 2, 4, 2, ET>", 8)]),
    "d4": dict(case=(64, C, 3, 2, CHEB, "gtu", 114, 1, 6, False), log=[("tc2_ln_fwd_kernel<64, 3, 1, 4, 4, ET>", 8)], seed=16),
    # [F5] peer forms above 256 nodes chosen by the default rule, not by set_tc2ln_peers
    "e4": dict(case=(32, C, 3, 3, CHEB, "gtu", 300, 1, 5, True), log=[("tc2_ln_fwd_kernel<64, 3, 2, 4, 4, ET>", 4), ("tc2_bwd_kernel<64, 3, true, 1", None)]),
    "e2": dict(case=(64, C, 3, 3, CHEB, "glu", 300, 17, 8, True), log=[("tc2_ln_fwd_kernel<64, 3, 3, 4, 2, ET>", 136)],
               seed=18, emu=(8, 1), emu_seed=12, emu_log=[("tc2_ln_fwd_kernel<64, 3, 3, 4, 2, ET>", 8)]),
    # Kt 2 / Kt 4 behind the thin first layer
    "f2": dict(case=(1, C, 2, 3, CHEB, "glu", 21, 2, 5, True), log=[("tc2_ln_fwd_kernel<64, 2, 4, 4, 1, ET>", 6), ("tc2_bwd_kernel<64, 2, true, 0", 4)]),
    "f4": dict(case=(1, C, 4, 2, CHEB, "gtu", 35, 2, 8, True), log=[("tc2_ln_fwd_kernel<64, 4, 4, 4, 1, ET>", 4), ("tc2_bwd_kernel<64, 4, true, 1", 6)]),
    # Kt 4 with two workgroups per slab (4 node tiles), eval, T2 = 1
    "f4p": dict(case=(1, C, 4, 3, CHEB, "gtu", 50, 1, 7, False), log=[("tc2_ln_fwd_kernel<64, 4, 2, 4, 2, ET>", 2), ("tc2_bwd_kernel<64, 4, false, 1", 4)]),
    # [B1] 520 items on the 512 workgroups the cap leaves
    "g": dict(case=(64, C, 3, 2, CHEB, "glu", 17, 260, 5, True), log=[("tc2_bwd_kernel<64, 3, true, 0", 512)],
              emu=(2, 3), emu_log=[("tc2_bwd_kernel<64, 3, true, 0", 4)]),
    # [F1] / [B4] c_in 16, GLU and GTU, training
    "h16": dict(case=(16, C, 3, 3, CHEB, "glu", 19, 2, 6, True), log=[("tc1_fwd_kernel<64, 16, 3, 0, ET>", None), ("tc1_bwd_kernel<64, 16, 3, 0, ET>", None)]),
    "h16t": dict(case=(16, C, 3, 3, CHEB, "gtu", 19, 2, 6, True), log=[("tc1_fwd_kernel<64, 16, 3, 1, ET>", None), ("tc1_bwd_kernel<64, 16, 3, 1, ET>", None)]),
    # [F1] / [B4] c_in 32, GTU, training, Kipf graph conv
    "h32": dict(case=(32, C, 3, 3, KIPF, "gtu", 33, 2, 7, True), log=[("tc1_fwd_kernel<64, 32, 3, 1, ET>", None), ("tc1_bwd_kernel<64, 32, 3, 1, ET>", None)], seed=12),
    # Ks = 1: b16p = g_bf16 && Ks > 1 is off, the non-plane graph-conv kernels run with ET = bf16
    "k1": dict(case=(64, C, 3, 1, CHEB, "glu", 35, 2, 6, True), log=[("gconv_fwd_kernel<1, 16, ET, 1>", None), ("gconv_bwd2_kernel<1, ET>", None)]),
    # Ks = 5 (configs[4]'s) on the slab path
    "k5": dict(case=(64, C, 3, 5, CHEB, "glu", 300, 2, 6, True), log=[("gconv_fwd_b16p_kernel<1, 16>", None), ("gconv_bwd2_kernel<1, bf16, true>", None)], gso_sym=6),
}


def few_slabs(case):
    """Fewer than 4 (b, t2) slabs: fwd.mean is reported, fwd.mean_over_std asserted (module docstring)."""
    c_in, channels, Kt, Ks, gct, act, N, B, T, training = case
    return B * (T - 2 * (Kt - 1)) < 4


def run(name, dev=DEV, label=None, case=None, on_half=None, pair=True):
    from stgcn_amd import ops
    row = CASES[name]
    case = case or row["case"]
    c_in, channels, Kt, Ks, gct, act, N, B, T, training = case
    bcfg = ops.BlockConfig(Kt=Kt, Ks=Ks, n_vertex=N, c_in=c_in, channels=channels, act_func=act, graph_conv_type=gct, droprate=0.5)
    plan = ops.query_plan(ops.make_desc(bcfg, B, T, training, c_in > 1, dtype=torch.bfloat16))
    assert plan.fused_tc2_bwd and not plan.stored_US2      # tc2_bwd_kernel<.., RECOMP = true, bf16>: the forward stores no gate inputs of tmp_conv2
    emu = str(dev) == "cpu" and row.get("emu")
    kw = dict(data_seed=row.get("emu_seed" if emu else "seed", 11))
    if row.get("gso_sym"):
        from tests.emu_util import sym_gso
        kw["gso"] = sym_gso(N, row["gso_sym"])
    stored, f32 = run_block_pair_bf16(dev, *case, on_half=on_half, **kw) if pair else run_block_case_bf16(dev, *case, **kw)
    print(label or name, f32, stored)
    if os.environ.get("STGCN_BF16_PATHS_REPORT"):
        report_bf16_paths(stored, f32, label or name, os.environ["STGCN_BF16_PATHS_REPORT"])
    return stored, f32, case


def check(stored, f32, case, pair=True):
    assert "slice.tc2_w.k0" in f32 and "fwd.mean_over_std" in f32 and "prod.nan_elements" in f32
    assert not pair or "prod.bitwise_clean_vs_poisoned" in f32
    assert_bf16_errors(stored, f32, report_only=("fwd.mean",) if few_slabs(case) else ())
    assert_slice_ratios(f32)


def bind():
    from tests.gpu_util import bind_hip
    return bind_hip()


@pytest.mark.parametrize("name", list(CASES))
def test_bf16_block_paths(name):
    bind()
    check(*run(name, on_half=span_recorder(name, "STGCN_BF16_LOG_SPANS")))


def path_rows(*names):
    return " or ".join(f"test_bf16_block_paths[{n}]" for n in names)


def test_every_bf16_row_takes_its_branch(tmp_path):
    """One child runs the table with the launch log on: every row launched the instance and the workgroup count it is listed for, in
    both of its runs."""
    log, spans = tmp_path / "launch.log", tmp_path / "spans.jsonl"
    out = run_child({"STGCN_LAUNCH_LOG": str(log), "STGCN_BF16_LOG_SPANS": str(spans)}, [THIS], "test_bf16_block_paths", timeout=900)
    assert passed(out) == len(CASES), out[-2000:]
    launches = read_launches(log, spans)
    assert len(launches) == 2 * len(CASES)
    check_rows_take_their_branch(launches, CASES, ("clean", "poisoned"))
    for name in CASES:      # the poisoned arena changes no launch
        assert launches[(name, "clean")] == launches[(name, "poisoned")], name


@pytest.mark.parametrize("parts", ["1,1", "2,3", "4,2"])
def test_bf16_graph_conv_slab_parts(parts):
    """STGCN_GC_PARTS (read once) over the 19 node tiles of e4 (Ks 3) and k5 (Ks 5): one part = 3 tiles per wave, beyond what the bf16-plane
    forward kernel holds (the non-plane kernel runs); two parts = gconv_fwd_b16p_kernel<2, 8>; four = <1, 16>; the slab backward in 1 / 3 / 2 parts."""
    out = run_child({"STGCN_GC_PARTS": parts}, [THIS], path_rows("e4", "k5"))
    assert passed(out) == 2, out[-2000:]


def test_bf16_dropout_mask_regenerated_with_philox():
    """STGCN_HOOK_MASK=philox: tc2_bwd_kernel<.., true, bf16> regenerates the dropout mask instead of reading it off the block output."""
    out = run_child({"STGCN_HOOK_MASK": "philox"}, [THIS], path_rows("d2", "f4"))
    assert passed(out) == 2, out[-2000:]


def test_bf16_reduction_big_table_forms():
    """STGCN_REDUCE_BIG=1 on the 512 partial blocks of row g."""
    out = run_child({"STGCN_REDUCE_BIG": "1"}, [THIS], path_rows("g"))
    assert passed(out) == 1, out[-2000:]


@pytest.mark.parametrize("parts", [1, 2])
def test_bf16_graph_conv_backward_forced_parts(parts, monkeypatch):
    """STGCN_GCBWD2_PARTS (read per call): gconv_bwd2_kernel<.., bf16, true> with 3 (one part) and 2 (two parts) node tiles per wave on the 19
    node tiles of e4; by occupancy it runs one tile per wave here."""
    bind()
    monkeypatch.setenv("STGCN_GCBWD2_PARTS", str(parts))
    check(*run("e4", label=f"e4 gcbwd2_parts={parts}"))


# shapes whose bf16 forward runs and whose backward has no bf16 kernels: (case, need_dx), and the stage that used to refuse them mid-sequence
REFUSED = {
    "c_in64_Kt2": ((64, C, 2, 3, CHEB, "glu", 17, 2, 5, True), True),                 # tc1_bwd_kernel is Kt 3 only: align_gate_bwd
    "c2_128": ((64, (64, 16, 128), 3, 3, CHEB, "glu", 17, 2, 6, True), True),         # no tc2_bwd_kernel<128>: ln_gate_bwd + row-tile kernels
    "c0_128_c_in16": ((16, (128, 16, 64), 3, 3, CHEB, "glu", 17, 2, 6, True), True),  # align_gate_bwd
    "T1_34": ((64, C, 3, 2, CHEB, "glu", 17, 1, 36, False), True),                    # T1 > 32 steps: ln_gate_bwd + row-tile kernels
    "thin_need_dx": ((2, C, 2, 3, CHEB, "glu", 17, 2, 5, True), True),                # thin layer with an input gradient: tconv_bwd_data.tc1
    "c_in64_no_dx": ((64, C, 3, 3, CHEB, "glu", 17, 2, 6, True), False),              # tc1_bwd_kernel always forms dx: k3 = 0 without need_dx
}
# every label stgcn_stblock_backward can launch under (stgcn_capi_bwd.inc and the leaf launchers it calls)
BACKWARD_LABELS = ("ln_bwd_rowstats", "ln_slab_consts", "ln_gate_bwd", "tc2_bwd", "tconv_bwd_", "gconv_bwd", "gconv_rows_bwd", "gso_gemm_bwd",
                   "tc1_bwd", "align_gate_bwd", "reduce")


def refused_shapes(dev):
    for name, (case, need_dx) in REFUSED.items():
        with pytest.raises(NotImplementedError, match="no bf16 backward for c_in=%d " % case[0]):      # STGCN_ERR_UNSUPPORTED, naming the shape
            run_block_case_bf16(dev, *case, need_dx=need_dx)


def check_refused_log(lines):
    """The launch log of refused_shapes: six forwards ran, no launch of any backward."""
    labels = [ln.split("\t")[0].split("@")[0] for ln in lines]
    assert labels.count("tconv_fwd.tc1") == labels.count("gconv_fwd") == len(REFUSED), labels
    assert not [lab for lab in labels if lab.startswith(BACKWARD_LABELS)], labels


def test_bf16_blocks_the_backward_cannot_run_are_refused():
    """No bf16 block the backward cannot run returns numbers: NotImplementedError (STGCN_ERR_UNSUPPORTED) from stgcn_stblock_backward."""
    bind()
    refused_shapes(DEV)


def test_refused_bf16_backward_launches_nothing(tmp_path):
    """The refusal comes before the backward's first launch and leaves the forward alone (what an eval-only caller relies on): in a child
    with the launch log on, six forwards and not one backward line."""
    log = tmp_path / "launch.log"
    out = run_child({"STGCN_LAUNCH_LOG": str(log)}, [THIS], "test_bf16_blocks_the_backward_cannot_run_are_refused")
    assert passed(out) == 1, out[-2000:]
    check_refused_log(log.read_text().splitlines())
