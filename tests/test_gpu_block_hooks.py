"""-m gpu: the LayerNorm hook epilogues (stgcn_ln_hook) of fp32 blocks, stage by stage, on the MI355X.  In a model the module Q that consumes
a block P's output writes P's LayerNorm-backward row partials while its input gradient is still on chip, and P runs with
desc.dy_rowstats_ready = 1; a block that stands alone (tests/test_gpu_block_paths.py) always forms them itself.  Every row here is a pair
P -> Q through tests/block_util.py's consumer mode: P is compared with the float64 stage oracle for the dy it received (y.grad), the row
partials Q wrote are read out of P's workspace, and each row runs as the stage tests launch it and as a training step does, bitwise equal.

Who writes P's row partials (the branch a row is in the table for; "launches" = ln_bwd_rowstats launches of the hooked backward):
launch_tc1_bwd (Q a block whose tmp_conv1 backward is the time-stepping kernel: c0 64, Kt 3, c_in = P's c2 = 64)
  [E1] epilogue F of tc1_bwd_x6_kernel<64, 64, 3, act>: e64 (GLU, mask read off y), e64p (mask regenerated, STGCN_HOOK_MASK=philox), e64e (GTU,
       eval: no mask), e64t, many, beta, big.  Ranges: Q offers B * node tiles items of T steps to min(max(items, items * T / tc1_min_steps()),
       CUs) workgroups (tc1_range_wgs) of equal MFMA weight, so the cuts fall inside items.  The last F of a range [sb, se) takes A.h or B.h by
       the parity of se - sb: e64 (4 items x 5 steps on 10 workgroups) cuts every item into ranges of 2, 1 (+ 1 of the next item) and 2 steps --
       both parities; e64t (4 items x 6 steps on 12) into ranges of 2 steps -- the even parity alone, at every position of an item;
       test_parity_rows_cut_both_parities (tests/test_emu_block_hooks.py) recomputes the cuts from the kernel's weights.  many: 260 items on
       256 workgroups, ranges that span items.  big: N 1024, P's tc2_bwd reads the hooked partials through ln_slab_consts_kernel
       (kLnBigColgroups: launch_ln_bwd_stats).
  [E2] the same in tc1_bwd_kernel<64, 64, 3, 0, float> (STGCN_MFMA_X6=0): e64f
  [E3] a hook the epilogue does not cover (dx_hook->C != c_in): unreachable from ops.py, _take_ln_hook hands over whole outputs only.
       The CIN 16 / 32 instances of the epilogue cannot be reached with a hook at all: a producer's c2 is 64 or 128 and the epilogue needs
       dx_hook->C == c_in; they run it with rs.rowstat == NULL in every test of tests/test_gpu_block_paths.py.
launch_tc1_bwd_data (Q's tmp_conv1 backward staged: tconv_bwd_data_kernel has no epilogue, launch_hook_rowstats follows it)
  [D1] c0 128: st128.  Kt != 3: stk2 (P on tc2_bwd_kernel<64, 2>).  c_in 128: c128 (C = 128 partials; P's tmp_conv2 backward staged, ln_gate_bwd
       reads them)
outblock_backward_impl (Q the output head)
  [H1] dense transposed conv (tconv_fwd4_body<PLAIN>, aa.rs) with the head's fused LayerNorm backward: h64 (C 64, training), h64e (eval, GTU:
       no-mask branch of ln_rowstat4), h128 (C 128)
  [H2] hook_pending behind launch_bwd_data (Ko * c_in != 256): hnd
  [H3] hook_pending behind the dense-shaped head whose dense_bwd is off (NC != 256): h64c.  A (64, 64) head is refused (c1 must be 128); (64, 128)
       has NC = 2 * c0 = 128 and takes this branch.  Its own LayerNorm pass is labelled head.ln_bwd_rowstats and is not counted.
launch_ln_bwd_stats (P): dy_rowstats_ready skips the pass on every row above; with STGCN_FUSE lacking 4 nothing is offered and P runs it
  (test_rows_without_the_rowstats_fusion); N * c2 / 4 >= kLnBigColgroups * 256: big.

Keys beyond tests/block_util.py's (bars FWD_TOL / GRAD_TOL / ORACLE32_TOL / 0 from there): hook.rowstat_g / _gx against the float64 sums,
oracle32.hook.* the same sums formed in np.float32 the way the kernels form them, hook.rowstat_nan, hook.dy_bitwise_vs_unhooked,
hook.rowstat_vs_own_pass_*, grad_none_ok.hook_launches.  tests/test_emu_block_hooks.py runs the rows that are small enough on the CPU emulator;
measured figures: profiles/block_hook_errors.md.
"""
import os

import pytest

from tests import hook_trust_util as trust
from tests.block_util import assert_errors, report_block_errors, run_block_pair
from tests.launch_log_util import passed, read_launches, run_child, span_recorder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THIS = "tests/test_gpu_block_hooks.py"
CHEB, KIPF = "cheb_graph_conv", "graph_conv"
P64, P128 = (64, (64, 16, 64)), (64, (64, 16, 128))
X6, F32 = "tc1_bwd_x6_kernel<64, 64, 3, ", "tc1_bwd_kernel<64, 64, 3, "

# name: case = P's (c_in, (c0, c1, c2), Kt, Ks, graph conv, act, N, B, T, training); consumer / shape: Q (tests/block_util.py make_consumer);
#       expect: ln_bwd_rowstats launches of the hooked backward; x6 / mask: STGCN_MFMA_X6 / STGCN_HOOK_MASK (read per call; None = default);
#       log: (kernel text, workgroups or None) the hooked backward must contain; order: "epi" (Q's epilogue wrote the partials) or "pending"
#       (the pass directly behind Q's transposed conv did); emu: (pretended CU count, B) for the emulator run (None: as is; False: too big)
# oracle32: oracle32.hook.rowstat_g / _gx, measured on the CPU (bar ORACLE32_TOL = 2.5e-4): a condition on the inputs alone
CASES = {
    # [E1] 4 items x 5 steps on 10 workgroups, ragged node tile      oracle32 1.0e-7 / 8.7e-8
    "e64": dict(case=(*P64, 3, 3, CHEB, "glu", 19, 2, 9, True), consumer="block", expect=1, log=[(X6 + "0>", 10)], order="epi"),
    # [E2] the fp32-MFMA kernel      oracle32 7.7e-8 / 1.2e-7 (dy is Q's: another kernel, other bits)
    "e64f": dict(case=(*P64, 3, 3, CHEB, "glu", 19, 2, 9, True), consumer="block", expect=1, x6="0", log=[(F32 + "0, ET>", 10)], order="epi"),
    # [E1] mask regenerated in hook_fetch from P's seed / offset (Q's seed is another)      oracle32 1.0e-7 / 8.7e-8
    "e64p": dict(case=(*P64, 3, 3, CHEB, "glu", 19, 2, 9, True), consumer="block", expect=1, mask="philox", log=[(X6 + "0>", 10)], order="epi"),
    # [E1] GTU, eval, Kipf: 3 items x 5 steps on 7 workgroups      oracle32 8.7e-8 / 8.4e-8
    "e64e": dict(case=(*P64, 3, 3, KIPF, "gtu", 33, 1, 9, False), consumer="block", expect=1, log=[(X6 + "1>", 7)], order="epi"),
    # [E1] 4 items x 6 steps on 12 workgroups: every range 2 steps      oracle32 5.3e-8 / 8.2e-8
    "e64t": dict(case=(*P64, 3, 3, CHEB, "glu", 50, 1, 10, True), consumer="block", expect=1, log=[(X6 + "0>", 12)], order="epi"),
    # [E1] 260 items on 256 workgroups      oracle32 1.1e-7 / 1.1e-7 at B 2 (the full batch is measured in the GPU run: profiles/block_hook_errors.md)
    "many": dict(case=(*P64, 3, 2, CHEB, "glu", 17, 130, 9, True), consumer="block", expect=1, log=[(X6 + "0>", 256)], order="epi", emu=(3, 2)),
    # [E1] |beta| >> |gamma|: y - keep_scale * beta cancels      oracle32 8.8e-8 / 4.4e-6
    "beta": dict(case=(*P64, 3, 3, CHEB, "glu", 19, 2, 9, True), consumer="block", expect=1, ln_scale=(0.05, 5.0), log=[(X6 + "0>", 10)], order="epi"),
    # [E1] N 1024: 64 items x 5 steps on 160 workgroups; P: ln_slab_consts over the hooked partials      oracle32: too big for the CPU suite, measured in the GPU run
    "big": dict(case=(*P64, 3, 2, CHEB, "glu", 1024, 1, 9, True), consumer="block", expect=1, log=[(X6 + "0>", 160), ("ln_slab_consts_kernel", None)],
                order="epi", emu=False),
    # [D1] Q's c0 = 128      oracle32 1.3e-7 / 6.6e-8
    "st128": dict(case=(*P64, 3, 3, CHEB, "glu", 19, 2, 9, True), consumer="block", shape=dict(channels=(128, 16, 64)), expect=2,
                  log=[("tconv_bwd_data_kernel<", None)], order="pending"),
    # [D1] Kt = 2 for both (T 5: P's T2 = Q's T = 3)      oracle32 6.1e-8 / 1.2e-7
    "stk2": dict(case=(*P64, 2, 3, CHEB, "glu", 19, 2, 5, True), consumer="block", expect=2,
                 log=[("tconv_bwd_data_kernel<", None), ("tc2_bwd_kernel<64, 2, true, 0", None)], order="pending"),
    # [D1] C = 128 partials, read by P's ln_gate_bwd      oracle32 7.7e-8 / 5.5e-8
    "c128": dict(case=(*P128, 3, 3, CHEB, "glu", 19, 2, 9, True), consumer="block", expect=2,
                 log=[("tconv_bwd_data_kernel<", None), ("ln_gate_bwd_kernel<float>", None)], order="pending"),
    # [H1] dense transposed conv epilogue, C 64      oracle32 7.5e-8 / 6.5e-8 (h64), 5.6e-8 / 1.4e-7 (h64e)
    "h64": dict(case=(*P64, 3, 3, CHEB, "glu", 19, 2, 8, True), consumer="head", expect=0, log=[("tconv_fwd4_kernel<", None)], order="epi"),
    "h64e": dict(case=(*P64, 3, 3, CHEB, "gtu", 50, 1, 8, False), consumer="head", expect=0, log=[("tconv_fwd4_kernel<", None)], order="epi"),
    # [H1] C 128, Ko 2      oracle32 8.0e-8 / 1.0e-7
    "h128": dict(case=(*P128, 3, 3, CHEB, "glu", 19, 2, 6, True), consumer="head", expect=0, log=[("tconv_fwd4_kernel<", None)], order="epi"),
    # [H2] Ko 3: the row-tile transposed conv, then the pending pass      oracle32 1.2e-7 / 1.3e-7
    "hnd": dict(case=(*P64, 3, 3, CHEB, "glu", 19, 2, 7, True), consumer="head", expect=1, log=[("tconv_bwd_data_kernel<", None)], order="pending"),
    # [H3] head (64, 128): dense_bwd off      oracle32 4.0e-8 / 7.6e-8
    "h64c": dict(case=(*P64, 3, 3, CHEB, "glu", 19, 2, 8, True), consumer="head", shape=dict(channels=(64, 128)), expect=1,
                 log=[("tconv_bwd_data_kernel<", None)], order="pending"),
}
HALVES = ("debug", "prod")


def rowstats_fusion_on():
    """STGCN_FUSE (read once by the library) has bit 4: consumers write the row partials.  Without it no hook is offered and P runs its own pass."""
    return bool(int(os.environ.get("STGCN_FUSE", str(0x7fffffff)), 0) & 4)


def run(name, dev=DEV, label=None, case=None, on_half=None):
    row = CASES[name]
    env = {"STGCN_MFMA_X6": row.get("x6"), "STGCN_HOOK_MASK": row.get("mask")}      # (both read per call by the library)
    prev = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is not None:
            os.environ[k] = v
        else:
            os.environ.pop(k, None)
    try:
        err = run_block_pair(dev, *(case or row["case"]), on_half=on_half, consumer=row["consumer"], consumer_shape=row.get("shape"),
                             ln_scale=row.get("ln_scale"), expect_rowstats=row["expect"] + (0 if rowstats_fusion_on() else 1))
    finally:
        for k, v in prev.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    print(label or name, err)
    if os.environ.get("STGCN_BLOCK_REPORT"):
        report_block_errors(err, label or name, os.environ["STGCN_BLOCK_REPORT"])
    return err


def assert_hook_keys(err):
    for k in ("hook.rowstat_g", "hook.rowstat_gx", "oracle32.hook.rowstat_g", "oracle32.hook.rowstat_gx", "hook.rowstat_nan", "hook.dy_bitwise_vs_unhooked",
              "hook.rowstat_vs_own_pass_g", "hook.rowstat_vs_own_pass_gx", "grad_none_ok.hook_launches", "prod.hook.rowstat_gx", "prod.hook.rowstat_nan",
              "prod.grad_none_ok.hook_launches", "prod.bitwise_vs_debug", "prod.grad.ln_w", "oracle32.grad.tc1_w"):
        assert k in err, k
    assert_errors(err)


@pytest.mark.parametrize("name", list(CASES))
def test_block_hooks(name):
    assert_hook_keys(run(name, on_half=span_recorder(name, "STGCN_BLOCK_LOG_SPANS")))


# ---- the launch log: which kernel wrote the partials --------------------------------------------------------------------------------------
Q_DX_LABELS = ("tc1_bwd", "tconv_bwd_data.tc1", "head.tconv_bwd_data")      # the launch of Q that forms P's dy


def check_hook_launch_log(launches, cases=CASES, halves=HALVES):
    """launches: tests/launch_log_util.py's {(row, span): [(label, kernel text, workgroups)]}; the span "<half>.hooked" is the backward from
    Q's output through P.  Per row and half: the kernel text and workgroup count the row is in the table for; every ln_bwd_rowstats launch
    accounted for by its place -- Q's own LayerNorm pass in front of Q's transposed conv, and behind that launch none (epilogue rows) or
    exactly one, directly behind a block's tconv_bwd_data.tc1 / in front of the head's reduction (pending rows)."""
    for name, row in cases.items():
        for half in halves:
            got = launches[(name, half + ".hooked")]
            assert got, (name, half)
            labels = [g[0] for g in got]
            for text, wgs in row["log"]:
                assert [g for g in got if text in g[1] and (wgs is None or g[2] == wgs)], f"row {name} ({half}): no '{text}' with {wgs} workgroups in {got}"
            iq = min(i for i, lab in enumerate(labels) if lab in Q_DX_LABELS)
            before, behind = labels[:iq], labels[iq + 1:]
            own_q = 1 if row["consumer"] == "block" else 0
            assert before.count("ln_bwd_rowstats") == own_q, (name, half, labels)
            if row["order"] == "epi":
                assert "ln_bwd_rowstats" not in behind, f"row {name} ({half}): a ln_bwd_rowstats launch behind Q's epilogue: {labels}"
            else:
                assert behind.count("ln_bwd_rowstats") == 1, (name, half, labels)
                at = behind.index("ln_bwd_rowstats")
                if row["consumer"] == "block":
                    assert at == 0, f"row {name} ({half}): the pending pass is not directly behind tconv_bwd_data.tc1: {labels}"
                else:
                    assert at < behind.index("head.reduce"), f"row {name} ({half}): the pending pass is not among the head's launches: {labels}"
            # P's tmp_conv2 backward starts behind all of it
            p_first = [i for i, lab in enumerate(behind) if lab in ("tc2_bwd", "ln_gate_bwd")]
            assert p_first and "ln_bwd_rowstats" not in behind[min(p_first):], (name, half, labels)
            assert labels.count("ln_bwd_rowstats") == row["expect"], (name, half, labels)


def test_every_hook_row_takes_its_branch(tmp_path):
    log, spans = tmp_path / "launch.log", tmp_path / "spans.jsonl"
    out = run_child({"STGCN_LAUNCH_LOG": str(log), "STGCN_BLOCK_LOG_SPANS": str(spans)}, [THIS], "test_block_hooks", timeout=900)
    assert passed(out) == len(CASES), out[-2000:]
    check_hook_launch_log(read_launches(log, spans))


def test_rows_without_the_rowstats_fusion():
    """STGCN_FUSE without bit 4 (read once: a child): no hook is offered, P forms the partials in a pass of its own -- one launch more per row
    (run() expects it) -- and every other key holds as before."""
    out = run_child({"STGCN_FUSE": str(0x7fffffff & ~4)}, [THIS], "test_block_hooks[e64] or test_block_hooks[h64]", timeout=600)
    assert passed(out) == 2, out[-2000:]


# ---- bf16: three rows the bf16 table has no consumer for, through its own harness and bars -----------------------------------------------
BF16_ROWS = {
    "eval_gtu": dict(case=(*P64, 3, 3, CHEB, "gtu", 19, 2, 9, False)),
    "philox": dict(case=(*P64, 3, 3, CHEB, "glu", 19, 2, 9, True), mask="philox"),
    "many": dict(case=(*P64, 3, 2, CHEB, "glu", 17, 130, 9, True), emu=(3, 2)),
}


def run_bf16(name, dev=DEV, case=None):
    from tests.bf16_util import assert_bf16_errors, run_block_case_bf16
    row = BF16_ROWS[name]
    prev = os.environ.get("STGCN_HOOK_MASK")
    if row.get("mask"):
        os.environ["STGCN_HOOK_MASK"] = row["mask"]
    else:
        os.environ.pop("STGCN_HOOK_MASK", None)
    try:
        stored, f32 = run_block_case_bf16(dev, *(case or row["case"]), consumer="block")
    finally:
        if prev is None:
            os.environ.pop("STGCN_HOOK_MASK", None)
        else:
            os.environ["STGCN_HOOK_MASK"] = prev
    assert f32["grad_none_ok.hook_epilogue_used"] == 0.0
    assert_bf16_errors(stored, f32)


@pytest.mark.parametrize("name", list(BF16_ROWS))
def test_bf16_block_consumer_rows(name):
    run_bf16(name)


# ---- range cuts -----------------------------------------------------------------------------------------------------------------------------
def test_hook_partials_do_not_depend_on_the_range_cuts():
    trust.check_range_cuts(DEV, small_cus=4)


# ---- the host-side trust rule (stgcn_amd/ops.py: LnHookState.matches, _take_ln_hook, _offer_ln_hook) -----------------------------------------
@pytest.mark.parametrize("tamper", trust.TAMPERS)
def test_producer_runs_its_own_pass_when_the_gradient_is_not_the_consumers(tamper):
    trust.check_tamper(DEV, tamper)


def test_forward_without_backward_leaves_no_offer_behind():
    trust.check_abandoned_forward(DEV)


def test_two_steps_on_the_same_caches():
    trust.check_two_steps(DEV)
