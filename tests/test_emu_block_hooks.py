"""The rows of tests/test_gpu_block_hooks.py that are small enough for the CPU emulator, through the same harness and bars; `many` pretends
to a small CU count at a smaller batch (ops.set_tc1_bwd_wgs), as tests/test_emu_block_paths.py does.  The emulator models neither MFMAs nor
wave scheduling: it is where mistakes of the table and of the oracle are found before a GPU is used."""
import pytest

from stgcn_amd import ops
from tests import hook_trust_util as trust
from tests.block_util import bind
from tests.launch_log_util import passed, read_launches, run_child
from tests.test_gpu_block_hooks import BF16_ROWS, CASES, assert_hook_keys, check_hook_launch_log, run, run_bf16

EMU_ROWS = [n for n, row in CASES.items() if row.get("emu", None) is not False]
AS_IS = [n for n in EMU_ROWS if not CASES[n].get("emu")]      # (rows whose launch geometry is the MI355X's: the emulator reports 256 CUs)


def emu_case(row):
    """(case, CU count to pretend to or 0)"""
    case, cus = list(row["case"]), 0
    if row.get("emu"):
        cus, case[7] = row["emu"]
    return tuple(case), cus


@pytest.mark.parametrize("name", EMU_ROWS)
def test_block_hooks_on_the_emulator(name):
    from tests.launch_log_util import span_recorder
    bind("cpu")
    case, cus = emu_case(CASES[name])
    prev = ops.set_tc1_bwd_wgs(cus)
    try:
        err = run(name, dev="cpu", label=name + " emu", case=case, on_half=span_recorder(name, "STGCN_BLOCK_LOG_SPANS"))
    finally:
        ops.set_tc1_bwd_wgs(prev)
    assert_hook_keys(err)
    assert ops.set_debug_stages(False) is False      # the harness restored the flag


def test_every_hook_row_takes_its_branch_on_the_emulator(tmp_path):
    """The launch-order assertions of the GPU module on the emulator's log of the rows that run as they are (a fresh process: the log is
    opened once), and `many` at 2 windows on 3 pretended CUs: 4 items on 3 workgroups, ranges that span items."""
    log, spans = tmp_path / "launch.log", tmp_path / "spans.jsonl"
    out = run_child({"STGCN_LAUNCH_LOG": str(log), "STGCN_BLOCK_LOG_SPANS": str(spans)}, ["tests/test_emu_block_hooks.py"],
                    "test_block_hooks_on_the_emulator", timeout=1500, marker="not gpu")
    assert passed(out) == len(EMU_ROWS), out[-2000:]
    launches = read_launches(log, spans)
    check_hook_launch_log(launches, {n: CASES[n] for n in AS_IS})
    many = dict(CASES["many"], log=[(CASES["many"]["log"][0][0], 3)])
    check_hook_launch_log(launches, {"many": many})


def test_rows_without_the_rowstats_fusion_on_the_emulator():
    """STGCN_FUSE without bit 4 (read once: a child): nothing is offered, P runs its own pass (run() expects one launch more)."""
    out = run_child({"STGCN_FUSE": str(0x7fffffff & ~4)}, ["tests/test_emu_block_hooks.py"],
                    "test_block_hooks_on_the_emulator[e64] or test_block_hooks_on_the_emulator[h64]", timeout=900, marker="not gpu")
    assert passed(out) == 2, out[-2000:]


def tc1_bwd_ranges(items, T, wgs, Kt=3, cin=64):
    """The (item, first step, end step) ranges tc1_bwd_body walks, from its own rule: workgroup g takes the units of the (item, step)
    sequence whose start weight lies in [Wtot * g / wgs, Wtot * (g + 1) / wgs), weights as tc1_bwd_step_weight."""
    T1 = T - Kt + 1
    w = [(Kt * (cin // 16) * 8 + 4 if s < T1 else 0) + 32 * sum(1 for k in range(Kt) if 0 <= s - k < T1) for s in range(T)]
    Wi = sum(w)

    def unit_at(pos):
        item, off, acc, step = pos // Wi, pos % Wi, 0, 0
        while step < T and acc < off:
            acc += w[step]
            step += 1
        return (item + 1, 0) if step >= T else (item, step)
    out = []
    for g in range(wgs):
        (i0, s0), (i1, s1) = unit_at(Wi * items * g // wgs), unit_at(Wi * items * (g + 1) // wgs)
        if i1 > items:
            i1, s1 = items, 0
        for item in range(i0, min(i1, items - 1) + 1):
            sb, se = (s0 if item == i0 else 0), (s1 if item == i1 else T)
            if sb < se:
                out.append((item, sb, se))
    return out


def test_parity_rows_cut_both_parities():
    """Rows e64 and e64t are in the table for the parity of se - sb, which selects the register set of a range's last F.  From the kernel's
    own cut rule: every (item, step) is walked exactly once, e64 has ranges of both parities, e64t ranges of 2 steps at each of the three
    positions of an item; together they end a range on an odd and an even count behind every kind of start (sb = 0, sb > 0)."""
    for name, items, T, wgs in (("e64", 4, 5, 10), ("e64t", 4, 6, 12), ("e64e", 3, 5, 7)):
        assert CASES[name]["log"][0][1] == wgs == min(max(items, items * T // 2), 256)
        rg = tc1_bwd_ranges(items, T, wgs)
        assert sorted((i, s) for i, sb, se in rg for s in range(sb, se)) == [(i, s) for i in range(items) for s in range(T)]
    e64 = tc1_bwd_ranges(4, 5, 10)
    assert {(se - sb) & 1 for _, sb, se in e64} == {0, 1}
    assert {((se - sb) & 1, sb > 0) for _, sb, se in e64} >= {(1, True), (0, False)}
    e64t = tc1_bwd_ranges(4, 6, 12)
    assert {(sb, se) for _, sb, se in e64t} == {(0, 2), (2, 4), (4, 6)}


@pytest.mark.parametrize("name", list(BF16_ROWS))
def test_bf16_block_consumer_rows_on_the_emulator(name):
    bind("cpu")
    case, cus = emu_case(BF16_ROWS[name])
    prev = ops.set_tc1_bwd_wgs(cus)
    try:
        run_bf16(name, dev="cpu", case=case)
    finally:
        ops.set_tc1_bwd_wgs(prev)


def test_hook_partials_do_not_depend_on_the_range_cuts_on_the_emulator():
    trust.check_range_cuts("cpu", small_cus=4)
