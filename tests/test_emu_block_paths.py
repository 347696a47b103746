"""The rows of tests/test_gpu_block_paths.py that are small enough for the CPU emulator, each as the stage tests launch it (debug_stages
on) and as a training step does (off, partial-sum arena poisoned with NaN): same harness, same bars.  Rows that take a branch by the
device's occupancy pretend to a small CU count (ops.set_tc1_bwd_wgs) at a smaller batch; what the emulator cannot show -- MFMA hardware,
real wave scheduling -- is what the -m gpu module is for."""
import os

import pytest

from stgcn_amd import ops
from tests.block_util import assert_errors, bind, run_block_case
from tests.test_gpu_block_paths import CASES, run

EMU_ROWS = [n for n, row in CASES.items() if row.get("emu", None) is not False]


def emu_case(name):
    """(case, CU count to pretend to or 0)"""
    row = CASES[name]
    case = list(row["case"])
    cus = 0
    if row.get("emu"):
        cus, case[7] = row["emu"]
    return tuple(case), cus


@pytest.mark.parametrize("name", EMU_ROWS)
def test_block_paths_on_the_emulator(name):
    bind("cpu")
    case, cus = emu_case(name)
    prev = ops.set_tc1_bwd_wgs(cus)
    try:
        err = run(name, dev="cpu", label=name + " emu", case=case)
    finally:
        ops.set_tc1_bwd_wgs(prev)
    assert err["prod.bitwise_vs_debug"] == 0 and err["prod.nan_elements"] == 0
    assert_errors(err)
    assert ops.set_debug_stages(False) is False      # the harness restored the flag


def test_occupancy_rows_take_their_branch_on_the_emulator(tmp_path):
    """Rows a and e with the pretended CU count reach the branches they are in the table for: the two-group form of tc2_ln_fwd and a
    tc2_bwd grid at its cap (a fresh process, because the launch log is opened once)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    log = tmp_path / "launch.log"
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_emu_block_paths.py", "-x", "-q", "-p", "no:cacheprovider", "-k",
                        "emulator[a] or emulator[e]"],
                       cwd=root, env=dict(os.environ, STGCN_LAUNCH_LOG=str(log)), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    lines = [ln.split("\t") for ln in log.read_text().splitlines()]
    assert any(ln[0].startswith("tc2_ln_fwd") and "7, 2, 1" in ln[1] and ln[2] == "8" for ln in lines)        # row a: B 2 x T2 4 slabs > 2 x 2 CUs
    assert any(ln[0].startswith("tc2_bwd") and ln[2] == "4" for ln in lines)                                   # row e: 6 items on 2 x 2 workgroups


def test_debug_flag_is_restored_after_a_failing_case():
    """The flag is process-global: a case that raises must not leave it set for whatever runs next."""
    bind("cpu")
    assert ops.set_debug_stages(False) is False
    with pytest.raises(Exception):
        run_block_case("cpu", 64, (64, 16, 64), 3, 0, "cheb_graph_conv", "glu", 17, 1, 6, True, debug_stages=True)      # Ks = 0 is refused
    assert ops.set_debug_stages(False) is False


def test_partial_arena_is_the_last_carve_of_the_workspace():
    """The harness poisons wsc.buf[ws_part : ws_part + part_floats] between forward and backward.  That must hit nothing the backward
    reads from the forward -- packed weights, chain words, row partials: every other carve of the plan lies in front of the arena."""
    bind("cpu")
    for c_in, channels, Kt in ((64, (64, 16, 64), 3), (1, (64, 16, 64), 3), (16, (128, 16, 128), 2)):
        bcfg = ops.BlockConfig(Kt=Kt, Ks=3, n_vertex=17, c_in=c_in, channels=channels, act_func="glu", graph_conv_type="cheb_graph_conv", droprate=0.5)
        plan = ops.query_plan(ops.make_desc(bcfg, 2, 6, True, c_in > 1))
        assert 0 < plan.part_floats and plan.ws_part + plan.part_floats <= plan.ws_floats < plan.ws_part + plan.part_floats + 64
        for f, _ in type(plan)._fields_:
            if f.startswith("ws_") and f not in ("ws_part", "ws_floats"):
                assert getattr(plan, f) <= plan.ws_part, f


def test_plan_outside_the_partial_arena_ignores_need_dx_and_training():
    """The weight pack of a model is planned with need_dx = 1 and training = 1 (ops.prepack_modules), the forward and backward that read it
    with the flags of their call: every offset the pack writes to, every saved-tensor offset and every structural flag must therefore be the
    same for the four (need_dx, training) combinations of a shape.  Only the partial-sum arena behind them (ws_part, part_floats, hence
    ws_floats) and fused_tc1_bwd, which needs the input gradient, may differ."""
    import itertools
    bind("cpu")
    free = ("ws_part", "ws_floats", "part_floats", "fused_tc1_bwd")
    shapes = 0
    for c_in, channels, Kt, N, B, T, gct, Ks in itertools.product(
            (1, 2, 16, 32, 64), ((64, 16, 64), (128, 16, 64), (64, 16, 128), (128, 16, 128)), (2, 3, 4), (17, 207, 440, 600), (1, 32), (9, 12),
            ("cheb_graph_conv", "graph_conv"), (2, 3)):
        bcfg = ops.BlockConfig(Kt=Kt, Ks=Ks, n_vertex=N, c_in=c_in, channels=channels, act_func="glu", graph_conv_type=gct, droprate=0.5)
        plans = [ops.query_plan(ops.make_desc(bcfg, B, T, training, need_dx)) for need_dx in (False, True) for training in (False, True)]
        fields = [f for f, _ in type(plans[0])._fields_ if f not in free]
        for plan in plans[1:]:
            for f in fields:
                assert getattr(plan, f) == getattr(plans[0], f), (f, c_in, channels, Kt, N, B, T, gct, Ks)
        shapes += 1
    assert shapes == 3840
