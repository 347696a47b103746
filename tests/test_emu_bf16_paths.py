"""The rows of tests/test_gpu_bf16_paths.py that are small enough for the CPU emulator, each run twice with a shared oracle (partial-sum
arena clean, then poisoned with NaN): same harness, same bars.  Rows that take a branch by the device's occupancy pretend to a small CU
count (ops.set_tc1_bwd_wgs) at a smaller batch; what the emulator cannot show -- MFMA hardware, real wave scheduling -- is what the
-m gpu module is for (rows b2 and c run there only)."""
import os

import pytest
import torch

from stgcn_amd import ops
from tests.block_util import bind
from tests.launch_log_util import check_rows_take_their_branch, passed, read_launches, run_child, span_recorder
from tests.test_gpu_bf16_paths import CASES, REFUSED, check, check_refused_log, refused_shapes, run

EMU_ROWS = [n for n, row in CASES.items() if row.get("emu", None) is not False]
OCCUPANCY_ROWS = {n: dict(row, log=row["emu_log"]) for n, row in CASES.items() if row.get("emu")}
THIS = "tests/test_emu_bf16_paths.py"


def emu_case(name):
    """(case, CU count to pretend to or 0)"""
    row = CASES[name]
    case = list(row["case"])
    cus = 0
    if row.get("emu"):
        cus, case[7] = row["emu"]
    return tuple(case), cus


@pytest.mark.parametrize("name", EMU_ROWS)
def test_bf16_block_paths_on_the_emulator(name):
    bind("cpu")
    case, cus = emu_case(name)
    prev = ops.set_tc1_bwd_wgs(cus)
    try:
        stored, f32, case = run(name, dev="cpu", label=name + " emu", case=case, on_half=span_recorder(name, "STGCN_BF16_LOG_SPANS"))
    finally:
        ops.set_tc1_bwd_wgs(prev)
    assert f32["prod.bitwise_clean_vs_poisoned"] == 0 and f32["prod.nan_elements"] == 0
    check(stored, f32, case)


def test_occupancy_rows_take_their_bf16_branch_on_the_emulator(tmp_path):
    """Rows a, e2 and g with the pretended CU count reach the branches they are in the table for: the two-group form of tc2_ln_fwd with
    tc1_fwd ranges cut inside items, the three-tile peer form above 256 nodes, and a tc2_bwd grid at its cap (a fresh process, because
    the launch log is opened once)."""
    log, spans = tmp_path / "launch.log", tmp_path / "spans.jsonl"
    out = run_child({"STGCN_LAUNCH_LOG": str(log), "STGCN_BF16_LOG_SPANS": str(spans)}, [THIS],
                    " or ".join(f"emulator[{n}]" for n in OCCUPANCY_ROWS), timeout=900, marker="not gpu")
    assert passed(out) == len(OCCUPANCY_ROWS), out[-2000:]
    launches = read_launches(log, spans)
    check_rows_take_their_branch(launches, OCCUPANCY_ROWS, ("clean", "poisoned"))


def test_bf16_blocks_the_backward_cannot_run_are_refused():
    bind("cpu")
    refused_shapes("cpu")


def test_refused_bf16_backward_launches_nothing(tmp_path):
    """The refusal comes in front of the backward's first launch: six forwards in the launch log, no backward line."""
    log = tmp_path / "launch.log"
    out = run_child({"STGCN_LAUNCH_LOG": str(log)}, [THIS], "test_bf16_blocks_the_backward_cannot_run_are_refused", marker="not gpu")
    assert passed(out) == 1, out[-2000:]
    check_refused_log(log.read_text().splitlines())


def test_supported_bf16_routes_are_what_the_launchers_can_run():
    """bf16_backward_ok refuses exactly the routes whose launchers carry STGCN_F32_ONLY: over a grid of shapes, a bf16 backward is admitted
    iff the plan fuses tmp_conv2's backward and tmp_conv1's runs fused or on the thin kernel without an input gradient -- and every row
    of the table is admitted."""
    import itertools
    bind("cpu")
    for c_in, channels, Kt, T, need_dx in itertools.product((1, 2, 16, 32, 64), ((64, 16, 64), (128, 16, 64), (64, 16, 128)), (2, 3, 4), (9, 40),
                                                         (False, True)):
        bcfg = ops.BlockConfig(Kt=Kt, Ks=3, n_vertex=17, c_in=c_in, channels=channels, act_func="glu", graph_conv_type="cheb_graph_conv", droprate=0.5)
        plan = ops.query_plan(ops.make_desc(bcfg, 2, T, True, need_dx, dtype=torch.bfloat16))
        ok = bool(plan.fused_tc2_bwd) and (bool(plan.fused_tc1_bwd) or (bool(plan.thin_tc1) and not need_dx))
        expect = channels == (64, 16, 64) and T == 9 and ((Kt == 3 and c_in >= 16 and need_dx) or (Kt * c_in <= 4 and not need_dx))
        assert ok == expect, (c_in, channels, Kt, T, need_dx)
    for name, (case, need_dx) in REFUSED.items():
        c_in, channels, Kt, Ks, gct, act, N, B, T, training = case
        bcfg = ops.BlockConfig(Kt=Kt, Ks=Ks, n_vertex=N, c_in=c_in, channels=channels, act_func=act, graph_conv_type=gct, droprate=0.5)
        plan = ops.query_plan(ops.make_desc(bcfg, B, T, training, need_dx, dtype=torch.bfloat16))
        assert not (plan.fused_tc2_bwd and (plan.fused_tc1_bwd or (plan.thin_tc1 and not need_dx))), name


def test_bf16_partial_arena_is_the_last_carve_of_the_workspace():
    """The harness poisons wsc.buf[ws_part : ws_part + part_floats] of a bf16 plan between forward and backward: every other carve of
    the plan -- packed weights, chain words, the row partials of a hooked LayerNorm, dYg / dA -- lies in front of the arena."""
    bind("cpu")
    for name, row in CASES.items():
        c_in, channels, Kt, Ks, gct, act, N, B, T, training = row["case"]
        bcfg = ops.BlockConfig(Kt=Kt, Ks=Ks, n_vertex=N, c_in=c_in, channels=channels, act_func=act, graph_conv_type=gct, droprate=0.5)
        plan = ops.query_plan(ops.make_desc(bcfg, B, T, training, c_in > 1, dtype=torch.bfloat16))
        assert 0 < plan.part_floats and plan.ws_part + plan.part_floats <= plan.ws_floats < plan.ws_part + plan.part_floats + 64, name
        for f, _ in type(plan)._fields_:
            if f.startswith("ws_") and f not in ("ws_part", "ws_floats"):
                assert getattr(plan, f) <= plan.ws_part, (name, f)
