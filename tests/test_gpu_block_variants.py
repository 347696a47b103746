"""-m gpu: (1) coverage of tests/test_gpu_block_paths.py as a checked fact -- the launch log of one run of the table shows that every row
took the kernel instance and the workgroup count it is in the table for, and that the production half of a fused row contains neither
debug launch; (2) the launcher knobs that are read once per process (STGCN_TCONV_TR, STGCN_BWD_DATA_WAVES, STGCN_GC_PARTS, STGCN_FUSE,
STGCN_LN_STATS_MIN_CHUNKS, STGCN_HOOK_MASK, STGCN_REDUCE_BIG), forced one by one on the MI355X over a few small rows of
tests/test_gpu_block.py::test_small_cases and of the table -- tests/test_emu_variants.py forces them on the emulator, which models
neither MFMA hardware nor real wave scheduling.

Every setting needs a fresh process: one child pytest at a time, each under its own time limit; a child that fails, dies or runs out of
time fails the test and is not started again.
"""
import os

import pytest

from tests.launch_log_util import check_rows_take_their_branch, passed, read_launches, run_child
from tests.test_gpu_block_paths import CASES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = "tests/test_gpu_block.py"
PATHS = "tests/test_gpu_block_paths.py"
DEBUG_LAUNCHES = ("ln_gate_bwd", "align_gate_bwd")


def small_rows(*ids):
    return "small_cases and (" + " or ".join(ids) + ")"


def path_rows(*names):
    return " or ".join(f"test_block_paths[{n}]" for n in names)


def check_launch_log(launches):
    """The assertions of test_every_row_takes_its_branch on a parsed log (also run on an emulator log by the CPU suite's scratch checks)."""
    check_rows_take_their_branch(launches, CASES, ("debug", "prod"))
    for name, row in CASES.items():
        labels_debug = [g[0] for g in launches[(name, "debug")]]
        labels_prod = [g[0] for g in launches[(name, "prod")]]
        for lab in row["fused"]:
            assert lab not in labels_prod, f"row {name}: the production half launches {lab}: {launches[(name, 'prod')]}"
            assert lab in labels_debug, f"row {name}: the debug half does not launch {lab}"
        for lab in DEBUG_LAUNCHES:      # a launch the block needs in production too (not fused there) appears once in either half
            if lab not in row["fused"]:
                assert labels_prod.count(lab) == labels_debug.count(lab) == 1, (name, lab, labels_prod, labels_debug)


def test_every_row_takes_its_branch(tmp_path):
    log, spans = tmp_path / "launch.log", tmp_path / "spans.jsonl"
    out = run_child({"STGCN_LAUNCH_LOG": str(log), "STGCN_BLOCK_LOG_SPANS": str(spans)}, [PATHS], "test_block_paths", timeout=900)
    assert passed(out) == len(CASES), out[-2000:]
    launches = read_launches(log, spans)
    assert len(launches) == 2 * len(CASES)
    check_launch_log(launches)


@pytest.mark.parametrize("fuse", ["default", "0"])
@pytest.mark.parametrize("tr", [32, 48, 64])
def test_gated_conv_tile_rows(tr, fuse):
    """tconv_fwd_kernel with 32 / 48 / 64-row tiles (the occupancy rule picks 16 at these sizes): on the c0 = 128 rows, whose tmp_conv1
    runs on it with the Align epilogue, and under STGCN_FUSE=0, where both temporal convs of every row do."""
    env = {"STGCN_TCONV_TR": str(tr)}
    if fuse == "default":
        out = run_child(env, [SMALL, PATHS], small_rows("glu-9-2-5-True") + " or " + path_rows("k"))
    else:
        out = run_child(dict(env, STGCN_FUSE="0"), [SMALL, PATHS], small_rows("glu-17-2-6-True", "35-1-5-False", "300-1-5-False") + " or " + path_rows("g"))
    assert passed(out) == (2 if fuse == "default" else 4), out[-2000:]


@pytest.mark.parametrize("waves", [4, 8])
def test_transposed_conv_wave_variants(waves):
    """tconv_bwd_data_kernel with 4 input-channel tiles on 4 / 8 waves (otherwise chosen by occupancy): row k, and the c_in = 64 rows
    under STGCN_FUSE=0."""
    out = run_child({"STGCN_BWD_DATA_WAVES": str(waves)}, [PATHS], path_rows("k"))
    assert passed(out) == 1, out[-2000:]
    out = run_child({"STGCN_BWD_DATA_WAVES": str(waves), "STGCN_FUSE": "0"}, [SMALL, PATHS], small_rows("glu-17-2-6-True") + " or " + path_rows("p2"))
    assert passed(out) == 2, out[-2000:]


@pytest.mark.parametrize("parts", ["1,1", "2,3", "4,2"])
def test_graph_conv_slab_parts(parts):
    """Workgroups per (b, t) slab of the slab-resident graph conv, forward / backward: Chebyshev Ks = 3 and 5, Kipf, and the 19 node tiles
    of the 300-node row (3 tiles per wave with one part, 2 with two)."""
    out = run_child({"STGCN_GC_PARTS": parts}, [SMALL], small_rows("glu-17-2-6-True", "35-1-5-False", "glu-9-2-5-True", "300-1-5-False"))
    assert passed(out) == 4, out[-2000:]


@pytest.mark.parametrize("env", [{"STGCN_FUSE": "0"}, {"STGCN_FUSE": str(0x7fffffff & ~2), "STGCN_LN_STATS_MIN_CHUNKS": "1"}],
                         ids=["fuse=0", "no-tc2_ln_fwd+slab-stats"])
def test_stage_per_launch_sequences(env):
    """STGCN_FUSE=0: the round-1 launch sequence (no fused kernel at all); STGCN_FUSE without bit 2 and the slab-statistics pre-pass
    forced: tconv_fwd.tc2 + ln_slab_stats + ln_fwd in front of the fused backward."""
    out = run_child(env, [SMALL, PATHS], small_rows("glu-17-2-6-True", "35-1-5-False") + " or " + path_rows("g", "p2"))
    assert passed(out) == 4, out[-2000:]


def test_dropout_mask_regenerated_with_philox():
    """STGCN_HOOK_MASK=philox: tc2_bwd_kernel regenerates the dropout mask instead of reading it off the block output."""
    out = run_child({"STGCN_HOOK_MASK": "philox"}, [SMALL, PATHS], small_rows("glu-17-2-6-True") + " or " + path_rows("p2", "c"))
    assert passed(out) == 3, out[-2000:]


def test_reduction_big_table_forms():
    """STGCN_REDUCE_BIG=1: reduce_kernel's forms for tables of >= 65 536 elements on small blocks, and on the 512 partial blocks of row e."""
    out = run_child({"STGCN_REDUCE_BIG": "1"}, [SMALL, PATHS], small_rows("glu-17-2-6-True", "glu-9-2-5-True") + " or " + path_rows("e"))
    assert passed(out) == 3, out[-2000:]


@pytest.mark.parametrize("parts", [1, 2])
def test_graph_conv_backward_forced_parts(parts, monkeypatch):
    """STGCN_GCBWD2_PARTS (read per call): gconv_bwd2_kernel with 3 (one part) and 2 (two parts) node tiles per wave on the 19 node tiles
    of a 300-node graph; by occupancy it runs one tile per wave here."""
    from tests.block_util import assert_errors, run_block_pair
    monkeypatch.setenv("STGCN_GCBWD2_PARTS", str(parts))
    err = run_block_pair("cuda:0", 64, (64, 16, 64), 3, 3, "cheb_graph_conv", "glu", 300, 1, 5, True)
    print(parts, err)
    assert_errors(err)
