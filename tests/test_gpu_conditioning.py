"""-m gpu: the table of tests/test_emu_conditioning.py on the MI355X -- the same rows, conditions, metrics and criterion
(tests/conditioning_util.py), with what the emulator cannot show: v_exp_f32 / v_rcp_f32 at 1 ulp and the MFMA summation order.  One row
more, too slow for the emulator: 600 nodes under an outlying and under a dead first row (the tiled graph conv and a 600-row
slab_stats_from_rows).

STGCN_COND_REPORT=<file>: one JSON line per run -- row, condition, product form, every key's error beside its float32-oracle twin
(profiles/conditioning_errors.md is made from it and from the emulator module's lines: tools/conditioning_report.py)."""
import pytest

from tests import conditioning_util as cu
from tests.block_util import bind

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("cond", list(cu.CONDITIONS))
@pytest.mark.parametrize("row,x6", cu.RUNS, ids=cu.RUN_IDS)
def test_condition(row, x6, cond):
    bind(DEV)
    err = cu.run_condition(DEV, row, cond, x6=x6)
    print(row, x6, cond, "worst ratio %.2f at %s" % cu.worst_ratio(err), err)
    cu.report(err, row, cond, x6, "debug", "gpu")
    assert "fwd.y" in err and "oracle32.fwd.G" in err and "oracle32.bwd.dA" in err and "kink.window_over_bar" in err
    cu.assert_condition(err, f"{row} {cond} x6={x6}")


@pytest.mark.parametrize("cond", cu.PROD_CONDITIONS)
@pytest.mark.parametrize("row", list(cu.ROWS))
def test_condition_as_production_launches_it(row, cond):
    """debug_stages off, the partial arena poisoned with NaN between forward and backward: the fused backward kernels see the condition."""
    bind(DEV)
    err = cu.run_condition(DEV, row, cond, debug_stages=False)
    print(row, cond, "prod: worst ratio %.2f at %s" % cu.worst_ratio(err), err)
    cu.report(err, row, cond, None, "prod", "gpu")
    cu.assert_condition(err, f"{row} {cond} production")


@pytest.mark.parametrize("cond", list(cu.CONDITIONS))
def test_sparse_operator_condition(cond):
    bind(DEV)
    err = cu.run_sparse_condition(DEV, cond)
    print("sparse", cond, "worst ratio %.2f at %s" % cu.worst_ratio(err), err)
    cu.report(err, "sparse-" + cu.SPARSE_ROW, cond, None, "debug", "gpu")
    cu.assert_condition(err, f"sparse {cond}")


@pytest.mark.parametrize("cond", cu.BIG_CONDITIONS)
def test_600_nodes_under_an_outlying_first_row(cond):
    from stgcn_amd import ops
    bind(DEV)
    case = cu.BIG_ROW
    bcfg = ops.BlockConfig(Kt=case[2], Ks=case[3], n_vertex=case[6], c_in=case[0], channels=case[1], act_func=case[5], graph_conv_type=case[4], droprate=0.5)
    plan = ops.query_plan(ops.make_desc(bcfg, case[7], case[8], True, True))
    assert plan.tiled_gc == 1      # what the row is in the table for
    err = cu.run_condition(DEV, "big", cond)
    print("big", cond, "worst ratio %.2f at %s" % cu.worst_ratio(err), err)
    cu.report(err, "big600", cond, None, "debug", "gpu")
    cu.assert_condition(err, f"big600 {cond}")


@pytest.mark.parametrize("what", list(cu.NONFINITE))
@pytest.mark.parametrize("row,x6", cu.NF_RUNS, ids=cu.NF_IDS)
def test_nonfinite_input(row, x6, what):
    bind(DEV)
    cu.assert_nonfinite(cu.run_nonfinite(DEV, row, what, x6=x6), row, what, x6)


@pytest.mark.parametrize("what", ["nan", "inf"])
@pytest.mark.parametrize("row", list(cu.HEAD_ROWS))
def test_head_hands_nonfinite_input_on(row, what):
    """The same contract for the output head's two forward forms, whose ReLU sits behind the LayerNorm that spreads the element over the
    item: every prediction of item 0 non-finite, item 1 bitwise that of the clean run."""
    got = cu.run_head_nonfinite(DEV, row, what)
    assert ("head.fc_fwd@0" if row == "fc_fwd" else "head.fwd@0") in got["kernels"], got      # the form the row is in the table for
    assert got["clean_nonfinite"] == 0 and got["chain_words"] == 0 and got["other_item_differs"] == 0, got
    assert got["oracle_nonfinite"] > 0 and got["finite_where_oracle_is_not"] == 0, got
