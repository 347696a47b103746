"""When may a block skip its own LayerNorm-backward row pass?  stgcn_amd/ops.py decides it on the host: a block's forward offers its
LayerNorm (_offer_ln_hook), the fused module that consumes the WHOLE output takes the offer (_take_ln_hook) and marks it ready for the
input gradient it wrote, and the block trusts the partials only if the gradient it receives is that very buffer, unedited
(LnHookState.matches).  A wrong yes gives stale partials and silently wrong dZ2, ln_w, tc2_w and everything upstream.  The cases here run
on the CPU emulator (tests/test_emu_hook_trust.py) and on the MI355X (tests/test_gpu_block_hooks.py) through tests/block_util.py's consumer
mode: one small pair P -> Q (N 19, B 2, training, dropout 0.5), P's gradients against the float64 stage oracle for the dy P actually
received, at block_util's bars; which pass ran is read off the number of ln_bwd_rowstats launches of the backward (Q's own LayerNorm
costs one; P's own pass is the second)."""
import numpy as np
import torch

from stgcn_amd import ops
from tests.block_util import TAMPERS, BlockOracle, assert_errors, bind, make_consumer, run_block_case
from tests.emu_util import params_in_field_order

CHEB = "cheb_graph_conv"
PAIR = (64, (64, 16, 64), 3, 3, CHEB, "glu", 19, 2, 9, True)      # P; Q: a block (64, (64, 16, 64)) on P's T2 = 5 steps
_control = {}


def control(dev):
    """The untampered pair, once per device: its keys hold, one ln_bwd_rowstats launch (Q's own), and the dy / w the tampered runs are
    measured against."""
    if str(dev) not in _control:
        out = {}
        err = run_block_case(dev, *PAIR, debug_stages=False, consumer="block", expect_rowstats=1, outputs=out)
        assert_errors(err)
        _control[str(dev)] = out
    return _control[str(dev)]


def check_tamper(dev, tamper):
    assert tamper in TAMPERS
    dy0 = control(dev)["dy"]
    out = {}
    err = run_block_case(dev, *PAIR, debug_stages=False, consumer="block", tamper=tamper, expect_rowstats=2, outputs=out)
    print(tamper, err)
    # precondition: P really received another gradient than the one Q's epilogue summed over (or the same values in another buffer)
    dy = out["dy"]
    if tamper == "inplace":
        assert np.array_equal(dy, 2 * dy0)
    elif tamper == "second_consumer":
        assert not np.array_equal(dy, dy0) and np.abs(dy - dy0).max() > 1.0      # (+ w, standard normal)
    elif tamper == "batch_slice":
        assert np.array_equal(dy[:1], dy0[:1]) and not dy[1:].any()
    else:
        assert np.array_equal(dy, dy0)
    assert err["grad_none_ok.hook_launches"] == 0, "P did not run its own ln_bwd_rowstats pass"
    assert err["hook.rowstat_nan"] == 0 and "grad.ln_w" in err and "grad.tc2_w" in err and "bwd.dx" in err and "hook.rowstat_gx" in err
    assert_errors(err)


def _forward_only(dev, caches, data_seed):
    """P and Q forward under grad on `caches`, other inputs, no backward; returns the tensors (kept alive by the caller or not)."""
    c_in, channels, Kt, Ks, gct, act, N, B, T, training = PAIR
    O = BlockOracle(*PAIR[:9], data_seed=data_seed, oracle32=False)
    bcfg = ops.BlockConfig(Kt=Kt, Ks=Ks, n_vertex=N, c_in=c_in, channels=channels, act_func=act, graph_conv_type=gct, droprate=0.5)
    gp, gt = ops.gso_prepare(torch.from_numpy(O.gso).to(dev), ops.graph_terms(bcfg))
    params = [None if t is None else t.clone().to(dev).requires_grad_(True) for t in params_in_field_order(O.p, "st_blocks.0.", gct)]
    x = torch.from_numpy(O.x_np).to(dev).requires_grad_(True)
    y = ops.st_conv_block(x, gp, gt, bcfg, params, training, 7, 1, caches["p"])
    y_key = y.permute(0, 2, 3, 1).data_ptr()
    assert y_key in ops._ln_hooks, "P's forward under grad offers its LayerNorm"
    out = make_consumer(dev, "block", None, channels[2], Kt, Ks, gct, act, N, O.T2, 0.5, gp, gt)(caches["q"])(y, training, 8, 1)
    assert y_key not in ops._ln_hooks, "Q's forward takes P's offer"
    return y, out


def check_abandoned_forward(dev):
    """A forward under grad whose backward never runs (an evaluation that forgot no_grad, a step that raised), then a real step on the same
    workspace caches: the abandoned offers are never marked ready, the step uses its own, and the table of offers stays bounded."""
    bind(dev)
    ops.clear_ln_hooks()
    caches = {"p": ops.WorkspaceCache(), "q": ops.WorkspaceCache()}
    kept = _forward_only(dev, caches, data_seed=5)      # (alive during the real step: its addresses cannot be handed out again)
    stale = [s for s, _ in ops._ln_hooks.values()]
    assert len(stale) == 1 and not stale[0].ready       # Q's own offer: nobody consumed Q's output
    err = run_block_case(dev, *PAIR, debug_stages=False, consumer="block", expect_rowstats=1, caches=caches)
    print("after an abandoned forward", err)
    assert_errors(err)
    assert [s for s, _ in ops._ln_hooks.values()] == stale and not stale[0].ready, "the real step leaves no offer of its own behind"
    del kept
    for seed in range(6, 16):                           # ten more abandoned forwards: the oldest offers are evicted
        _forward_only(dev, caches, data_seed=seed)
    assert len(ops._ln_hooks) <= 8 and all(not s.ready for s, _ in ops._ln_hooks.values())
    assert stale[0] not in [s for s, _ in ops._ln_hooks.values()]
    ops.clear_ln_hooks()
    assert not ops._ln_hooks


def check_two_steps(dev):
    """Two steps in a row on the same caches with different inputs (the harness fills the row-partial region with NaN before each
    backward): the second step's partials and gradients are the second step's."""
    bind(dev)
    caches = {}
    for data_seed in (11, 12):
        err = run_block_case(dev, *PAIR, debug_stages=False, consumer="block", expect_rowstats=1, caches=caches, data_seed=data_seed)
        print("step with data seed", data_seed, err)
        assert err["hook.rowstat_nan"] == 0 and "hook.rowstat_gx" in err
        assert_errors(err)
    assert set(caches) == {"p", "q"}


def check_range_cuts(dev, small_cus=4):
    """tc1_bwd's comment made checkable: the explicit fmafs in F exist so that the row partials of a range's last step round like the
    others'.  Pair e64 at B 1, N 33 under a pretended small CU count and the default one; ops.set_tc2ln_peers(1) keeps P's forward route
    the same under both.  The knob is set before P's forward and restored after the whole backward (plans and workspace sizes depend on it)."""
    bind(dev)
    case = (64, (64, 16, 64), 3, 3, CHEB, "glu", 33, 1, 9, True)
    qcfg = ops.BlockConfig(Kt=3, Ks=3, n_vertex=33, c_in=64, channels=(64, 16, 64), act_func="glu", graph_conv_type=CHEB, droprate=0.5)
    runs = []
    for cus in (small_cus, 0):
        prev_wgs, prev_peers = ops.set_tc1_bwd_wgs(cus), ops.set_tc2ln_peers(1)
        try:
            out = {}
            err = run_block_case(dev, *case, debug_stages=False, consumer="block", expect_rowstats=1, outputs=out)
            out["q_part_floats"] = ops.query_plan(ops.make_desc(qcfg, 1, 5, True, True)).part_floats
        finally:
            ops.set_tc1_bwd_wgs(prev_wgs)
            ops.set_tc2ln_peers(prev_peers)
        print("pretended CUs", cus, err)
        assert_errors(err)
        runs.append(out)
    a, b = runs
    bits = lambda v: np.ascontiguousarray(v).view(np.uint32)
    # precondition: Q's tc1_bwd ran on different workgroup counts (one partial block each: 3 items x 5 steps give 4 and 7), the same forward
    assert a["q_part_floats"] != b["q_part_floats"]
    assert np.array_equal(bits(a["y"]), bits(b["y"]))
    assert np.array_equal(bits(a["dy"]), bits(b["dy"])), "Q's input gradient depends on where the ranges were cut"
    diff = int((bits(a["hook.rowstat"]) != bits(b["hook.rowstat"])).sum())
    assert diff == 0, f"{diff} row partials depend on where the ranges were cut"
