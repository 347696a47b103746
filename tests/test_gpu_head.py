"""-m gpu: the output head's launch paths, stage by stage, on the MI355X against the float64 stage oracle (tests/head_util.py).

Every branch of head_geom / stgcn_outblock_forward / outblock_backward_impl (stgcn_amd/csrc/stgcn_capi_head.inc) that the C2 / C3 head
(c_in 64, channels (128, 128), Ko 4, T = Ko, need_dx, 32 <= N <= 325) does not take has a row in CASES; the numbers in brackets are the
numbered branches of that list.  tests/test_emu_head.py runs the rows that are small enough on the CPU emulator.
"""
import os

import numpy as np
import pytest
import torch

from tests.head_util import assert_head_errors, report_head_errors, run_head_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# name: (c_in, (c0, c1), Ko, N, B, T, act, training, need_dx)
# oracle32: the worst per-tensor / per-slice gradient metric of the stage oracle run in np.float32 against its float64 run, on these
# inputs (head_util's "oracle32.*" keys; the bar is GRAD_TOL / 4 = 2.5e-4) -- what fp32 rounding alone does, measured on the CPU.
CASES = {
    # [6] N < 32: no one-launch forward is admitted -> tconv_fwd4 + fc_fwd_kernel<1> with the LayerNorm fused; dense fused backward
    "a": (64, (128, 128), 4, 21, 2, 4, "glu", True, True),      # oracle32 5.4e-7
    # [1] T1 = 3: launch_tconv_fwd, separate head.ln_fwd, launch_bwd_data with CPin/16 = 4 on the PK_TCONV_BWD pack, un-fused ln_gate_bwd
    "b": (64, (128, 128), 4, 45, 3, 6, "gtu", False, True),      # oracle32 8.0e-7
    # [1] Ko * c_in = 192: not dense at T1 = 1, KP = 192 (KCH = 12), general bwd_data
    "c": (64, (128, 128), 3, 37, 2, 3, "glu", True, True),      # oracle32 4.1e-7
    # [2] dense backward writing dx with outC = 32, outT = 8
    "d": (32, (128, 128), 8, 37, 2, 8, "gtu", False, True),      # oracle32 6.8e-7
    # [2] dense backward with outC = 16, outT = 16
    "e": (16, (128, 128), 16, 33, 2, 16, "glu", True, True),      # oracle32 6.0e-7
    # [2] dense backward with c_in = c0 = 128 (outC = 128, outT = 2), no align
    "f": (128, (128, 128), 2, 40, 2, 2, "gtu", False, True),      # oracle32 1.0e-6
    # [3] [4] [1] c0 = 64 with the align conv folded in (tc_aw / tc_ab reduction jobs), T1 = 2, bwd_data CPin/16 = 8
    "g": (128, (64, 128), 2, 35, 2, 3, "glu", True, True),      # oracle32 6.8e-7
    # [3] c0 = 64 at T1 = 1: fc_bwd_kernel<1,1>, head.ln_bwd_rowstats, un-fused ln_gate_bwd, fc1 packed with KCH = 4, bwd_data CPin/16 = 4
    "h": (64, (64, 128), 4, 70, 3, 4, "gtu", False, True),      # oracle32 6.6e-7
    # [1] [3] CPin/16 = 1, KP = 32
    "i": (16, (64, 128), 2, 33, 2, 2, "glu", True, True),      # oracle32 3.0e-7
    # [5] need_dx = 0: un-fused ln_gate_bwd fed by fc_bwd's epilogue row partials (plain ln_spg / ln_sg grouping); no dx is formed
    "j": (64, (128, 128), 4, 70, 3, 4, "gtu", False, False),      # oracle32 5.1e-7
    # [7] 520 * 128 / 4 / 256 = 65 >= kLnBigColgroups: head.ln_slab_consts and the 4096-based grouping; fused_ln_bwd off (colgroups >= 64)
    "k": (64, (128, 128), 4, 520, 2, 4, "glu", True, True),      # oracle32 9.3e-7
    # [8] N > 1024: one launch of head_fwd_kernel<4> by ticket (tk4) in the default form, un-fused LayerNorm backward (fused_ln_bwd off);
    #     the separate head.ln_fwd launch (fuse_ln off) is reached by the "0" form of this row in test_head_stages_forward_forms
    "l": (64, (128, 128), 4, 1040, 2, 4, "gtu", False, True),      # oracle32 1.5e-6
    # [8] N > 2048: two-launch forward
    "m": (64, (128, 128), 4, 2064, 1, 4, "glu", True, True),      # oracle32 1.1e-6
    # [9] 33 000 rows > 32 768: one_round = false in the weight-gradient geometry (un-paired head.fc1_bwd_weight / head.tconv_bwd_weight);
    #     its default forward is one head_fwd_kernel<4> launch (N <= 2048) -- the forward half of [9], fc_fwd_kernel<2> chosen by the row
    #     count (no STGCN_HEAD_FC_TILE) on a 1032-workgroup grid, with head.ln_fwd, is the "0" form of this row in
    #     test_head_stages_forward_forms
    "n": (64, (128, 128), 4, 1100, 30, 4, "gtu", False, True),      # oracle32 7.0e-6
    # [11] thin head, Ko * c_in = 16
    "o": (4, (128, 128), 4, 33, 2, 4, "glu", True, True),      # oracle32 4.3e-7
    # [11] thin head, Ko * c_in = 12, c_in = 1, c0 = 64
    "p": (1, (64, 128), 12, 33, 2, 12, "gtu", False, True),      # oracle32 6.2e-7
    # [1] [3] c_in = 32, not dense (c0 = 64, T1 = 2): launch_bwd_data with CPin/16 = 2
    "q": (32, (64, 128), 4, 37, 2, 5, "glu", True, True),      # oracle32 6.9e-7
}


def run(name, dev=DEV, label=None, **kw):
    c_in, channels, Ko, N, B, T, act, training, need_dx = CASES[name]
    err = run_head_case(dev, c_in, channels, Ko, N, B, T, act, training, need_dx=need_dx, **kw)
    print(label or name, err)
    if os.environ.get("STGCN_HEAD_REPORT"):
        report_head_errors(err, label or name, os.environ["STGCN_HEAD_REPORT"])
    return err


@pytest.mark.parametrize("name", list(CASES))
def test_head_stages(name):
    assert_head_errors(run(name))


@pytest.mark.parametrize("name", ["a", "h", "k"])
def test_head_stages_fc_tile_32(name, monkeypatch):
    """[10] 32-row tiles of the fc kernels in the backward: fc_bwd_kernel<2,2> (a, k) and <2,1> (h)."""
    monkeypatch.setenv("STGCN_HEAD_FC_TILE", "32")
    assert_head_errors(run(name, label=name + " fc_tile=32"))


@pytest.mark.parametrize("name,mode", [("l", "0"), ("l", "5"), ("n", "0"), ("d", "0"), ("d", "3"), ("d", "5")])
def test_head_stages_forward_forms(name, mode, monkeypatch):
    """Every form of the forward on a head that is not the C2 / C3 one: two launches ("0"; l: with the separate head.ln_fwd; n: with
    fc_fwd_kernel<2> chosen by the row count, [9]), 32- / 64-row tiles by ticket ("3" / "5")."""
    monkeypatch.setenv("STGCN_HEAD_FUSE", mode)
    assert_head_errors(run(name, label=name + " fuse=" + mode))


@pytest.mark.parametrize("name", ["h", "b"])
def test_head_fused_mse_loss(name):
    """stgcn_outblock_backward_loss (ops.mse_backward) through fc_bwd_kernel<1,1> (h) and at T1 = 3 (b): the loss value and every gradient
    against the oracle applied to dout = 2 grad_scale (pred - target) / n."""
    err = run(name, label=name + " fused-loss", loss_scale=0.5)
    assert "loss.rel" in err
    assert_head_errors(err)


# bf16: the general transposed conv (launch_bwd_data) has no bf16 variant, so a bf16 head whose backward is not dense (b: T1 = 3; g, h:
# c0 = 64) and has to form dx is refused -- loudly, in the backward call (STGCN_ERR_UNSUPPORTED -> NotImplementedError, a RuntimeError)
BF16_REFUSED = ("b", "g", "h")
BF16_REFUSAL = "head.tconv_bwd_data: no bf16 variant"


def head_bf16_case(dev, name):
    from tests.bf16_util import assert_bf16_errors, run_head_case_bf16
    from tests.head_util import bind
    bind(dev)
    c_in, channels, Ko, N, B, T, act, training, need_dx = CASES[name]
    go = lambda: run_head_case_bf16(dev, N, B, c_in=c_in, channels=channels, Ko=Ko, act=act, training=training, T=T, need_dx=need_dx)
    if name in BF16_REFUSED:
        with pytest.raises(RuntimeError, match=BF16_REFUSAL):
            go()
        return
    stored, f32 = go()
    print(name, "bf16", stored, f32)
    if os.environ.get("STGCN_HEAD_REPORT"):
        report_head_errors({"stored": stored, "f32": f32}, name + " bf16", os.environ["STGCN_HEAD_REPORT"])
    assert_bf16_errors(stored, f32)


@pytest.mark.parametrize("name", ["a", "b", "g", "h", "j", "l", "n"])
def test_head_bf16(name):
    head_bf16_case(DEV, name)


@pytest.mark.parametrize("n_his", [11, 13])
def test_model_with_a_non_dense_head(n_his):
    """[12] n_his = 11 / 13 (Ko = 3 / 5): the head's backward is not dense, so block 1's LayerNorm hook is served by a separate
    ln_bwd_rowstats pass over dx (hook_pending).  Loss, prediction and every gradient against the float64 model oracle, at the bars
    test_model_matches_reference_golden holds tiny_cheb_f32 to."""
    model_case(DEV, n_his)


def model_case(dev, n_his, N=20, B=2):
    import types
    from oracle import stgcn_oracle as orc
    from stgcn_amd import models
    from tests.head_util import bind
    from tests.helpers import maxabs
    bind(dev)
    blocks = [[1], [64, 16, 64], [64, 16, 64], [128, 128], [1]]
    cfg = orc.OracleConfig(Kt=3, Ks=3, n_his=n_his, droprate=0.0, blocks=blocks)
    assert cfg.Ko == n_his - 8
    rs = np.random.RandomState(n_his)
    a = rs.uniform(-1, 1, (N, N)) * (rs.uniform(size=(N, N)) < 0.6)
    gso = (a / max(1.0, np.abs(np.linalg.eigvals(a)).max())).astype(np.float32)
    p = orc.random_params(cfg, N, seed=n_his)
    args = types.SimpleNamespace(Kt=3, Ks=3, act_func="glu", graph_conv_type="cheb_graph_conv", gso=torch.from_numpy(gso).to(dev),
                                 enable_bias=True, droprate=0.0, n_his=n_his)
    model = models.STGCNChebGraphConv(args, blocks, N)
    model.load_state_dict(p, strict=True)
    model = model.to(dev).train()
    x_np, y_np = rs.standard_normal((B, 1, n_his, N)).astype(np.float32), rs.standard_normal((B, N)).astype(np.float32)
    x, y = torch.from_numpy(x_np).to(dev), torch.from_numpy(y_np).to(dev)
    out = model(x)
    loss = torch.nn.MSELoss()(out.view(B, -1), y)
    loss.backward()
    p64 = {k: v.double() for k, v in p.items()}
    x64, y64, g64 = torch.from_numpy(x_np).double(), torch.from_numpy(y_np).double(), torch.from_numpy(gso).double()
    out_ref = orc.stgcn_forward(x64, g64, p64, cfg)
    loss_ref, grads = orc.loss_and_grads(x64, y64, g64, p64, cfg)
    assert maxabs(out.detach().cpu().numpy(), out_ref.numpy()) <= 1e-4
    assert abs(loss.item() - float(loss_ref)) <= 1e-4 * abs(float(loss_ref))
    for k, prm in model.named_parameters():
        if grads[k] is None:
            assert prm.grad is None, k
            continue
        r = grads[k].numpy()
        g = prm.grad.cpu().numpy()
        assert abs(float(np.abs(g.astype(np.float64)).sum()) - float(np.abs(r).sum())) <= 1e-3 * float(np.abs(r).sum()) + 1e-9, k
        assert maxabs(g, r) <= 1e-3 * max(1e-30, float(np.abs(r).max())) + 1e-7, k
