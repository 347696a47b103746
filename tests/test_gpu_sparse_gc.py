"""-m gpu: the sparse graph shift operator on MI355X (stgcn_kernels_gcsparse.hip.h; harness: tests/sparse_gc_util.py).  All six stage
cases against the float64 stage oracle, the prepare round trip from device arrays, the registry rule, the dense tiled path on the
densified operator, bitwise reproducibility, bf16 activations against the dense tiled bf16 path, and a whole model with a sparse
``gso``: a 3-step trajectory against the oracle, GraphedTrainStep replays against eager fused steps, GraphedEvalPass against the host loop."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import sparse_gc_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BLOCKS = [[1], [64, 16, 64], [64, 16, 64], [128, 128], [1]]


@pytest.mark.parametrize("name", list(U.CASES))
def test_sparse_block_against_stage_oracle(name):
    O, out = U.run_case(DEV, name)
    err = U.stage_errors(O, out)
    print(name, err)
    U.assert_errors(err)


def test_prepare_round_trip_from_device_arrays():
    from stgcn_amd import ops
    U.bind(DEV)
    n = 600
    rows, cols, vals, empty, full, _ = U.ring_entries(n)
    _, coo = U.ring_gso(n)
    m = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    m.sort_indices()
    mt = m.T.tocsr()
    mt.sort_indices()
    gp, gt = ops.gso_prepare(coo.to(DEV), 3)
    assert gp.blob.is_cuda and U.decode_matches(gp, m) and U.decode_matches(gt, mt)
    dense, csr = U.dense_case_gso(35)
    bad = csr.col_indices().clone()
    bad[0] = 35
    with pytest.raises(ValueError, match="column index"):
        ops.gso_prepare(torch.sparse_csr_tensor(csr.crow_indices(), bad, csr.values(), size=(35, 35)).to(DEV), 3)
    crow = csr.crow_indices().clone()
    crow[2] = crow[3] + 1
    with pytest.raises(ValueError, match="monoton"):
        ops.gso_prepare(torch.sparse_csr_tensor(crow, csr.col_indices(), csr.values(), size=(35, 35)).to(DEV), 3)


def test_unregistered_operator_is_refused_before_any_launch():
    """A CSR descriptor with the DENSE operator's buffer: STGCN_ERR_INVALID, no launch (empty launch profile), every buffer keeps its fill."""
    from stgcn_amd import _lib, ops
    from tests.emu_util import params_in_field_order
    L = U.bind(DEV)
    c_in, channels, Kt, Ks, gct, act, N, B, T, training, _ = U.CASES["n21"]
    O = U.case_oracle("n21")
    bcfg = ops.BlockConfig(Kt=Kt, Ks=Ks, n_vertex=N, c_in=c_in, channels=channels, act_func=act, graph_conv_type=gct, droprate=0.5, sparse_gso=True)
    desc = ops.make_desc(bcfg, B, T, False, False)
    plan = ops.query_plan(desc)
    prm = [None if t is None else t.to(DEV) for t in params_in_field_order(O.p, "st_blocks.0.", gct)]
    pst = ops._param_struct(_lib.StblockParams, prm)
    x_cl = torch.from_numpy(np.ascontiguousarray(O.x_np.transpose(0, 2, 3, 1))).to(DEV)
    dense = torch.from_numpy(U.dense_case_gso(N)[0]).to(DEV)
    dense_gp, dense_gt = ops.gso_prepare(dense, 3)
    before = dense_gp.clone()
    y = torch.full((B, plan.T2, N, channels[2]), 7.0, device=DEV)
    saved = torch.full((plan.saved_floats,), 7.0, device=DEV)
    ws = torch.full((plan.ws_floats,), 7.0, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    L.dll.stgcn_profile_enable(1)
    rc = L.dll.stgcn_stblock_forward(C.byref(desc), C.byref(pst), x_cl.data_ptr(), dense_gp.data_ptr(), y.data_ptr(), saved.data_ptr(), ws.data_ptr(),
                                     1, 1, None, stream)
    msg = L.dll.stgcn_last_error().decode()
    gst = ops._param_struct(_lib.StblockGrads, [None] * len(_lib.PARAM_FIELDS))
    rc_b = L.dll.stgcn_stblock_backward(C.byref(desc), C.byref(pst), x_cl.data_ptr(), dense_gt.data_ptr(), y.data_ptr(), y.data_ptr(), saved.data_ptr(),
                                        ws.data_ptr(), C.byref(gst), None, 1, 1, None, stream)
    buf = C.create_string_buffer(1 << 14)
    L.dll.stgcn_profile_collect(buf, len(buf))
    L.dll.stgcn_profile_enable(0)
    torch.cuda.synchronize()
    assert rc == 2 and "not a blob" in msg and rc_b == 2
    assert buf.value.decode() == "{}"
    assert bool((y == 7.0).all()) and bool((saved == 7.0).all()) and bool((ws == 7.0).all()) and torch.equal(dense_gp, before)


@pytest.mark.parametrize("name", ["n21", "n150_ks4", "n600_ring"])
def test_sparse_equals_dense_tiled_path_forward(name):
    """A, X_k, G, y against the dense tiled path on the densified operator (set_gc_tiled_min_nodes(1)), at the y bar of
    tests/test_gpu_gctile.py::test_tiled_equals_slab_resident_on_c2.  Gradients are held to the oracle (the stage cases above)."""
    from stgcn_amd import ops
    U.bind(DEV)
    _, a = U.run_case(DEV, name, sparse=True)
    prev = ops.set_gc_tiled_min_nodes(1)
    try:
        _, b = U.run_case(DEV, name, sparse=False)
    finally:
        ops.set_gc_tiled_min_nodes(prev)
    rel = lambda p, q: float(np.abs(p - q).max() / max(1.0, float(np.abs(p).max())))
    errs = {k: rel(a[k], b[k]) for k in ["A", "G", "y"] + [k for k in a if k.startswith("X")]}
    print(name, errs)
    assert all(v < 2e-5 for v in errs.values()), errs


@pytest.mark.parametrize("name", ["n150_ks4", "n600_ring"])
def test_two_runs_are_bitwise_identical(name):
    _, a = U.run_case(DEV, name)
    _, b = U.run_case(DEV, name)
    for k in ["y", "dx", "dA"] + [k for k in a if k.startswith("grad.")]:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


@pytest.mark.parametrize("name", U.BF16_CASES)
def test_bf16_activations_track_the_dense_tiled_bf16_path(name):
    """rms error of X_k, y, dx and every gradient against the float64 oracle: at most 1.25 x the dense tiled bf16 path's on the same case
    (the sparse path keeps L in fp32, so it should be smaller; the 25 % covers different rounding points).  With STGCN_SPARSE_REPORT=<file>
    both columns are appended to it as one JSON line per case (profiles/sparse_gc_stage_errors.md is made from them)."""
    from stgcn_amd import ops
    U.bind(DEV)
    O, a = U.run_case(DEV, name, sparse=True, dtype=torch.bfloat16)
    prev = ops.set_gc_tiled_min_nodes(1)
    try:
        _, b = U.run_case(DEV, name, sparse=False, dtype=torch.bfloat16)
    finally:
        ops.set_gc_tiled_min_nodes(prev)
    ea, eb = U.rms_errors(O, a), U.rms_errors(O, b)
    print(name, {k: (ea[k], eb[k]) for k in ea})
    if os.environ.get("STGCN_SPARSE_REPORT"):
        with open(os.environ["STGCN_SPARSE_REPORT"], "a") as fh:
            fh.write(json.dumps({"case": name, "sparse": ea, "dense": eb}) + "\n")
    bad = {k: (ea[k], eb[k]) for k in ea if not ea[k] <= 1.25 * eb[k]}
    assert not bad, bad


# ---- whole model: STGCNChebGraphConv, N = 40, batch 4, the reference channel plan, a sparse gso
N_MODEL, B_MODEL = 40, 4


def _model(droprate=0.0, seed=3, params=None):
    from stgcn_amd import models
    U.bind(DEV)
    _, coo = U.ring_gso(N_MODEL)
    args = types.SimpleNamespace(Kt=3, Ks=3, act_func="glu", graph_conv_type="cheb_graph_conv", gso=coo.to(DEV), enable_bias=True,
                                 droprate=droprate, n_his=12)
    torch.manual_seed(seed)
    m = models.STGCNChebGraphConv(args, BLOCKS, N_MODEL)
    if params is not None:
        m.load_state_dict(params, strict=True)
    return m.to(DEV)


def test_training_trajectory_matches_oracle():
    """3 AdamW steps (dropout off) against the oracle's own trajectory on the densified operator, at the bars of
    tests/test_gpu_model.py::test_training_trajectory_matches_oracle: losses rtol 1e-4, every parameter within 1e-4."""
    from oracle import stgcn_oracle as orc
    from stgcn_amd.train import make_optimizer, train_step
    cfg = orc.OracleConfig(Kt=3, Ks=3, n_his=12, droprate=0.0, blocks=BLOCKS)
    params = orc.random_params(cfg, N_MODEL, seed=5)
    model = _model(params=params)
    assert all(b.cfg.sparse_gso for b in model.modules() if type(b).__name__ == "STConvBlock")
    rs = np.random.RandomState(6)
    x = torch.from_numpy(rs.standard_normal((B_MODEL, 1, 12, N_MODEL))).float()
    y = torch.from_numpy(rs.standard_normal((B_MODEL, N_MODEL))).float()
    dense = torch.from_numpy(U.ring_gso(N_MODEL)[0]).double()
    p64 = {k: v.detach().clone().double() for k, v in params.items()}
    state, ref_losses = {}, []
    for _ in range(3):
        loss, _ = orc.train_step(x.double(), y.double(), dense, p64, cfg, state)
        ref_losses.append(float(loss))
    model.train()
    opt = make_optimizer(model)
    losses = [float(train_step(model, opt, x.to(DEV), y.to(DEV)).item()) for _ in range(3)]
    assert np.allclose(losses, ref_losses, rtol=1e-4), (losses, ref_losses)
    for k, v in model.state_dict().items():
        ref = p64[k].numpy()
        assert abs(float(v.double().abs().sum()) - np.abs(ref).sum()) <= 1e-4 * np.abs(ref).sum() + 1e-9, k
        assert float(np.abs(v.cpu().numpy() - ref).max()) <= 1e-4, k


def test_graphed_fused_step_equals_eager_fused_steps():
    """GraphedTrainStep replays against eager fused steps of a twin, as tests/test_gpu_optim_kinds.py compares them (AdamW)."""
    from stgcn_amd import DropoutStream
    from stgcn_amd.train import GradArena, GraphedTrainStep, fused_train_step, make_optimizer, train_step
    g = torch.Generator().manual_seed(4)
    xs = torch.randn(5, B_MODEL, 1, 12, N_MODEL, generator=g).to(DEV)
    ys = torch.randn(5, B_MODEL, N_MODEL, generator=g).to(DEV)
    DropoutStream.use_device_counter(torch.device(DEV))
    DropoutStream.manual_seed(3)
    try:
        m1 = _model()
        o1 = make_optimizer(m1, capturable=True)
        gs = GraphedTrainStep(m1, o1, xs[0], ys[0], warmup=2)
        assert gs.fused
        l1 = [float(gs(xs[i], ys[i]).item()) for i in range(1, 5)]
        torch.cuda.synchronize()
        gs.close()
    finally:
        DropoutStream.disable_device_counter()
    m2 = _model()
    o2 = make_optimizer(m2)
    train_step(m2, o2, xs[0], ys[0])
    arena = GradArena([p for p in m2.parameters() if p.grad is not None])
    for _ in range(2):
        fused_train_step(m2, o2, xs[0], ys[0], arena)
    l2 = [float(fused_train_step(m2, o2, xs[i], ys[i], arena).item()) for i in range(1, 5)]
    assert np.allclose(l1, l2, rtol=1e-5, atol=0), (l1, l2)
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    for k in sd1:
        assert float((sd1[k] - sd2[k]).abs().max()) <= 2e-5, k


def test_graphed_eval_pass_equals_host_metrics():
    from stgcn_amd import data
    from stgcn_amd.train import GraphedEvalPass
    model = _model(droprate=0.5)
    rs = np.random.RandomState(9)
    raw = 50.0 + 10.0 * rs.standard_normal((40, N_MODEL))
    z = data.ZScore().fit(raw)
    series = z.transform(raw)
    n_his, n_pred = 12, 3
    with GraphedEvalPass(model, series, n_his, n_pred, B_MODEL, scaler=z) as ev:
        assert ev.graph is not None
        got = ev.run()
        assert ev.run() == got
    sampler = data.WindowSampler(series, n_his, n_pred, DEV)
    mse = data.evaluate_model(model, torch.nn.MSELoss(), sampler.batches(B_MODEL))
    mae, rmse, wmape = data.evaluate_metric(model, sampler.batches(B_MODEL), z)
    assert got["windows"] == len(sampler)
    assert abs(got["mse"] - mse) <= 1e-4 and abs(got["mae"] - mae) <= 1e-4 and abs(got["rmse"] - rmse) <= 1e-4 and abs(got["wmape"] - wmape) <= 1e-5, \
        (got, mse, mae, rmse, wmape)
