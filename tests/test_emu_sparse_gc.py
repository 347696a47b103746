"""Sparse graph shift operator on the CPU emulator (stgcn_kernels_gcsparse.hip.h, harness: tests/sparse_gc_util.py): the CSR operator
products on the tiled recursion against the float64 stage oracle, the prepare round trip and its refusals, the registry rule, the
comparison with the dense tiled path, bitwise reproducibility, bf16 activations, the module path and the broadcast of a sparse
operator between two gloo ranks.  Every test fails without the feature: a sparse ``gso`` raises there."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from stgcn_amd import _lib, ops
from tests import sparse_gc_util as U
from tests.emu_util import bind_emulator

DEV = "cpu"


@pytest.mark.parametrize("name", U.EMU_CASES)
def test_sparse_block_against_stage_oracle(name):
    O, out = U.run_case(DEV, name)
    U.assert_errors(U.stage_errors(O, out))


def test_prepare_round_trip_and_refusals():
    bind_emulator()
    # operator (ii): unsorted COO with a duplicate, an empty row, a full row and a stored zero
    n = 40
    rows, cols, vals, empty, full, zero_at = U.ring_entries(n)
    _, coo = U.ring_gso(n)
    m = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()      # (tocsr sums the duplicates and sorts the columns)
    m.sort_indices()
    assert m.nnz == rows.size - 1 and m[zero_at] == 0.0 and m.indptr[empty + 1] == m.indptr[empty] and m.indptr[full + 1] - m.indptr[full] == n
    gp, gt = ops.gso_prepare(coo, 3)
    mt = m.T.tocsr()
    mt.sort_indices()
    assert U.decode_matches(gp, m) and U.decode_matches(gt, mt)
    assert np.flatnonzero((gp.decode()[2] == 0.0)).size == 1            # the explicit zero stays a stored entry
    # operator (i) as CSR, and through data.gso_tensor(sparse=True)
    dense, csr = U.dense_case_gso(21)
    from stgcn_amd import data
    for t in (csr, data.gso_tensor(sp.csr_matrix(dense), DEV, sparse=True)):
        assert t.layout == torch.sparse_csr
        gp, gt = ops.gso_prepare(t, 3)
        md = sp.csr_matrix(dense)
        md.sort_indices()
        mdt = sp.csr_matrix(dense.T)
        mdt.sort_indices()
        assert U.decode_matches(gp, md) and U.decode_matches(gt, mdt)
    # refusals, on the host, before anything is prepared
    crow, col, val = csr.crow_indices().clone(), csr.col_indices().clone(), csr.values().clone()
    bad_col = col.clone()
    bad_col[3] = 21
    with pytest.raises(ValueError, match="column index"):
        ops.gso_prepare(torch.sparse_csr_tensor(crow, bad_col, val, size=(21, 21)), 3)
    bad_row = crow.clone()
    bad_row[4], bad_row[5] = crow[5], crow[4] - 1
    assert bad_row[5] < bad_row[4]
    with pytest.raises(ValueError, match="monoton"):
        ops.gso_prepare(torch.sparse_csr_tensor(bad_row, col, val, size=(21, 21)), 3)
    with pytest.raises(ValueError, match="column index"):
        ops.gso_prepare(torch.sparse_coo_tensor(torch.tensor([[0, 1], [2, -1]]), torch.tensor([1.0, 2.0]), size=(21, 21)), 3)
    # the library checks what it is handed as well (a caller that skips the Python layer)
    L = _lib.lib()
    rp = torch.tensor([0, 1, 2, 2], dtype=torch.int32)
    blob = torch.zeros(64)
    cl_, vl = torch.tensor([0, 3], dtype=torch.int32), torch.ones(2)
    rc = L.dll.stgcn_gso_csr_prepare(rp.data_ptr(), cl_.data_ptr(), vl.data_ptr(), 3, 2, blob.data_ptr(), None)
    assert rc == 2 and "outside" in L.dll.stgcn_last_error().decode()
    # a row pointer that overshoots nnz before it comes back (0, 5, 2 with nnz = 2): refused from rowptr alone, `col` is never walked
    rp2, cl2 = torch.tensor([0, 5, 2], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32)
    rc = L.dll.stgcn_gso_csr_prepare(rp2.data_ptr(), cl2.data_ptr(), vl.data_ptr(), 2, 2, blob.data_ptr(), None)
    assert rc == 2 and "rowptr" in L.dll.stgcn_last_error().decode()
    assert L.dll.stgcn_gso_csr_release(blob.data_ptr()) == 2             # nothing was registered


def test_unregistered_operator_is_refused_before_any_launch():
    """A CSR descriptor with a dense buffer in the operator's place: STGCN_ERR_INVALID, and nothing ran -- the output, `saved` and the
    workspace keep their fill, the launch profile stays empty.  A blob prepared for another N and a released blob are refused too."""
    L = bind_emulator()
    c_in, channels, Kt, Ks, gct, act, N, B, T, training, _ = U.CASES["n21"]
    O = U.case_oracle("n21")
    bcfg = ops.BlockConfig(Kt=Kt, Ks=Ks, n_vertex=N, c_in=c_in, channels=channels, act_func=act, graph_conv_type=gct, droprate=0.5, sparse_gso=True)
    desc = ops.make_desc(bcfg, B, T, False, False)
    assert desc.graph_conv == 2
    plan = ops.query_plan(desc)
    from tests.emu_util import params_in_field_order
    pst = ops._param_struct(_lib.StblockParams, params_in_field_order(O.p, "st_blocks.0.", gct))
    x_cl = torch.from_numpy(np.ascontiguousarray(O.x_np.transpose(0, 2, 3, 1)))
    dense = torch.from_numpy(U.dense_case_gso(N)[0]).contiguous()
    dense_before = dense.clone()
    _, other = U.dense_case_gso(N + 1)
    gp_other, _ = ops.gso_prepare(other, 3)
    gp_ok, gt_ok = ops.gso_prepare(U.dense_case_gso(N)[1], 3)
    released = gp_ok.blob
    gp_ok._finalizer()                                                    # (what collecting the object does)
    for operand, what in ((dense, "not a blob"), (gp_other.blob, "prepared for N = 22"), (released, "not a blob")):
        y = torch.full((B, plan.T2, N, channels[2]), 7.0)
        saved = torch.full((plan.saved_floats,), 7.0)
        ws = torch.full((plan.ws_floats,), 7.0)
        L.dll.stgcn_profile_enable(1)
        rc = L.dll.stgcn_stblock_forward(C.byref(desc), C.byref(pst), x_cl.data_ptr(), operand.data_ptr(), y.data_ptr(), saved.data_ptr(), ws.data_ptr(),
                                         1, 1, None, None)
        msg = L.dll.stgcn_last_error().decode()
        buf = C.create_string_buffer(1 << 14)
        L.dll.stgcn_profile_collect(buf, len(buf))
        L.dll.stgcn_profile_enable(0)
        assert rc == 2 and what in msg, (rc, msg)
        assert buf.value.decode() == "{}", buf.value
        assert bool((y == 7.0).all()) and bool((saved == 7.0).all()) and bool((ws == 7.0).all())
        gst = ops._param_struct(_lib.StblockGrads, [None] * len(_lib.PARAM_FIELDS))
        rc = L.dll.stgcn_stblock_backward(C.byref(desc), C.byref(pst), x_cl.data_ptr(), operand.data_ptr(), y.data_ptr(), y.data_ptr(), saved.data_ptr(),
                                          ws.data_ptr(), C.byref(gst), None, 1, 1, None, None)
        assert rc == 2 and what in L.dll.stgcn_last_error().decode()
        assert bool((ws == 7.0).all())
    assert torch.equal(dense, dense_before)


def test_dense_descriptor_bytes_unchanged():
    bind_emulator()
    for gct, code in (("cheb_graph_conv", 0), ("graph_conv", 1)):
        a = ops.BlockConfig(3, 3, 21, 1, (64, 16, 64), "glu", gct, 0.5)                       # positional, as before the field existed
        b = ops.BlockConfig(Kt=3, Ks=3, n_vertex=21, c_in=1, channels=(64, 16, 64), act_func="glu", graph_conv_type=gct, droprate=0.5,
                            sparse_gso=True)
        assert a.sparse_gso is False
        da, db = ops.make_desc(a, 2, 7, True, False), ops.make_desc(b, 2, 7, True, False)
        assert da.graph_conv == code and db.graph_conv == code + 2
        db.graph_conv = code
        assert bytes(da) == bytes(db)


@pytest.mark.parametrize("name", ["n21", "n35_kipf"])
def test_sparse_equals_dense_tiled_path_forward(name):
    """Forward stages against the dense tiled path on the densified operator (the two sum in different orders: round-off only)."""
    bind_emulator()
    _, a = U.run_case(DEV, name, sparse=True)
    prev = ops.set_gc_tiled_min_nodes(1)
    try:
        _, b = U.run_case(DEV, name, sparse=False)
    finally:
        ops.set_gc_tiled_min_nodes(prev)
    rel = lambda p, q: float(np.abs(p - q).max() / max(1.0, float(np.abs(p).max())))      # the y bar of test_tiled_equals_slab_resident_on_c2
    for k in ["A", "G", "y"] + [k for k in a if k.startswith("X")]:
        assert rel(a[k], b[k]) < 2e-5, k


def test_two_runs_are_bitwise_identical():
    _, a = U.run_case(DEV, "n21")
    _, b = U.run_case(DEV, "n21")
    for k in ["y", "dA"] + [k for k in a if k.startswith("grad.")]:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    _, a = U.run_case(DEV, "n35_kipf")
    _, b = U.run_case(DEV, "n35_kipf")
    for k in ["y", "dx"] + [k for k in a if k.startswith("grad.")]:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_bf16_activations_track_the_dense_tiled_bf16_path():
    """bf16 activations, 21-node case (the 150- and 600-node cases run on the GPU): rms error of X_k, y, dx and every gradient against
    the float64 oracle at most 1.25 x the dense tiled bf16 path's on the same case -- the sparse path keeps L in fp32, so it should be
    smaller; the 25 % covers different rounding points."""
    bind_emulator()
    O, a = U.run_case(DEV, "n21", sparse=True, dtype=torch.bfloat16)
    prev = ops.set_gc_tiled_min_nodes(1)
    try:
        _, b = U.run_case(DEV, "n21", sparse=False, dtype=torch.bfloat16)
    finally:
        ops.set_gc_tiled_min_nodes(prev)
    ea, eb = U.rms_errors(O, a), U.rms_errors(O, b)
    print({k: (ea[k], eb[k]) for k in ea})
    bad = {k: (ea[k], eb[k]) for k in ea if not ea[k] <= 1.25 * eb[k]}
    assert not bad, bad


def _model(gso, N):
    from stgcn_amd import models
    args = types.SimpleNamespace(Kt=3, Ks=3, act_func="glu", graph_conv_type="cheb_graph_conv", gso=gso, enable_bias=True, droprate=0.0, n_his=12)
    torch.manual_seed(3)
    return models.STGCNChebGraphConv(args, [[1], [64, 16, 64], [64, 16, 64], [128, 128], [1]], N)


def test_module_with_sparse_gso_matches_dense_module():
    """layers.STConvBlock: a sparse `gso` attribute selects the CSR path (no data_ptr() of a sparse tensor is taken), the prepared
    operator is cached on the index / value arrays, and a training step gives the dense module's loss and gradients to round-off."""
    bind_emulator()
    from stgcn_amd.train import make_optimizer, train_step
    N = 12
    dense, csr = U.dense_case_gso(N, seed=2)
    rs = np.random.RandomState(0)
    x, y = torch.from_numpy(rs.standard_normal((2, 1, 12, N))).float(), torch.from_numpy(rs.standard_normal((2, N))).float()
    ms, md = _model(csr, N), _model(torch.from_numpy(dense), N)
    blocks = [m for m in ms.modules() if type(m).__name__ == "STConvBlock"]
    assert all(b.cfg.sparse_gso for b in blocks)
    ls = float(train_step(ms, make_optimizer(ms), x, y))
    ld = float(train_step(md, make_optimizer(md), x, y))
    assert all(isinstance(b._gso_cache[1], ops.SparseGso) for b in blocks)
    cached = [b._gso_cache[1] for b in blocks]
    ms(x)
    assert all(b._gso_cache[1] is c for b, c in zip(blocks, cached))                       # same arrays: no second prepare
    assert abs(ls - ld) <= 1e-5 * max(1.0, abs(ld))
    for (k, p), (_, q) in zip(ms.named_parameters(), md.named_parameters()):
        assert (p.grad is None) == (q.grad is None), k
        if p.grad is not None:
            assert float((p.grad - q.grad).abs().max()) <= 2e-5 * max(1.0, float(q.grad.abs().max())), k


def test_operator_of_the_other_kind_is_refused():
    """A block's route is fixed by the operator it was built with: replacing a dense `gso` by a sparse one (or the reverse) raises at the
    next forward instead of rewriting the block's configuration under plans and workspaces made from it."""
    bind_emulator()
    N = 12
    dense, csr = U.dense_case_gso(N, seed=2)
    x = torch.zeros(1, 1, 12, N)
    for first, second in ((torch.from_numpy(dense), csr), (csr, torch.from_numpy(dense))):
        m = _model(first, N)
        for b in m.modules():
            if type(b).__name__ == "STConvBlock":
                b.gso = second
        with pytest.raises(ValueError, match="was built with a"):
            m(x)


def _sync_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from stgcn_amd.train import init_distributed, sync_operators
    torch.set_num_threads(1)
    init_distributed("gloo")
    bind_emulator()
    N = 12
    _, gso = U.dense_case_gso(N, seed=2 + rank)      # every rank built ITS OWN operator, with its own number of stored entries
    if rank == 1:      # ... and with other index / value types than rank 0 sends (int32 / float64 against int64 / float32)
        gso = torch.sparse_csr_tensor(gso.crow_indices().to(torch.int32), gso.col_indices().to(torch.int32), gso.values().double(), size=(N, N))
    model = _model(gso, N)
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.standard_normal((2, 1, 12, N))).float()
    before = model(x).detach().clone()
    sync_operators(model)
    blocks = [m for m in model.modules() if type(m).__name__ == "STConvBlock"]
    after = model(x).detach().clone()
    torch.save({"gso": [b.gso.to_dense() for b in blocks], "layout": [str(b.gso.layout) for b in blocks], "before": before, "after": after,
                "inner": [b.graph_conv.cheb_graph_conv.gso.to_dense() for b in blocks]}, out + f".{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_sync_operators_broadcasts_a_sparse_operator(tmp_path):
    import torch.multiprocessing as mp
    from tests.test_dp_gloo import _free_port
    out = str(tmp_path / "s")
    mp.spawn(_sync_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = torch.load(out + ".0"), torch.load(out + ".1")
    g0 = torch.from_numpy(U.dense_case_gso(12, seed=2)[0])
    for r in (r0, r1):
        assert all(l == "torch.sparse_csr" for l in r["layout"])
        for g in r["gso"] + r["inner"]:
            assert torch.equal(g, g0)
    assert torch.equal(r0["before"], r0["after"])
    assert not torch.equal(r1["before"], r1["after"])
    assert torch.equal(r0["after"], r1["after"])
