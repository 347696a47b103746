"""Harness of the sparse graph shift operator (stgcn_kernels_gcsparse.hip.h: CSR operator products on the tiled recursion), shared by
tests/test_emu_sparse_gc.py and tests/test_gpu_sparse_gc.py.

One block is run through the bound library with the operator handed over as a ``torch.sparse_csr`` / ``sparse_coo`` tensor
(``BlockConfig.sparse_gso``) and every stage the sparse path touches -- A, X_k, G, y, then dA, dx and all parameter gradients -- is
compared with the float64 stage oracle (tests/block_util.py: BlockOracle, slice_metrics, bar, assert_errors, unchanged).  The same
runner also takes the DENSE operator, so that the dense tiled path can be run on the densified operator for comparison.

Operators (all non-symmetric, so a wrong transpose shows):
  dense_case_gso(n)   (i)  tests.emu_util.nonsym_gso stored as CSR: every row is long, about 0.6 n entries
  ring_gso(n)         (ii) a ring with 4 neighbours per node plus one EMPTY row, one FULL row and one stored explicit zero, handed over
                           as unsorted COO with a duplicated entry; rows scaled to absolute row sums <= 1 as tests.emu_util.big_gso
"""
import ctypes as C

import numpy as np
import scipy.sparse as sp
import torch

from stgcn_amd import _lib, ops
from tests.bf16_util import bf16_numpy, bf16_tensor, seg_bf16
from tests.block_util import FWD_TOL, BlockOracle, assert_errors, bar, bind, cl, rel, slice_metrics      # noqa: F401 (re-exported)
from tests.emu_util import nonsym_gso, params_in_field_order

# c_in, channels, Kt, Ks, gct, act, N, B, T, training, operator
CASES = {
    "n21": (1, (64, 16, 64), 3, 3, "cheb_graph_conv", "glu", 21, 2, 7, True, "dense"),
    "n35_kipf": (64, (64, 16, 64), 3, 1, "graph_conv", "gtu", 35, 1, 5, False, "dense"),
    "n9_ks5": (16, (128, 16, 64), 2, 5, "cheb_graph_conv", "glu", 9, 2, 5, True, "dense"),             # N < 16
    "n16_ks1": (32, (64, 16, 128), 3, 1, "cheb_graph_conv", "glu", 16, 1, 5, False, "dense"),          # no product at all
    "n150_ks4": (64, (64, 16, 64), 3, 4, "cheb_graph_conv", "glu", 150, 3, 9, True, "dense"),          # 21 slabs: more than 16 and ragged
    "n600_ring": (64, (64, 16, 64), 3, 3, "cheb_graph_conv", "glu", 600, 1, 5, True, "ring"),          # operator (ii)
}
EMU_CASES = ("n21", "n35_kipf", "n9_ks5", "n16_ks1")      # what the emulator affords in a few seconds each; all six run on the GPU
BF16_CASES = ("n21", "n150_ks4", "n600_ring")


def dense_case_gso(n, seed=5):
    """Operator (i): (dense float32 matrix, sparse_csr tensor of its non-zeros)."""
    a = nonsym_gso(n, seed)
    m = sp.csr_matrix(a)
    m.sort_indices()
    t = torch.sparse_csr_tensor(torch.from_numpy(m.indptr.astype(np.int64)), torch.from_numpy(m.indices.astype(np.int64)),
                                torch.from_numpy(m.data.astype(np.float32)), size=(n, n))
    return a, t


def ring_entries(n, seed=7):
    """Operator (ii) as unsorted COO entries with one duplicate: (rows, cols, vals, empty row, full row, (row, col) of the stored zero)."""
    rs = np.random.RandomState(seed)
    empty, full, zero_at = 5 % n, (n // 2 + 1) % n, (3 % n, 4 % n)
    rows, cols, vals = [], [], []
    for i in range(n):
        if i == empty:
            continue
        nb = range(n) if i == full else [(i + d) % n for d in (-2, -1, 1, 2)]
        for j in nb:
            rows.append(i)
            cols.append(j)
            vals.append(rs.uniform(-1, 1))
    rows, cols, vals = np.array(rows), np.array(cols), np.array(vals, dtype=np.float64)
    vals[(rows == zero_at[0]) & (cols == zero_at[1])] = 0.0                       # a STORED zero
    dense = np.zeros((n, n))
    np.add.at(dense, (rows, cols), vals)
    vals = vals / np.abs(dense).sum(1).max()                                        # infinity norm <= 1 (big_gso's scaling)
    k = int(np.flatnonzero(rows == (empty + 1) % n)[0])                             # the duplicate: entry k split into two halves
    rows, cols = np.append(rows, rows[k]), np.append(cols, cols[k])
    vals = np.append(vals, 0.5 * vals[k])
    vals[k] *= 0.5
    perm = rs.permutation(rows.size)                                                # unsorted
    return rows[perm], cols[perm], vals[perm].astype(np.float32), empty, full, zero_at


def ring_gso(n, seed=7):
    """Operator (ii): (dense float32 matrix with the duplicates summed, uncoalesced sparse_coo tensor)."""
    rows, cols, vals, *_ = ring_entries(n, seed)
    dense = np.zeros((n, n), np.float32)
    np.add.at(dense, (rows, cols), vals)
    t = torch.sparse_coo_tensor(torch.from_numpy(np.stack([rows, cols]).astype(np.int64)), torch.from_numpy(vals), size=(n, n))
    assert not t.is_coalesced()
    return dense, t


def case_operator(name):
    N, kind = CASES[name][6], CASES[name][10]
    return dense_case_gso(N) if kind == "dense" else ring_gso(N)


_oracles = {}


def case_oracle(name):
    """The inputs and the float64 oracle of a case, computed once and shared by every test that runs it."""
    if name not in _oracles:
        dense, _ = case_operator(name)
        _oracles[name] = BlockOracle(*CASES[name][:9], gso=dense, oracle32=False)
    return _oracles[name]


def run_case(dev, name, sparse=True, dtype=torch.float32, seed=99, offset=3, oracle=None):
    """One forward + backward of case `name` on `dev`: sparse=True through the CSR path, False through whatever path the DENSE operator
    takes under the current knobs.  Returns (O, out): the case's BlockOracle with its forward computed for this run's dropout mask, and a
    dict of float arrays -- A, X1.., G, y (channels-last), dA, dx (channels-last or None), grad.<param> -- read back from the library's
    buffers (bf16 tensors converted).  oracle: a BlockOracle of the case's shape and operator with inputs of the caller's own
    (tests/conditioning_util.py); None: the shared case_oracle(name)."""
    L = bind(dev)
    cuda = str(dev).startswith("cuda")
    c_in, channels, Kt, Ks, gct, act, N, B, T, training, _ = CASES[name]
    O = case_oracle(name) if oracle is None else oracle
    assert O.args == CASES[name][:9]
    bf = dtype == torch.bfloat16
    dense, sparse_t = case_operator(name)
    bcfg = ops.BlockConfig(Kt=Kt, Ks=Ks, n_vertex=N, c_in=c_in, channels=tuple(channels), act_func=act, graph_conv_type=gct, droprate=O.pdrop,
                           sparse_gso=bool(sparse))
    gp, gt = ops.gso_prepare((sparse_t if sparse else torch.from_numpy(dense)).to(dev), ops.graph_terms(bcfg))
    assert isinstance(gp, ops.SparseGso) == bool(sparse)
    params = [None if t is None else t.clone().to(dev).requires_grad_(True) for t in params_in_field_order(O.p, "st_blocks.0.", gct)]
    to_dev = (lambda a: bf16_tensor(a, dev)) if bf else (lambda a: torch.from_numpy(a).to(dev))
    x = to_dev(O.x_np).requires_grad_(c_in > 1)
    desc = ops.make_desc(bcfg, B, T, training, c_in > 1, dtype=dtype)
    plan = ops.query_plan(desc)
    assert plan.tiled_gc == 1 or not sparse
    if sparse:
        assert plan.NP == (N + 15) // 16 * 16 and plan.ws_XT == plan.ws_part      # no dense padding, no bf16 operand form
    wsc = ops.WorkspaceCache()
    y = ops.st_conv_block(x, gp, gt, bcfg, params, training, seed, offset, wsc)
    y.backward(to_dev(O.dy_np))
    if cuda:
        torch.cuda.synchronize()
    keep = None
    if training:
        keep = ops.dropout_mask(B * O.T2 * N * channels[2], O.pdrop, seed, offset, dev).cpu().numpy().reshape(B, O.T2, N, channels[2]) > 0
    O.forward(keep)
    # the autograd ctx keeps `saved`: a second forward into our own buffers gives it back
    saved = torch.empty(plan.saved_floats, device=dev)
    ws2 = torch.empty(plan.ws_floats, device=dev)
    y2 = torch.empty(B, O.T2, N, channels[2], dtype=dtype, device=dev)
    pst = ops._param_struct(_lib.StblockParams, [None if t is None else t.detach() for t in params])
    x_cl = x.detach().permute(0, 2, 3, 1).contiguous()
    stream = torch.cuda.current_stream().cuda_stream if cuda else None
    L.check(L.dll.stgcn_stblock_forward(C.byref(desc), C.byref(pst), x_cl.data_ptr(), gp.data_ptr(), y2.data_ptr(), saved.data_ptr(),
                                        ws2.data_ptr(), seed, offset, None, stream), "fwd")
    if cuda:
        torch.cuda.synchronize()
    svn, ws = saved.cpu().numpy(), wsc.buf.cpu().numpy()
    T1, c1 = plan.T1, channels[1]
    shape = (B, T1, N, c1)
    n_el = int(np.prod(shape))
    act_units = (n_el + 1) // 2 if bf else n_el

    def seg(buf, off):
        return seg_bf16(buf, off, shape) if bf else buf[off:off + n_el].reshape(shape)

    terms = 2 if gct == "graph_conv" else Ks
    out = {"A": seg(svn, plan.sv_A), "G": seg(svn, plan.sv_G), "dA": seg(ws, plan.ws_dA)}
    for k in range(1, terms):
        out[f"X{k}"] = seg(svn, plan.sv_Xk + (k - 1) * act_units)
    tonp = bf16_numpy if bf else (lambda t: t.detach().cpu().numpy())
    out["y"] = cl(tonp(y))
    out["y2_differs"] = float((y2.view(torch.int16 if bf else torch.int32) != y.detach().permute(0, 2, 3, 1).contiguous().view(torch.int16 if bf else torch.int32)).sum().item())
    out["dx"] = cl(tonp(x.grad)) if c_in > 1 else None
    for nm, prm in zip(_lib.PARAM_FIELDS, params):
        if prm is not None and prm.grad is not None:
            out["grad." + nm] = prm.grad.cpu().numpy()
    return O, out


def oracle_refs(O, out):
    """The float64 references of everything run_case returned: {key: array} with the keys of `out` (ReLU units within FWD_TOL of zero on
    the side the library's G took, as tests/block_util.py does)."""
    c_in, channels, Kt, Ks, gct, act, N, B, T = O.args
    bp, y_ref, sv = O.fwd[np.float64]
    dx_ref, g_ref, stages, _, _, info = O.backward(out["G"].astype(np.float32))
    ref = {"A": sv["A"], "G": sv["G"], "y": y_ref, "dA": stages["dA"], "dx": dx_ref}
    for k in range(1, 2 if gct == "graph_conv" else Ks):
        ref[f"X{k}"] = sv["Xs"][k]
    for nm, g in g_ref.items():
        if g is not None and "grad." + nm in out:
            ref["grad." + nm] = np.asarray(g).reshape(out["grad." + nm].shape)
    return ref, info


def stage_errors(O, out):
    """{key: error} of a run against the float64 stage oracle, with the keys and bars of tests/block_util.py: fwd.A, fwd.X<k>, fwd.G, fwd.y
    (absolute), bwd.dA, bwd.dx, grad.<param> and the slice.* keys (relative to the reference's maximum), kink.* (bar 0)."""
    c_in, channels, Kt, Ks, gct, act, N, B, T = O.args
    ref, info = oracle_refs(O, out)
    err = dict(info)
    for k in ["A", "G", "y"] + [k for k in ref if k.startswith("X")]:
        err["fwd." + k] = float(np.abs(out[k].astype(np.float64) - ref[k]).max())
    err["fwd.y_repeat_bitwise"] = out["y2_differs"]
    err["bwd.dA"] = rel(out["dA"], ref["dA"])
    got = {nm: out.get("grad." + nm) for nm in _lib.PARAM_FIELDS}
    r64 = {nm: ref.get("grad." + nm) for nm in _lib.PARAM_FIELDS}
    err.update(slice_metrics(got, r64, out["dx"], ref["dx"], out["y"], ref["y"], Kt, N, gct))
    for nm in _lib.PARAM_FIELDS:      # no gradient where the oracle has one (or the reverse) is an error, not a skipped key
        if (got[nm] is None) != (r64[nm] is None):
            err["grad_none_ok." + nm] = 1.0
    return err


def rms_errors(O, out):
    """{key: rms(got - oracle) / rms(oracle)} over X_k, y, dx and every parameter gradient (the bf16 comparison of the two paths)."""
    ref, _ = oracle_refs(O, out)
    rms = lambda a: float(np.sqrt((np.asarray(a, np.float64) ** 2).mean()))
    keys = [k for k in ref if k.startswith("X")] + ["y"] + (["dx"] if out["dx"] is not None else []) + [k for k in ref if k.startswith("grad.")]
    return {k: rms(out[k].astype(np.float64) - ref[k]) / max(1e-30, rms(ref[k])) for k in keys}


def decode_matches(sg, m):
    """A prepared ``ops.SparseGso`` against a scipy CSR matrix with sorted indices and summed duplicates: same structure, same values."""
    rowptr, col, val = sg.decode()
    return (np.array_equal(rowptr, m.indptr) and np.array_equal(col, m.indices) and np.array_equal(val, m.data.astype(np.float32))
            and sg.N == m.shape[0] and sg.nnz == m.nnz)
