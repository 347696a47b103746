#!/usr/bin/env python3
"""Sparse against dense graph shift operator at the C5 block shapes (8192 nodes, Ks 5, batch 16; BASELINE.json configs[4]), on ONE
operator: a seeded graph with a fixed number of entries per row runs through the dense tiled path (densified) and through the CSR path,
alternating in one invocation, after a warm-up.  Times are the library's own kernel timer (hipEvent pairs, eager launches).

    python tools/sparse_gc_ab.py [--per-row 16 64] [--dtypes f32 bf16] [--blocks 0 1] [--iters 5] [--reps 2] [--md profiles/sparse_gc_cost.md]

Prints one JSON line per (entries per row, dtype, block): per-launch us of the gso_spmm_* and of the gso_gemm_* launches, their ratio, the
block's forward + backward time on either path, and the bytes one sparse launch gathers (nnz x slabs x 16 channels x element size,
computed from shapes).  --md writes the same rows as a table."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stgcn_amd import _lib, ops  # noqa: E402
from tests.emu_util import block_case, params_in_field_order  # noqa: E402

DEV = "cuda:0"


def fixed_degree_operator(n, per_row, seed):
    """(crow, col, val): per_row distinct random columns in every row, values U(-1, 1) / per_row (infinity norm <= 1), columns sorted."""
    rs = np.random.RandomState(seed)
    col = np.empty((n, per_row), np.int64)
    for i in range(n):
        col[i] = np.sort(rs.choice(n, per_row, replace=False))
    val = (rs.uniform(-1, 1, (n, per_row)) / per_row).astype(np.float32)
    return np.arange(0, n * per_row + 1, per_row, dtype=np.int64), col.reshape(-1), val.reshape(-1)


def profile(L, fn, iters):
    L.dll.stgcn_profile_enable(1)
    for i in range(iters):
        fn(i)
    torch.cuda.synchronize()
    buf = C.create_string_buffer(1 << 15)
    L.check(L.dll.stgcn_profile_collect(buf, len(buf)), "collect")
    L.dll.stgcn_profile_enable(0)
    return json.loads(buf.value.decode())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--Ks", type=int, default=5)
    ap.add_argument("--per-row", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--dtypes", nargs="+", default=["f32", "bf16"], choices=["f32", "bf16"])
    ap.add_argument("--blocks", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    L = _lib.lib()
    assert L.backend == "hip-gfx950"
    channels, Kt, gct = (64, 16, 64), 3, "cheb_graph_conv"
    rows = []
    for per_row in a.per_row:
        crow, col, val = fixed_degree_operator(a.N, per_row, seed=per_row)
        csr = torch.sparse_csr_tensor(torch.from_numpy(crow), torch.from_numpy(col), torch.from_numpy(val), size=(a.N, a.N)).to(DEV)
        dense = csr.to_dense()
        sp_ops = ops.gso_prepare(csr, a.Ks)
        de_ops = ops.gso_prepare(dense, a.Ks)
        del dense
        for dt in a.dtypes:
            dtype = torch.bfloat16 if dt == "bf16" else torch.float32
            for block in a.blocks:
                c_in, T = (1, 12) if block == 0 else (64, 8)
                _, p = block_case(c_in, channels, Kt, a.Ks, gct, "glu", a.N, a.B, T)
                g = torch.Generator().manual_seed(0)
                x = torch.randn(a.B, c_in, T, a.N, generator=g).to(DEV).to(dtype).requires_grad_(c_in > 1)
                dy = torch.randn(a.B, channels[2], T - 4, a.N, generator=g).to(DEV).to(dtype)
                paths = {}
                for name, (gp, gt), sparse in (("dense", de_ops, False), ("sparse", sp_ops, True)):
                    bcfg = ops.BlockConfig(Kt=Kt, Ks=a.Ks, n_vertex=a.N, c_in=c_in, channels=channels, act_func="glu", graph_conv_type=gct, droprate=0.5,
                                           tag=block, sparse_gso=sparse)
                    params = [None if t is None else t.clone().to(DEV).requires_grad_(True) for t in params_in_field_order(p, "st_blocks.0.", gct)]
                    wsc = ops.WorkspaceCache()

                    def step(i, gp=gp, gt=gt, bcfg=bcfg, params=params, wsc=wsc):
                        ops.st_conv_block(x, gp, gt, bcfg, params, True, 7, i + 1, wsc).backward(dy)
                    paths[name] = step
                for step in paths.values():          # warm-up of both paths
                    for i in range(2):
                        step(i)
                torch.cuda.synchronize()
                acc = {"dense": {}, "sparse": {}}
                for _ in range(a.reps):              # alternating
                    for name, step in paths.items():
                        for k, v in profile(L, step, a.iters).items():
                            e = acc[name].setdefault(k, [0, 0.0])
                            e[0] += v["calls"]
                            e[1] += v["total_ms"]
                per_launch = lambda d, prefix: 1e3 * sum(v[1] for k, v in d.items() if k.startswith(prefix)) / max(1, sum(v[0] for k, v in d.items() if k.startswith(prefix)))
                total = lambda d: 1e3 * sum(v[1] for v in d.values()) / (a.reps * a.iters)
                slabs = a.B * (T - Kt + 1)
                row = {"per_row": per_row, "dtype": dt, "block": block, "slabs": slabs,
                       "spmm_us": round(per_launch(acc["sparse"], "gso_spmm"), 1), "gemm_us": round(per_launch(acc["dense"], "gso_gemm"), 1),
                       "block_sparse_us": round(total(acc["sparse"]), 1), "block_dense_us": round(total(acc["dense"]), 1),
                       "gathered_MB": round(a.N * per_row * slabs * 16 * (2 if dt == "bf16" else 4) / 1e6, 1),
                       "launches_per_step": sum(v[0] for k, v in acc["sparse"].items() if k.startswith("gso_spmm")) // (a.reps * a.iters)}
                row["ratio"] = round(row["spmm_us"] / row["gemm_us"], 4)
                row["gather_GBps"] = round(row["gathered_MB"] * 1e3 / row["spmm_us"], 1)
                rows.append(row)
                print(json.dumps(row), flush=True)
        del sp_ops, de_ops
        torch.cuda.empty_cache()
    if a.md:
        with open(a.md, "w") as fh:
            fh.write("| entries / row | activations | block | slabs | gso_spmm us / launch | gso_gemm us / launch | sparse / dense | gathered MB / launch | "
                     "gather GB/s | block fwd + bwd sparse us | dense us |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                fh.write(f"| {r['per_row']} | {r['dtype']} | {r['block']} | {r['slabs']} | {r['spmm_us']} | {r['gemm_us']} | {r['ratio']} | {r['gathered_MB']} | "
                         f"{r['gather_GBps']} | {r['block_sparse_us']} | {r['block_dense_us']} |\n")
    return rows


if __name__ == "__main__":
    main()
