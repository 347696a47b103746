// Sparse graph shift operator: the operator products of the tiled graph conv (stgcn_kernels_gctile.hip.h) from a CSR operator.
// Road networks of the sizes the tiled path was added for (thousands of nodes) have tens of neighbours per sensor; the dense GEMM
// pays 2 NP^2 16 slabs FLOPs per term whatever L contains, this kernel pays nnz 16 slabs FMAs and gathers nnz rows of 64 B (fp32) or
// 32 B (bf16) per slab.  It has exactly the semantics of gso_gemm_kernel,
//     out[s][n][c] = alpha * sum_m M[n][m] X[s][m][c] + b1 * Z1[s][n][c] + b2 * Z2[s][n][c]        n < N, s < slabs
// (Z1 / Z2 nullable; out may alias Z1 or Z2: every element is read and written by the same lane; X must not alias out), so it drops
// into launch_gconv_fwd_tiled / launch_gconv_bwd_tiled and the row passes, the X_k and the Clenshaw buffers stay what they are.
//
// GATHER form only: the forward reads CSR(L), the backward CSR(L^T) built once at prepare time.  A destination element is summed by
// ONE lane over its row's entries in stored order -- no atomics, two runs leave identical bits.  fp32 accumulation; the operator values
// stay fp32 for both activation types.
//
// Blob (stgcn_gso_csr_layout / stgcn_gso_csr_prepare), in 4-byte words:
//     [0, 16)                     header: kCsrMagic, N, nnz, then zeros
//     [16, 16 + rup4(N + 1))      rowptr, int32
//     [.., + rup4(nnz))           col, int32: sorted and unique within a row
//     [.., + rup4(nnz))           val, fp32
#pragma once
#include "stgcn_device.hip.h"

namespace stgcn {

constexpr unsigned kCsrMagic = 0x31525343u;   // "CSR1"
constexpr int kCsrHdr = 16;
constexpr int kSpSlabs = 16;                  // slabs of a workgroup's slab group: one wave-instruction covers all of them
constexpr int kSpInflight = 8;                // operator entries a wave keeps in flight
inline long csr_rup4(long v) { return (v + 3) / 4 * 4; }
inline long csr_off_col(int N) { return kCsrHdr + csr_rup4((long)N + 1); }
inline long csr_off_val(int N, long nnz) { return csr_off_col(N) + csr_rup4(nnz); }
inline long csr_blob_floats(int N, long nnz) { return csr_off_val(N, nnz) + csr_rup4(nnz); }

// device arrays -> blob (one launch: header, rowptr, col, val)
__global__ __launch_bounds__(256) void gso_csr_pack_kernel(const int* rowptr, const int* col, const float* val, int N, int nnz, float* blob) {
    int* const bi = reinterpret_cast<int*>(blob);
    const long oc = kCsrHdr + ((long)N + 1 + 3) / 4 * 4, ov = oc + ((long)nnz + 3) / 4 * 4, total = ov + ((long)nnz + 3) / 4 * 4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int w = 0;
        if (i < kCsrHdr) w = i == 0 ? (int)kCsrMagic : i == 1 ? N : i == 2 ? nnz : 0;
        else if (i < oc) w = i - kCsrHdr <= N ? rowptr[i - kCsrHdr] : 0;
        else if (i < ov) w = i - oc < nnz ? col[i - oc] : 0;
        else if (i - ov < nnz) w = __builtin_bit_cast(int, val[i - ov]);
        bi[i] = w;
    }
}

struct GsoSpmmArgs {
    const int* rowptr;   // [N + 1]
    const int* col;      // [nnz]
    const float* val;    // [nnz]
    const float* X;      // [slabs][N][16] ET
    const float* Z1;
    const float* Z2;
    float* out;
    float alpha, b1, b2;
    int N, node_chunks, nodes_per_wg, slab_groups;   // a workgroup: nodes_per_wg consecutive destination nodes x 16 slabs
    long slabs;
};

// Workgroup = 4 waves on one (slab group, node run) item; items that share a slab group are consecutive and xcd_item gives consecutive
// items to one XCD, so the X rows a group gathers are re-read through ONE L2.  Wave w takes the run's nodes w, w + 4, ..: neighbouring
// destination nodes of a road graph share source rows, and the four waves then gather them at the same time.
// Lane = (slab lane >> 2 of the group, channels 4 (lane & 3) ..+3): one wave-instruction reads the rows X[s][col][:] of ONE operator
// entry for 16 slabs -- 16 segments of 64 B (fp32) / 32 B (bf16).  (col, val) are wave-uniform; the compiler reads them with vector
// loads of one address all the same (it does not prove the index arrays unwritten, so no s_load), which is why they are requested a
// batch ahead: the kSpInflight gathers of a batch are issued back to back (checked in the ISA).  A row longer than that is walked in order by its one wave: correct for any length, and
// as fast as the entry stream allows; rows of thousands of entries among rows of tens would want the split of a work queue, which no
// measured operator asks for (DESIGN.md "Sparse graph shift operator").
template <typename ET>
__global__ __launch_bounds__(256) void gso_spmm_kernel(GsoSpmmArgs a) {
    const ET* const X_ = et_ptr<ET>(a.X);
    const ET* const Z1_ = et_ptr<ET>(a.Z1);
    const ET* const Z2_ = et_ptr<ET>(a.Z2);
    ET* const out_ = et_ptr<ET>(a.out);
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int item = xcd_item((int)blockIdx.x, a.node_chunks * a.slab_groups);
    const int sg = item / a.node_chunks, chunk = item - sg * a.node_chunks;
    const long slab = (long)sg * kSpSlabs + (lane >> 2);
    const bool in = slab < a.slabs;
    const long slabc = in ? slab : a.slabs - 1;                       // (clamped: the gathers below are unconditional)
    const ET* const xs = X_ + (size_t)slabc * a.N * 16 + 4 * (lane & 3);
    const int n_end = (chunk + 1) * a.nodes_per_wg < a.N ? (chunk + 1) * a.nodes_per_wg : a.N;
    for (int n = chunk * a.nodes_per_wg + w; n < n_end; n += 4) {
        const int e0 = a.rowptr[n], e1 = a.rowptr[n + 1];
        f32x4 acc = zero4();
        // The index stream runs one batch AHEAD of the gathers: (col, val) of a batch are requested together, and those of the next batch
        // right behind this batch's gathers, so no gather waits for an index load issued after the gather before it -- the kSpInflight
        // gathers of a batch leave back to back and a batch costs one memory latency, not one per entry.
        int cj[kSpInflight];
        float vj[kSpInflight];
        auto load_entries = [&](int e) {
#pragma unroll
            for (int j = 0; j < kSpInflight; ++j) {
                const bool ok = e + j < e1;
                const int ej = ok ? e + j : e1 - 1;                    // (past the row: its last entry again, weight 0)
                cj[j] = a.col[ej];
                const float vv = a.val[ej];                            // (unconditional: a select, not a branch around the load)
                vj[j] = ok ? vv : 0.f;
            }
        };
        if (e0 < e1) load_entries(e0);
        for (int e = e0; e < e1; e += kSpInflight) {
            Raw4<ET> xr[kSpInflight];
            float v[kSpInflight];
#pragma unroll
            for (int j = 0; j < kSpInflight; ++j) {
                xr[j] = ldraw4(xs + (size_t)cj[j] * 16);
                v[j] = vj[j];
            }
            if (e + kSpInflight < e1) load_entries(e + kSpInflight);
#pragma unroll
            for (int j = 0; j < kSpInflight; ++j) {
                const f32x4 x = cvt4(xr[j]);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = fmaf(v[j], x[i], acc[i]);
            }
        }
        if (in) {
            const size_t o = ((size_t)slab * a.N + n) * 16 + 4 * (lane & 3);
            f32x4 r;
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] = a.alpha * acc[i];
            if (a.Z1) {
                const f32x4 z = ldx4(Z1_ + o);
#pragma unroll
                for (int i = 0; i < 4; ++i) r[i] += a.b1 * z[i];
            }
            if (a.Z2) {
                const f32x4 z = ldx4(Z2_ + o);
#pragma unroll
                for (int i = 0; i < 4; ++i) r[i] += a.b2 * z[i];
            }
            stx4(out_ + o, r);
        }
    }
}

}  // namespace stgcn
