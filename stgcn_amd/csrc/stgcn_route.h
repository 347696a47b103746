// Host side only: which kernels serve an ST block, and with which geometry.  route_block() decides that ONCE per call; the plan, the weight
// pack, the forward, the backward and the gradient flush all read the BlockRoute it returns (as the output head reads its HeadGeom).
// Included by stgcn_capi.hip behind the kernel headers; the LDS-size functions it calls describe a kernel's layout and live with the kernels.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include "../../include/stgcn_hip.h"

namespace stgcn {

inline int64_t rup(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// ---- environment knobs: every getenv of the host code.  "read once": latched at first use; "read per call": the tests switch it between calls
inline int env_int(const char* name, int unset) {
    const char* e = getenv(name);
    return e ? atoi(e) : unset;
}
inline bool env_not_zero(const char* name) {   // on unless the value starts with '0'
    const char* e = getenv(name);
    return !(e && e[0] == '0');
}
// STGCN_FUSE=<bit mask> (read once): which fused kernels replace the stage-per-launch path.  Default: everything on; 0 reproduces the round-1
// launch sequence (A/B runs, stage tests).
//    1 = tc2_bwd_kernel (LayerNorm/dropout/gate backward + tmp_conv2 weight gradient + transposed conv in one launch).
//    2 = tc2_ln_fwd_kernel (tmp_conv2 + gate + LayerNorm + dropout of one slab per workgroup).
//    4 = LayerNorm-backward row partials in the epilogue of the kernel that produces dy (stgcn_ln_hook).
//    8 = tc1_bwd_kernel (Align + gate backward + tmp_conv1 weight gradient + transposed conv in one launch).
//   16 = tc1_fwd_kernel (time-stepping tmp_conv1 + gate + Align forward, weights stationary).
enum FuseBit { FUSE_TC2_BWD = 1, FUSE_TC2_LN_FWD = 2, FUSE_ROWSTATS = 4, FUSE_TC1_BWD = 8, FUSE_TC1_FWD = 16, FUSE_HEAD_LN_FWD = 32, FUSE_HEAD_LN_BWD = 64 };
inline int fuse_mask() { static const int m = env_int("STGCN_FUSE", 0x7fffffff); return m; }
// The thin first layer (K = Kt * c_in <= 4) as wave-per-tile kernels (round 5, stgcn_kernels_thin.hip.h); STGCN_THIN=0 selects the row-tile
// kernels of rounds 1 - 4 (A/B runs; the stage tests run both).  Read per call.
inline bool thin_wave_tiles() { return env_not_zero("STGCN_THIN"); }
// "bf16x6" product form of the fp32 blocks (Frag3, stgcn_device.hip.h): fp32-accurate products on the bf16 matrix pipe, operands split once at
// their producer -- the default of tc1_fwd / tc2_ln_fwd / tc1_bwd since round 6 (measured error against the fp64 stage oracle equal to the
// fp32-MFMA path's, profiles/r6-29_x6_errors.txt).  STGCN_MFMA_X6=0 selects v_mfma_f32_16x16x4_f32 for every product (read per call: bench.py
// reports that step as config.secondary_fp32_mfma, the stage tests run both).
inline bool mfma_x6() { return env_not_zero("STGCN_MFMA_X6"); }
// Where the backward takes the dropout mask of a block's LayerNorm from (tc2_bwd_kernel, the stgcn_ln_hook epilogues): read off the block
// output y -- the forward stores a dropped element as -0.0 and a kept exact zero as +0.0 (drop_encode, stgcn_device.hip.h), so the test is
// exact (round 4's "kept iff y != 0" lost a kept zero: ADVICE r4) -- or regenerated (Philox: ~100 VALU instructions per 4 elements in the
// consumers' time steps; measured on C2 fp32, pass r5-01: tc2_bwd 29.1 + 21.1 -> 28.3 + 20.2 us, tc1_bwd 61.7 -> 60.1, step 0.3756 -> 0.3679 ms).
// STGCN_HOOK_MASK=philox / y forces one (read per call: tests run both forms of both types).
inline bool hook_mask_from_y() {
    const char* e = getenv("STGCN_HOOK_MASK");
    return !(e && e[0] == 'p');
}
// STGCN_LAUNCH_LOG=<file> (read once): see launch_log
inline FILE* launch_log_file() { static FILE* f = getenv("STGCN_LAUNCH_LOG") ? fopen(getenv("STGCN_LAUNCH_LOG"), "w") : nullptr; return f; }
// STGCN_TCONV4=0 (read once, A/B knob): the head's conv and its dense transposed conv leave tconv_fwd4_kernel
inline bool tconv4_off() { static const bool off = env_int("STGCN_TCONV4", 1) == 0; return off; }
// STGCN_HEAD_FC_TILE = 16 | 32 (read per call: the tests switch it): rows of an fc tile of the head, 0 when unset
inline int head_fc_tile_knob() {
    const char* e = getenv("STGCN_HEAD_FC_TILE");
    return !e ? 0 : atoi(e) == 32 ? 32 : 16;
}
// The head's forward as ONE launch (head_fwd_kernel, stgcn_kernels_fwd.hip.h): default on; STGCN_HEAD_FUSE=0 restores the conv + fc launches
// (A/B runs), 2 / 4 admit only the 32- / 64-row tile (tests).  Read per call.  The exchange of the row statistics relies on write-through stores.
inline int head_fuse_mode() {
#if !STGCN_WT_STORES
    return 0;
#else
    return env_int("STGCN_HEAD_FUSE", 1);
#endif
}
// tuning / test knobs that force one instance of a leaf launcher (0 = its heuristic); read once unless said otherwise
inline int ln_stats_min_chunks() { static const int v = env_int("STGCN_LN_STATS_MIN_CHUNKS", 8); return v; }   // chunks per slab from which ln_slab_stats_kernel runs
inline int force_tconv_tile_rows() { static const int v = env_int("STGCN_TCONV_TR", 0); return v; }
inline int force_gemm_ntw() { static const int v = env_int("STGCN_GEMM_NTW", 0); return v; }
inline int force_gemm_bf16_bk() { static const int v = env_int("STGCN_GEMM_BF16_BK", 0); return v; }
inline int gemm_big_bk() { static const int v = env_int("STGCN_GEMM_BIG_BK", 64) == 32 ? 32 : 64; return v; }   // r3-17: 64-deep steps 6 % faster
inline int force_bwd_data_waves() { static const int v = env_int("STGCN_BWD_DATA_WAVES", 0); return v; }
inline int force_gcbwd2_parts() { return env_int("STGCN_GCBWD2_PARTS", 0); }   // (read per call: the tests force geometries)
inline void gc_parts_override(int& fwd, int& bwd) {   // STGCN_GC_PARTS=<f>,<b>
    static int f = 0, b = 0, init = 0;
    if (!init) {
        init = 1;
        const char* e = getenv("STGCN_GC_PARTS");
        if (e) sscanf(e, "%d,%d", &f, &b);
    }
    if (f > 0) fwd = f;
    if (b > 0) bwd = b;
}
inline bool reduce_log() { static const bool on = getenv("STGCN_REDUCE_LOG") != nullptr; return on; }   // diagnostic: the partial-sum tables one launch folds
// element count of a batch from which stgcn_eval_accumulate takes the partial-slab form (STGCN_EVAL_BIG, read per call: the tests force
// either form on one shape -- 0 forces the slabs, a huge value the single workgroup)
inline long eval_big_threshold() { const char* e = getenv("STGCN_EVAL_BIG"); return e ? atol(e) : 32768; }

// ---- runtime knobs (stgcn_set_*) and the shape predicates of the fused kernels -------------------------------------------------------------
// stage tests: also write the on-chip intermediates of the fused kernels (dZ2) to their round-1 workspace slots
inline int g_debug_stages = 0;
// test knob (stgcn_set_tc1_bwd_wgs): pretend the device has this many CUs (0 = ask the runtime).  The launch heuristics that size a
// grid by the CU count -- the (item, step) ranges of the two tc1 kernels, the wave count of tc2_ln_fwd -- then take their small-device
// branches on the emulator too: ranges cut inside items, the 8-wave variant of tc2_ln_fwd
inline int g_tc1_bwd_wgs = 0;
inline int runtime_cus() {
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    }
    return cus;
}
inline int device_cus() { return g_tc1_bwd_wgs > 0 ? g_tc1_bwd_wgs : runtime_cus(); }
// workgroups per slab of tc2_ln_fwd_kernel (round 6): 1 when the slabs alone fill the device; 2 / 4 when PP * slabs workgroups still fit the
// compute units one each (the peers exchange their LayerNorm statistics through L2).  stgcn_set_tc2ln_peers forces 1 / 2 / 4 (0 = this rule).
constexpr int kTc2LnMaxPeers = 4;
inline int g_tc2ln_peers = 0;
inline int tc2_ln_peers(int N, long slabs2) {
    const int tiles = (N + 15) / 16;
    int pp = 1;
    if (g_tc2ln_peers > 0) pp = g_tc2ln_peers;
    else if (4 * slabs2 <= device_cus()) pp = 4;
    else if (2 * slabs2 <= device_cus()) pp = 2;
    if (N > 384) pp = 1;                       // (the peer instances hold at most 24 node tiles per slab)
    while (pp > 1 && tiles < 2 * pp) pp >>= 1;   // at least two node tiles per workgroup
    return pp;
}
inline bool tc2_ln_fwd_fused_ok(int c1, int c2, int Kt, int N) {
    return (fuse_mask() & FUSE_TC2_LN_FWD) && c1 == 16 && c2 == 64 && Kt >= 2 && Kt <= 4 && N <= 448 && tc2_ln_fwd_lds_bytes(Kt, N) <= 150 * 1024;
}
// tc2_bwd_kernel recomputes the gate inputs of tmp_conv2 (and the forward does not store them) for bf16 activations, reads the stored
// ones for fp32 (see the kernel's header comment for the measurement)
inline bool tc2_recompute(int dtype_bf16) { return dtype_bf16 != 0; }
// fewest output steps a range of the two tc1 time-stepping kernels is cut down to when a batch offers fewer (window, node tile) items than
// the device has compute units (measured at C2 shapes, profiles/r6-08_tc1_small_batch_ranges.txt: bs 4 tc1_bwd 36.0 -> 21.6 us, tc1_fwd
// 17.6 -> 11.2 us with 2; 1 and 3 are slower -- more partial blocks for the reduction / longer chains)
inline int tc1_min_steps() { return 2; }
// workgroups of a tc1 time-stepping kernel: `per_cu` per CU, each walking an equal-weight range of the (window, node tile, step) sequence.
// Small batches offer fewer items than that: the ranges are then cut INSIDE items (at least tc1_min_steps steps each) instead of leaving one
// workgroup to walk a whole item alone -- the launch is one workgroup's chain, whatever the batch (round 6)
inline int tc1_range_wgs(long items, int steps, int per_cu) {
    const long want = (long)device_cus() * per_cu, by_steps = items * (long)steps / tc1_min_steps(), most = items > by_steps ? items : by_steps;
    return (int)(most < want ? most : want);
}
inline bool tc1_ts_shape(int c_in, int c0, int c1, int Kt) { return c0 == 64 && c1 == 16 && Kt == 3 && (c_in == 16 || c_in == 32 || c_in == 64); }
// shapes tc1_bwd_kernel covers (whether a call uses it also depends on need_dx: the kernel always forms the input gradient)
inline bool tc1_bwd_shape_ok(int c_in, int c0, int c1, int Kt) {
    return (fuse_mask() & FUSE_TC1_BWD) && tc1_ts_shape(c_in, c0, c1, Kt) && tc1_bwd_lds_bytes(c0, c_in, Kt) <= 150 * 1024;
}
inline bool tc1_fwd_shape_ok(int c_in, int c0, int c1, int Kt) { return (fuse_mask() & FUSE_TC1_FWD) && tc1_ts_shape(c_in, c0, c1, Kt); }
// c2 = 64 only: the bound counts the recompute staging (as for bf16), and tc2_bwd_lds_bytes(128, 3, T1 = 3, T2 = 1) is already 113 936
// bytes (80 656 without the staging) against the 81 920 allowed, so no c2 = 128 block can pass it and the dispatch has no such instance
inline bool tc2_bwd_fused_ok(int c1, int c2, int Kt, int T1, int T2) {
    return (fuse_mask() & FUSE_TC2_BWD) && c1 == 16 && c2 == 64 && Kt >= 2 && Kt <= 4 && T1 <= kTsMaxT && tc2_bwd_lds_bytes(c2, Kt, T1, T2) <= 80 * 1024;
}

// ---- which graph-conv implementation a block uses (plan, launchers and stgcn_gso_prepare must agree) -------
// Slab-resident kernels (gconv_fwd_kernel / gconv_bwd_kernel): up to 512 nodes and as many terms as the backward's LDS
// footprint allows; everything else runs the tiled GEMM path of stgcn_kernels_gctile.hip.h.  The node threshold is a
// runtime knob (stgcn_set_gc_tiled_min_nodes) so that both paths can be compared on the same graph.
inline int g_gc_tiled_min_n = 513;
// arithmetic of the operator products on the tiled path: 0 = fp32 MFMA (exact fp32, default), 1 = bf16x3 (split operands,
// fp32-class), 2 = bf16 (stgcn_set_gc_precision; see stgcn_kernels_gctile.hip.h)
inline int g_gc_precision = 0;
// operator products of the slab-resident graph conv (N <= 512): 0 exact fp32 MFMAs, 1 bf16x3 (stgcn_kernels_gcslab16.hip.h)
inline int g_slab_gc_precision = 0;
// matrix products of the BACKWARD kernels of fp32 blocks: 0 exact fp32 MFMAs (default), 1 "bf16x3" (Mma<f32x>: split operands, three bf16
// MFMAs per product, ~2^-16 relative -- inside the 1e-3 gradient bar, outside "exact fp32"; stgcn_set_bwd_precision)
inline int g_bwd_precision = 0;
inline long gc_operand_cols(long slabs) { return (slabs * 16 + 127) / 128 * 128; }   // CP: rows of the bf16 operand form
// rows ALLOCATED per operand plane: the wide column tiles of gso_gemm_bf16_big_kernel (up to 320 columns) may run past CP
inline long gc_operand_alloc(long slabs) { return gc_operand_cols(slabs) + 384; }
// Leading dimension (bf16 elements) of every 16-bit plane (operator hi / lo, operand form).  NP itself is a power-of-two
// multiple of 128 for the sizes that matter (8192 nodes: 16 KiB rows), so the 128 rows of a tile would all start in the same
// L2 channel; the pad (stgcn_set_gc_ld_pad, multiple of 8 elements) staggers them.
inline int g_gc_ld_pad = 0;
inline int gc_plane_ld(int NP) { return NP + g_gc_ld_pad; }
inline bool gc_is_tiled(int N, int terms) {
    if (N >= g_gc_tiled_min_n) return true;
    const long NP = (N + 15) / 16 * 16;
    return ((long)terms * 16 * (NP + 4) + NP * 20) * (long)sizeof(float) > 160 * 1024;
}
inline int gc_padded_nodes(int N, int terms) { return gc_is_tiled(N, terms) ? (N + kGtBM - 1) / kGtBM * kGtBM : (N + 15) / 16 * 16; }
// Sparse operator (graph_conv = STGCN_GC_*_CSR; stgcn_kernels_gcsparse.hip.h): the recursion of the tiled path for ANY node count, its
// operator products through gso_spmm_kernel.  No dense matrix, hence no padded node count beyond the row tiles' (NP = roundup16(N)) and
// no bf16 operand form (ws_XT = 0).  Decided here, from the descriptor alone, so that every entry point that re-derives the route agrees.
inline bool gc_is_csr(int graph_conv) { return graph_conv == STGCN_GC_CHEB_CSR || graph_conv == STGCN_GC_KIPF_CSR; }
inline bool gc_is_kipf(int graph_conv) { return graph_conv == STGCN_GC_KIPF || graph_conv == STGCN_GC_KIPF_CSR; }
// destination nodes per workgroup of gso_spmm_kernel: 4, one node per wave.  STGCN_SPMM_NODES (read once; a multiple of 4) is the knob
// the sweep of profiles/sparse_gc_cost.md is made with.  Measured at the C5 block-0 shape, 16 entries per row, fp32 / bf16 us per launch:
// 4 nodes 234 / 132, 8: 242 / 138, 16: 252 / 145, 32: 264 / 155, 64: 290 / 185 -- short workgroups, many of them in flight per CU
inline int spmm_nodes_per_wg() {
    static const int v = [] { const int e = env_int("STGCN_SPMM_NODES", 4); return e < 4 ? 4 : e > 1024 ? 1024 : e / 4 * 4; }();
    return v;
}

// ================================================================================================
// Geometry of the backward launches and of the partial-sum arena
// ================================================================================================
struct WgradGeom {
    int M, Mtiles, MTW, mchunks, Mpad, NC, rows_per_chunk, chunks;
    long off;   // arena offset: [chunks][Mpad*NC] then [chunks][NC] bias partials
    long floats;
};
// LayerNorm backward on big slabs (N * C / 4 >= 64 * 256 float4 columns, e.g. the 8192-node graph): every workgroup of
// ln_gate_bwd_kernel would rebuild the slab constants c1, c2 from N row partials (colgroups x slabs x N x 8 B: 4 GB at
// C5), so a tiny kernel forms them once per slab (ln_slab_consts_kernel) and the workgroups read two floats per slab.
constexpr int kLnBigColgroups = 64;
struct BwdGeom {
    int ln_spg, ln_sg;       // slabs per group / groups for the LayerNorm parameter partials
    int al_wgs;              // workgroups of align_gate_bwd (grid-stride over 64-row tiles)
    WgradGeom w1, w2;
    long off_ln_g, off_ln_b, off_gc, off_al, total;
    int gc_stride;           // floats per slab in the graph-conv partials: (terms + 1) * 256
    int gc_count;            // partial blocks of the graph conv: slabs (slab kernels) or workgroups of the tiled row pass
    int gc_tiles_per_wg;     // tiled row pass: 16-row tiles per workgroup
    int al_stride;           // floats per workgroup in the align partials: c0*c1 + c1 (+ 16*2*c0 + 2*c0 on the thin path)
    int thin;                // first layer handled by the thin kernels (Kt*c_in <= 4, c0 == 64, c1 == 16)
    int k1;                  // tmp_conv2 / LayerNorm backward fused into tc2_bwd_kernel (no dZ2, no w2 partials; ln_sg = B)
    int node_tiles;          // ceil(N / 16)
    int k1_wgs, k1_stride;   // workgroups (min(B * node_tiles, 2 per CU)) and floats per workgroup (Kt*16*NC2 + NC2) of its dW_eff2 | db_eff2 partials
    long off_k1;
    int k3;                  // tmp_conv1 / Align backward fused into tc1_bwd_kernel (needs need_dx): no dZ1, no w1 / align partials
    int k3_wgs, k3_stride;   // workgroups (one per CU, fewer for small batches) and floats per workgroup
    long off_k3;
};

inline WgradGeom wgrad_geom(long rows, int K, int NC, long off, int target_wgs = 256) {
    WgradGeom g;
    g.M = K;
    g.Mtiles = (K + 15) / 16;
    g.MTW = g.Mtiles <= 3 ? g.Mtiles : 4;   // m-tiles per workgroup (1, 2, 3 or 4)
    g.mchunks = (g.Mtiles + g.MTW - 1) / g.MTW;
    g.Mpad = g.mchunks * g.MTW * 16;
    g.NC = NC;
    // aim at ~target_wgs workgroups in total (256: one per CU; fewer partials to write and re-read), >= 64 rows per chunk
    long target = target_wgs / g.mchunks;
    if (target < 1) target = 1;
    long rpc = (rows + target - 1) / target;
    rpc = (rpc + 63) / 64 * 64;   // whole 64-row reduction steps
    if (rpc < 64) rpc = 64;
    g.rows_per_chunk = (int)rpc;
    g.chunks = (int)((rows + rpc - 1) / rpc);
    g.off = off;
    g.floats = (long)g.chunks * ((long)g.Mpad * NC + NC);
    return g;
}

inline BwdGeom bwd_geom(int B, int T, int N, int c_in, int c0, int c1, int c2, int Kt, int terms, int need_dx, bool sparse_gc = false) {
    BwdGeom g;
    const int T1 = T - Kt + 1, T2 = T1 - Kt + 1;
    const long rows1 = (long)B * T1 * N, rows2 = (long)B * T2 * N, slabs1 = (long)B * T1, slabs2 = (long)B * T2;
    const long n = (long)N * c2, n4 = n / 4;
    const int colgroups = (int)((n4 + kThreads - 1) / kThreads);
    int sg = (512 + colgroups - 1) / colgroups;   // ~512 workgroups
    if (colgroups >= kLnBigColgroups) sg = (4096 + colgroups - 1) / colgroups;   // big slabs (N*C >= 64 K): ~4096 workgroups, short slab walks
    if (sg > slabs2) sg = (int)slabs2;
    if (sg < 1) sg = 1;
    g.ln_spg = (int)((slabs2 + sg - 1) / sg);
    g.ln_sg = (int)((slabs2 + g.ln_spg - 1) / g.ln_spg);
    g.k1 = tc2_bwd_fused_ok(c1, c2, Kt, T1, T2) ? 1 : 0;
    g.node_tiles = (N + 15) / 16;
    {   // tc2_bwd_kernel: whole (window, node tile) items per workgroup, at most two workgroups per CU (its residency: 8 waves of ~100 VGPRs,
        // 57 KB of LDS) -- beyond that a workgroup walks several items and keeps ONE partial block (C2: 416 items -> unchanged)
        const long items = (long)B * g.node_tiles, cap = 2L * device_cus();
        g.k1_wgs = (int)(items < cap ? items : cap);
    }
    g.k1_stride = Kt * 16 * 2 * c2 + 2 * c2;
    if (g.k1) {   // one LayerNorm-parameter partial per window
        g.ln_spg = T2;
        g.ln_sg = B;
    }
    const long tiles1 = (rows1 + kTileRows - 1) / kTileRows;
    g.thin = (Kt * c_in <= 4 && c0 == 64 && c1 == 16) ? 1 : 0;   // thin_tc1_bwd_kernel keeps K <= 4 rows of W_eff in registers
    // grid-stride workgroups of align_gate_bwd (23.5 KB of LDS each: several per CU for latency hiding).  The thin
    // first-layer kernel carries a 13 KB partial per workgroup, so fewer, longer workgroups win there
    // (measured; 512 = 2 resident workgroups per CU at 62 KB of LDS -- a 513th would wait for a second round).
    // (pass r5-04: 256 / 384 / 512 / 768 workgroups are within noise at C2 and C3; at the 1.3 M rows of the 8192-node graph 768 -- three per
    //  CU, the wave-per-tile form's residency -- take 74 us against 81; the row-tile form of STGCN_THIN=0 holds two)
    const int al_cap = g.thin ? (rows1 >= (1L << 18) && thin_wave_tiles() ? 768 : 512) : 1024;
    g.al_wgs = (int)(tiles1 < al_cap ? tiles1 : al_cap);
    long o = 0;
    auto take = [&](long f) { long at = o; o += (f + 63) / 64 * 64; return at; };
    g.off_ln_g = take((long)g.ln_sg * n);
    g.off_ln_b = take((long)g.ln_sg * n);
    g.gc_stride = (terms + 1) * 256;
    g.gc_count = (int)slabs1;
    g.gc_tiles_per_wg = 0;
    if (sparse_gc || gc_is_tiled(N, terms)) {   // ~1024 workgroups, whole groups of 4 tiles (one per wave)
        const long tiles16 = (rows1 + 15) / 16;
        long per = (tiles16 + 1023) / 1024;
        per = (per + 3) / 4 * 4;
        g.gc_tiles_per_wg = (int)per;
        g.gc_count = (int)((tiles16 + per - 1) / per);
    }
    g.off_gc = take((long)g.gc_count * g.gc_stride);
    g.al_stride = c0 * c1 + c1 + (g.thin ? 16 * 2 * c0 + 2 * c0 : 0);
    g.off_al = take((long)g.al_wgs * g.al_stride);
    g.w1 = wgrad_geom(rows1, Kt * c_in, 2 * c0, 0);
    g.w1.off = take(g.w1.floats);
    g.w2 = wgrad_geom(rows2, Kt * c1, 2 * c2, 0);
    g.w2.off = take(g.k1 ? 0 : g.w2.floats);
    g.off_k1 = take(g.k1 ? (long)g.k1_wgs * g.k1_stride : 0);
    g.k3 = (need_dx && !g.thin && tc1_bwd_shape_ok(c_in, c0, c1, Kt)) ? 1 : 0;
    g.k3_wgs = tc1_range_wgs((long)B * g.node_tiles, T, 1);
    g.k3_stride = tc1_bwd_part_floats(c0, c_in, Kt);
    g.off_k3 = take(g.k3 ? (long)g.k3_wgs * g.k3_stride : 0);
    g.total = o;
    return g;
}

// workgroups (4 waves) of the thin forward: two 16-row tiles per wave, at most four workgroups per CU
inline int thin_fwd_wgs(int64_t rows) {
    constexpr int tpw = 2;   // tiles per wave
    const int64_t tiles = (rows + 15) / 16, want = (tiles + 4 * tpw - 1) / (4 * tpw), cap = 4L * device_cus();
    return (int)(want < 1 ? 1 : want < cap ? want : cap);
}

// ---- the route of one ST block call --------------------------------------------------------------------------------------------------------
enum Tc1FwdForm { TC1_FWD_TSTEP, TC1_FWD_THIN, TC1_FWD_ROWTILE };   // tc1_fwd(_x6)_kernel | thin_tc1_fwd_kernel | launch_tconv_fwd
enum BwdForm { BWD_FUSED, BWD_THIN, BWD_STAGED };                   // one time-stepping launch | thin first layer | stage-per-launch kernels

struct BlockRoute {
    // ---- sizes derived from the descriptor
    int T1, T2, NP, KP1, KP2, NC1, NC2, CP_in, CP1, terms;
    int64_t rows0, rows1, rows2, slabs1, slabs2;
    bool bf16;
    // ---- what the weight pack must hold.  From shapes and the fuse mask ONLY, never from need_dx, training or the input taps: the pack launch
    //      of a model (stgcn_prepack) is planned with other flags than the forward and backward that read what it wrote
    bool recompute_tc1;      // K = Kt * c_in <= 16: recomputing Z in backward beats storing 2 x rows1 x c0 (U1 / S1 are not stored)
    bool thin;               // K <= 4, c0 64, c1 16: first layer on the thin kernels (forward: unless STGCN_THIN=0)
    bool dense_W1;           // PK_TCONV_DENSE of tmp_conv1: the recompute and both time-stepping tc1 kernels read it
    bool dense_Wa;           // PK_ALIGN_DENSE: the time-stepping tc1 kernels
    bool dense_Wa_slot;      // its workspace slot (also carved, unused, for the thin layer: ABI offsets)
    bool dense_W2;           // PK_TCONV_DENSE of tmp_conv2: tc2_bwd_kernel
    // ---- forward
    Tc1FwdForm tc1_fwd;
    bool tc1_fwd_x6;         // (time-stepping form) bf16x6 products
    int tc1_fwd_wgs;
    size_t tc1_fwd_lds;
    bool tc2_ln_fused;       // tmp_conv2 + gate + LayerNorm + dropout in tc2_ln_fwd_kernel<64, Kt, tpw, groups, peers>
    bool tc2_ln_x6;
    int tc2_ln_tpw, tc2_ln_groups, tc2_ln_peers, tc2_ln_threads;   // node tiles per wave, tile groups, workgroups per slab
    size_t tc2_ln_lds;
    bool stored_US2;         // the forward stores the gate inputs of tmp_conv2
    // ---- backward
    BwdGeom bg;
    BwdForm tc2_bwd;         // BWD_FUSED (tc2_bwd_kernel) | BWD_STAGED
    bool tc2_bwd_recompute;
    size_t tc2_bwd_lds;
    BwdForm tc1_bwd;         // BWD_FUSED (tc1_bwd(_x6)_kernel) | BWD_THIN | BWD_STAGED
    bool thin_bwd_waves;     // (thin form) wave-per-tile kernel, else the row-tile one
    bool tc1_bwd_x6;
    size_t tc1_bwd_lds;
    bool tiled_gc;           // graph conv on the tiled GEMM path
    bool sparse_gc;          // ... its operator products from a CSR operator (gso_spmm_kernel); implies tiled_gc
    bool bf16_bwd_ok;        // (bf16 calls) every backward stage of this route has a bf16 instance: see bf16_backward_ok
};

// The stage-per-launch backward kernels of round 1 are fp32 only (STGCN_F32_ONLY in their launchers).  A bf16 block's backward therefore
// needs tmp_conv2 on tc2_bwd_kernel, and tmp_conv1 on tc1_bwd_kernel or on the thin kernel -- the thin kernel only without an input
// gradient, which the fp32 transposed conv would have to form.  stgcn_stblock_backward refuses every other bf16 route before its first launch.
inline bool bf16_backward_ok(BwdForm tc2_bwd, BwdForm tc1_bwd, int need_dx) {
    return tc2_bwd == BWD_FUSED && (tc1_bwd == BWD_FUSED || (tc1_bwd == BWD_THIN && !need_dx));
}

inline BlockRoute route_block(const stgcn_stblock_desc* d) {
    BlockRoute r;
    r.T1 = d->T - d->Kt + 1;
    r.T2 = r.T1 - d->Kt + 1;
    r.terms = gc_is_kipf(d->graph_conv) ? 2 : d->Ks;
    r.sparse_gc = gc_is_csr(d->graph_conv);
    r.tiled_gc = r.sparse_gc || gc_is_tiled(d->N, r.terms);
    r.NP = r.sparse_gc ? (d->N + 15) / 16 * 16 : gc_padded_nodes(d->N, r.terms);
    r.KP1 = (int)rup((int64_t)d->Kt * d->c_in, 16);
    r.KP2 = (int)rup((int64_t)d->Kt * d->c1, 16);
    r.NC1 = 2 * d->c0;
    r.NC2 = 2 * d->c2;
    r.CP_in = (int)rup(d->c_in, 16);
    r.CP1 = (int)rup(d->c1, 16);
    r.rows0 = (int64_t)d->B * d->T * d->N;
    r.rows1 = (int64_t)d->B * r.T1 * d->N;
    r.rows2 = (int64_t)d->B * r.T2 * d->N;
    r.slabs1 = (int64_t)d->B * r.T1;
    r.slabs2 = (int64_t)d->B * r.T2;
    r.bf16 = d->dtype == STGCN_DTYPE_BF16;
    r.bg = bwd_geom(d->B, d->T, d->N, d->c_in, d->c0, d->c1, d->c2, d->Kt, r.terms, d->need_dx, r.sparse_gc);
    const bool x6 = mfma_x6() && !r.bf16;
    const bool tc1_fwd_ok = tc1_fwd_shape_ok(d->c_in, d->c0, d->c1, d->Kt), tc1_bwd_ok = tc1_bwd_shape_ok(d->c_in, d->c0, d->c1, d->Kt);
    // ---- packs
    const bool tc1_ts = (tc1_bwd_ok || tc1_fwd_ok) && d->Kt * d->c_in > 4;   // a time-stepping tc1 kernel may serve this shape
    r.recompute_tc1 = d->Kt * d->c_in <= 16;
    r.thin = r.bg.thin;
    r.dense_W1 = r.recompute_tc1 || tc1_ts;
    r.dense_Wa = tc1_ts && !r.thin;
    r.dense_Wa_slot = tc1_ts || r.thin;
    r.dense_W2 = r.bg.k1;
    // ---- tmp_conv1 forward
    // the time-stepping kernel reads dense windows only: weights stationary in registers, every input tile read once (stgcn_kernels_tstep.hip.h)
    if (!r.recompute_tc1 && !d->x_bstride && !d->x_index_dev && tc1_fwd_ok) r.tc1_fwd = TC1_FWD_TSTEP;
    else if (r.thin && thin_wave_tiles()) r.tc1_fwd = TC1_FWD_THIN;   // one wave per 16-row tile, no LDS, no barrier (stgcn_kernels_thin.hip.h)
    else r.tc1_fwd = TC1_FWD_ROWTILE;
    r.tc1_fwd_x6 = x6;
    r.tc1_fwd_lds = tc1_fwd_lds_bytes(d->c_in, d->Kt, x6);
    // one workgroup per CU for fp32 (its steps are bound by the fp32 matrix pipe: a second chain on the CU made it 12 % slower), two for bf16
    // activations (8 x cheaper MFMAs leave a latency chain: C3 34.2 -> 27.1 us, r3-31)
    r.tc1_fwd_wgs = tc1_range_wgs((long)d->B * r.bg.node_tiles, r.T1, r.bf16 ? 2 : 1);
    // ---- tmp_conv2 + LayerNorm forward
    r.tc2_ln_fused = tc2_ln_fwd_fused_ok(d->c1, d->c2, d->Kt, d->N);
    // workgroups per slab (round 6): a slab is one serial chain of ~15 us whatever the batch, so a launch that leaves compute units idle
    // (block 1 of C2: 128 slabs; every small batch) cuts the slab's node tiles over PP workgroups that exchange their statistics
    r.tc2_ln_peers = tc2_ln_peers(d->N, r.slabs2);
    // 16 waves (4 tile groups) when the grid leaves room for it: at most ~2 workgroups per CU
    // (up to 384 nodes = 6 tiles per wave of a four-group workgroup: C3's 325-node slabs ran on 8 waves, one workgroup per CU, two rounds)
    // (the 6-tile form only for bf16 activations: with fp32 fragments it needs more than the 128 registers of a 16-wave workgroup)
    const bool wide = d->N <= (r.bf16 ? 384 : 256) && r.slabs2 <= 2L * device_cus();
    // "bf16x6" products: the 16-wave forms of up to 256 nodes, so x6 implies wide (4 taps: 8 weight plane triples spill)
    r.tc2_ln_x6 = x6 && d->N <= 256 && r.slabs2 <= 2L * device_cus() && d->Kt <= 3;
    if (r.tc2_ln_peers == 2) r.tc2_ln_tpw = d->N <= 256 ? 2 : 3;
    else if (r.tc2_ln_peers == 4) r.tc2_ln_tpw = d->N <= 256 ? 1 : 2;
    else if (wide) r.tc2_ln_tpw = d->N <= 256 ? 4 : 6;
    else r.tc2_ln_tpw = d->N <= 224 ? 7 : 14;   // 8 waves: 7 row tiles per wave of a two-group workgroup, or 14
    r.tc2_ln_groups = r.tc2_ln_tpw >= 7 ? 2 : 4;
    r.tc2_ln_threads = r.tc2_ln_groups * 256;
    r.tc2_ln_lds = tc2_ln_fwd_lds_bytes(d->Kt, d->N, r.tc2_ln_x6);
    // ---- backward
    r.tc2_bwd = r.bg.k1 ? BWD_FUSED : BWD_STAGED;
    r.tc2_bwd_recompute = tc2_recompute(r.bf16);
    r.tc2_bwd_lds = tc2_bwd_lds_bytes(d->c2, d->Kt, r.T1, r.T2, r.tc2_bwd_recompute);
    r.stored_US2 = !r.tc2_ln_fused || !r.bg.k1 || g_debug_stages || !r.tc2_bwd_recompute;
    r.tc1_bwd = r.bg.k3 ? BWD_FUSED : r.thin ? BWD_THIN : BWD_STAGED;
    r.thin_bwd_waves = thin_wave_tiles();
    r.tc1_bwd_x6 = x6 && g_bwd_precision == 0 && tc1_bwd_lds_bytes(d->c0, d->c_in, d->Kt, true) <= 160 * 1024;   // "bf16x6" weight-gradient products
    r.tc1_bwd_lds = tc1_bwd_lds_bytes(d->c0, d->c_in, d->Kt, r.tc1_bwd_x6);
    r.bf16_bwd_ok = bf16_backward_ok(r.tc2_bwd, r.tc1_bwd, d->need_dx);
    return r;
}

}  // namespace stgcn
