// Kernels of the fused output head ('TNFF' OutputBlock, reference model/layers.py:260-284):
//   temporal conv (Ko taps) + GLU  -> tconv_fwd_kernel (stgcn_kernels_fwd.hip.h)
//   LayerNorm([N, c0])             -> ln_fwd_kernel
//   fc1 + ReLU + dropout + fc2     -> fc_fwd_kernel            (layers.py:279-282)
// and their backward: fc_bwd_kernel here, LayerNorm / conv backward from stgcn_kernels_bwd.hip.h.
#pragma once
#include "stgcn_kernels_fwd.hip.h"

namespace stgcn {

// ================================================================================================
// fc1 (c0 -> c1) + ReLU + inverted dropout + fc2 (c1 -> 1) on TR-row tiles of the LayerNorm output.
//   hd  = dropout(relu(yln @ W1^T + b1))      saved for backward
//   out = hd @ w2 + b2                        one value per (b, n) row
// wave w owns output-channel tiles w + 4j (NT = c1 / 64); c1 must be 128 (32 float4 columns per row, one
// per lane of a half-wave, so the fc2 dot product is a half-wave shuffle reduction).
// With ln.U set the head's LayerNorm (layers.py:278) runs in the tile staging instead of in its own launch: the rows of a tile belong
// to one or two (b, t) slabs, whose statistics every workgroup rebuilds from the conv epilogue's row partials (N float2 per slab);
// yln is still written (the fc1 weight gradient reads it), mean / rstd by the workgroup that holds the slab's first row.
// ================================================================================================
struct FcFwdArgs {
    TapSrc ts;            // yln [rows][c0] (taps = 1)
    LnFwdArgs ln;         // fused LayerNorm: U, S, gamma, beta, rowstat, y (= yln), mean, rstd, N, C, act, eps; ln.U == null: yln is an input
    const float* W1p;     // packed PK_LIN_FWD: K = c0, cols = c1
    const float* b1;      // [c1] or null
    const float* w2;      // [c1]
    const float* b2;      // [1] or null
    float* hd;            // [rows][c1]
    float* out;           // [rows]
    int KCH, c1, training;
    float keep_scale;
    uint32_t thresh;
    uint64_t seed, offset;
    const uint64_t* offset_dev;
};

template <int WM, typename ET>
__global__ __launch_bounds__(256) void fc_fwd_kernel(FcFwdArgs a) {
    constexpr int TR = WM * 16, NT = 2;
    extern __shared__ float stgcn_smem[];
    float* At = stgcn_smem + kTileHdr;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, l15 = lane & 15;
    const long row0 = (long)xcd_item(blockIdx.x, gridDim.x) * TR;
    const int KP = a.KCH * 16;   // = c0 <= 128
    // every load of the tile is requested up front: the fc1 weight fragments of the whole K (<= 8 chunks), then the rows
    PreW<NT, 8> w;
    pre_load_weights<NT, 8>(w, a.W1p, a.KCH, wave, 4);
    if (a.ln.U) {
        const int N = a.ln.N, C = a.ln.C, c4n0 = C >> 2, lda0 = KP + 4;
        const long rows = a.ts.rows, rend = row0 + TR < rows ? row0 + TR : rows;
        for (long slab = row0 / N; slab * N < rend; ++slab) {   // (uniform: every thread walks the same slabs)
            float mean, rstd;
            slab_stats_from_rows(a.ln.rowstat + (size_t)slab * N, N, C, a.ln.eps, stgcn_smem, mean, rstd);
            if (slab * N >= row0 && threadIdx.x == 0) {
                a.ln.mean[slab] = mean;
                a.ln.rstd[slab] = rstd;
            }
            for (int idx = threadIdx.x; idx < TR * c4n0; idx += kThreads) {
                const int row = idx / c4n0, c4 = idx - row * c4n0;
                const long R = row0 + row;
                if (R >= rows || R / N != slab) continue;
                const int n = (int)(R - slab * N);
                const f32x4 u = ldx4(et_ptr<ET>(a.ln.U) + (size_t)R * C + 4 * c4), sg = ldx4(et_ptr<ET>(a.ln.S) + (size_t)R * C + 4 * c4);
                const f32x4 ga = ld4(a.ln.gamma + (size_t)n * C + 4 * c4), be = ld4(a.ln.beta + (size_t)n * C + 4 * c4);
                f32x4 o;
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = (gate_fwd(u[i], sg[i], a.ln.act) - mean) * rstd * ga[i] + be[i];
                st4(At + row * lda0 + 4 * c4, o);
                stx4_wt(et_ptr<ET>(a.ln.y) + (size_t)R * C + 4 * c4, o);
            }
        }
        for (int idx = threadIdx.x; idx < TR * c4n0; idx += kThreads) {   // rows past the end of the last tile
            const int row = idx / c4n0, c4 = idx - row * c4n0;
            if (row0 + row >= rows) st4(At + row * lda0 + 4 * c4, zero4());
        }
    } else {
        stage_tile_fwd<TR, 4, kThreads, ET>(a.ts, row0, KP, At, KP + 4);
    }
    __syncthreads();
    f32x4 acc[WM][NT];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = zero4();
    pre_mma<WM, NT, 8, ET>(acc, At, KP + 4, 0, a.KCH, w);
    __syncthreads();
    const int c1 = a.c1, ldz = c1 + 4;
    float* Zt = At;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int col = (wave + 4 * j) * 16 + l15;
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) Zt[(i * 16 + 4 * g + r) * ldz + col] = acc[i][j][r];
    }
    __syncthreads();
    const uint64_t off = a.offset + (a.offset_dev ? *a.offset_dev : 0);
    const int c4n = c1 >> 2, c4sh = pow2_shift(c4n);   // 32
    const float b2 = a.b2 ? a.b2[0] : 0.f;
    for (int idx = threadIdx.x; idx < TR * c4n; idx += kThreads) {
        const int row = fast_div(idx, c4n, c4sh), c4 = idx - row * c4n;
        const long R = row0 + row;
        f32x4 h = ld4(Zt + row * ldz + 4 * c4);
        const f32x4 w2 = ld4(a.w2 + 4 * c4);
        if (a.b1) {
            const f32x4 b1 = ld4(a.b1 + 4 * c4);
#pragma unroll
            for (int i = 0; i < 4; ++i) h[i] += b1[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) h[i] = relu_f(h[i]);
        if (a.training) {
            const f32x4 k = dropout_scale4((uint64_t)R * c4n + c4, a.seed, off, a.thresh, a.keep_scale);
#pragma unroll
            for (int i = 0; i < 4; ++i) h[i] *= k[i];
        }
        float p = h[0] * w2[0] + h[1] * w2[1] + h[2] * w2[2] + h[3] * w2[3];
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) p += __shfl_xor(p, m);   // the 32 lanes of a half-wave hold one row
        if (R < a.ts.rows) {
            stx4_wt(et_ptr<ET>(a.hd) + (size_t)R * c1 + 4 * c4, h);
            if (c4 == 0) a.out[R] = p + b2;
        }
    }
}

// ================================================================================================
// Backward of fc2 / dropout / ReLU / fc1 on TR-row tiles (grid-stride, so that partials stay few):
//   dh1 = dout[row] * w2[c] * (hd != 0 ? keep_scale : 0)            (relu' and the dropout mask in one test)
//   dyln = dh1 @ W1                                                   -> [rows][c0]
//   partials: dw2[c] = sum_rows dout * hd ; db2 = sum_rows dout       (dW1 / db1 come from tconv_bwd_weight_kernel)
// ================================================================================================
struct FcBwdArgs {
    const float* dout;    // [rows]
    const float* hd;      // [rows][c1]
    const float* w2;      // [c1]
    const float* W1d;     // packed PK_LIN_BWD: K = c1, cols = c0
    float* dh1;           // [rows][c1]
    float* dyln;          // [rows][c0]
    float* part;          // [wgs][c1 + 2]: dw2 | db2 | sum of the loss terms / n
    long rows;
    int c0, c1, KCH;      // KCH = c1 / 16
    float grad_scale;     // keep_scale when dropout was active, else 1
    // fused loss (pred != null): dout[R] = d loss / d pred[R] * loss_scale (loss_term: 2 (pred[R] - target[R]) / n for MSE) is formed here
    // instead of read from `dout`
    const float* pred;
    const float* target;
    const long* target_index;   // nullable: target += *target_index * target_index_stride
    long target_index_stride;
    // window table (nullable; needs target_index): the target_window_elems values of window b are read at
    // target + target_window[*target_index + b] * target_index_stride  (label_ptr)
    const long* target_window;
    unsigned target_window_elems;
    float loss_scale;
    int loss_kind;        // kLossMse / kLossMae / kLossHuber (checked on the host)
    float loss_delta;     // Huber's switch point (> 0, finite)
    // masked loss (fc_bwd_kernel<.., MASKED = true> only; see the masked forms below): one byte per label, addressed as `target`, and the
    // observed labels per label row of mask_row_elems labels, addressed the same way in units of rows
    const uint8_t* valid;
    const int* row_valid;
    int mask_row_elems;
    LnRowstatOut rs;      // row partials of the head's LayerNorm backward (dyln is its output gradient); rs.rowstat == null: off
};

// Address of label element e of a batch: index mode (tab == nullptr) y already carries the index shift; table mode, window b = e / per_w
// reads its row at y + tab[b] * stride (tab = the table at the batch position).  The label base is offset by n_his + n_pred - 1 series rows,
// so the table of window starts that places the inputs (TapSrc.win_tab) places the labels too.
__device__ __forceinline__ const float* label_ptr(const float* y, const long* tab, long stride, unsigned per_w, long e) {
    if (!tab) return y + e;
    const unsigned eu = (unsigned)e, b = eu / per_w;   // (n < 2^31: checked on the host)
    return y + tab[b] * stride + (eu - b * per_w);
}

// ---- The loss kinds (STGCN_LOSS_*): nn.MSELoss(), nn.L1Loss(), nn.HuberLoss(delta), each a mean over the n predictions ----------------
//     kind    term of d = pred - target                                   d term / d d
//     MSE     d^2                                                         2 d
//     MAE     |d|                                                         sgn(d)
//     Huber   0.5 d^2 if |d| < delta, else delta (|d| - 0.5 delta)        d if |d| < delta, else delta sgn(d)
// sgn(+-0) = 0 as in torch; a NaN difference gives a NaN derivative in EVERY kind (torch's L1 backward turns it into 0): predictions go NaN
// when an in-launch wait gives up, and that has to show in the gradients as well as in the loss value -- `d > 0 ? 1 : d < 0 ? -1 : d`.
// loss_term adds the term to `sum` and returns the derivative over loss_dfactor(kind).  The sum is taken inside each kind's branch and MSE's
// 2 is a factor of its own so that the MSE path keeps the very operations it had before there were kinds (sum += d * d as one fused
// multiply-add; 2 * d / n * scale, resp. (2 * scale / n) * d, in that order): its results stay bit for bit.  `kind` is uniform.
constexpr int kLossMse = 0, kLossMae = 1, kLossHuber = 2;

__device__ __forceinline__ float loss_dfactor(int kind) { return kind == kLossMse ? 2.0f : 1.0f; }

__device__ __forceinline__ float loss_term(int kind, float delta, float d, float& sum) {
    if (kind == kLossMse) {
        sum += d * d;
        return d;
    }
    const float ad = fabsf(d), sg = d > 0.f ? 1.f : d < 0.f ? -1.f : d;
    if (kind == kLossMae) {
        sum += ad;
        return sg;
    }
    if (ad < delta) {
        sum += 0.5f * d * d;
        return d;
    }
    sum += delta * (ad - 0.5f * delta);   // (NaN lands here: |NaN| < delta is false)
    return delta * sg;
}

// ---- The masked forms (stgcn_loss_mask): train on observed labels only --------------------------------------------------------------
//     loss = sum over valid of term / n_valid ;  dpred[e] = valid[e] ? dterm * grad_scale / n_valid : +0.0
// A masked element is SELECTED out: its label and prediction are still loaded (finite or not), its term never reaches the sum and its
// gradient is the constant +0.0, so NaN- or inf-coded missing readings cost nothing.  `valid` (one byte per label) is addressed exactly
// as the labels are (label_at with the same base shift, table, stride and window size); `row_valid` (int32 observed labels per label row
// of row_elems labels) the same way in units of rows.  n_valid is the INTEGER sum of the launch's own rows / row_elems counts, formed by
// every workgroup for itself before it touches an element: exact, order-free, no launch and no host value -- it follows the index word
// and the window table of a captured step.  n_valid == 0: loss 0, every gradient element +0.0.
template <typename T>
__device__ __forceinline__ T label_at(const T* y, const long* tab, long stride, unsigned per_w, long e) {   // label_ptr for any element type
    if (!tab) return y[e];
    const unsigned eu = (unsigned)e, b = eu / per_w;
    return y[tab[b] * stride + (eu - b * per_w)];
}

// the observed labels among the launch's n_rows label rows: thread-strided integer sum, butterfly, the wave sums through `slots` (LDS,
// one int per wave).  Every thread of the workgroup calls and gets the same value; ends with a barrier.
template <int THREADS>
__device__ __forceinline__ int mask_count(const int* row_valid, const long* tab, long stride_rows, unsigned rows_per_w, long n_rows, int* slots) {
    int c = 0;
    for (long r = threadIdx.x; r < n_rows; r += THREADS) c += label_at<int>(row_valid, tab, stride_rows, rows_per_w, r);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m);
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = c;
    __syncthreads();
    int n = 0;
    for (int w = 0; w < THREADS / 64; ++w) n += slots[w];
    return n;
}

// MASKED (the fused loss only): the masked form above.  A template parameter, so that the unmasked instances keep their instructions.
template <int WM, int NT, typename ET, bool MASKED = false>
__global__ __launch_bounds__(256) void fc_bwd_kernel(FcBwdArgs a) {
    constexpr int TR = WM * 16;
    extern __shared__ float stgcn_smem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, l15 = lane & 15;
    const int c1 = a.c1, c0 = a.c0, lda = c1 + 4, c4n = c1 >> 2;
    float* At = stgcn_smem;                // [TR][lda]
    float* red = stgcn_smem + TR * lda;    // [8][c1] + [8] + [8]
    const long tiles = (a.rows + TR - 1) / TR;
    const int c4 = tid % c4n, rsub = tid / c4n;            // c4n == 32 -> rsub in 0..7, fixed channel group per thread
    f32x4 dw2 = zero4();
    float db2 = 0.f, lsum = 0.f;
    const f32x4 w2 = ld4(a.w2 + 4 * c4);
    const float* tgt = a.target;
    const long* ttab = nullptr;
    if (a.pred && a.target_window) ttab = a.target_window + *a.target_index;
    else if (a.pred && a.target_index) tgt += *a.target_index * a.target_index_stride;
    float inv_n = 1.0f / (float)a.rows;
    const uint8_t* vld = a.valid;
    if (MASKED) {   // 1 / n_valid from the row counts of this launch's labels (red is not written before the tile loop's first barrier)
        const int re = a.mask_row_elems;
        const int* rv = a.row_valid;
        if (!ttab && a.target_index) {
            vld += *a.target_index * a.target_index_stride;
            rv += *a.target_index * (a.target_index_stride / re);
        }
        const int nv = mask_count<kThreads>(rv, ttab, a.target_index_stride / re, a.target_window_elems / (unsigned)re, a.rows / re,
                                            reinterpret_cast<int*>(red));
        inv_n = nv > 0 ? 1.0f / (float)nv : 0.f;
    }
    PreW<NT, 8> w;   // fc1 weight fragments of the whole K = c1 (8 chunks), requested before the first tile is touched
    pre_load_weights<NT, 8>(w, a.W1d, a.KCH, wave, 4);
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long row0 = t * TR;
        __syncthreads();
        for (int row = rsub; row < TR; row += kThreads / c4n) {
            const long R = row0 + row;
            f32x4 d = zero4();
            if (R < a.rows) {
                float go;
                if (MASKED) {
                    const float df = a.pred[R] - *label_ptr(tgt, ttab, a.target_index_stride, a.target_window_elems, R);
                    const bool ok = label_at<uint8_t>(vld, ttab, a.target_index_stride, a.target_window_elems, R) != 0;
                    float ls = lsum;   // (the term is added as the unmasked form adds it, and kept only for an observed label)
                    const float gv = loss_dfactor(a.loss_kind) * loss_term(a.loss_kind, a.loss_delta, df, ls) * inv_n * a.loss_scale;
                    go = ok ? gv : 0.f;
                    lsum = ok ? ls : lsum;
                } else if (a.pred) {   // uniform
                    const float df = a.pred[R] - *label_ptr(tgt, ttab, a.target_index_stride, a.target_window_elems, R);
                    go = loss_dfactor(a.loss_kind) * loss_term(a.loss_kind, a.loss_delta, df, lsum) * inv_n * a.loss_scale;   // (lsum: only c4 == 0's is used)
                } else {
                    go = a.dout[R];
                }
                const f32x4 h = ldx4(et_ptr<ET>(a.hd) + (size_t)R * c1 + 4 * c4);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    d[i] = h[i] != 0.f ? go * w2[i] * a.grad_scale : 0.f;
                    dw2[i] += go * h[i];
                }
                if (c4 == 0) db2 += go;
                stx4_wt(et_ptr<ET>(a.dh1) + (size_t)R * c1 + 4 * c4, d);
            }
            st4(At + row * lda + 4 * c4, d);
        }
        __syncthreads();
        f32x4 acc[WM][NT];
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = zero4();
        pre_mma<WM, NT, 8, ET>(acc, At, lda, 0, a.KCH, w);
        if (a.rs.rowstat && c0 == c1) {
            // dyln through the LDS tile: 16-byte row-major stores, and the LayerNorm-backward row partials while the row is on chip
            __syncthreads();   // every wave is done reading At
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int col = (wave + 4 * j) * 16 + l15;
#pragma unroll
                for (int i = 0; i < WM; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) At[(i * 16 + 4 * g + r) * lda + col] = acc[i][j][r];
            }
            __syncthreads();
            const uint64_t hoff = ln_rowstat_offset(a.rs);
            for (int row = rsub; row < TR; row += kThreads / c4n) {   // c4n lanes (half a wave for c0 = 128) hold one row
                const long R = row0 + row;
                const bool rin = R < a.rows;
                const f32x4 v = et_round4<ET>(ld4(At + row * lda + 4 * c4));   // (the row partials below see what the tensor holds)
                if (rin) stx4_wt(et_ptr<ET>(a.dyln) + (size_t)R * c0 + 4 * c4, v);
                const long slab = rin ? R / a.rs.N : 0;
                const int node = rin ? (int)(R - slab * a.rs.N) : 0;
                float2 p = rin ? ln_rowstat4<ET>(a.rs, hoff, v, slab, node, 4 * c4) : make_float2(0.f, 0.f);
                for (int m = c4n >> 1; m >= 1; m >>= 1) {
                    p.x += __shfl_xor(p.x, m);
                    p.y += __shfl_xor(p.y, m);
                }
                if (rin && c4 == 0) a.rs.rowstat[R] = p;
            }
        } else {
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int col = (wave + 4 * j) * 16 + l15;
#pragma unroll
                for (int i = 0; i < WM; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const long R = row0 + i * 16 + 4 * g + r;
                        if (R < a.rows && col < c0) stx1(et_ptr<ET>(a.dyln) + (size_t)R * c0 + col, acc[i][j][r]);
                    }
            }
        }
    }
    __syncthreads();
    st4(red + rsub * c1 + 4 * c4, dw2);
    if (c4 == 0) {
        red[8 * c1 + rsub] = db2;
        red[8 * c1 + 8 + rsub] = lsum;
    }
    __syncthreads();
    float* part = a.part + (size_t)blockIdx.x * (c1 + 2);
    if (tid < c1) {
        float s = 0.f;
        for (int k = 0; k < kThreads / c4n; ++k) s += red[k * c1 + tid];
        part[tid] = s;
    }
    if (tid == 0) {
        float s = 0.f;
        for (int k = 0; k < kThreads / c4n; ++k) s += red[8 * c1 + k];
        part[c1] = s;
        float l = 0.f;
        for (int k = 0; k < kThreads / c4n; ++k) l += red[8 * c1 + 8 + k];
        part[c1 + 1] = l * inv_n;
    }
}

// ================================================================================================
// Multi-tensor AdamW (torch.optim.AdamW as configured at main.py:148: amsgrad False, maximize False):
//     p *= 1 - lr*wd ; m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
// One launch updates every live parameter tensor (those with a gradient); the pointer table travels in the
// kernel arguments.  t and lr may come from device memory so that a captured hipGraph stays correct.
// ================================================================================================
struct AdamwTensor {
    float* p;
    const float* g;
    float* m;
    float* v;
    long n;
};
constexpr int kAdamwMaxTensors = 48;
constexpr int kAdamwChunk = 512;    // small chunks: ~500 workgroups for the 245 K parameters (the kernel is pure latency)
struct AdamwArgs {
    AdamwTensor t[kAdamwMaxTensors];
    int start[kAdamwMaxTensors + 1];
    int count;
    float lr, b1, b2, eps, wd;
    float lb1, lb2;       // log(beta1), log(beta2) computed in double on the host
    long step;
    const long* step_dev;
    const float* lr_dev;
};

__global__ __launch_bounds__(256) void adamw_kernel(AdamwArgs a) {
    int jb = 0;
    while (jb + 1 < a.count && (int)blockIdx.x >= a.start[jb + 1]) ++jb;
    const AdamwTensor& T = a.t[jb];
    const long base = ((long)blockIdx.x - a.start[jb]) * kAdamwChunk;
    // bias corrections 1 - beta^t: -expm1f(t * log(beta)) keeps full relative accuracy for small t (a double-precision
    // pow() here is a multi-microsecond serial latency chain in every thread of a kernel that moves only 1 MB)
    const float t = (float)(a.step_dev ? *a.step_dev : a.step);
    const float lr = a.lr_dev ? *a.lr_dev : a.lr;
    const float bc1 = -expm1f(t * a.lb1);
    const float rs2 = rsqrtf(-expm1f(t * a.lb2));
    const float decay = 1.0f - lr * a.wd, step_size = lr / bc1;
#pragma unroll
    for (int k = 0; k < kAdamwChunk / kThreads; ++k) {
        const long e = base + k * kThreads + threadIdx.x;
        if (e < T.n) {
            const float g = T.g[e];
            const float m = a.b1 * T.m[e] + (1.0f - a.b1) * g;
            const float v = a.b2 * T.v[e] + (1.0f - a.b2) * g * g;
            T.m[e] = m;
            T.v[e] = v;
            T.p[e] = T.p[e] * decay - step_size * (m / (sqrtf(v) * rs2 + a.eps));
        }
    }
}

// The clip form (stgcn_optim_step_clip): adamw_kernel with every gradient element multiplied once by the clip coefficient that
// stgcn_grad_norm / the flush epilogue left in the clip state (clip_publish, stgcn_device.hip.h).  A kernel of its own, so that
// adamw_kernel compiles to the instructions it always had.
__global__ __launch_bounds__(256) void adamw_clip_kernel(AdamwArgs a, const double* clip_state) {
    int jb = 0;
    while (jb + 1 < a.count && (int)blockIdx.x >= a.start[jb + 1]) ++jb;
    const AdamwTensor& T = a.t[jb];
    const long base = ((long)blockIdx.x - a.start[jb]) * kAdamwChunk;
    // bias corrections 1 - beta^t: -expm1f(t * log(beta)) keeps full relative accuracy for small t (a double-precision
    // pow() here is a multi-microsecond serial latency chain in every thread of a kernel that moves only 1 MB)
    const float t = (float)(a.step_dev ? *a.step_dev : a.step);
    const float lr = a.lr_dev ? *a.lr_dev : a.lr;
    const float bc1 = -expm1f(t * a.lb1);
    const float rs2 = rsqrtf(-expm1f(t * a.lb2));
    const float decay = 1.0f - lr * a.wd, step_size = lr / bc1;
    const float coef = clip_coef(clip_state);
#pragma unroll
    for (int k = 0; k < kAdamwChunk / kThreads; ++k) {
        const long e = base + k * kThreads + threadIdx.x;
        if (e < T.n) {
            const float g = coef * T.g[e];
            const float m = a.b1 * T.m[e] + (1.0f - a.b1) * g;
            const float v = a.b2 * T.v[e] + (1.0f - a.b2) * g * g;
            T.m[e] = m;
            T.v[e] = v;
            T.p[e] = T.p[e] * decay - step_size * (m / (sqrtf(v) * rs2 + a.eps));
        }
    }
}

// ================================================================================================
// The global gradient norm of a tensor table (stgcn_grad_norm): the table and the chunks of adamw_kernel (only g and n are read), walked by
// a grid-stride loop of at most kClipMaxWgs workgroups.  Squares and sums are fp64; the order is fixed by the table alone: thread-strided
// chunks, a butterfly over the wave, the wave sums in wave order, then the slots (clip_publish, stgcn_device.hip.h).
// ================================================================================================
constexpr int kClipMaxWgs = 256;
__global__ __launch_bounds__(256) void grad_norm_kernel(AdamwArgs a, ClipArgs c) {
    extern __shared__ float stgcn_smem[];
    double* red = reinterpret_cast<double*>(stgcn_smem);   // [4 waves]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunks = a.start[a.count];
    double s = 0.0;
    int jb = 0;
    for (int ch = (int)blockIdx.x; ch < chunks; ch += (int)gridDim.x) {
        while (jb + 1 < a.count && ch >= a.start[jb + 1]) ++jb;
        const AdamwTensor& T = a.t[jb];
        const long base = ((long)ch - a.start[jb]) * kAdamwChunk;
#pragma unroll
        for (int k = 0; k < kAdamwChunk / kThreads; ++k) {
            const long e = base + k * kThreads + tid;
            if (e < T.n) {
                const double g = (double)T.g[e];
                s = fma(g, g, s);
            }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += shfl_xor_f64(s, m);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (wave != 0) return;
    clip_publish(c, lane < kThreads / 64 ? red[lane] : 0.0, lane);
}

// ================================================================================================
// Multi-tensor NAdamW / Lion (main.py:150 / :152): adamw_kernel's table and chunking, the per-element arithmetic of
// nadamw_element / lion_element (stgcn_kernels_bwd.hip.h, shared with the fused epilogue of reduce_kernel<KIND>).
// Lion has no exp_avg_sq: T.v is never touched.  NAdamW's running product mu_1..mu_t: see OptimExtra.
// ================================================================================================
template <int KIND>
__global__ __launch_bounds__(256) void optim_kernel(AdamwArgs a, OptimExtra x) {
    int jb = 0;
    while (jb + 1 < a.count && (int)blockIdx.x >= a.start[jb + 1]) ++jb;
    const AdamwTensor& T = a.t[jb];
    const long base = ((long)blockIdx.x - a.start[jb]) * kAdamwChunk;
    const float t = (float)(a.step_dev ? *a.step_dev : a.step);
    const OptimScalars s = optim_scalars<KIND>(t, a.lr_dev ? *a.lr_dev : a.lr, a.b1, a.lb2, a.wd, x);
#pragma unroll
    for (int k = 0; k < kAdamwChunk / kThreads; ++k) {
        const long e = base + k * kThreads + threadIdx.x;
        if (e < T.n) {
            float p = T.p[e], m = T.m[e];
            if (KIND == kOptNadamw) {
                float v = T.v[e];
                nadamw_element(T.g[e], p, m, v, a.b2, a.eps, s, x);
                T.v[e] = v;
            } else {
                lion_element(T.g[e], p, m, a.b1, a.b2, s, x);
            }
            T.m[e] = m;
            T.p[e] = p;
            if (KIND == kOptNadamw && x.mu_dev && jb == x.mu_job && e == 0) x.mu_dev[(long)t & 1] = s.mu_prod;
        }
    }
}

// the clip form of optim_kernel<KIND> (stgcn_optim_step_clip), a kernel of its own like adamw_clip_kernel
template <int KIND>
__global__ __launch_bounds__(256) void optim_clip_kernel(AdamwArgs a, OptimExtra x, const double* clip_state) {
    int jb = 0;
    while (jb + 1 < a.count && (int)blockIdx.x >= a.start[jb + 1]) ++jb;
    const AdamwTensor& T = a.t[jb];
    const long base = ((long)blockIdx.x - a.start[jb]) * kAdamwChunk;
    const float t = (float)(a.step_dev ? *a.step_dev : a.step);
    const OptimScalars s = optim_scalars<KIND>(t, a.lr_dev ? *a.lr_dev : a.lr, a.b1, a.lb2, a.wd, x);
    const float coef = clip_coef(clip_state);
#pragma unroll
    for (int k = 0; k < kAdamwChunk / kThreads; ++k) {
        const long e = base + k * kThreads + threadIdx.x;
        if (e < T.n) {
            float p = T.p[e], m = T.m[e];
            const float g = coef * T.g[e];
            if (KIND == kOptNadamw) {
                float v = T.v[e];
                nadamw_element(g, p, m, v, a.b2, a.eps, s, x);
                T.v[e] = v;
            } else {
                lion_element(g, p, m, a.b1, a.b2, s, x);
            }
            T.m[e] = m;
            T.p[e] = p;
            if (KIND == kOptNadamw && x.mu_dev && jb == x.mu_job && e == 0) x.mu_dev[(long)t & 1] = s.mu_prod;
        }
    }
}

// ================================================================================================
// The loss of a training step (mean over all n = B*N elements) and its gradient in ONE launch; nn.MSELoss() (main.py:136):
//     loss = mean((pred - y)^2) ;  dpred = 2 (pred - y) * grad_scale / n
// and likewise nn.L1Loss() / nn.HuberLoss(delta) (loss_term above).
// The reference's loss + l.backward() head is 5 ATen launches (mse, mean, ones_like fill, mse_backward, scale) for 6624
// elements; every launch of this path costs 5-8 us whatever its size.  One workgroup of 1024 threads, fixed summation
// order (bitwise reproducible).
// ================================================================================================
__global__ __launch_bounds__(1024) void loss_grad_kernel(int kind, float delta, const float* pred, const float* y, long n, float gscale,
                                                          float* loss, float* dpred, const long* y_idx_dev, long y_idx_stride,
                                                          const long* y_tab, unsigned y_per_w) {
    const long* tab = nullptr;   // window table at the batch position (label_ptr)
    if (y_tab) tab = y_tab + *y_idx_dev;
    else if (y_idx_dev) y += *y_idx_dev * y_idx_stride;   // labels straight from the resident series (device-side windowing)
    extern __shared__ float stgcn_smem[];   // [16] wave sums
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float k = loss_dfactor(kind) * gscale / (float)n;
    float acc = 0.f;
    for (long e = tid; e < n; e += 1024) {
        const float d = pred[e] - *label_ptr(y, tab, y_idx_stride, y_per_w, e);
        dpred[e] = k * loss_term(kind, delta, d, acc);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
    if (lane == 0) stgcn_smem[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        float s = 0.f;
        for (int w = 0; w < 16; ++w) s += stgcn_smem[w];
        loss[0] = s / (float)n;
    }
}

// The masked form (stgcn_loss_grad_masked; the semantics at label_at above): the same single workgroup, the same walk and summation order,
// n_valid from the row counts first.  With every label observed (n_valid == n, uniform) it performs the operations of loss_grad_kernel on
// the same values: that launch bit for bit.  Otherwise nothing pins the gradient to those operations, and three fp32 roundings (the
// difference, 1 / n_valid, the product) can leave an element 1.8e-7 off: the element is formed in fp64 from the fp32 inputs and rounded
// once (loss_dterm64; one fp64 multiply per element of a launch that is all latency).  The loss value is summed as the unmasked form sums it.
__device__ __forceinline__ double loss_dterm64(int kind, float delta, double d) {   // d term / d d over loss_dfactor(kind), as loss_term returns it
    if (kind == kLossMse) return d;
    const double sg = d > 0.0 ? 1.0 : d < 0.0 ? -1.0 : d;   // (sgn(+-0) = 0, NaN stays NaN)
    if (kind == kLossMae) return sg;
    return fabs(d) < (double)delta ? d : (double)delta * sg;
}

__global__ __launch_bounds__(1024) void loss_grad_masked_kernel(int kind, float delta, const float* pred, const float* y, long n, float gscale,
                                                                 float* loss, float* dpred, const long* y_idx_dev, long y_idx_stride,
                                                                 const long* y_tab, unsigned y_per_w, const uint8_t* valid,
                                                                 const int* row_valid, int row_elems) {
    const long* tab = nullptr;
    if (y_tab) tab = y_tab + *y_idx_dev;
    else if (y_idx_dev) {
        y += *y_idx_dev * y_idx_stride;
        valid += *y_idx_dev * y_idx_stride;
        row_valid += *y_idx_dev * (y_idx_stride / row_elems);
    }
    extern __shared__ float stgcn_smem[];   // [16] wave sums (the row counts first, then the terms)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nv = mask_count<1024>(row_valid, tab, y_idx_stride / row_elems, y_per_w / (unsigned)row_elems, n / row_elems,
                                    reinterpret_cast<int*>(stgcn_smem));
    __syncthreads();   // the counts are read before the slots take the wave sums
    const bool full = (long)nv == n;
    const float k = nv > 0 ? loss_dfactor(kind) * gscale / (float)nv : 0.f;
    const double kd = nv > 0 ? (double)loss_dfactor(kind) * (double)gscale / (double)nv : 0.0;
    float acc = 0.f;
    for (long e = tid; e < n; e += 1024) {
        const float p = pred[e], t = *label_ptr(y, tab, y_idx_stride, y_per_w, e);
        const float d = p - t;
        const bool ok = label_at<uint8_t>(valid, tab, y_idx_stride, y_per_w, e) != 0;
        float s = acc;
        float g = k * loss_term(kind, delta, d, s);
        if (!full) g = (float)(kd * loss_dterm64(kind, delta, (double)p - (double)t));
        dpred[e] = ok ? g : 0.f;
        acc = ok ? s : acc;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
    if (lane == 0) stgcn_smem[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        float s = 0.f;
        for (int w = 0; w < 16; ++w) s += stgcn_smem[w];
        loss[0] = nv > 0 ? s / (float)nv : 0.f;
    }
}

// ================================================================================================
// Evaluation metrics of one minibatch, added into a device-resident state that a whole pass over a split shares
// (script/utility.py:90-101 evaluate_model, :103-121 evaluate_metric), in ONE launch per batch:
//     state[0] += sum (p - y)^2                 z-scored units (the validation loss)
//     state[1] += sum |d| ; state[2] += sum d^2 ; d = (y - p) * scale[node]   (the inverse transform's mean cancels)
//     state[3] += sum (y * scale[node] + mean[node])                           (WMAPE's denominator)
//     state[4] += elements counted
// over the windows b >= first_valid of the batch (the overlapped last batch of a split counts only its new windows).  Terms are formed in
// fp32, sums are carried in fp64 (a split has ~10^6 elements).  The summation order is fixed: thread-strided walks, a butterfly over
// the wave (fp64 travels through the 32-bit shuffles as two words), the wave sums in wave order.  Two forms, by grid size:
//   * one workgroup adds its sums straight into the state;
//   * G > 1 workgroups leave their four sums in the state's partial slabs (state[8 + 4 g ..]), and the LAST ARRIVER at the ticket word
//     (state[6]) adds them up in g order -- never in arrival order, never with floating-point atomics.  Hand-off: plain slab stores by
//     wave 0, drained, agent release, drained, relaxed ticket add; the workgroup that draws G - 1 takes an agent acquire and reads the
//     slabs with the acquiring wave's own loads.  It re-arms the ticket (stgcn_eval_arm zeroes it before the first launch of a pass).
// With `pos` (device words: [0] first window of the batch, [1] first_valid, [2] batches done) the launch reads its position from there
// and ADVANCES it for the next batch: k -> k + 1, start = min(k B, num - B), first_valid = min(B, k B - start), so that a captured batch
// needs no launches of its own to move on.  Every workgroup has read the words before it draws its ticket; the last arriver writes them.
// ================================================================================================
constexpr int kEvalThreads = 1024;
constexpr int kEvalMaxWgs = 64;
constexpr int kEvalHdr = 8;       // fp64 words ahead of the partial slabs: four sums, the count, a spare, the ticket word, a spare
struct EvalAccArgs {
    const float* pred;     // [B][N]
    const float* target;   // label row of window 0 (row b of the batch: + (start + b) * tstride when pos is set, else + b * N)
    const float* scale;    // [N] or null (identity)
    const float* mean;     // [N] or null
    double* state;
    long* pos;             // nullable
    long tstride;
    long first_valid;      // used when pos is null
    long num;              // windows of the split (pos only)
    int B, N;
};

__device__ __forceinline__ void eval_finish(const EvalAccArgs& a, long fv, long k) {   // one thread, after the sums of the batch are in
    a.state[4] += (double)((a.B - fv) * (long)a.N);
    if (a.pos) {
        const long done = (k + 1) * a.B;
        const long start = done < a.num - a.B ? done : a.num - a.B;
        a.pos[0] = start;
        a.pos[1] = done - start < a.B ? done - start : a.B;
        a.pos[2] = k + 1;
    }
}

__global__ __launch_bounds__(1024) void eval_acc_kernel(EvalAccArgs a) {
    extern __shared__ float stgcn_smem[];
    double* red = reinterpret_cast<double*>(stgcn_smem);   // [16 waves][4]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long start = 0, fv = a.first_valid, k = 0;
    if (a.pos) {
        start = a.pos[0];
        fv = a.pos[1];
        k = a.pos[2];
        start = start < 0 ? 0 : (start > a.num - a.B ? a.num - a.B : start);   // (never past the series, whatever the words hold)
    }
    fv = fv < 0 ? 0 : (fv > a.B ? a.B : fv);
    const float* y = a.target + start * a.tstride;
    const long n = (long)a.B * a.N;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (long e = fv * a.N + (long)blockIdx.x * kEvalThreads + tid; e < n; e += (long)gridDim.x * kEvalThreads) {
        const int node = (int)(e % a.N);
        const float p = a.pred[e], t = y[e];
        const float sc = a.scale ? a.scale[node] : 1.0f, mu = a.mean ? a.mean[node] : 0.0f;
        const float dz = p - t, d = (t - p) * sc;
        s0 += (double)(dz * dz);
        s1 += (double)fabsf(d);
        s2 += (double)(d * d);
        s3 += (double)(t * sc + mu);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        s0 += shfl_xor_f64(s0, m);
        s1 += shfl_xor_f64(s1, m);
        s2 += shfl_xor_f64(s2, m);
        s3 += shfl_xor_f64(s3, m);
    }
    if (lane == 0) {
        red[wave * 4 + 0] = s0;
        red[wave * 4 + 1] = s1;
        red[wave * 4 + 2] = s2;
        red[wave * 4 + 3] = s3;
    }
    __syncthreads();
    if (wave != 0) return;
    double t = 0.0;   // lanes 0..3 of wave 0 own one sum each
    if (lane < 4)
        for (int w = 0; w < kEvalThreads / 64; ++w) t += red[w * 4 + lane];
    if (gridDim.x == 1) {
        if (lane < 4) a.state[lane] += t;
        if (lane == 0) eval_finish(a, fv, k);
        return;
    }
    if (lane < 4) a.state[kEvalHdr + 4 * blockIdx.x + lane] = t;
    unsigned* const ticket = reinterpret_cast<unsigned*>(a.state + 6);
    chain_drain_stores();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    chain_drain_stores();   // (fence first, its own wait kept, then the ticket)
    unsigned drawn = 0u;
    if (lane == 0) drawn = chain_add(ticket, 1u);
    drawn = __shfl(drawn, 0);
    if (drawn != gridDim.x - 1u) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    chain_drain_stores();
    if (lane < 4) {
        double tot = 0.0;
        for (unsigned g = 0; g < gridDim.x; ++g) tot += a.state[kEvalHdr + 4 * g + lane];
        a.state[lane] += tot;
    }
    if (lane == 0) {
        eval_finish(a, fv, k);
        chain_st(ticket, 0u);
    }
}

// ================================================================================================
// The masked form (stgcn_eval_accumulate_masked): the sums of eval_acc_kernel over the OBSERVED labels of the counted windows (`valid`,
// one byte per label, addressed as `target`), and two more:
//     state[4] += observed elements             (a sum of ones here, not (B - first_valid) * N)
//     state[5] += sum |d| / |y scale + mean|    (MAPE's numerator; an observed raw label of 0 makes it inf, as in the literature's code)
// A masked element is selected out: whatever its label or prediction holds adds nothing.  The same thread-strided walk, butterfly, wave
// order and ticket hand-off; six sums per workgroup, so the partial slabs are state[8 + 6 g ..].  With every label observed, words 0..4
// take the very values eval_acc_kernel gives them.
// ================================================================================================
constexpr int kEvalMaskedSums = 6;
__device__ __forceinline__ void eval_finish_masked(const EvalAccArgs& a, long k) {   // the position words only: the count is one of the sums
    if (a.pos) {
        const long done = (k + 1) * a.B;
        const long start = done < a.num - a.B ? done : a.num - a.B;
        a.pos[0] = start;
        a.pos[1] = done - start < a.B ? done - start : a.B;
        a.pos[2] = k + 1;
    }
}

__global__ __launch_bounds__(1024) void eval_acc_masked_kernel(EvalAccArgs a, const uint8_t* valid) {
    constexpr int S = kEvalMaskedSums;
    extern __shared__ float stgcn_smem[];
    double* red = reinterpret_cast<double*>(stgcn_smem);   // [16 waves][6]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long start = 0, fv = a.first_valid, k = 0;
    if (a.pos) {
        start = a.pos[0];
        fv = a.pos[1];
        k = a.pos[2];
        start = start < 0 ? 0 : (start > a.num - a.B ? a.num - a.B : start);   // (never past the series, whatever the words hold)
    }
    fv = fv < 0 ? 0 : (fv > a.B ? a.B : fv);
    const float* y = a.target + start * a.tstride;
    const uint8_t* v = valid + start * a.tstride;
    const long n = (long)a.B * a.N;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0;
    for (long e = fv * a.N + (long)blockIdx.x * kEvalThreads + tid; e < n; e += (long)gridDim.x * kEvalThreads) {
        const int node = (int)(e % a.N);
        const float p = a.pred[e], t = y[e];
        const bool ok = v[e] != 0;
        const float sc = a.scale ? a.scale[node] : 1.0f, mu = a.mean ? a.mean[node] : 0.0f;
        const float dz = p - t, d = (t - p) * sc, raw = t * sc + mu;
        if (ok) {
            s0 += (double)(dz * dz);
            s1 += (double)fabsf(d);
            s2 += (double)(d * d);
            s3 += (double)raw;
            s4 += 1.0;
            s5 += (double)(fabsf(d) / fabsf(raw));
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        s0 += shfl_xor_f64(s0, m);
        s1 += shfl_xor_f64(s1, m);
        s2 += shfl_xor_f64(s2, m);
        s3 += shfl_xor_f64(s3, m);
        s4 += shfl_xor_f64(s4, m);
        s5 += shfl_xor_f64(s5, m);
    }
    if (lane == 0) {
        red[wave * S + 0] = s0;
        red[wave * S + 1] = s1;
        red[wave * S + 2] = s2;
        red[wave * S + 3] = s3;
        red[wave * S + 4] = s4;
        red[wave * S + 5] = s5;
    }
    __syncthreads();
    if (wave != 0) return;
    double t = 0.0;   // lanes 0..5 of wave 0 own one sum each
    if (lane < S)
        for (int w = 0; w < kEvalThreads / 64; ++w) t += red[w * S + lane];
    if (gridDim.x == 1) {
        if (lane < S) a.state[lane] += t;
        if (lane == 0) eval_finish_masked(a, k);
        return;
    }
    if (lane < S) a.state[kEvalHdr + S * blockIdx.x + lane] = t;
    unsigned* const ticket = reinterpret_cast<unsigned*>(a.state + 6);
    chain_drain_stores();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    chain_drain_stores();   // (fence first, its own wait kept, then the ticket)
    unsigned drawn = 0u;
    if (lane == 0) drawn = chain_add(ticket, 1u);
    drawn = __shfl(drawn, 0);
    if (drawn != gridDim.x - 1u) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    chain_drain_stores();
    if (lane < S) {
        double tot = 0.0;
        for (unsigned g = 0; g < gridDim.x; ++g) tot += a.state[kEvalHdr + S * g + lane];
        a.state[lane] += tot;
    }
    if (lane == 0) {
        eval_finish_masked(a, k);
        chain_st(ticket, 0u);
    }
}

// a new pass: the sums, the count, the ticket word and the position words start from zero
__global__ __launch_bounds__(64) void eval_arm_kernel(double* state, long* pos) {
    if (threadIdx.x < kEvalHdr) state[threadIdx.x] = 0.0;
    if (pos && threadIdx.x < 4) pos[threadIdx.x] = 0;
}

}  // namespace stgcn
