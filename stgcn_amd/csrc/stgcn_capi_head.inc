// Output head, model-level pack, gradient flush, optimizers and evaluation: helpers, then the entry points (included by stgcn_capi.hip).

namespace {
struct HeadGeom {
    int T1, NC, KP, KCH, CPin, ln_spg, ln_sg, fc_wgs;
    int dense_bwd;        // T1 == 1: the transposed conv is ONE dense GEMM dZ[B*N x NC] @ [NC x Ko*c_in] (tconv_fwd4_kernel<PLAIN>)
    int fused_ln_bwd;     // LayerNorm + gate backward in the staging pass of that GEMM (LnGateBwdIn): dgamma partials per slab, dbeta from dyln
    int64_t rows, rows_in, slabs;
    WgradGeom wc, wf;     // conv weights, fc1 weights
    long off_ln_g, off_ln_b, off_fc, total;
};

int head_check(const stgcn_outblock_desc* d) {
    if (!d) return fail(STGCN_ERR_INVALID, "desc is NULL");
    if (d->B < 1 || d->T < 1 || d->N < 1 || d->c_in < 1 || d->Ko < 1) return fail(STGCN_ERR_INVALID, "B/T/N/c_in/Ko must be positive");
    if (d->T < d->Ko) return fail(STGCN_ERR_INVALID, "T=%d shorter than Ko=%d", d->T, d->Ko);
    if (d->act != STGCN_ACT_GLU && d->act != STGCN_ACT_GTU) return fail(STGCN_ERR_INVALID, "act must be glu or gtu");
    if (!(d->droprate >= 0.f && d->droprate < 1.f)) return fail(STGCN_ERR_INVALID, "droprate must be in [0, 1)");   // (this form refuses NaN too)
    if (!(d->c0 == 64 || d->c0 == 128)) return fail(STGCN_ERR_UNSUPPORTED, "output-head conv channels must be 64 or 128 (got %d)", d->c0);
    if (d->c1 != 128) return fail(STGCN_ERR_UNSUPPORTED, "output-head fc1 width must be 128 (got %d)", d->c1);
    if (d->c_end != 1) return fail(STGCN_ERR_UNSUPPORTED, "end_channel must be 1 (got %d)", d->c_end);
    if ((d->c_in & 3) != 0 && d->Ko * d->c_in > 16) return fail(STGCN_ERR_UNSUPPORTED, "c_in=%d must be a multiple of 4", d->c_in);
    if (d->dtype != STGCN_DTYPE_F32 && d->dtype != STGCN_DTYPE_BF16) return fail(STGCN_ERR_INVALID, "dtype must be STGCN_DTYPE_F32 or STGCN_DTYPE_BF16");
    return STGCN_OK;
}

HeadGeom head_geom(const stgcn_outblock_desc* d) {
    HeadGeom g;
    g.T1 = d->T - d->Ko + 1;
    g.NC = 2 * d->c0;
    g.KP = (int)rup((int64_t)d->Ko * d->c_in, 16);
    g.KCH = g.KP / 16;
    g.CPin = (int)rup(d->c_in, 16);
    g.dense_bwd = !tconv4_off() && g.T1 == 1 && g.NC == 256 && d->Ko * d->c_in == 256 && (d->c_in & 3) == 0;
    g.rows = (int64_t)d->B * g.T1 * d->N;
    g.rows_in = (int64_t)d->B * d->T * d->N;
    g.slabs = (int64_t)d->B * g.T1;
    const long n = (long)d->N * d->c0, n4 = n / 4;
    const int colgroups = (int)((n4 + kThreads - 1) / kThreads);
    int sg = (512 + colgroups - 1) / colgroups;
    if (colgroups >= kLnBigColgroups) sg = (4096 + colgroups - 1) / colgroups;   // big slabs: see BwdGeom
    if (sg > g.slabs) sg = (int)g.slabs;
    if (sg < 1) sg = 1;
    g.ln_spg = (int)((g.slabs + sg - 1) / sg);
    g.ln_sg = (int)((g.slabs + g.ln_spg - 1) / g.ln_spg);
    // (the partial arena below is sized for both variants: need_dx may differ between the calls that share one workspace -- the weight
    // pack of a step is issued for the training descriptor, an evaluation forward runs with need_dx = 0 -- and its size must not)
    const bool fusable = (fuse_mask() & FUSE_HEAD_LN_BWD) && (fuse_mask() & FUSE_ROWSTATS) && g.dense_bwd && d->c0 == 128 && d->c1 == 128 &&
                         d->N <= 1024 && colgroups < kLnBigColgroups;
    const long sg_plain = g.ln_sg, sg_max = fusable && g.slabs > sg_plain ? g.slabs : sg_plain;
    g.fused_ln_bwd = fusable && d->need_dx;
    if (g.fused_ln_bwd) { g.ln_spg = 1; g.ln_sg = (int)g.slabs; }   // one dgamma partial per slab
    const long tiles = (g.rows + head_fc_tile_rows() - 1) / head_fc_tile_rows();
    g.fc_wgs = (int)(tiles < 512 * 32 / head_fc_tile_rows() / 2 ? tiles : 512 * 32 / head_fc_tile_rows() / 2);   // <= 256 (32-row tiles) / 512 (16-row tiles)
    long o = 0;
    auto take = [&](long f) { long at = o; o += (f + 63) / 64 * 64; return at; };
    g.off_ln_g = take(sg_max * n);
    // (bf16: the final reduction cannot read dbeta's summands out of the bf16 gradient tensor, the fused staging pass writes them as fp32)
    g.off_ln_b = take((d->dtype == STGCN_DTYPE_BF16 ? sg_max : sg_plain) * n);
    g.off_fc = take((long)g.fc_wgs * (d->c1 + 2));
    // The two weight gradients share ONE launch (wgrad_pair_kernel) of 100-KB-LDS workgroups, one per CU: together they aim at one resident
    // round (conv : fc1 = 5 : 3 by their work per row), not at one round EACH -- 416 workgroups at C2 were two rounds of short workgroups and
    // 40 % more partial blocks for the final reduction to read
    constexpr int t_conv = 160, t_fc = 96;
    // (measured, pass r4-20: C2 pair 25.5 -> 24.5 us and 0.5 us less in the reduction, C3 step - 2 us; at C5's 131 072 rows the longer
    //  workgroups lose, 115 -> 142 us: big heads keep one round each)
    const bool one_round = g.rows <= 32768;
    g.wc = wgrad_geom(g.rows, d->Ko * d->c_in, g.NC, 0, one_round ? t_conv : 256);
    g.wc.off = take(g.wc.floats);
    g.wf = wgrad_geom(g.rows, d->c0, d->c1, 0, one_round ? t_fc : 256);
    g.wf.off = take(g.wf.floats);
    g.total = o;
    return g;
}

void reduce_jobs_head(ReduceList& L, const stgcn_outblock_desc* d, const HeadGeom& g, const float* part, const float* dyln,
                             const stgcn_outblock_grads* G) {
    {
        const WgradGeom& w = g.wc;
        const float* wp = part + w.off;
        const float* bp = wp + (long)w.chunks * w.Mpad * w.NC;
        const long ps = (long)w.Mpad * w.NC;
        // (partials transposed: dW^T[o][k*c_in + i], Mpad floats per column -- see tconv_bwd_weight_body)
        L.add(G->tc_w, wp, w.chunks, ps, w.NC, d->Ko, d->c_in, w.Mpad, d->c_in, 1, (long)d->c_in * d->Ko, 1, d->Ko);
        L.add_flat(G->tc_b, bp, w.chunks, w.NC, w.NC);
        if (d->c_in > d->c0) {
            L.add(G->tc_aw, wp + (long)(d->Ko - 1) * d->c_in, w.chunks, ps, 1, d->c0, d->c_in, 0, w.Mpad, 1, 0, d->c_in, 1);
            L.add_flat(G->tc_ab, bp, w.chunks, w.NC, d->c0);
        }
    }
    {
        const WgradGeom& w = g.wf;   // src dW^T[o][i] (Mpad floats per column) -> fc1.weight[o][i]
        const float* wp = part + w.off;
        const float* bp = wp + (long)w.chunks * w.Mpad * w.NC;
        L.add(G->fc1_w, wp, w.chunks, (long)w.Mpad * w.NC, 1, d->c1, d->c0, 0, w.Mpad, 1, 0, d->c0, 1);
        L.add_flat(G->fc1_b, bp, w.chunks, w.NC, d->c1);
    }
    L.add_flat(G->fc2_w, part + g.off_fc, g.fc_wgs, d->c1 + 2, d->c1);
    L.add_flat(G->fc2_b, part + g.off_fc + d->c1, g.fc_wgs, d->c1 + 2, 1);
    if (G->loss) L.add_flat(G->loss, part + g.off_fc + d->c1 + 1, g.fc_wgs, d->c1 + 2, 1);   // fused loss: sum of the workgroups' partial means
    const int n = d->N * d->c0;
    L.add_flat(G->ln_w, part + g.off_ln_g, g.ln_sg, n, n);
    if (g.fused_ln_bwd && d->dtype == STGCN_DTYPE_F32) L.add_flat(G->ln_b, dyln, g.ln_sg, n, n);      // dbeta[n][c] = sum over slabs of dy: straight from the (fp32) gradient tensor
    else L.add_flat(G->ln_b, part + g.off_ln_b, g.ln_sg, n, n);
}

bool pack_fill_head(PackList& L, const stgcn_outblock_desc* d, const stgcn_outblock_params* P, const stgcn_outblock_plan& pl, float* ws,
                    bool all) {
    const HeadGeom g = head_geom(d);
    bool ok = true;
    ok &= L.add(PK_TCONV_FWD, g.NC * g.KP, ws + pl.ws_Wp, P->tc_w, P->tc_b, P->tc_aw, P->tc_ab, d->c_in, d->c0, d->Ko, g.KCH);
    if (d->need_dx || all) {
        if (g.dense_bwd)   // same footprint (NC x Ko*c_in floats), K = NC
            ok &= L.add(PK_TCONV_BWDT, g.NC * d->Ko * d->c_in, ws + pl.ws_Wd, P->tc_w, P->tc_b, P->tc_aw, P->tc_ab, d->c_in, d->c0, d->Ko, g.NC / 16);
        else
            ok &= L.add(PK_TCONV_BWD, d->Ko * g.NC * g.CPin, ws + pl.ws_Wd, P->tc_w, P->tc_b, P->tc_aw, P->tc_ab, d->c_in, d->c0, d->Ko,
                        d->Ko * g.NC / 16);
    }
    ok &= L.add(PK_TCONV_BIAS, g.NC, ws + pl.ws_b, P->tc_w, P->tc_b, P->tc_aw, P->tc_ab, d->c_in, d->c0, d->Ko, 0);
    ok &= L.add(PK_LIN_FWD, d->c0 * d->c1, ws + pl.ws_W1p, P->fc1_w, nullptr, nullptr, nullptr, d->c0, d->c1, 1, d->c0 / 16);
    ok &= L.add(PK_LIN_BWD, d->c1 * d->c0, ws + pl.ws_W1d, P->fc1_w, nullptr, nullptr, nullptr, d->c0, d->c1, 1, d->c1 / 16);
    ok &= L.add(PK_ZERO, (int)pl.chain_words, ws + pl.ws_chain, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0);   // control words of the fused forward
    return ok;
}

int prepack_impl(int32_t n_blocks, const stgcn_prepack_block* blocks, const stgcn_outblock_desc* hd, const stgcn_outblock_params* hp,
                 float* hws, int32_t n_counters, const stgcn_step_counter* counters, void* stream, bool park) {
    if (n_blocks < 0 || (n_blocks > 0 && !blocks)) return fail(STGCN_ERR_INVALID, "stgcn_prepack: bad block list");
    if (n_counters < 0 || n_counters > kMaxStepCounters || (n_counters > 0 && !counters))
        return fail(STGCN_ERR_INVALID, "stgcn_prepack: at most %d step counters", kMaxStepCounters);
    STGCN_FLUSH_PENDING_PACK();   // (a pack parked by an earlier call that no forward picked up)
    // one launch for the whole model while the job table holds it; models with many ST blocks (Kt = 2, n_his = 12 allows 5) spill into
    // further launches (the step counters ride on the first one)
    g_prof_tag = 0;
    PackList L;
    L.pa.ncounters = n_counters;
    for (int k = 0; k < n_counters; ++k) {
        if (!counters[k].ptr) return fail(STGCN_ERR_INVALID, "stgcn_prepack: NULL step counter %d", k);
        L.pa.cptr[k] = reinterpret_cast<long*>(counters[k].ptr); L.pa.cinc[k] = (long)counters[k].inc; L.pa.cmod[k] = (long)counters[k].mod;
    }
    auto flush_list = [&]() -> int {
        const int rc = launch_pack_list("prepack", L, (hipStream_t)stream);
        L = PackList();
        return rc;
    };
    // appends one module's jobs; a module that does not fit behind the jobs collected so far starts a new launch
    auto append = [&](auto&& fill) -> int {
        PackList trial = L;
        if (!fill(trial)) {
            if (L.nj == 0) return fail(STGCN_ERR_UNSUPPORTED, "stgcn_prepack: one module needs more than %d pack jobs", kMaxPackJobs);
            const int rc = flush_list();
            if (rc) return rc;
            trial = L;
            if (!fill(trial)) return fail(STGCN_ERR_UNSUPPORTED, "stgcn_prepack: pack job table overflow");
        }
        L = trial;
        return STGCN_OK;
    };
    for (int i = 0; i < n_blocks; ++i) {
        const stgcn_prepack_block& b = blocks[i];
        if (!b.desc || !b.params || !b.ws) return fail(STGCN_ERR_INVALID, "stgcn_prepack: NULL entry in block %d", i);
        BlockRoute r;
        stgcn_stblock_plan pl;
        int rc = route_and_plan(b.desc, &r, &pl);
        if (!rc) rc = append([&](PackList& T) { return pack_fill_block(T, b.desc, r, b.params, pl, b.ws, true); });
        if (rc) return rc;
    }
    if (hd) {
        if (!hp || !hws) return fail(STGCN_ERR_INVALID, "stgcn_prepack: head params / ws are NULL");
        stgcn_outblock_plan pl;
        int rc = stgcn_outblock_plan_query(hd, &pl);
        if (!rc) rc = append([&](PackList& T) { return pack_fill_head(T, hd, hp, pl, hws, true); });
        if (rc) return rc;
    }
    if (L.nj == 0 && L.pa.ncounters == 0) return STGCN_OK;
    if (park && L.nj > 0) {   // parked: the next entry point fuses it with the thin first layer or launches it (flush_pending_pack)
        g_pending_pack.valid = true;
        g_pending_pack.L = L;
        g_pending_pack.st = (hipStream_t)stream;
        return STGCN_OK;
    }
    return launch_pack_list("prepack", L, (hipStream_t)stream);
}

// STGCN_LOSS_* and Huber's delta, refused before anything is launched
int check_loss_kind(const char* who, int32_t kind, float delta) {
    if (kind != STGCN_LOSS_MSE && kind != STGCN_LOSS_MAE && kind != STGCN_LOSS_HUBER)
        return fail(STGCN_ERR_INVALID, "%s: unknown loss kind %d (STGCN_LOSS_MSE = 0, _MAE = 1, _HUBER = 2)", who, (int)kind);
    if (kind == STGCN_LOSS_HUBER && !(delta > 0.f && isfinite(delta)))
        return fail(STGCN_ERR_INVALID, "%s: Huber delta = %g must be finite and positive", who, (double)delta);
    return STGCN_OK;
}

// the mask of a masked loss entry, refused before anything is launched: n labels in whole rows of row_elems, and -- where the labels are
// read through an index word or a window table -- a stride and a window size in whole rows, so that row_valid can be addressed like them
int check_loss_mask(const char* who, const stgcn_loss_mask* mk, int64_t n, bool indexed, int64_t stride, bool table, int64_t window_floats) {
    if (!mk || !mk->valid || !mk->row_valid) return fail(STGCN_ERR_INVALID, "%s: NULL mask (valid / row_valid)", who);
    if (mk->row_elems <= 0) return fail(STGCN_ERR_INVALID, "%s: row_elems = %d must be positive", who, (int)mk->row_elems);
    if (n % mk->row_elems != 0)
        return fail(STGCN_ERR_INVALID, "%s: n = %lld labels are not whole rows of row_elems = %d", who, (long long)n, (int)mk->row_elems);
    if (indexed && (stride < 0 || stride % mk->row_elems != 0))
        return fail(STGCN_ERR_INVALID, "%s: the label stride %lld is not a multiple of row_elems = %d (row_valid is addressed in rows)", who,
                    (long long)stride, (int)mk->row_elems);
    if (table && window_floats % mk->row_elems != 0)
        return fail(STGCN_ERR_INVALID, "%s: %lld labels per window are not a multiple of row_elems = %d", who, (long long)window_floats,
                    (int)mk->row_elems);
    return STGCN_OK;
}

int outblock_backward_impl(const stgcn_outblock_desc* d, const stgcn_outblock_params* P, const float* x, const float* dout,
                           const stgcn_head_loss* hl, const stgcn_loss_mask* mk, const float* saved, float* ws,
                           const stgcn_outblock_grads* G, float* dx, const stgcn_ln_hook* dx_hook, void* stream) {
    STGCN_FLUSH_PENDING_PACK();
    stgcn_outblock_plan pl;
    int rc = stgcn_outblock_plan_query(d, &pl);
    if (rc) return rc;
    if (!P || !x || (!dout && !hl) || !saved || !ws || !G) return fail(STGCN_ERR_INVALID, "stgcn_outblock_backward: NULL buffer");
    if (d->need_dx && !dx) return fail(STGCN_ERR_INVALID, "stgcn_outblock_backward: need_dx set but dx is NULL");
    rc = check_dx_hook("stgcn_outblock_backward", dx_hook, d->N, d->c_in, d->need_dx, d->dtype);
    if (rc) return rc;
    const HeadGeom g = head_geom(d);
    if (mk) {
        rc = check_loss_mask("stgcn_outblock_backward_loss_masked", mk, g.rows, hl->target_index_dev != nullptr, hl->target_index_stride,
                             hl->target_window_dev != nullptr, g.rows / d->B);
        if (rc) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    g_prof_tag = 0;
    g_bf16 = d->dtype == STGCN_DTYPE_BF16;
    float* part = ws + pl.ws_part;
    const int training = d->training && d->droprate > 0.f;
    const bool own_rowstats = (fuse_mask() & FUSE_ROWSTATS) && d->c0 == d->c1 && d->c0 == 128;

    // ---- fc2 / dropout / relu / fc1 backward ------------------------------------------------------------------
    {
        FcBwdArgs a = zeroed<FcBwdArgs>();
        a.dout = dout; a.hd = saved + pl.sv_hd; a.w2 = P->fc2_w; a.W1d = ws + pl.ws_W1d; a.dh1 = ws + pl.ws_dh1; a.dyln = ws + pl.ws_dyln;
        a.part = part + g.off_fc; a.rows = g.rows; a.c0 = d->c0; a.c1 = d->c1; a.KCH = d->c1 / 16;
        a.grad_scale = training ? 1.0f / (1.0f - d->droprate) : 1.0f;
        if (hl) {
            a.pred = hl->pred; a.target = hl->target; a.target_index = reinterpret_cast<const long*>(hl->target_index_dev);
            a.target_index_stride = (long)hl->target_index_stride; a.loss_scale = hl->grad_scale;
            a.loss_kind = hl->kind; a.loss_delta = hl->delta;
            a.target_window = reinterpret_cast<const long*>(hl->target_window_dev); a.target_window_elems = (unsigned)(g.rows / d->B);
        }
        if (mk) { a.valid = mk->valid; a.row_valid = mk->row_valid; a.mask_row_elems = mk->row_elems; }
        if (own_rowstats) {   // the head's LayerNorm-backward row partials in this kernel's epilogue (dyln is that LayerNorm's output gradient)
            a.rs.rowstat = reinterpret_cast<float2*>(ws + pl.ws_rowstat_b); a.rs.U = saved + pl.sv_U; a.rs.S = saved + pl.sv_S; a.rs.gamma = P->ln_w;
            a.rs.mean = saved + pl.sv_mean; a.rs.rstd = saved + pl.sv_rstd; a.rs.N = d->N; a.rs.C = d->c0; a.rs.act = d->act; a.rs.training = 0;
            a.rs.keep_scale = 1.f;
        }
        const size_t lds = (size_t)(head_fc_tile_rows() * (d->c1 + 4) + 8 * d->c1 + 16) * sizeof(float);
        if (mk) {   // the masked instances: the same grid, block, LDS and label
            if (head_fc_tile_rows() == 16) {
                if (d->c0 == 128) STGCN_LAUNCH_ETB("head.fc_bwd", st, (fc_bwd_kernel<1, 2, ET, true>), dim3(g.fc_wgs), dim3(kThreads), lds, a);
                else STGCN_LAUNCH_ETB("head.fc_bwd", st, (fc_bwd_kernel<1, 1, ET, true>), dim3(g.fc_wgs), dim3(kThreads), lds, a);
            } else if (d->c0 == 128) STGCN_LAUNCH_ETB("head.fc_bwd", st, (fc_bwd_kernel<2, 2, ET, true>), dim3(g.fc_wgs), dim3(kThreads), lds, a);
            else STGCN_LAUNCH_ETB("head.fc_bwd", st, (fc_bwd_kernel<2, 1, ET, true>), dim3(g.fc_wgs), dim3(kThreads), lds, a);
        } else if (head_fc_tile_rows() == 16) {
            if (d->c0 == 128) STGCN_LAUNCH_ETB("head.fc_bwd", st, (fc_bwd_kernel<1, 2, ET>), dim3(g.fc_wgs), dim3(kThreads), lds, a);
            else STGCN_LAUNCH_ETB("head.fc_bwd", st, (fc_bwd_kernel<1, 1, ET>), dim3(g.fc_wgs), dim3(kThreads), lds, a);
        } else if (d->c0 == 128) STGCN_LAUNCH_ETB("head.fc_bwd", st, (fc_bwd_kernel<2, 2, ET>), dim3(g.fc_wgs), dim3(kThreads), lds, a);
        else STGCN_LAUNCH_ETB("head.fc_bwd", st, (fc_bwd_kernel<2, 1, ET>), dim3(g.fc_wgs), dim3(kThreads), lds, a);
    }
    // ---- fc1 weight gradient (needs dh1 only) ----------------------------------------------------------------------------
    TconvBwdWeightArgs wa = zeroed<TconvBwdWeightArgs>();
    wa.ts = make_taps(saved + pl.sv_yln, d->c0, 1, d->N, g.T1, g.T1, 1, g.rows);
    wa.dZ = ws + pl.ws_dh1; wa.part = part + g.wf.off; wa.NC = d->c1; wa.Mpad = g.wf.Mpad; wa.rows_per_chunk = g.wf.rows_per_chunk;
    wa.chunks = g.wf.chunks;
    const TconvBwdWeightArgs wfc = wa;      // (kept: it may share the conv weight gradient's launch at the end of the call)
    TconvBwdWeightArgs wcv = wa;
    wcv.ts.src = x; wcv.ts.C = d->c_in; wcv.ts.taps = d->Ko; wcv.ts.Tsrc = d->T; wcv.ts.Tdst = g.T1;
    wcv.dZ = ws + pl.ws_dZ; wcv.part = part + g.wc.off; wcv.NC = g.NC; wcv.Mpad = g.wc.Mpad; wcv.rows_per_chunk = g.wc.rows_per_chunk;
    wcv.chunks = g.wc.chunks;
    const bool pair = wgrad_pair_ok(wcv, g.wc, wfc, g.wf);
    if (!pair) {
        rc = launch_bwd_weight("head.fc1_bwd_weight", wfc, g.wf, st);
        if (rc) return rc;
    }
    // ---- LayerNorm + gate backward ---------------------------------------------------------------------------------
    LnBwdArgs ln = zeroed<LnBwdArgs>();
    ln.dy = ws + pl.ws_dyln; ln.U = saved + pl.sv_U; ln.S = saved + pl.sv_S; ln.gamma = P->ln_w;
    ln.mean = saved + pl.sv_mean; ln.rstd = saved + pl.sv_rstd; ln.rowstat = reinterpret_cast<float2*>(ws + pl.ws_rowstat_b);
    ln.dZ = ws + pl.ws_dZ; ln.dgam_part = part + g.off_ln_g; ln.dbet_part = part + g.off_ln_b;
    ln.n = d->N * d->c0; ln.N = d->N; ln.C = d->c0; ln.act = d->act; ln.training = 0; ln.spg = g.ln_spg; ln.slabs = g.slabs;
    ln.keep_scale = 1.f; ln.thresh = 0;
    if (!own_rowstats)
        STGCN_LAUNCH_ET("head.ln_bwd_rowstats", st, (ln_bwd_rowstats_kernel<ET>), dim3(cdiv(g.slabs * (ln.n / 4), kThreads)), dim3(kThreads), 0, ln);
    if (cdiv(ln.n / 4, kThreads) >= kLnBigColgroups) {
        ln.slabconst = reinterpret_cast<float2*>(ws + pl.ws_rowstat_b + 2 * g.rows);
        STGCN_LAUNCH("head.ln_slab_consts", st, ln_slab_consts_kernel, dim3((unsigned)g.slabs), dim3(kThreads), 64, ln);
    }
    const bool fused_ln = g.fused_ln_bwd && own_rowstats;   // LayerNorm + gate backward inside the dense transposed conv below
    if (!fused_ln)
        STGCN_LAUNCH_ET("head.ln_gate_bwd", st, (ln_gate_bwd_kernel<ET>), dim3(cdiv(ln.n / 4, kThreads), g.ln_sg), dim3(kThreads),
                        (8 + 2 * g.ln_spg) * sizeof(float), ln);
    // ---- conv backward-data ---------------------------------------------------------------------------------------------
    bool hook_pending = false;
    if (d->need_dx && g.dense_bwd) {
        Tconv4Args aa = zeroed<Tconv4Args>();
        aa.f.ts = make_taps(ws + pl.ws_dZ, g.NC, 1, d->N, 1, 1, 1, g.rows);
        aa.f.Wp = ws + pl.ws_Wd; aa.f.KCH = g.NC / 16; aa.f.Cout = 128;
        aa.out = dx; aa.outT = d->T; aa.outC = d->c_in;
        const bool epi = dx_hook && dx_hook->rowstat && dx_hook->C == d->c_in && (d->c_in == 64 || d->c_in == 128) && dx_hook->N == d->N;
        if (epi) aa.rs = rowstat_out(dx_hook);
        if (fused_ln) {
            aa.lnb.dy = ln.dy; aa.lnb.U = ln.U; aa.lnb.S = ln.S; aa.lnb.gamma = ln.gamma; aa.lnb.mean = ln.mean; aa.lnb.rstd = ln.rstd;
            aa.lnb.rowstat = ln.rowstat; aa.lnb.dZ = ln.dZ; aa.lnb.dgam = ln.dgam_part; aa.lnb.N = d->N; aa.lnb.C = d->c0; aa.lnb.act = d->act;
            aa.lnb.dbet = g_bf16 ? ln.dbet_part : nullptr;
        }
        rc = launch_tconv_fwd4<true>("head.tconv_bwd_data", aa, st);
        if (rc) return rc;
        if (dx_hook && dx_hook->rowstat && !epi) hook_pending = true;
    } else if (d->need_dx) {
        TconvBwdDataArgs a = zeroed<TconvBwdDataArgs>();
        a.ts = make_taps(ws + pl.ws_dZ, g.NC, d->Ko, d->N, g.T1, d->T, -1, g.rows_in);
        a.Wp = ws + pl.ws_Wd; a.KCH = d->Ko * g.NC / 16; a.Cin = d->c_in; a.Gmask = nullptr; a.dX = dx;
        rc = launch_bwd_data("head.tconv_bwd_data", a, g.CPin / 16, st);
        if (rc) return rc;
        if (dx_hook && dx_hook->rowstat) hook_pending = true;
    }
    // ---- conv weight gradient (needs dZ, which the fused transposed conv above writes) --------------------------------------------
    rc = pair ? launch_wgrad_pair("head.wgrad_pair", wcv, g.wc, wfc, g.wf, st) : launch_bwd_weight("head.tconv_bwd_weight", wcv, g.wc, st);
    if (rc) return rc;
    if (hook_pending) {   // the kernel that formed dx had no epilogue for it
        rc = launch_hook_rowstats(dx_hook, dx, (long)d->B * d->T, st);
        if (rc) return rc;
    }
    // ---- final reduction (deferred to stgcn_grad_flush when asked) ------------------------------------------------------------
    if (d->defer_reduce) return STGCN_OK;
    ReduceList RL;
    reduce_jobs_head(RL, d, g, part, ws + pl.ws_dyln, G);
    return launch_reduce_list("head.reduce", RL, st);
}
// the job list of a whole-model flush with the optimizer table attached (stgcn_grad_flush, stgcn_grad_flush_optim); need_v: the kind keeps
// exp_avg_sq (every kind but Lion)
int flush_job_list(ReduceList& RL, const char* who, int32_t n_blocks, const stgcn_flush_block* blocks, const stgcn_outblock_desc* head_desc,
                   const stgcn_outblock_grads* head_grads, float* head_ws, const stgcn_adamw_tensor* opt, int32_t opt_count, bool need_v) {
    if (n_blocks < 0 || (n_blocks > 0 && !blocks)) return fail(STGCN_ERR_INVALID, "%s: bad block table", who);
    for (int i = 0; i < n_blocks; ++i) {
        const stgcn_stblock_desc* d = blocks[i].desc;
        BlockRoute r;
        stgcn_stblock_plan pl;
        int rc = route_and_plan(d, &r, &pl);
        if (rc) return rc;
        if (!blocks[i].grads || !blocks[i].ws) return fail(STGCN_ERR_INVALID, "%s: NULL pointer in block %d", who, i);
        reduce_jobs_block(RL, d, r, blocks[i].ws + pl.ws_part, blocks[i].grads);
    }
    if (head_desc) {
        stgcn_outblock_plan pl;
        int rc = stgcn_outblock_plan_query(head_desc, &pl);
        if (rc) return rc;
        if (!head_grads || !head_ws) return fail(STGCN_ERR_INVALID, "%s: NULL head pointer", who);
        const HeadGeom g = head_geom(head_desc);
        reduce_jobs_head(RL, head_desc, g, head_ws + pl.ws_part, head_ws + pl.ws_dyln, head_grads);
    }
    if (opt_count > 0) {
        int matched = 0;
        for (int k = 0; k < RL.nj; ++k)
            for (int i = 0; i < opt_count; ++i)
                if (opt[i].grad == RL.ra.job[k].dst) {
                    if (!opt[i].param || !opt[i].exp_avg || (need_v && !opt[i].exp_avg_sq)) return fail(STGCN_ERR_INVALID, "%s: NULL pointer in optimizer entry %d", who, i);
                    RL.ra.job[k].p = opt[i].param; RL.ra.job[k].m = opt[i].exp_avg; RL.ra.job[k].v = opt[i].exp_avg_sq;
                    if (((reinterpret_cast<uintptr_t>(opt[i].param) | reinterpret_cast<uintptr_t>(opt[i].exp_avg) | reinterpret_cast<uintptr_t>(opt[i].exp_avg_sq)) & 15) != 0)
                        RL.ra.job[k].dvec = 0;   // (the 16-byte form of the state update needs aligned state tensors)
                    ++matched;
                    break;
                }
        if (matched != opt_count) return fail(STGCN_ERR_INVALID, "%s: %d of %d optimizer entries have no gradient in this flush", who, opt_count - matched, opt_count);
    }
    return STGCN_OK;
}

// NAdamW / Lion constants beyond ReduceArgs / AdamwArgs, formed in double like torch forms them
OptimExtra optim_extra(const stgcn_optim_hyper* h) {
    OptimExtra x = zeroed<OptimExtra>();
    x.omb1 = (float)(1.0 - h->beta1);
    x.omb2 = (float)(1.0 - h->beta2);
    x.mu_k = (float)(h->momentum_decay * log(0.96));
    x.mu_prod = h->mu_product;
    x.mu_dev = h->kind == STGCN_OPT_NADAMW ? h->mu_product_dev : nullptr;
    x.mu_job = -1;
    return x;
}
int check_optim_hyper(const stgcn_optim_hyper* h, const char* who) {
    if (!h) return fail(STGCN_ERR_INVALID, "%s: NULL hyper-parameters", who);
    if (h->kind != STGCN_OPT_ADAMW && h->kind != STGCN_OPT_NADAMW && h->kind != STGCN_OPT_LION)
        return fail(STGCN_ERR_INVALID, "%s: unknown optimizer kind %d", who, (int)h->kind);
    return STGCN_OK;
}
}  // namespace

int stgcn_outblock_plan_query(const stgcn_outblock_desc* d, stgcn_outblock_plan* p) {
    int rc = head_check(d);
    if (rc) return rc;
    if (!p) return fail(STGCN_ERR_INVALID, "plan is NULL");
    const HeadGeom g = head_geom(d);
    memset(p, 0, sizeof(*p));
    p->T1 = g.T1; p->rows = g.rows; p->rows_in = g.rows_in; p->out_floats = g.rows * d->c_end;
    int64_t o = 0;
    auto take = [&](int64_t n) { int64_t at = o; o += rup(n, 64); return at; };
    const bool bf = d->dtype == STGCN_DTYPE_BF16;
    auto act = [&](int64_t n) { return bf ? (n + 1) / 2 : n; };   // 4-byte units of an activation tensor of n elements
    p->sv_U = take(act(g.rows * d->c0));
    p->sv_S = take(act(g.rows * d->c0));
    p->sv_mean = take(g.slabs);
    p->sv_rstd = take(g.slabs);
    p->sv_yln = take(act(g.rows * d->c0));
    p->sv_hd = take(act(g.rows * d->c1));
    p->sv_rowstat = take(2 * g.rows);
    p->saved_floats = o;
    o = 0;
    p->chain_words = kChainHdr + g.slabs;   // fused forward (head_fwd_kernel): one arrival counter per LayerNorm slab
    p->ws_chain = take(p->chain_words);     // (first: the offset must not depend on anything the calls sharing one workspace may differ in)
    p->ws_Wp = take((int64_t)g.NC * g.KP);
    p->ws_Wd = take((int64_t)d->Ko * g.NC * g.CPin);
    p->ws_b = take(g.NC);
    p->ws_W1p = take((int64_t)d->c0 * d->c1);
    p->ws_W1d = take((int64_t)d->c1 * d->c0);
    p->ws_rowstat_b = take(2 * g.rows + 2 * g.slabs);   // row partials, then the per-slab constants (big slabs only)
    p->ws_dh1 = take(act(g.rows * d->c1));
    p->ws_dyln = take(act(g.rows * d->c0));
    p->ws_dZ = take(act(g.rows * g.NC));
    p->part_floats = g.total;
    p->ws_part = take(g.total);
    p->ws_floats = o;
    return STGCN_OK;
}

int stgcn_prepack(int32_t n_blocks, const stgcn_prepack_block* blocks, const stgcn_outblock_desc* hd, const stgcn_outblock_params* hp,
                  float* hws, int32_t n_counters, const stgcn_step_counter* counters, void* stream) {
    return prepack_impl(n_blocks, blocks, hd, hp, hws, n_counters, counters, stream, false);
}
int stgcn_prepack_flush(void) {   // launches a pack that stgcn_prepack_park left parked on this thread (no-op otherwise)
    return flush_pending_pack();
}
int stgcn_prepack_park(int32_t n_blocks, const stgcn_prepack_block* blocks, const stgcn_outblock_desc* hd, const stgcn_outblock_params* hp,
                       float* hws, int32_t n_counters, const stgcn_step_counter* counters, void* stream) {
    return prepack_impl(n_blocks, blocks, hd, hp, hws, n_counters, counters, stream, true);
}

int stgcn_outblock_forward(const stgcn_outblock_desc* d, const stgcn_outblock_params* P, const float* x, float* out, float* saved,
                           float* ws, uint64_t seed, uint64_t offset, const uint64_t* offset_dev, void* stream) {
    STGCN_FLUSH_PENDING_PACK();
    stgcn_outblock_plan pl;
    int rc = stgcn_outblock_plan_query(d, &pl);
    if (rc) return rc;
    if (!P || !x || !out || !saved || !ws) return fail(STGCN_ERR_INVALID, "stgcn_outblock_forward: NULL buffer");
    if (!P->tc_w || !P->tc_b || !P->ln_w || !P->ln_b || !P->fc1_w || !P->fc2_w)
        return fail(STGCN_ERR_INVALID, "stgcn_outblock_forward: missing parameter pointer");
    if (d->c_in > d->c0 && !P->tc_aw) return fail(STGCN_ERR_INVALID, "tc_aw required when c_in > c0");
    const HeadGeom g = head_geom(d);
    hipStream_t st = (hipStream_t)stream;
    g_prof_tag = 0;
    g_bf16 = d->dtype == STGCN_DTYPE_BF16;

    if (!d->prepacked) {
        PackList L;
        if (!pack_fill_head(L, d, P, pl, ws, false)) return fail(STGCN_ERR_INVALID, "pack job table overflow");
        rc = launch_pack_list("head.pack", L, st);
        if (rc) return rc;
    }

    TconvFwdArgs t = zeroed<TconvFwdArgs>();
    t.ts = make_taps(x, d->c_in, d->Ko, d->N, d->T, g.T1, 1, g.rows);
    t.Wp = ws + pl.ws_Wp; t.bias = ws + pl.ws_b; t.KCH = g.KCH; t.Cout = d->c0; t.act = d->act;
    t.U = saved + pl.sv_U; t.S = saved + pl.sv_S; t.rowstat = reinterpret_cast<float2*>(saved + pl.sv_rowstat);

    // ---- the whole forward in ONE launch (head_fwd_kernel): the conv's row tiles exchange their LayerNorm row statistics through per-window
    //      arrival counters and go on with LayerNorm + fc1 + ReLU + dropout + fc2 on the rows they hold in LDS.  Needs every tile of the launch
    //      resident at once (they wait for each other): 32-row tiles, else 64-row tiles, else the separate launches below.
    if (head_fuse_mode() && g.T1 == 1 && d->c0 == 128 && d->c1 == 128 && tconv4_ok(t)) {
        constexpr int KC = 4;
        // Round 5 (VERDICT r4 weak 2 / ADVICE r4): the DEFAULT is the ticket form -- a tile's peers lie at most two windows = 2 * ceil(N / TR) + 1
        // tiles ahead in start order, so it only needs a residency well above that span and makes no assumption about dispatch order, about the
        // device being this launch's alone (a second process, an RCCL kernel, another stream's head) or about the grid fitting one round.  The
        // blockIdx forms (whole grid resident at once) remain as STGCN_HEAD_FUSE=2 / 4 for A/B runs and tests.
        int tm = 0, ticket = 0;
        {
            const int forced = head_fuse_mode() > 1 ? head_fuse_mode() : 0;   // STGCN_HEAD_FUSE=2 / 4: that tile height by blockIdx; 3 / 5: 32- / 64-row tiles by ticket
            const size_t l2 = (size_t)(tconv2_lds_floats(g.KP, 256, 32) + 48) * sizeof(float), l4 = (size_t)(tconv2_lds_floats(g.KP, 256, 64) + 48) * sizeof(float);
            const int cap2 = STGCN_ET_VALUE(wg_capacity(head_fwd_kernel<2, KC, ET>, 512, l2));
            const int cap4 = STGCN_ET_VALUE(wg_capacity(head_fwd_kernel<4, KC, ET>, 512, l4));
            const int t2 = cdiv(g.rows, 32), t4 = cdiv(g.rows, 64);
            // a tile height is admissible by ticket when the residency is well above the span a tile can wait over
            const bool tk2 = d->N >= 32 && d->N <= 1024 && cap2 >= 4 * cdiv(d->N, 32) + 16, tk4 = d->N >= 64 && d->N <= 2048 && cap4 >= 4 * cdiv(d->N, 64) + 16;
            if (forced == 2) { if (d->N >= 32 && t2 <= cap2) tm = 2; }
            else if (forced == 4) { if (d->N >= 64 && t4 <= cap4) tm = 4; }
            else if (forced == 3) { if (tk2) { tm = 2; ticket = 1; } }
            else if (forced == 5) { if (tk4) { tm = 4; ticket = 1; } }
            // default: the smallest tile whose grid is ONE resident round (C2: 207 tiles of 32 rows; C3: 325 tiles of 64 -- its 650 32-row tiles
            // on 512 slots ran 53 us against 38, pass r5-01), else the 32-row tiles in several rounds
            else if (tk2 && t2 <= cap2) { tm = 2; ticket = 1; }
            else if (tk4 && t4 <= cap4) { tm = 4; ticket = 1; }
            else if (tk2) { tm = 2; ticket = 1; }
            else if (tk4) { tm = 4; ticket = 1; }
        }
        if (tm) {
            Tconv4Args aa = zeroed<Tconv4Args>();
            aa.f = t;
            HeadFcTail f = zeroed<HeadFcTail>();
            const int TR = 16 * tm, tiles = cdiv(g.rows, TR);
            f.chain.words = reinterpret_cast<unsigned*>(ws + pl.ws_chain); f.chain.ncount = (int)g.slabs; f.chain.total = (unsigned)tiles;
            f.chain.spin = g_chain_spin_ticks;
            f.gamma = P->ln_w; f.beta = P->ln_b; f.yln = saved + pl.sv_yln; f.mean = saved + pl.sv_mean; f.rstd = saved + pl.sv_rstd;
            f.eps = d->ln_eps;
            f.W1p = ws + pl.ws_W1p; f.b1 = P->fc1_b; f.w2 = P->fc2_w; f.b2 = P->fc2_b; f.hd = saved + pl.sv_hd; f.out = out;
            f.training = d->training && d->droprate > 0.f;
            f.keep_scale = 1.0f / (1.0f - d->droprate); f.thresh = drop_thresh(d->droprate); f.seed = seed; f.offset = offset;
            f.offset_dev = offset_dev;
            f.use_ticket = ticket;
            const size_t lds = (size_t)(tconv2_lds_floats(g.KP, 256, TR) + 48) * sizeof(float);   // + 48: the block reduction of two windows' statistics, the ticket word
            if (tm == 2) STGCN_LAUNCH_ET("head.fwd", st, (head_fwd_kernel<2, KC, ET>), dim3(tiles), dim3(512), lds, aa, f);
            else STGCN_LAUNCH_ET("head.fwd", st, (head_fwd_kernel<4, KC, ET>), dim3(tiles), dim3(512), lds, aa, f);
            return STGCN_OK;
        }
    }
    rc = launch_tconv_fwd("head.tconv_fwd", t, st);
    if (rc) return rc;

    LnFwdArgs ln = zeroed<LnFwdArgs>();
    ln.U = saved + pl.sv_U; ln.S = saved + pl.sv_S; ln.gamma = P->ln_w; ln.beta = P->ln_b; ln.y = saved + pl.sv_yln;
    ln.mean = saved + pl.sv_mean; ln.rstd = saved + pl.sv_rstd; ln.rowstat = reinterpret_cast<const float2*>(saved + pl.sv_rowstat);
    ln.n = d->N * d->c0; ln.N = d->N; ln.C = d->c0; ln.act = d->act; ln.training = 0;
    ln.eps = d->ln_eps; ln.keep_scale = 1.f; ln.thresh = 0;
    // the LayerNorm rides in the staging of the fc kernel when its tile covers whole rows (K = c0 in one piece) and T1 = 1 (a slab is
    // N consecutive rows); every workgroup re-reads the N row partials of its slabs, so big graphs keep the separate launch
    const bool fuse_ln = (fuse_mask() & FUSE_HEAD_LN_FWD) && g.T1 == 1 && d->c0 % 16 == 0 && d->c0 <= 128 && d->N <= 1024;
    if (!fuse_ln) {
        rc = launch_ln_fwd("head.ln_fwd", ln, g.slabs, st);
        if (rc) return rc;
    }

    FcFwdArgs f = zeroed<FcFwdArgs>();
    if (fuse_ln) f.ln = ln;
    f.ts = make_taps(saved + pl.sv_yln, d->c0, 1, d->N, g.T1, g.T1, 1, g.rows);
    f.W1p = ws + pl.ws_W1p; f.b1 = P->fc1_b; f.w2 = P->fc2_w; f.b2 = P->fc2_b; f.hd = saved + pl.sv_hd; f.out = out;
    f.KCH = d->c0 / 16; f.c1 = d->c1; f.training = d->training && d->droprate > 0.f;
    f.keep_scale = 1.0f / (1.0f - d->droprate); f.thresh = drop_thresh(d->droprate); f.seed = seed; f.offset = offset;
    f.offset_dev = offset_dev;
    // (big heads: 32-row tiles halve the fc1 weight bytes a row streams -- C5 fc_fwd 72 -> 59 us, pass r4-31; the backward kernel loses with them)
    const int fct = (head_fc_tile_knob() || g.rows <= 32768) ? head_fc_tile_rows() : 32;
    const size_t lds = (size_t)(kTileHdr + fct * (128 + 4)) * sizeof(float);
    if (fct == 16) STGCN_LAUNCH_ET("head.fc_fwd", st, (fc_fwd_kernel<1, ET>), dim3(cdiv(g.rows, 16)), dim3(kThreads), lds, f);
    else STGCN_LAUNCH_ET("head.fc_fwd", st, (fc_fwd_kernel<2, ET>), dim3(cdiv(g.rows, 32)), dim3(kThreads), lds, f);
    return STGCN_OK;
}

int stgcn_outblock_chain_status(const stgcn_outblock_desc* d, const float* ws, uint32_t* sticky, void* stream) {
    STGCN_FLUSH_PENDING_PACK();
    stgcn_outblock_plan pl;
    const int rc = stgcn_outblock_plan_query(d, &pl);
    if (rc) return rc;
    return read_chain_sticky("stgcn_outblock_chain_status", ws, pl.ws_chain, sticky, stream);
}

int stgcn_outblock_backward(const stgcn_outblock_desc* d, const stgcn_outblock_params* P, const float* x, const float* dout,
                            const float* saved, float* ws, const stgcn_outblock_grads* G, float* dx, void* stream) {
    return outblock_backward_impl(d, P, x, dout, nullptr, nullptr, saved, ws, G, dx, nullptr, stream);
}

int stgcn_outblock_backward_hook(const stgcn_outblock_desc* d, const stgcn_outblock_params* P, const float* x, const float* dout,
                                 const float* saved, float* ws, const stgcn_outblock_grads* G, float* dx, const stgcn_ln_hook* dx_hook,
                                 void* stream) {
    return outblock_backward_impl(d, P, x, dout, nullptr, nullptr, saved, ws, G, dx, dx_hook, stream);
}

namespace {
int check_head_loss(const char* who, const stgcn_head_loss* hl, const stgcn_outblock_grads* G) {
    if (!hl || !hl->pred || !hl->target) return fail(STGCN_ERR_INVALID, "%s: NULL pred / target", who);
    if (!G || !G->loss) return fail(STGCN_ERR_INVALID, "%s: grads->loss is NULL", who);
    const int rc = check_loss_kind(who, hl->kind, hl->delta);
    if (rc) return rc;
    if (hl->target_window_dev && !hl->target_index_dev)
        return fail(STGCN_ERR_INVALID, "%s: target_window_dev (window table) needs target_index_dev != NULL", who);
    return STGCN_OK;
}
}  // namespace

int stgcn_outblock_backward_loss(const stgcn_outblock_desc* d, const stgcn_outblock_params* P, const float* x, const stgcn_head_loss* hl,
                                 const float* saved, float* ws, const stgcn_outblock_grads* G, float* dx, const stgcn_ln_hook* dx_hook,
                                 void* stream) {
    const int rc = check_head_loss("stgcn_outblock_backward_loss", hl, G);
    if (rc) return rc;
    return outblock_backward_impl(d, P, x, nullptr, hl, nullptr, saved, ws, G, dx, dx_hook, stream);
}

int stgcn_outblock_backward_loss_masked(const stgcn_outblock_desc* d, const stgcn_outblock_params* P, const float* x,
                                        const stgcn_head_loss* hl, const stgcn_loss_mask* mask, const float* saved, float* ws,
                                        const stgcn_outblock_grads* G, float* dx, const stgcn_ln_hook* dx_hook, void* stream) {
    const int rc = check_head_loss("stgcn_outblock_backward_loss_masked", hl, G);
    if (rc) return rc;
    if (!mask || !mask->valid || !mask->row_valid || mask->row_elems <= 0)
        return fail(STGCN_ERR_INVALID, "stgcn_outblock_backward_loss_masked: NULL mask (valid / row_valid) or row_elems <= 0");
    return outblock_backward_impl(d, P, x, nullptr, hl, mask, saved, ws, G, dx, dx_hook, stream);
}

namespace {
// clip_state: null = stgcn_adamw_step as it always was; else the clip form of the same launch (stgcn_optim_step_clip)
int adamw_step_impl(const stgcn_adamw_tensor* tensors, int32_t count, float lr, float beta1, float beta2, float eps, float weight_decay,
                    int64_t step, const int64_t* step_dev, const float* lr_dev, const double* clip_state, void* stream) {
    STGCN_FLUSH_PENDING_PACK();
    if (count < 0 || (count > 0 && !tensors)) return fail(STGCN_ERR_INVALID, "stgcn_adamw_step: bad tensor table");
    hipStream_t st = (hipStream_t)stream;
    for (int off = 0; off < count; off += kAdamwMaxTensors) {
        AdamwArgs a = zeroed<AdamwArgs>();
        const int n = count - off < kAdamwMaxTensors ? count - off : kAdamwMaxTensors;
        for (int i = 0; i < n; ++i) {
            const stgcn_adamw_tensor& t = tensors[off + i];
            if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq || t.numel < 0) return fail(STGCN_ERR_INVALID, "stgcn_adamw_step: NULL pointer in entry %d", off + i);
            a.t[i].p = t.param; a.t[i].g = t.grad; a.t[i].m = t.exp_avg; a.t[i].v = t.exp_avg_sq; a.t[i].n = (long)t.numel;
            a.start[i + 1] = a.start[i] + cdiv(t.numel, kAdamwChunk);
        }
        a.count = n; a.lr = lr; a.b1 = beta1; a.b2 = beta2; a.eps = eps; a.wd = weight_decay; a.step = (long)step;
        a.lb1 = (float)log((double)beta1); a.lb2 = (float)log((double)beta2);
        a.step_dev = reinterpret_cast<const long*>(step_dev); a.lr_dev = lr_dev;
        g_prof_tag = 0;
        if (a.start[n] > 0) {
            if (clip_state) STGCN_LAUNCH("adamw_clip", st, adamw_clip_kernel, dim3(a.start[n]), dim3(kThreads), 0, a, clip_state);
            else STGCN_LAUNCH("adamw", st, adamw_kernel, dim3(a.start[n]), dim3(kThreads), 0, a);
        }
    }
    return STGCN_OK;
}

// the workgroups of the norm launch over entries [off, off + n) of a table, and the fp64 words a table's norm needs
int grad_norm_wgs(const stgcn_adamw_tensor* tensors, int off, int n) {
    long chunks = 0;
    for (int i = 0; i < n; ++i) chunks += cdiv(tensors[off + i].numel, kAdamwChunk);
    return chunks < 1 ? 1 : (chunks > kClipMaxWgs ? kClipMaxWgs : (int)chunks);
}
int grad_clip_words_impl(const stgcn_adamw_tensor* tensors, int32_t count, const char* who, int64_t* words) {
    if (count < 0 || (count > 0 && !tensors)) return fail(STGCN_ERR_INVALID, "%s: bad tensor table", who);
    int wgs = 1;
    for (int off = 0; off < count; off += kAdamwMaxTensors) {
        const int n = count - off < kAdamwMaxTensors ? count - off : kAdamwMaxTensors;
        for (int i = 0; i < n; ++i)
            if (tensors[off + i].numel < 0) return fail(STGCN_ERR_INVALID, "%s: negative numel in entry %d", who, off + i);
        const int w = grad_norm_wgs(tensors, off, n);
        wgs = w > wgs ? w : wgs;
    }
    *words = STGCN_CLIP_HDR_WORDS + wgs;
    return STGCN_OK;
}
int check_clip(const stgcn_grad_clip* c, int64_t need, const char* who) {
    if (!c || !c->state) return fail(STGCN_ERR_INVALID, "%s: NULL clip state", who);
    if (!(c->max_norm > 0.f)) return fail(STGCN_ERR_INVALID, "%s: max_norm = %g must be > 0", who, (double)c->max_norm);
    if (c->state_words < need)
        return fail(STGCN_ERR_INVALID, "%s: a clip state of %lld words is too small, %lld needed", who, (long long)c->state_words, (long long)need);
    return STGCN_OK;
}
}  // namespace

int stgcn_adamw_step(const stgcn_adamw_tensor* tensors, int32_t count, float lr, float beta1, float beta2, float eps,
                     float weight_decay, int64_t step, const int64_t* step_dev, const float* lr_dev, void* stream) {
    return adamw_step_impl(tensors, count, lr, beta1, beta2, eps, weight_decay, step, step_dev, lr_dev, nullptr, stream);
}

int stgcn_grad_flush(int32_t n_blocks, const stgcn_flush_block* blocks, const stgcn_outblock_desc* head_desc,
                     const stgcn_outblock_grads* head_grads, float* head_ws, const stgcn_adamw_tensor* opt, int32_t opt_count,
                     const stgcn_adamw_hyper* hyper, void* stream) {
    STGCN_FLUSH_PENDING_PACK();
    if (opt_count < 0 || (opt_count > 0 && (!opt || !hyper))) return fail(STGCN_ERR_INVALID, "stgcn_grad_flush: optimizer table without hyper-parameters");
    ReduceList RL;
    int rc = flush_job_list(RL, "stgcn_grad_flush", n_blocks, blocks, head_desc, head_grads, head_ws, opt, opt_count, true);
    if (rc) return rc;
    if (opt_count > 0) {
        RL.ra.lr = hyper->lr; RL.ra.b1 = hyper->beta1; RL.ra.b2 = hyper->beta2; RL.ra.eps = hyper->eps; RL.ra.wd = hyper->weight_decay;
        RL.ra.lb1 = (float)log((double)hyper->beta1); RL.ra.lb2 = (float)log((double)hyper->beta2);
        RL.ra.step = (long)hyper->step; RL.ra.step_dev = reinterpret_cast<const long*>(hyper->step_dev); RL.ra.lr_dev = hyper->lr_dev;
    }
    g_prof_tag = 0;
    return launch_reduce_list(opt_count > 0 ? "reduce_adamw" : "reduce_all", RL, (hipStream_t)stream);
}

namespace {
int optim_step_impl(const char* who, const stgcn_adamw_tensor* tensors, int32_t count, const stgcn_optim_hyper* hyper, const double* clip_state,
                    void* stream) {
    if (hyper->kind == STGCN_OPT_ADAMW)
        return adamw_step_impl(tensors, count, (float)hyper->lr, (float)hyper->beta1, (float)hyper->beta2, (float)hyper->eps, (float)hyper->weight_decay,
                               hyper->step, hyper->step_dev, hyper->lr_dev, clip_state, stream);
    STGCN_FLUSH_PENDING_PACK();
    if (count < 0 || (count > 0 && !tensors)) return fail(STGCN_ERR_INVALID, "%s: bad tensor table", who);
    const bool lion = hyper->kind == STGCN_OPT_LION;
    hipStream_t st = (hipStream_t)stream;
    for (int off = 0; off < count; off += kAdamwMaxTensors) {
        AdamwArgs a = zeroed<AdamwArgs>();
        const int n = count - off < kAdamwMaxTensors ? count - off : kAdamwMaxTensors;
        for (int i = 0; i < n; ++i) {
            const stgcn_adamw_tensor& t = tensors[off + i];
            if (!t.param || !t.grad || !t.exp_avg || (!lion && !t.exp_avg_sq) || t.numel < 0)
                return fail(STGCN_ERR_INVALID, "%s: NULL pointer in entry %d", who, off + i);
            a.t[i].p = t.param; a.t[i].g = t.grad; a.t[i].m = t.exp_avg; a.t[i].v = lion ? nullptr : t.exp_avg_sq; a.t[i].n = (long)t.numel;
            a.start[i + 1] = a.start[i] + cdiv(t.numel, kAdamwChunk);
        }
        a.count = n; a.lr = (float)hyper->lr; a.b1 = (float)hyper->beta1; a.b2 = (float)hyper->beta2; a.eps = (float)hyper->eps;
        a.wd = (float)hyper->weight_decay; a.step = (long)hyper->step;
        a.lb1 = (float)log(hyper->beta1); a.lb2 = (float)log(hyper->beta2);
        a.step_dev = reinterpret_cast<const long*>(hyper->step_dev); a.lr_dev = hyper->lr_dev;
        OptimExtra x = optim_extra(hyper);
        int first = -1;   // the running product advances once per step: element 0 of the first non-empty tensor of the first launch
        for (int i = 0; off == 0 && i < n && first < 0; ++i)
            if (a.t[i].n > 0) first = i;
        x.mu_job = first;
        g_prof_tag = 0;
        if (a.start[n] > 0) {
            if (clip_state) {
                if (lion) STGCN_LAUNCH("lion_clip", st, optim_clip_kernel<kOptLion>, dim3(a.start[n]), dim3(kThreads), 0, a, x, clip_state);
                else STGCN_LAUNCH("nadamw_clip", st, optim_clip_kernel<kOptNadamw>, dim3(a.start[n]), dim3(kThreads), 0, a, x, clip_state);
            } else if (lion) STGCN_LAUNCH("lion", st, optim_kernel<kOptLion>, dim3(a.start[n]), dim3(kThreads), 0, a, x);
            else STGCN_LAUNCH("nadamw", st, optim_kernel<kOptNadamw>, dim3(a.start[n]), dim3(kThreads), 0, a, x);
        }
    }
    return STGCN_OK;
}
}  // namespace

int stgcn_optim_step(const stgcn_adamw_tensor* tensors, int32_t count, const stgcn_optim_hyper* hyper, void* stream) {
    const int rc = check_optim_hyper(hyper, "stgcn_optim_step");
    if (rc) return rc;
    return optim_step_impl("stgcn_optim_step", tensors, count, hyper, nullptr, stream);
}

int stgcn_grad_clip_words(const stgcn_adamw_tensor* tensors, int32_t count, int64_t* words) {
    if (!words) return fail(STGCN_ERR_INVALID, "stgcn_grad_clip_words: words is NULL");
    return grad_clip_words_impl(tensors, count, "stgcn_grad_clip_words", words);
}

int stgcn_grad_norm(const stgcn_adamw_tensor* tensors, int32_t count, const stgcn_grad_clip* clip, void* stream) {
    STGCN_FLUSH_PENDING_PACK();
    int64_t need = 0;
    int rc = grad_clip_words_impl(tensors, count, "stgcn_grad_norm", &need);
    if (rc) return rc;
    rc = check_clip(clip, need, "stgcn_grad_norm");
    if (rc) return rc;
    for (int i = 0; i < count; ++i)
        if (!tensors[i].grad && tensors[i].numel > 0) return fail(STGCN_ERR_INVALID, "stgcn_grad_norm: NULL gradient in entry %d", i);
    hipStream_t st = (hipStream_t)stream;
    // a table longer than one launch's argument block: every launch adds its sum to state[0], the last one forms total and coef (ONE norm)
    const int launches = count > 0 ? cdiv(count, kAdamwMaxTensors) : 1;
    for (int l = 0; l < launches; ++l) {
        const int off = l * kAdamwMaxTensors;
        AdamwArgs a = zeroed<AdamwArgs>();
        const int n = count - off < kAdamwMaxTensors ? count - off : kAdamwMaxTensors;
        for (int i = 0; i < n; ++i) {
            a.t[i].g = tensors[off + i].grad; a.t[i].n = (long)tensors[off + i].numel;
            a.start[i + 1] = a.start[i] + cdiv(tensors[off + i].numel, kAdamwChunk);
        }
        a.count = n;
        ClipArgs c;
        c.state = clip->state; c.max_norm = clip->max_norm; c.first = l == 0; c.last = l == launches - 1;
        g_prof_tag = 0;
        STGCN_LAUNCH("grad_norm", st, grad_norm_kernel, dim3(grad_norm_wgs(tensors, off, n)), dim3(kThreads), (kThreads / 64) * sizeof(double), a, c);
    }
    return STGCN_OK;
}

int stgcn_optim_step_clip(const stgcn_adamw_tensor* tensors, int32_t count, const stgcn_optim_hyper* hyper, const stgcn_grad_clip* clip,
                          void* stream) {
    int rc = check_optim_hyper(hyper, "stgcn_optim_step_clip");
    if (rc) return rc;
    int64_t need = 0;
    rc = grad_clip_words_impl(tensors, count, "stgcn_optim_step_clip", &need);
    if (rc) return rc;
    rc = check_clip(clip, need, "stgcn_optim_step_clip");
    if (rc) return rc;
    return optim_step_impl("stgcn_optim_step_clip", tensors, count, hyper, clip->state, stream);
}

int stgcn_grad_flush_clip_words(int32_t n_blocks, const stgcn_flush_block* blocks, const stgcn_outblock_desc* head_desc,
                                const stgcn_outblock_grads* head_grads, float* head_ws, int64_t* words) {
    if (!words) return fail(STGCN_ERR_INVALID, "stgcn_grad_flush_clip_words: words is NULL");
    ReduceList RL;
    const int rc = flush_job_list(RL, "stgcn_grad_flush_clip_words", n_blocks, blocks, head_desc, head_grads, head_ws, nullptr, 0, false);
    if (rc) return rc;
    *words = STGCN_CLIP_HDR_WORDS + (RL.ra.start[RL.nj] > 1 ? RL.ra.start[RL.nj] : 1);
    return STGCN_OK;
}

int stgcn_grad_flush_clip(int32_t n_blocks, const stgcn_flush_block* blocks, const stgcn_outblock_desc* head_desc,
                          const stgcn_outblock_grads* head_grads, float* head_ws, const stgcn_grad_clip* clip, void* stream) {
    STGCN_FLUSH_PENDING_PACK();
    ReduceList RL;
    int rc = flush_job_list(RL, "stgcn_grad_flush_clip", n_blocks, blocks, head_desc, head_grads, head_ws, nullptr, 0, false);
    if (rc) return rc;
    if (RL.overflow) return fail(STGCN_ERR_INVALID, "stgcn_grad_flush_clip: more than %d reduction jobs in one launch", kMaxReduceJobs);
    if (RL.nj == 0 || RL.ra.start[RL.nj] < 1) return fail(STGCN_ERR_INVALID, "stgcn_grad_flush_clip: nothing to flush");
    rc = check_clip(clip, STGCN_CLIP_HDR_WORDS + (int64_t)RL.ra.start[RL.nj], "stgcn_grad_flush_clip");
    if (rc) return rc;
    RL.ra.njobs = RL.nj;
    ReduceClipArgs a = zeroed<ReduceClipArgs>();
    static_cast<ReduceArgs&>(a) = RL.ra;
    a.c.state = clip->state; a.c.max_norm = clip->max_norm; a.c.first = 1; a.c.last = 1;
    a.skip_job = -1;      // the loss value of the fused head rides in the flush as a job of its own: no gradient, not in the norm
    for (int k = 0; k < RL.nj; ++k)
        if (head_desc && head_grads->loss && RL.ra.job[k].dst == head_grads->loss) a.skip_job = k;
    g_prof_tag = 0;
    STGCN_LAUNCH("reduce_norm", (hipStream_t)stream, reduce_kernel<kOptNorm>, dim3(RL.ra.start[RL.nj]), dim3(kThreads), kThreads * 4 * sizeof(float), a);
    return STGCN_OK;
}

int stgcn_grad_flush_optim(int32_t n_blocks, const stgcn_flush_block* blocks, const stgcn_outblock_desc* head_desc,
                           const stgcn_outblock_grads* head_grads, float* head_ws, const stgcn_adamw_tensor* opt, int32_t opt_count,
                           const stgcn_optim_hyper* hyper, void* stream) {
    int rc = check_optim_hyper(hyper, "stgcn_grad_flush_optim");
    if (rc) return rc;
    if (hyper->kind == STGCN_OPT_ADAMW) {
        stgcn_adamw_hyper h = zeroed<stgcn_adamw_hyper>();
        h.lr = (float)hyper->lr; h.beta1 = (float)hyper->beta1; h.beta2 = (float)hyper->beta2; h.eps = (float)hyper->eps;
        h.weight_decay = (float)hyper->weight_decay; h.step = hyper->step; h.step_dev = hyper->step_dev; h.lr_dev = hyper->lr_dev;
        return stgcn_grad_flush(n_blocks, blocks, head_desc, head_grads, head_ws, opt, opt_count, &h, stream);
    }
    STGCN_FLUSH_PENDING_PACK();
    if (opt_count < 1 || !opt) return fail(STGCN_ERR_INVALID, "stgcn_grad_flush_optim: empty optimizer table");
    const bool lion = hyper->kind == STGCN_OPT_LION;
    ReduceList RL;
    rc = flush_job_list(RL, "stgcn_grad_flush_optim", n_blocks, blocks, head_desc, head_grads, head_ws, opt, opt_count, !lion);
    if (rc) return rc;
    if (RL.overflow) return fail(STGCN_ERR_INVALID, "stgcn_grad_flush_optim: more than %d reduction jobs in one launch", kMaxReduceJobs);
    RL.ra.lr = (float)hyper->lr; RL.ra.b1 = (float)hyper->beta1; RL.ra.b2 = (float)hyper->beta2; RL.ra.eps = (float)hyper->eps;
    RL.ra.wd = (float)hyper->weight_decay; RL.ra.lb1 = (float)log(hyper->beta1); RL.ra.lb2 = (float)log(hyper->beta2);
    RL.ra.step = (long)hyper->step; RL.ra.step_dev = reinterpret_cast<const long*>(hyper->step_dev); RL.ra.lr_dev = hyper->lr_dev;
    OptimExtra x = optim_extra(hyper);
    for (int k = 0; k < RL.nj && x.mu_job < 0; ++k)      // the running product advances at element 0 of the first optimizer job
        if (RL.ra.job[k].p && (long)RL.ra.job[k].n0 * RL.ra.job[k].n1 * RL.ra.job[k].n2 > 0) x.mu_job = k;
    if (lion)
        for (int k = 0; k < RL.nj; ++k) RL.ra.job[k].v = nullptr;
    g_prof_tag = 0;
    return launch_reduce_list_optim(lion ? "reduce_lion" : "reduce_nadamw", RL, hyper->kind, x, (hipStream_t)stream);
}

namespace {
// the argument checks the masked and the unmasked loss launch share
int check_loss_grad(const char* who, int32_t kind, float delta, const float* pred, const float* target, int64_t n, const float* loss,
                    const float* dpred, const int64_t* target_index_dev, const int64_t* target_window_dev, int64_t window_floats) {
    const int rc = check_loss_kind(who, kind, delta);
    if (rc) return rc;
    if (!pred || !target || !loss || !dpred || n < 1) return fail(STGCN_ERR_INVALID, "%s: NULL buffer or n < 1", who);
    if (target_window_dev) {
        if (!target_index_dev) return fail(STGCN_ERR_INVALID, "%s: target_window_dev (window table) needs target_index_dev != NULL", who);
        if (window_floats < 1 || n % window_floats != 0 || n >= (1ll << 31))
            return fail(STGCN_ERR_INVALID, "%s: n = %lld must be a multiple of window_floats = %lld and below 2^31", who, (long long)n,
                        (long long)window_floats);
    }
    return STGCN_OK;
}
}  // namespace

int stgcn_loss_grad(int32_t kind, float delta, const float* pred, const float* target, int64_t n, float grad_scale, float* loss, float* dpred,
                    const int64_t* target_index_dev, int64_t target_index_stride, const int64_t* target_window_dev, int64_t window_floats,
                    void* stream) {
    STGCN_FLUSH_PENDING_PACK();
    const int rc = check_loss_grad("stgcn_loss_grad", kind, delta, pred, target, n, loss, dpred, target_index_dev, target_window_dev, window_floats);
    if (rc) return rc;
    g_prof_tag = 0;
    const char* label = kind == STGCN_LOSS_MSE ? "mse_loss_grad" : "loss_grad";   // (the MSE launch keeps the label the kernel timer's readers know)
    STGCN_LAUNCH(label, (hipStream_t)stream, loss_grad_kernel, dim3(1), dim3(1024), 16 * sizeof(float), (int)kind, delta, pred, target,
                 (long)n, grad_scale, loss, dpred, reinterpret_cast<const long*>(target_index_dev), (long)target_index_stride,
                 reinterpret_cast<const long*>(target_window_dev), target_window_dev ? (unsigned)window_floats : 0u);
    return STGCN_OK;
}

int stgcn_loss_grad_masked(int32_t kind, float delta, const float* pred, const float* target, int64_t n, float grad_scale, float* loss,
                           float* dpred, const int64_t* target_index_dev, int64_t target_index_stride, const int64_t* target_window_dev,
                           int64_t window_floats, const stgcn_loss_mask* mask, void* stream) {
    STGCN_FLUSH_PENDING_PACK();
    int rc = check_loss_grad("stgcn_loss_grad_masked", kind, delta, pred, target, n, loss, dpred, target_index_dev, target_window_dev, window_floats);
    if (rc) return rc;
    rc = check_loss_mask("stgcn_loss_grad_masked", mask, n, target_index_dev != nullptr, target_index_stride, target_window_dev != nullptr,
                         window_floats);
    if (rc) return rc;
    g_prof_tag = 0;
    STGCN_LAUNCH("loss_grad_masked", (hipStream_t)stream, loss_grad_masked_kernel, dim3(1), dim3(1024), 16 * sizeof(float), (int)kind, delta, pred,
                 target, (long)n, grad_scale, loss, dpred, reinterpret_cast<const long*>(target_index_dev), (long)target_index_stride,
                 reinterpret_cast<const long*>(target_window_dev), target_window_dev ? (unsigned)window_floats : 0u, mask->valid, mask->row_valid,
                 (int)mask->row_elems);
    return STGCN_OK;
}

int stgcn_mse_loss_grad(const float* pred, const float* target, int64_t n, float grad_scale, float* loss, float* dpred,
                        const int64_t* target_index_dev, int64_t target_index_stride, void* stream) {
    return stgcn_loss_grad(STGCN_LOSS_MSE, 0.f, pred, target, n, grad_scale, loss, dpred, target_index_dev, target_index_stride, nullptr, 0, stream);
}

int stgcn_mse_loss_grad_windows(const float* pred, const float* target, int64_t n, float grad_scale, float* loss, float* dpred,
                                const int64_t* target_index_dev, int64_t target_index_stride, const int64_t* target_window_dev,
                                int64_t window_floats, void* stream) {
    return stgcn_loss_grad(STGCN_LOSS_MSE, 0.f, pred, target, n, grad_scale, loss, dpred, target_index_dev, target_index_stride, target_window_dev,
                           window_floats, stream);
}

int stgcn_eval_arm(double* state, int64_t* pos, void* stream) {
    STGCN_FLUSH_PENDING_PACK();
    if (!state) return fail(STGCN_ERR_INVALID, "stgcn_eval_arm: state is NULL");
    g_prof_tag = 0;
    STGCN_LAUNCH("eval_arm", (hipStream_t)stream, eval_arm_kernel, dim3(1), dim3(64), 0, state, reinterpret_cast<long*>(pos));
    return STGCN_OK;
}

namespace {
// checks, kernel arguments and grid shared by the masked and the unmasked accumulate launch
int eval_acc_setup(const char* who, const float* pred, const float* target, int32_t B, int32_t N, const float* scale, const float* mean,
                   int64_t first_valid, int64_t* pos, int64_t target_stride, int64_t num_windows, double* state, EvalAccArgs* out, int* wgs_out) {
    if (!state) return fail(STGCN_ERR_INVALID, "%s: state is NULL", who);
    if (!pred || !target) return fail(STGCN_ERR_INVALID, "%s: NULL pred / target", who);
    if (B < 1 || N < 1) return fail(STGCN_ERR_INVALID, "%s: n = B * N must be positive (B=%d, N=%d)", who, B, N);
    if ((scale == nullptr) != (mean == nullptr)) return fail(STGCN_ERR_INVALID, "%s: scale and mean come together (both or neither)", who);
    if (first_valid < 0 || first_valid >= B) return fail(STGCN_ERR_INVALID, "%s: first_valid=%lld outside [0, B=%d)", who, (long long)first_valid, B);
    if (pos) {
        if (first_valid != 0) return fail(STGCN_ERR_INVALID, "%s: with position words first_valid is read from them (pass 0)", who);
        if (num_windows < B) return fail(STGCN_ERR_INVALID, "%s: %lld windows are fewer than one batch of %d", who, (long long)num_windows, B);
        if (target_stride < 0) return fail(STGCN_ERR_INVALID, "%s: negative target stride", who);
    }
    EvalAccArgs a;
    a.pred = pred; a.target = target; a.scale = scale; a.mean = mean; a.state = state;
    a.pos = reinterpret_cast<long*>(pos);
    a.tstride = (long)target_stride; a.first_valid = (long)first_valid; a.num = (long)num_windows;
    a.B = B; a.N = N;
    const long n = (long)B * N;
    int wgs = 1;
    if (n >= eval_big_threshold()) {
        wgs = cdiv(n, 2 * kEvalThreads);
        wgs = wgs < 2 ? 2 : (wgs > kEvalMaxWgs ? kEvalMaxWgs : wgs);
    }
    *out = a;
    *wgs_out = wgs;
    return STGCN_OK;
}
}  // namespace

int stgcn_eval_accumulate(const float* pred, const float* target, int32_t B, int32_t N, const float* scale, const float* mean,
                          int64_t first_valid, int64_t* pos, int64_t target_stride, int64_t num_windows, double* state, void* stream) {
    STGCN_FLUSH_PENDING_PACK();
    EvalAccArgs a;
    int wgs = 1;
    const int rc = eval_acc_setup("stgcn_eval_accumulate", pred, target, B, N, scale, mean, first_valid, pos, target_stride, num_windows, state, &a, &wgs);
    if (rc) return rc;
    g_prof_tag = 0;
    STGCN_LAUNCH("eval_acc", (hipStream_t)stream, eval_acc_kernel, dim3(wgs), dim3(kEvalThreads), (kEvalThreads / 64) * 4 * sizeof(double), a);
    return STGCN_OK;
}

int stgcn_eval_accumulate_masked(const float* pred, const float* target, int32_t B, int32_t N, const float* scale, const float* mean,
                                 int64_t first_valid, int64_t* pos, int64_t target_stride, int64_t num_windows, double* state,
                                 const uint8_t* valid, void* stream) {
    STGCN_FLUSH_PENDING_PACK();
    EvalAccArgs a;
    int wgs = 1;
    const int rc = eval_acc_setup("stgcn_eval_accumulate_masked", pred, target, B, N, scale, mean, first_valid, pos, target_stride, num_windows, state,
                                  &a, &wgs);
    if (rc) return rc;
    if (!valid) return fail(STGCN_ERR_INVALID, "stgcn_eval_accumulate_masked: valid is NULL");
    static_assert(STGCN_EVAL_MASKED_STATE_WORDS == kEvalHdr + kEvalMaxWgs * kEvalMaskedSums, "masked state size");
    g_prof_tag = 0;
    STGCN_LAUNCH("eval_acc_masked", (hipStream_t)stream, eval_acc_masked_kernel, dim3(wgs), dim3(kEvalThreads),
                 (kEvalThreads / 64) * kEvalMaskedSums * sizeof(double), a, valid);
    return STGCN_OK;
}

#ifdef STGCN_PHASE_TIMING
// diagnostic build only: select which kernel stamps its phases, read the stamps back (host buffer of 4096*16 int64)
extern "C" int stgcn_debug_phase_select(int kid) {   // (diagnostic entries: not in include/stgcn_hip.h)
    hipMemcpyToSymbol(HIP_SYMBOL(stgcn_phase_kid), &kid, sizeof(int));
    static long long zeros[4096 * 16];
    hipMemcpyToSymbol(HIP_SYMBOL(stgcn_phase_buf), zeros, sizeof(zeros));
    return STGCN_OK;
}
extern "C" int stgcn_debug_phase_read(long long* out) {
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out, HIP_SYMBOL(stgcn_phase_buf), sizeof(long long) * 4096 * 16);
    return STGCN_OK;
}
#endif
