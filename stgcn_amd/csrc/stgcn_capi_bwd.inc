// Backward entry point (included inside the extern "C" block of stgcn_capi.hip).

int stgcn_stblock_backward(const stgcn_stblock_desc* d, const stgcn_stblock_params* P, const float* x, const float* gso_t_pad,
                           const float* dy, const float* y, const float* saved, float* ws, const stgcn_stblock_grads* G, float* dx, uint64_t seed,
                           uint64_t offset, const uint64_t* offset_dev, void* stream) {
    return stgcn_stblock_backward_hook(d, P, x, gso_t_pad, dy, y, saved, ws, G, dx, seed, offset, offset_dev, nullptr, stream);
}

int stgcn_stblock_backward_hook(const stgcn_stblock_desc* d, const stgcn_stblock_params* P, const float* x, const float* gso_t_pad,
                                const float* dy, const float* y, const float* saved, float* ws, const stgcn_stblock_grads* G, float* dx, uint64_t seed,
                                uint64_t offset, const uint64_t* offset_dev, const stgcn_ln_hook* dx_hook, void* stream) {
    STGCN_FLUSH_PENDING_PACK();
    stgcn_stblock_plan pl;
    int rc = stgcn_stblock_plan_query(d, &pl);
    if (rc) return rc;
    if (!P || !x || !gso_t_pad || !dy || !saved || !ws || !G) return fail(STGCN_ERR_INVALID, "stgcn_stblock_backward: NULL buffer");
    if (!d->dy_rowstats_ready && !y) return fail(STGCN_ERR_INVALID, "stgcn_stblock_backward: y (the forward's output) is required unless dy_rowstats_ready is set");
    if (d->need_dx && !dx) return fail(STGCN_ERR_INVALID, "stgcn_stblock_backward: need_dx set but dx is NULL");
    if (dx_hook && dx_hook->rowstat && (dx_hook->N != d->N || dx_hook->C != d->c_in || !d->need_dx))
        return fail(STGCN_ERR_INVALID, "stgcn_stblock_backward: dx_hook describes a LayerNorm over [%d, %d], the input gradient is [%d, %d] per slab",
                    dx_hook->N, dx_hook->C, d->N, d->c_in);
    const Derived v = derive(d);
    const BwdGeom bg = bwd_geom(d->B, d->T, d->N, d->c_in, d->c0, d->c1, d->c2, d->Kt, v.terms, d->need_dx);
    hipStream_t st = (hipStream_t)stream;
    g_prof_tag = d->reserved;
    g_bf16 = d->dtype == STGCN_DTYPE_BF16;
    if (dx_hook && dx_hook->rowstat && dx_hook->dtype != d->dtype)
        return fail(STGCN_ERR_INVALID, "stgcn_stblock_backward: dx_hook describes tensors of another dtype than this call");
    float* part = ws + pl.ws_part;
    const int training = d->training && d->droprate > 0.f;

    // ---- LayerNorm + dropout + gate (tmp_conv2) backward ---------------------------------------------
    LnBwdArgs ln;
    memset(&ln, 0, sizeof(ln));
    ln.dy = dy; ln.y = y; ln.beta = P->ln_b; ln.U = saved + pl.sv_U2; ln.S = saved + pl.sv_S2; ln.gamma = P->ln_w;
    ln.mean = saved + pl.sv_mean; ln.rstd = saved + pl.sv_rstd; ln.rowstat = reinterpret_cast<float2*>(ws + pl.ws_rowstat_b);
    ln.dZ = ws + pl.ws_dZ2; ln.dgam_part = part + bg.off_ln_g; ln.dbet_part = part + bg.off_ln_b;
    ln.n = d->N * d->c2; ln.N = d->N; ln.C = d->c2; ln.act = d->act; ln.training = training; ln.spg = bg.ln_spg; ln.slabs = v.slabs2;
    ln.keep_scale = 1.0f / (1.0f - d->droprate); ln.thresh = drop_thresh(d->droprate); ln.seed = seed; ln.offset = offset; ln.offset_dev = offset_dev;
    if (!d->dy_rowstats_ready)   // (else: the producer of dy wrote the row partials in its epilogue, stgcn_ln_hook)
        STGCN_LAUNCH_ET("ln_bwd_rowstats", st, (ln_bwd_rowstats_kernel<ET>), dim3(cdiv(v.slabs2 * (ln.n / 4), kThreads)), dim3(kThreads), 0, ln);
    if (cdiv(ln.n / 4, kThreads) >= kLnBigColgroups) {
        ln.slabconst = reinterpret_cast<float2*>(ws + pl.ws_rowstat_b + 2 * v.rows2);
        STGCN_LAUNCH("ln_slab_consts", st, ln_slab_consts_kernel, dim3((unsigned)v.slabs2), dim3(kThreads), 64, ln);
    }
    if (bg.k1) {
        // ---- LayerNorm + dropout + gate backward, weight gradient and transposed conv of tmp_conv2 in one time-stepping launch ----
        Tc2BwdArgs a;
        memset(&a, 0, sizeof(a));
        const bool recomp = tc2_recompute(g_bf16);
        a.y = hook_mask_from_y() ? y : nullptr;   // the dropout mask of this block's LayerNorm: read off its output (dropped = -0.0; both activation types) or regenerated (STGCN_HOOK_MASK=philox)
        a.dy = dy; a.U = saved + pl.sv_U2; a.S = saved + pl.sv_S2; a.Wp = ws + pl.ws_W2p; a.bias = ws + pl.ws_b2; a.gamma = P->ln_w; a.mean = saved + pl.sv_mean; a.rstd = saved + pl.sv_rstd;
        a.rowstat = ln.rowstat; a.slabconst = ln.slabconst; a.G = saved + pl.sv_G; a.Wd = ws + pl.ws_W2dense; a.dYg = ws + pl.ws_dYg;
        a.part = part + bg.off_k1; a.dgam_part = part + bg.off_ln_g; a.dbet_part = part + bg.off_ln_b;
        a.B = d->B; a.T1 = v.T1; a.T2 = v.T2; a.N = d->N; a.act = d->act; a.training = training; a.node_tiles = bg.node_tiles;
        a.keep_scale = ln.keep_scale; a.thresh = ln.thresh; a.seed = seed; a.offset = offset; a.offset_dev = offset_dev;
        const size_t lds = tc2_bwd_lds_bytes(d->c2, d->Kt, v.T1, v.T2, recomp);
        const dim3 grid((unsigned)bg.k1_wgs), blk(512);   // 4 E waves + 4 M waves
        if (g_debug_stages && !g_bf16)   // stage tests: dZ2 (which the fused kernel keeps on chip) from the stage-per-launch kernel; it writes the same
                              // per-window LayerNorm-parameter partials (ln_spg = T2, ln_sg = B), which the fused kernel then overwrites
            STGCN_LAUNCH("ln_gate_bwd", st, (ln_gate_bwd_kernel<float>), dim3(cdiv(ln.n / 4, kThreads), bg.ln_sg), dim3(kThreads),
                         (8 + 2 * bg.ln_spg) * sizeof(float), ln);
#define STGCN_TC2_BWD(C2_, KT_)                                                                                        \
        do {                                                                                                           \
            if (training && d->act == STGCN_ACT_GLU) STGCN_LAUNCH_ETB("tc2_bwd", st, (tc2_bwd_kernel<C2_, KT_, true, 0, RC_, ET>), grid, blk, lds, a);   \
            else if (training) STGCN_LAUNCH_ETB("tc2_bwd", st, (tc2_bwd_kernel<C2_, KT_, true, 1, RC_, ET>), grid, blk, lds, a);      \
            else if (d->act == STGCN_ACT_GLU) STGCN_LAUNCH_ETB("tc2_bwd", st, (tc2_bwd_kernel<C2_, KT_, false, 0, RC_, ET>), grid, blk, lds, a);       \
            else STGCN_LAUNCH_ETB("tc2_bwd", st, (tc2_bwd_kernel<C2_, KT_, false, 1, RC_, ET>), grid, blk, lds, a);                 \
        } while (0)
#define STGCN_TC2_BWD_RC(C2_, KT_) do { if (recomp) { constexpr bool RC_ = true; STGCN_TC2_BWD(C2_, KT_); } else { constexpr bool RC_ = false; STGCN_TC2_BWD(C2_, KT_); } } while (0)
        if (d->c2 == 64) {
            if (d->Kt == 2) STGCN_TC2_BWD_RC(64, 2); else if (d->Kt == 3) STGCN_TC2_BWD_RC(64, 3); else STGCN_TC2_BWD_RC(64, 4);
        } else {
            STGCN_TC2_BWD_RC(128, 3);
        }
#undef STGCN_TC2_BWD_RC
#undef STGCN_TC2_BWD
    } else {
    STGCN_F32_ONLY("ln_gate_bwd + row-tile weight / data gradients of tmp_conv2");
    STGCN_LAUNCH("ln_gate_bwd", st, (ln_gate_bwd_kernel<float>), dim3(cdiv(ln.n / 4, kThreads), bg.ln_sg), dim3(kThreads),
                 (8 + 2 * bg.ln_spg) * sizeof(float), ln);

    // ---- weight gradient of tmp_conv2 (needs only dZ2) ---------------------------------------------------------------
    TconvBwdWeightArgs wa;
    memset(&wa, 0, sizeof(wa));
    wa.ts.src = saved + pl.sv_G; wa.ts.C = d->c1; wa.ts.taps = d->Kt; wa.ts.N = d->N; wa.ts.Tsrc = v.T1; wa.ts.Tdst = v.T2; wa.ts.dir = 1;
    wa.ts.rows = v.rows2;
    wa.dZ = ws + pl.ws_dZ2; wa.part = part + bg.w2.off; wa.NC = v.NC2; wa.Mpad = bg.w2.Mpad; wa.rows_per_chunk = bg.w2.rows_per_chunk;
    wa.chunks = bg.w2.chunks;
    rc = launch_bwd_weight("tconv_bwd_weight.tc2", wa, bg.w2, st);
    if (rc) return rc;

    // ---- tmp_conv2 backward-data (+ relu mask) : dZ2 -> dYg ---------------------------------------------
    {
        TconvBwdDataArgs a;
        memset(&a, 0, sizeof(a));
        a.ts.src = ws + pl.ws_dZ2; a.ts.C = v.NC2; a.ts.taps = d->Kt; a.ts.N = d->N; a.ts.Tsrc = v.T2; a.ts.Tdst = v.T1; a.ts.dir = -1;
        a.ts.rows = v.rows1;
        a.Wp = ws + pl.ws_W2d; a.KCH = d->Kt * v.NC2 / 16; a.Cin = d->c1; a.Gmask = saved + pl.sv_G; a.dX = ws + pl.ws_dYg;
        rc = launch_bwd_data("tconv_bwd_data.tc2", a, v.CP1 / 16, st);
        if (rc) return rc;
    }
    }

    // ---- graph conv backward -----------------------------------------------------------------------------
    {
        GconvBwdArgs a;
        memset(&a, 0, sizeof(a));
        a.dY = ws + pl.ws_dYg; a.X0 = saved + pl.sv_A; a.Xk = saved + pl.sv_Xk; a.LTp = gso_t_pad; a.W = P->gc_w;
        a.dA = ws + pl.ws_dA; a.part = part + bg.off_gc; a.N = d->N; a.NP = v.NP; a.Ks = v.terms;
        a.kipf = d->graph_conv == STGCN_GC_KIPF; a.slabs = v.slabs1;
        a.Gk = pl.tiled_gc ? ws + pl.ws_Gk : nullptr; a.tiles_per_wg = bg.gc_tiles_per_wg; a.wgs = bg.gc_count;
        a.XT = pl.tiled_gc && v.terms > 1 ? ws + pl.ws_XT : nullptr;
        rc = launch_gconv_bwd(a, st);
        if (rc) return rc;
    }

    if (bg.k3) {
        // ---- Align + gate backward, weight gradient and transposed conv of tmp_conv1 (+ the row partials of the LayerNorm in front of
        //      x) in one time-stepping launch; dZ1 stays on chip -----------------------------------------------------------------------
        if (g_debug_stages && !g_bf16) {   // stage tests: dZ1 from the stage-per-launch kernel (its dWa partials go to their own, unused slot)
            AlignBwdArgs da;
            memset(&da, 0, sizeof(da));
            da.dA = ws + pl.ws_dA; da.WaT = ws + pl.ws_WaT; da.dZ = ws + pl.ws_dZ1; da.U = saved + pl.sv_U1; da.S = saved + pl.sv_S1;
            da.part = part + bg.off_al; da.rows = v.rows1; da.c0 = d->c0; da.c1 = d->c1; da.KCH = v.CP1 / 16; da.act = d->act;
            const size_t dlds = (size_t)(64 * (d->c1 + 4) + 64 * (d->c0 + 4) + 16 * d->c1) * sizeof(float);
            STGCN_LAUNCH("align_gate_bwd", st, (align_gate_bwd_kernel<1>), dim3(bg.al_wgs), dim3(kThreads), dlds, da);
        }
        Tc1BwdArgs a;
        memset(&a, 0, sizeof(a));
        a.dA = ws + pl.ws_dA; a.U = saved + pl.sv_U1; a.S = saved + pl.sv_S1; a.x = x; a.WaD = ws + pl.ws_WaDense; a.Wd = ws + pl.ws_W1dense;
        a.dx = dx; a.part = part + bg.off_k3; a.B = d->B; a.T = d->T; a.T1 = v.T1; a.N = d->N; a.node_tiles = bg.node_tiles;
        const bool epi = dx_hook && dx_hook->rowstat && dx_hook->C == d->c_in && dx_hook->N == d->N;
        if (epi) a.rs = rowstat_out(dx_hook);
        const bool x6 = mfma_x6() && !g_bf16 && g_bwd_precision == 0 && tc1_bwd_lds_bytes(d->c0, d->c_in, d->Kt, true) <= 160 * 1024;   // "bf16x6" weight-gradient products
        const size_t lds = tc1_bwd_lds_bytes(d->c0, d->c_in, d->Kt, x6);
        const dim3 grid((unsigned)bg.k3_wgs), blk(768);
#define STGCN_TC1_BWD(CIN_)                                                                                    \
        do {                                                                                                   \
            if (x6 && d->act == STGCN_ACT_GLU) STGCN_LAUNCH("tc1_bwd", st, (tc1_bwd_x6_kernel<64, CIN_, 3, 0>), grid, blk, lds, a);   \
            else if (x6) STGCN_LAUNCH("tc1_bwd", st, (tc1_bwd_x6_kernel<64, CIN_, 3, 1>), grid, blk, lds, a);             \
            else if (d->act == STGCN_ACT_GLU) STGCN_LAUNCH_ETB("tc1_bwd", st, (tc1_bwd_kernel<64, CIN_, 3, 0, ET>), grid, blk, lds, a);   \
            else STGCN_LAUNCH_ETB("tc1_bwd", st, (tc1_bwd_kernel<64, CIN_, 3, 1, ET>), grid, blk, lds, a);             \
        } while (0)
        if (d->c_in == 64) STGCN_TC1_BWD(64); else if (d->c_in == 32) STGCN_TC1_BWD(32); else STGCN_TC1_BWD(16);
#undef STGCN_TC1_BWD
        if (dx_hook && dx_hook->rowstat && !epi) {   // hook of a shape the epilogue does not cover: a pass over dx
            LnBwdArgs hl;
            memset(&hl, 0, sizeof(hl));
            const LnRowstatOut o = rowstat_out(dx_hook);
            hl.dy = dx; hl.y = o.y; hl.beta = o.beta; hl.gamma = o.gamma; hl.rowstat = o.rowstat;
            hl.n = o.N * o.C; hl.N = o.N; hl.C = o.C; hl.act = o.act; hl.training = o.training; hl.slabs = (long)d->B * d->T;
            hl.keep_scale = o.keep_scale; hl.thresh = o.thresh; hl.seed = o.seed; hl.offset = o.offset; hl.offset_dev = o.offset_dev;
            STGCN_LAUNCH_ET("ln_bwd_rowstats", st, (ln_bwd_rowstats_kernel<ET>), dim3(cdiv(hl.slabs * (hl.n / 4), kThreads)), dim3(kThreads), 0, hl);
        }
    } else {
    // ---- Align(c0 -> c1) + gate (tmp_conv1) backward ---------------------------------------------------------
    if (bg.thin) {   // thin first layer: recompute + gate backward + weight gradient in one kernel, dZ1 only if dx is needed
        ThinBwdArgs a;
        memset(&a, 0, sizeof(a));
        a.dA = ws + pl.ws_dA; a.Wd = ws + pl.ws_W1dense; a.bias = ws + pl.ws_b1; a.WaT = ws + pl.ws_WaT;
        a.dZ = d->need_dx ? ws + pl.ws_dZ1 : nullptr; a.part = part + bg.off_al; a.rows = v.rows1; a.c0 = d->c0; a.act = d->act;
        a.ts.src = x; a.ts.C = d->c_in; a.ts.taps = d->Kt; a.ts.N = d->N; a.ts.Tsrc = d->T; a.ts.Tdst = v.T1; a.ts.dir = 1; a.ts.rows = v.rows1;
        a.ts.bstride = d->x_bstride; a.ts.idx_dev = reinterpret_cast<const long*>(d->x_index_dev); a.ts.idx_stride = d->x_index_stride; a.ts.win_tab = reinterpret_cast<const long*>(d->x_window_dev);
        if (thin_wave_tiles()) {   // wave-per-tile form (stgcn_kernels_thin.hip.h): same arguments, same partials
            if (d->act == STGCN_ACT_GLU) STGCN_LAUNCH_ETB("align_gate_bwd", st, (thin_tc1_bwd2_kernel<ET, 0>), dim3(bg.al_wgs), dim3(kThreads), thin_bwd2_lds_bytes(), a);
            else STGCN_LAUNCH_ETB("align_gate_bwd", st, (thin_tc1_bwd2_kernel<ET, 1>), dim3(bg.al_wgs), dim3(kThreads), thin_bwd2_lds_bytes(), a);
        } else {
        const size_t lds = (size_t)(64 * 20 + 64 * (d->c0 + 4) + 64 * (2 * d->c0 + 4) + 64 * 20 + 256) * sizeof(float);
        STGCN_LAUNCH_ETB("align_gate_bwd", st, (thin_tc1_bwd_kernel<ET>), dim3(bg.al_wgs), dim3(kThreads), lds, a);
        }
    } else {
        STGCN_F32_ONLY("align_gate_bwd");
        AlignBwdArgs a;
        memset(&a, 0, sizeof(a));
        a.dA = ws + pl.ws_dA; a.WaT = ws + pl.ws_WaT; a.dZ = ws + pl.ws_dZ1;
        if (pl.recompute_tc1) {
            a.U = nullptr; a.S = nullptr; a.Wd = ws + pl.ws_W1dense; a.bias = ws + pl.ws_b1; a.KPd = v.KP1;
            a.ts.src = x; a.ts.C = d->c_in; a.ts.taps = d->Kt; a.ts.N = d->N; a.ts.Tsrc = d->T; a.ts.Tdst = v.T1; a.ts.dir = 1; a.ts.rows = v.rows1;
            a.ts.bstride = d->x_bstride; a.ts.idx_dev = reinterpret_cast<const long*>(d->x_index_dev); a.ts.idx_stride = d->x_index_stride; a.ts.win_tab = reinterpret_cast<const long*>(d->x_window_dev);
        } else {
            a.U = saved + pl.sv_U1; a.S = saved + pl.sv_S1;
        }
        a.part = part + bg.off_al; a.rows = v.rows1; a.c0 = d->c0; a.c1 = d->c1; a.KCH = v.CP1 / 16; a.act = d->act;
        const size_t lds = (size_t)(64 * (d->c1 + 4) + 64 * (d->c0 + 4) + 16 * d->c1) * sizeof(float);
        if (d->c0 == 64) STGCN_LAUNCH("align_gate_bwd", st, (align_gate_bwd_kernel<1>), dim3(bg.al_wgs), dim3(kThreads), lds, a);
        else STGCN_LAUNCH("align_gate_bwd", st, (align_gate_bwd_kernel<2>), dim3(bg.al_wgs), dim3(kThreads), lds, a);
    }

    // ---- weight gradient of tmp_conv1 (needs dZ1; the thin first layer accumulated it inside thin_tc1_bwd_kernel) ----
    if (!bg.thin) {
        TconvBwdWeightArgs wa;
        memset(&wa, 0, sizeof(wa));
        wa.ts.taps = d->Kt; wa.ts.N = d->N; wa.ts.dir = 1;
        wa.ts.src = x; wa.ts.C = d->c_in; wa.ts.Tsrc = d->T; wa.ts.Tdst = v.T1; wa.ts.rows = v.rows1;
        wa.ts.bstride = d->x_bstride; wa.ts.idx_dev = reinterpret_cast<const long*>(d->x_index_dev); wa.ts.idx_stride = d->x_index_stride; wa.ts.win_tab = reinterpret_cast<const long*>(d->x_window_dev);
        wa.dZ = ws + pl.ws_dZ1; wa.part = part + bg.w1.off; wa.NC = v.NC1; wa.Mpad = bg.w1.Mpad; wa.rows_per_chunk = bg.w1.rows_per_chunk;
        wa.chunks = bg.w1.chunks;
        rc = launch_bwd_weight("tconv_bwd_weight.tc1", wa, bg.w1, st);
        if (rc) return rc;
    }
    // ---- tmp_conv1 backward-data : dZ1 -> dx ---------------------------------------------------------------
    if (d->need_dx) {
        TconvBwdDataArgs a;
        memset(&a, 0, sizeof(a));
        a.ts.src = ws + pl.ws_dZ1; a.ts.C = v.NC1; a.ts.taps = d->Kt; a.ts.N = d->N; a.ts.Tsrc = v.T1; a.ts.Tdst = d->T; a.ts.dir = -1;
        a.ts.rows = v.rows0;
        a.Wp = ws + pl.ws_W1d; a.KCH = d->Kt * v.NC1 / 16; a.Cin = d->c_in; a.Gmask = nullptr; a.dX = dx;
        rc = launch_bwd_data("tconv_bwd_data.tc1", a, v.CP_in / 16, st);
        if (rc) return rc;
        if (dx_hook && dx_hook->rowstat) {   // no epilogue in this kernel: the hooked LayerNorm's row partials from a pass over dx
            LnBwdArgs hl;
            memset(&hl, 0, sizeof(hl));
            const LnRowstatOut o = rowstat_out(dx_hook);
            hl.dy = dx; hl.y = o.y; hl.beta = o.beta; hl.gamma = o.gamma; hl.rowstat = o.rowstat;
            hl.n = o.N * o.C; hl.N = o.N; hl.C = o.C; hl.act = o.act; hl.training = o.training; hl.slabs = (long)d->B * d->T;
            hl.keep_scale = o.keep_scale; hl.thresh = o.thresh; hl.seed = o.seed; hl.offset = o.offset; hl.offset_dev = o.offset_dev;
            STGCN_LAUNCH_ET("ln_bwd_rowstats", st, (ln_bwd_rowstats_kernel<ET>), dim3(cdiv(hl.slabs * (hl.n / 4), kThreads)), dim3(kThreads), 0, hl);
        }
    }

    }

    // ---- final reduction into the reference's parameter layouts (deferred to stgcn_grad_flush when asked) ------------
    if (d->defer_reduce) return STGCN_OK;
    ReduceList RL;
    reduce_jobs_block(RL, d, v, bg, part, G);
    return launch_reduce_list("reduce", RL, st);
}
