// Backward of the ST block: its stage launchers, then the entry points (included by stgcn_capi.hip).

namespace {
// row partials of a hooked LayerNorm from a pass over dx ([slabs][N][C]): for producers of dx that have no epilogue for them
int launch_hook_rowstats(const stgcn_ln_hook* hook, const float* dx, long slabs, hipStream_t st) {
    LnBwdArgs hl = zeroed<LnBwdArgs>();
    const LnRowstatOut o = rowstat_out(hook);
    hl.dy = dx; hl.y = o.y; hl.beta = o.beta; hl.gamma = o.gamma; hl.rowstat = o.rowstat;
    hl.n = o.N * o.C; hl.N = o.N; hl.C = o.C; hl.act = o.act; hl.training = o.training; hl.slabs = slabs;
    hl.keep_scale = o.keep_scale; hl.thresh = o.thresh; hl.seed = o.seed; hl.offset = o.offset; hl.offset_dev = o.offset_dev;
    STGCN_LAUNCH_ET("ln_bwd_rowstats", st, (ln_bwd_rowstats_kernel<ET>), dim3(cdiv(hl.slabs * (hl.n / 4), kThreads)), dim3(kThreads), 0, hl);
    return STGCN_OK;
}

// the backward's call: the buffers only it has, and its stages
struct BlockBwdCall : BlockCall {
    const float* gso_t_pad;
    const float* dy;
    const float* y;
    float* dx;
    const stgcn_ln_hook* dx_hook;
    LnBwdArgs ln;   // LayerNorm backward: shared by every tmp_conv2 stage (launch_ln_bwd_stats fills it)

    // fills ln; the row partials (unless the producer of dy wrote them in its epilogue, stgcn_ln_hook) and, for big slabs, the per-slab constants
    int launch_ln_bwd_stats() {
        ln = zeroed<LnBwdArgs>();
        ln.dy = dy; ln.y = y; ln.beta = P->ln_b; ln.U = saved + pl.sv_U2; ln.S = saved + pl.sv_S2; ln.gamma = P->ln_w;
        ln.mean = saved + pl.sv_mean; ln.rstd = saved + pl.sv_rstd; ln.rowstat = reinterpret_cast<float2*>(ws + pl.ws_rowstat_b);
        ln.dZ = ws + pl.ws_dZ2; ln.dgam_part = part() + r.bg.off_ln_g; ln.dbet_part = part() + r.bg.off_ln_b;
        ln.n = d->N * d->c2; ln.N = d->N; ln.C = d->c2; ln.act = d->act; ln.training = training(); ln.spg = r.bg.ln_spg; ln.slabs = r.slabs2;
        ln.keep_scale = keep_scale(); ln.thresh = drop_thresh(d->droprate); ln.seed = seed; ln.offset = offset; ln.offset_dev = offset_dev;
        if (!d->dy_rowstats_ready)
            STGCN_LAUNCH_ET("ln_bwd_rowstats", st, (ln_bwd_rowstats_kernel<ET>), dim3(cdiv(r.slabs2 * (ln.n / 4), kThreads)), dim3(kThreads), 0, ln);
        if (cdiv(ln.n / 4, kThreads) >= kLnBigColgroups) {
            ln.slabconst = reinterpret_cast<float2*>(ws + pl.ws_rowstat_b + 2 * r.rows2);
            STGCN_LAUNCH("ln_slab_consts", st, ln_slab_consts_kernel, dim3((unsigned)r.slabs2), dim3(kThreads), 64, ln);
        }
        return STGCN_OK;
    }
    // LayerNorm + dropout + gate backward on its own: dZ2 and the LayerNorm-parameter partials (BWD_STAGED; the stage tests' dZ2 beside BWD_FUSED)
    int launch_ln_gate_bwd() {
        const BwdGeom& bg = r.bg;
        STGCN_LAUNCH("ln_gate_bwd", st, (ln_gate_bwd_kernel<float>), dim3(cdiv(ln.n / 4, kThreads), bg.ln_sg), dim3(kThreads),
                     (8 + 2 * bg.ln_spg) * sizeof(float), ln);
        return STGCN_OK;
    }
    // LayerNorm + dropout + gate backward, weight gradient and transposed conv of tmp_conv2 in one time-stepping launch (BWD_FUSED)
    int launch_tc2_bwd() {
        if (g_debug_stages && !g_bf16) {   // stage tests: dZ2 (which the fused kernel keeps on chip) from the stage-per-launch kernel; it writes the same
                                           // per-window LayerNorm-parameter partials (ln_spg = T2, ln_sg = B), which the fused kernel then overwrites
            const int rc = launch_ln_gate_bwd();
            if (rc) return rc;
        }
        Tc2BwdArgs a = zeroed<Tc2BwdArgs>();
        a.y = hook_mask_from_y() ? y : nullptr;   // the dropout mask of this block's LayerNorm: read off its output (dropped = -0.0; both activation types) or regenerated (STGCN_HOOK_MASK=philox)
        a.dy = dy; a.U = ln.U; a.S = ln.S; a.Wp = ws + pl.ws_W2p; a.bias = ws + pl.ws_b2; a.gamma = ln.gamma; a.mean = ln.mean; a.rstd = ln.rstd;
        a.rowstat = ln.rowstat; a.slabconst = ln.slabconst; a.G = saved + pl.sv_G; a.Wd = ws + pl.ws_W2dense; a.dYg = ws + pl.ws_dYg;
        a.part = part() + r.bg.off_k1; a.dgam_part = ln.dgam_part; a.dbet_part = ln.dbet_part;
        a.B = d->B; a.T1 = r.T1; a.T2 = r.T2; a.N = d->N; a.act = d->act; a.training = ln.training; a.node_tiles = r.bg.node_tiles;
        a.keep_scale = ln.keep_scale; a.thresh = ln.thresh; a.seed = seed; a.offset = offset; a.offset_dev = offset_dev;
        const bool recomp = r.tc2_bwd_recompute;
        const int training = ln.training;
        const size_t lds = r.tc2_bwd_lds;
        const dim3 grid((unsigned)r.bg.k1_wgs), blk(512);   // 4 E waves + 4 M waves
#define STGCN_TC2_BWD(C2_, KT_)                                                                                        \
        do {                                                                                                               \
            if (training && d->act == STGCN_ACT_GLU) STGCN_LAUNCH_ETB("tc2_bwd", st, (tc2_bwd_kernel<C2_, KT_, true, 0, RC_, ET>), grid, blk, lds, a);   \
            else if (training) STGCN_LAUNCH_ETB("tc2_bwd", st, (tc2_bwd_kernel<C2_, KT_, true, 1, RC_, ET>), grid, blk, lds, a);      \
            else if (d->act == STGCN_ACT_GLU) STGCN_LAUNCH_ETB("tc2_bwd", st, (tc2_bwd_kernel<C2_, KT_, false, 0, RC_, ET>), grid, blk, lds, a);       \
            else STGCN_LAUNCH_ETB("tc2_bwd", st, (tc2_bwd_kernel<C2_, KT_, false, 1, RC_, ET>), grid, blk, lds, a);                 \
        } while (0)
#define STGCN_TC2_BWD_RC(C2_, KT_) do { if (recomp) { constexpr bool RC_ = true; STGCN_TC2_BWD(C2_, KT_); } else { constexpr bool RC_ = false; STGCN_TC2_BWD(C2_, KT_); } } while (0)
        // (c2 = 64 only: see tc2_bwd_fused_ok)
        if (d->Kt == 2) STGCN_TC2_BWD_RC(64, 2); else if (d->Kt == 3) STGCN_TC2_BWD_RC(64, 3); else STGCN_TC2_BWD_RC(64, 4);
#undef STGCN_TC2_BWD_RC
#undef STGCN_TC2_BWD
        return STGCN_OK;
    }
    // the same on the stage-per-launch kernels (BWD_STAGED): dZ2, then the weight gradient of tmp_conv2 and its transposed conv (+ relu mask) -> dYg
    int launch_staged_tc2_bwd() {
        STGCN_F32_ONLY("ln_gate_bwd + row-tile weight / data gradients of tmp_conv2");
        int rc = launch_ln_gate_bwd();
        if (rc) return rc;
        TconvBwdWeightArgs wa = zeroed<TconvBwdWeightArgs>();
        wa.ts = make_taps(saved + pl.sv_G, d->c1, d->Kt, d->N, r.T1, r.T2, 1, r.rows2);
        wa.dZ = ws + pl.ws_dZ2; wa.part = part() + r.bg.w2.off; wa.NC = r.NC2; wa.Mpad = r.bg.w2.Mpad; wa.rows_per_chunk = r.bg.w2.rows_per_chunk;
        wa.chunks = r.bg.w2.chunks;
        rc = launch_bwd_weight("tconv_bwd_weight.tc2", wa, r.bg.w2, st);
        if (rc) return rc;
        TconvBwdDataArgs a = zeroed<TconvBwdDataArgs>();
        a.ts = make_taps(ws + pl.ws_dZ2, r.NC2, d->Kt, d->N, r.T2, r.T1, -1, r.rows1);
        a.Wp = ws + pl.ws_W2d; a.KCH = d->Kt * r.NC2 / 16; a.Cin = d->c1; a.Gmask = saved + pl.sv_G; a.dX = ws + pl.ws_dYg;
        return launch_bwd_data("tconv_bwd_data.tc2", a, r.CP1 / 16, st);
    }
    int launch_block_gconv_bwd() {
        GconvBwdArgs a = zeroed<GconvBwdArgs>();
        a.dY = ws + pl.ws_dYg; a.X0 = saved + pl.sv_A; a.Xk = saved + pl.sv_Xk; a.LTp = gso_t_pad; a.W = P->gc_w;
        a.dA = ws + pl.ws_dA; a.part = part() + r.bg.off_gc; a.N = d->N; a.NP = r.NP; a.Ks = r.terms;
        a.kipf = gc_is_kipf(d->graph_conv); a.slabs = r.slabs1;
        a.Gk = r.tiled_gc ? ws + pl.ws_Gk : nullptr; a.tiles_per_wg = r.bg.gc_tiles_per_wg; a.wgs = r.bg.gc_count;
        a.XT = r.tiled_gc && !r.sparse_gc && r.terms > 1 ? ws + pl.ws_XT : nullptr;
        return launch_gconv_bwd(a, r.tiled_gc, st, r.sparse_gc);
    }
    // Align + gate backward on its own: dZ1 and the Align partials (BWD_STAGED; the stage tests' dZ1 beside BWD_FUSED, whose dWa partials it
    // sends to their own, then unused, slot).  Gate inputs as stored by the forward, or recomputed from x (K <= 16)
    int launch_align_gate_bwd() {
        STGCN_F32_ONLY("align_gate_bwd");
        AlignBwdArgs a = zeroed<AlignBwdArgs>();
        a.dA = ws + pl.ws_dA; a.WaT = ws + pl.ws_WaT; a.dZ = ws + pl.ws_dZ1;
        if (r.recompute_tc1) {
            a.Wd = ws + pl.ws_W1dense; a.bias = ws + pl.ws_b1; a.KPd = r.KP1;
            a.ts = input_taps();
        } else {
            a.U = saved + pl.sv_U1; a.S = saved + pl.sv_S1;
        }
        a.part = part() + r.bg.off_al; a.rows = r.rows1; a.c0 = d->c0; a.c1 = d->c1; a.KCH = r.CP1 / 16; a.act = d->act;
        const size_t lds = (size_t)(64 * (d->c1 + 4) + 64 * (d->c0 + 4) + 16 * d->c1) * sizeof(float);
        if (d->c0 == 64) STGCN_LAUNCH("align_gate_bwd", st, (align_gate_bwd_kernel<1>), dim3(r.bg.al_wgs), dim3(kThreads), lds, a);
        else STGCN_LAUNCH("align_gate_bwd", st, (align_gate_bwd_kernel<2>), dim3(r.bg.al_wgs), dim3(kThreads), lds, a);
        return STGCN_OK;
    }
    // Align + gate backward, weight gradient, transposed conv of tmp_conv1 (+ a hooked LayerNorm's row partials) in one launch (BWD_FUSED)
    int launch_tc1_bwd() {
        if (g_debug_stages && !g_bf16) {
            const int rc = launch_align_gate_bwd();
            if (rc) return rc;
        }
        Tc1BwdArgs a = zeroed<Tc1BwdArgs>();
        a.dA = ws + pl.ws_dA; a.U = saved + pl.sv_U1; a.S = saved + pl.sv_S1; a.x = x; a.WaD = ws + pl.ws_WaDense; a.Wd = ws + pl.ws_W1dense;
        a.dx = dx; a.part = part() + r.bg.off_k3; a.B = d->B; a.T = d->T; a.T1 = r.T1; a.N = d->N; a.node_tiles = r.bg.node_tiles;
        const bool hooked = dx_hook && dx_hook->rowstat, epi = hooked && dx_hook->C == d->c_in && dx_hook->N == d->N;
        if (epi) a.rs = rowstat_out(dx_hook);
        const bool x6 = r.tc1_bwd_x6;
        const size_t lds = r.tc1_bwd_lds;
        const dim3 grid((unsigned)r.bg.k3_wgs), blk(768);
#define STGCN_TC1_BWD(CIN_)                                                                                    \
        do {                                                                                                       \
            if (x6 && d->act == STGCN_ACT_GLU) STGCN_LAUNCH("tc1_bwd", st, (tc1_bwd_x6_kernel<64, CIN_, 3, 0>), grid, blk, lds, a);   \
            else if (x6) STGCN_LAUNCH("tc1_bwd", st, (tc1_bwd_x6_kernel<64, CIN_, 3, 1>), grid, blk, lds, a);             \
            else if (d->act == STGCN_ACT_GLU) STGCN_LAUNCH_ETB("tc1_bwd", st, (tc1_bwd_kernel<64, CIN_, 3, 0, ET>), grid, blk, lds, a);   \
            else STGCN_LAUNCH_ETB("tc1_bwd", st, (tc1_bwd_kernel<64, CIN_, 3, 1, ET>), grid, blk, lds, a);             \
        } while (0)
        if (d->c_in == 64) STGCN_TC1_BWD(64); else if (d->c_in == 32) STGCN_TC1_BWD(32); else STGCN_TC1_BWD(16);
#undef STGCN_TC1_BWD
        if (hooked && !epi) return launch_hook_rowstats(dx_hook, dx, (long)d->B * d->T, st);   // a hook of a shape the epilogue does not cover
        return STGCN_OK;
    }
    // thin first layer (BWD_THIN): recompute + gate backward + weight gradient in one kernel, dZ1 only if dx is needed
    int launch_thin_bwd() {
        ThinBwdArgs a = zeroed<ThinBwdArgs>();
        a.dA = ws + pl.ws_dA; a.Wd = ws + pl.ws_W1dense; a.bias = ws + pl.ws_b1; a.WaT = ws + pl.ws_WaT;
        a.dZ = d->need_dx ? ws + pl.ws_dZ1 : nullptr; a.part = part() + r.bg.off_al; a.rows = r.rows1; a.c0 = d->c0; a.act = d->act;
        a.ts = input_taps();
        const dim3 grid(r.bg.al_wgs), blk(kThreads);
        if (!r.thin_bwd_waves) {   // the row-tile form (STGCN_THIN=0)
            const size_t lds = (size_t)(64 * 20 + 64 * (d->c0 + 4) + 64 * (2 * d->c0 + 4) + 64 * 20 + 256) * sizeof(float);
            STGCN_LAUNCH_ETB("align_gate_bwd", st, (thin_tc1_bwd_kernel<ET>), grid, blk, lds, a);
        } else if (d->act == STGCN_ACT_GLU) STGCN_LAUNCH_ETB("align_gate_bwd", st, (thin_tc1_bwd2_kernel<ET, 0>), grid, blk, thin_bwd2_lds_bytes(), a);
        else STGCN_LAUNCH_ETB("align_gate_bwd", st, (thin_tc1_bwd2_kernel<ET, 1>), grid, blk, thin_bwd2_lds_bytes(), a);
        return STGCN_OK;
    }
    // weight gradient of tmp_conv1 from dZ1 (BWD_STAGED; the thin kernel accumulates its own)
    int launch_tc1_bwd_weight() {
        TconvBwdWeightArgs wa = zeroed<TconvBwdWeightArgs>();
        wa.ts = input_taps();
        wa.dZ = ws + pl.ws_dZ1; wa.part = part() + r.bg.w1.off; wa.NC = r.NC1; wa.Mpad = r.bg.w1.Mpad; wa.rows_per_chunk = r.bg.w1.rows_per_chunk;
        wa.chunks = r.bg.w1.chunks;
        return launch_bwd_weight("tconv_bwd_weight.tc1", wa, r.bg.w1, st);
    }
    // transposed conv of tmp_conv1, dZ1 -> dx (BWD_THIN, BWD_STAGED); this kernel has no epilogue for a hooked LayerNorm
    int launch_tc1_bwd_data() {
        TconvBwdDataArgs a = zeroed<TconvBwdDataArgs>();
        a.ts = make_taps(ws + pl.ws_dZ1, r.NC1, d->Kt, d->N, r.T1, d->T, -1, r.rows0);
        a.Wp = ws + pl.ws_W1d; a.KCH = d->Kt * r.NC1 / 16; a.Cin = d->c_in; a.Gmask = nullptr; a.dX = dx;
        const int rc = launch_bwd_data("tconv_bwd_data.tc1", a, r.CP_in / 16, st);
        if (rc || !(dx_hook && dx_hook->rowstat)) return rc;
        return launch_hook_rowstats(dx_hook, dx, (long)d->B * d->T, st);
    }
};
}  // namespace

int stgcn_stblock_backward(const stgcn_stblock_desc* d, const stgcn_stblock_params* P, const float* x, const float* gso_t_pad,
                           const float* dy, const float* y, const float* saved, float* ws, const stgcn_stblock_grads* G, float* dx, uint64_t seed,
                           uint64_t offset, const uint64_t* offset_dev, void* stream) {
    return stgcn_stblock_backward_hook(d, P, x, gso_t_pad, dy, y, saved, ws, G, dx, seed, offset, offset_dev, nullptr, stream);
}

int stgcn_stblock_backward_hook(const stgcn_stblock_desc* d, const stgcn_stblock_params* P, const float* x, const float* gso_t_pad,
                                const float* dy, const float* y, const float* saved, float* ws, const stgcn_stblock_grads* G, float* dx, uint64_t seed,
                                uint64_t offset, const uint64_t* offset_dev, const stgcn_ln_hook* dx_hook, void* stream) {
    STGCN_FLUSH_PENDING_PACK();
    BlockBwdCall c{{d, P, {}, {}, x, const_cast<float*>(saved), ws, seed, offset, offset_dev, (hipStream_t)stream}, gso_t_pad, dy, y, dx, dx_hook, {}};
    int rc = route_and_plan(d, &c.r, &c.pl);
    if (rc) return rc;
    if (c.r.bf16 && !c.r.bf16_bwd_ok)   // up front: the launchers' STGCN_F32_ONLY would refuse the same shapes after earlier stages have run
        return fail(STGCN_ERR_UNSUPPORTED, "stgcn_stblock_backward: no bf16 backward for c_in=%d channels=(%d, %d, %d) Kt=%d T=%d need_dx=%d "
                    "(bf16 blocks need tc2_bwd_kernel, and tc1_bwd_kernel or the thin first layer without an input gradient)",
                    d->c_in, d->c0, d->c1, d->c2, d->Kt, d->T, d->need_dx);
    if (!P || !x || !gso_t_pad || !dy || !saved || !ws || !G) return fail(STGCN_ERR_INVALID, "stgcn_stblock_backward: NULL buffer");
    if (!d->dy_rowstats_ready && !y) return fail(STGCN_ERR_INVALID, "stgcn_stblock_backward: y (the forward's output) is required unless dy_rowstats_ready is set");
    if (d->need_dx && !dx) return fail(STGCN_ERR_INVALID, "stgcn_stblock_backward: need_dx set but dx is NULL");
    rc = check_dx_hook("stgcn_stblock_backward", dx_hook, d->N, d->c_in, d->need_dx, d->dtype);
    if (rc) return rc;
    if (c.r.sparse_gc) {   // the transposed operator must be a registered blob for this N: refused before the block's first launch
        CsrInfo ci;
        rc = csr_lookup("stgcn_stblock_backward", gso_t_pad, d->N, &ci);
        if (rc) return rc;
    }
    g_prof_tag = d->reserved;
    g_bf16 = c.r.bf16;

    rc = c.launch_ln_bwd_stats();
    if (rc) return rc;
    rc = c.r.tc2_bwd == BWD_FUSED ? c.launch_tc2_bwd() : c.launch_staged_tc2_bwd();
    if (rc) return rc;
    rc = c.launch_block_gconv_bwd();
    if (rc) return rc;
    if (c.r.tc1_bwd == BWD_FUSED) {
        rc = c.launch_tc1_bwd();
    } else {
        rc = c.r.tc1_bwd == BWD_THIN ? c.launch_thin_bwd() : c.launch_align_gate_bwd();
        if (!rc && c.r.tc1_bwd == BWD_STAGED) rc = c.launch_tc1_bwd_weight();
        if (!rc && d->need_dx) rc = c.launch_tc1_bwd_data();
    }
    if (rc) return rc;

    // ---- final reduction into the reference's parameter layouts (deferred to stgcn_grad_flush when asked) ------------
    if (d->defer_reduce) return STGCN_OK;
    ReduceList RL;
    reduce_jobs_block(RL, d, c.r, c.part(), G);
    return launch_reduce_list("reduce", RL, c.st);
}
