// Second-order MAML (included inside class Engine).
//
// Reference semantics: lightning/systems/base_adaptor.py:107 `first_order = not train` — training
// differentiates the query loss THROUGH the five inner SGD steps (learn2learn `create_graph=True`).
// Here, without autograd: with phi_k = phi_{k-1} - a * grad_phi L_s(phi_{k-1}, theta_e) the meta-gradient is
//     v_K = grad_phi L_q(phi_K, theta_e),  e = grad_theta_e L_q
//     for k = K..1:   (u_phi, u_e) = Hess L_s(phi_{k-1}, theta_e) . (v_k, 0)
//                     v_{k-1} = v_k - a u_phi ;  e -= a u_e
//     d/d theta_adapted = v_0 ,  d/d theta_e = e .
// Each Hessian-vector product is the tangent of one forward+backward pass of the support batch in the
// direction v_k (forward-over-reverse): forward_t() propagates tangents of every saved activation,
// backward_t() propagates the primal activation gradients together with their tangents and writes the
// tangent of every parameter gradient (= H v) into `hv`.  The fast weights of every inner step stay
// resident in HBM (fast_hist, K x tasks x 94 MB), v and e live in the per-task gradient buffer.

// ---- buffers ------------------------------------------------------------------------------------
std::vector<LayerBuf> tdecB;           // tangents of the decoder's saved activations
// an ADAPTED encoder (adapt.modules lists it, config/algorithm/dev.yaml:28-33) carries a forward tangent too: its blocks' tangents, the
// tangent of the embedding output and the tangent twins of the phoneme-space backward scratch
std::vector<LayerBuf> tencB;
TS t_emb, tgP1, tgPqkv, tgPh, tdSp, tgPm;
// frame-level pitch / energy (modules.py:139-148): tangents of the variance adaptor's second half on the frame rectangle
TS t_xr0, t_xr1, t_xr2, tgRx, tgFx, tgRf1, tgRf2, tdpred_r[2];
PredBuf tpitR, teneR;
PredBuf tdurB, tpitB, teneB;
std::vector<PostBuf> tpostB;           // c = t_conv, a = t_act, stats = [S1 | S0] of the forward tangent
TS t_spk, t_x0, t_x1, t_x2, t_dec_in, t_mel;
TS tgFm;
TS tgPf1, tgPf2, tgP0, tgF0, tgF1, tgFqkv, tgFh, tdSf, tgR0, tgR1, tgRm, tgRz, tgMelF, tdspk, tdpred[3];
float *hv = nullptr, *fast_hist = nullptr;
int so_steps_cap = 0;
bool so_ready = false;
// Deferred Hessian-vector weight gradients (under-filled launches only, like engine.h: LayerGrad for the first-order backward): the four
// hv(W) products of a decoder layer read the layer's gradient tangents (tdc, tgh, tda, tgqkv) and the primal gradients behind the two
// dropouts (dc, da); written into buffers of the LAYER'S own instead of the shared tangent scratch they no longer have to run before the
// next layer overwrites it — they go out as ONE multi-problem launch per layer on the side stream, beside the tangent dgrad chain.
struct TLayerGrad { TS tdc, tgh, tda, tgqkv, dc, da; };
std::vector<TLayerGrad> tdecG;
// ... and of the PostNet layers (round 5): the BatchNorm backward's primal / tangent outputs of layer i in buffers of the layer's own, so that
// its hv(W) product can leave the tangent launch for the side stream as well
struct TPostGrad { TS dc, tdc; };
std::vector<TPostGrad> tpostG;
char* arena_so_defer_post = nullptr;
char* arena_so_defer = nullptr;

void layout_so() {
    const int d = cfg.d_model, f = cfg.vp_filter;
    layout_layers(tdecB, cfg.dec_layers, capMf, score_ts(1));
    if (encoder_adapted()) {
        layout_layers(tencB, cfg.enc_layers, capMp, score_ts(0));
        t_emb = rows(capMp, d); tgP1 = rows(capMp, d); tgPqkv = rows(capMp, 3 * d); tgPh = rows(capMp, cfg.d_ff); tdSp = flat(score_ts(0));
        tgPm = rows(capMp, d);
    }
    if (any_frame_level()) {
        t_xr0 = rows(capMr, d); t_xr1 = rows(capMr, d); t_xr2 = rows(capMr, d); tgRx = rows(capMr, d); tgFx = rows(capMf, d);
        tgRf1 = rows(capMr, f); tgRf2 = rows(capMr, f); tdpred_r[0] = rows(capMr, 1); tdpred_r[1] = rows(capMr, 1);
        for (PredBuf* pb : {&tpitR, &teneR}) layout_pred(*pb, capMr);
    }
    for (PredBuf* pb : {&tdurB, &tpitB, &teneB}) layout_pred(*pb, capMp);
    tpostB.resize(cfg.postnet_layers);
    for (int i = 0; i < cfg.postnet_layers; ++i) {
        const int c = postP[i].cout;
        tpostB[i].c = rows(capMr, c); tpostB[i].a = rows(capMr, c); tpostB[i].stats = flat(2LL * c); tpostB[i].dgamma_tmp = flat(2LL * c);
    }
    t_spk = flat((long long)cap_B * d); t_x0 = rows(capMp, d); t_x1 = rows(capMp, d); t_x2 = rows(capMp, d);
    t_dec_in = rows(capMf, d); t_mel = rows(capMr, cfg.n_mel);
    tgFm = rows(capMf, d);
    tgPf1 = rows(capMp, f); tgPf2 = rows(capMp, f); tgP0 = rows(capMp, d);
    tgF0 = rows(capMf, d); tgF1 = rows(capMf, d); tgFqkv = rows(capMf, 3 * d); tgFh = rows(capMf, cfg.d_ff); tdSf = flat(score_ts(1));
    const int pc = std::max(cfg.postnet_dim, cfg.n_mel);
    tgR0 = rows(capMr, pc); tgR1 = rows(capMr, pc); tgRm = rows(capMr, cfg.n_mel); tgRz = rows(capMr, cfg.n_mel);
    tgMelF = rows(capMf, cfg.n_mel);
    tdspk = flat((long long)cap_B * d);
    for (int i = 0; i < 3; ++i) tdpred[i] = rows(capMp, 1);
}

// second arena (allocated on first use: first-order users do not pay for it)
char* arena_so = nullptr;
int enable_second_order(int max_steps) {
    if (so_ready && max_steps <= so_steps_cap) return 0;
    if (!so_ready) {
        char* save_arena = arena; size_t save_off = arena_off; bool save_dry = arena_dry;
        arena_dry = true; arena_off = 0; layout_so();
        const size_t bytes = arena_off + 256;
        DEV_CHECK(mem.alloc(arena_so, bytes));
        DEV_CHECK(hipMemset(arena_so, 0, bytes));
        arena = arena_so; arena_dry = false; arena_off = 0; layout_so();
        arena = save_arena; arena_off = save_off; arena_dry = save_dry;
        DEV_CHECK(mem.alloc(hv, (size_t)n_total * cap_tasks * sizeof(float)));
        DEV_CHECK(hipMemset(hv, 0, (size_t)n_total * cap_tasks * sizeof(float)));
        if (defer_tasks > 0 && cfg.dec_layers > 0) {   // per-layer tangent-gradient buffers of the deferred hv(W) products (see TLayerGrad)
            const int d = cfg.d_model;
            const long long per_row = 4LL * d + cfg.d_ff + 3LL * d;
            const size_t bytes = (size_t)defer_tasks * cfg.dec_layers * (size_t)(capMf + 2 * G) * per_row * sizeof(float) + 4096;
            if (mem.alloc_zeroed(arena_so_defer, bytes) == hipSuccess) {
                char* cur = arena_so_defer;
                auto rows_d = [&](int C) {
                    const long long ts = (long long)(capMf + 2 * G) * C;
                    float* p0 = (float*)cur;
                    cur += (size_t)ts * defer_tasks * sizeof(float);
                    return TS{p0 + (long long)G * C, ts};
                };
                tdecG.resize(cfg.dec_layers);
                for (TLayerGrad& t : tdecG) { t.tdc = rows_d(d); t.tgh = rows_d(cfg.d_ff); t.tda = rows_d(d); t.tgqkv = rows_d(3 * d); t.dc = rows_d(d); t.da = rows_d(d); }
            } else {   // (the device cannot hold them: the hv(W) products stay in the tangent launches)
                mem.give_back(arena_so_defer);
                tdecG.clear();
            }
        }
        if (defer_tasks > 0 && cfg.postnet_layers > 0) {
            const int pc = std::max(cfg.postnet_dim, cfg.n_mel);
            const size_t bytes = (size_t)defer_tasks * cfg.postnet_layers * 2 * (size_t)(capMr + 2 * G) * pc * sizeof(float) + 4096;
            if (mem.alloc_zeroed(arena_so_defer_post, bytes) == hipSuccess) {
                char* cur = arena_so_defer_post;
                auto rows_r = [&](int C) {
                    const long long ts = (long long)(capMr + 2 * G) * C;
                    float* p0 = (float*)cur;
                    cur += (size_t)ts * defer_tasks * sizeof(float);
                    return TS{p0 + (long long)G * C, ts};
                };
                tpostG.resize(cfg.postnet_layers);
                for (TPostGrad& t : tpostG) { t.dc = rows_r(pc); t.tdc = rows_r(pc); }
            } else {
                mem.give_back(arena_so_defer_post);
                tpostG.clear();
            }
        }
    }
    so_steps_cap = 0;   // (the history goes back to the heap before it is taken again: nothing to replay until the new one is there)
    DEV_CHECK(mem.alloc(fast_hist, (size_t)std::max<long long>(n_adapt, 4) * cap_tasks * max_steps * sizeof(float)));
    so_steps_cap = max_steps;
    so_ready = true;
    return 0;
}

// tangent of a parameter = the current direction v (kept in the per-task gradient buffer); non-adapted
// parameters have no tangent
TS Wt(long long off) const { return off >= adapt_start ? TS{grad + off, n_total} : TS{nullptr, 0}; }
TS Hv(long long off) const { return TS{hv + off, n_total}; }

// ---- paired launches --------------------------------------------------------------------------------
// Every tangent of a product is a pair of products into one output (t(XW) = tX W + X tW).  Default: one dual-source launch per pair
// (GemmArgs::A2, gemm.h) — round 3 measured it against a plain launch followed by an accumulating one: 492 -> 476 ms on the 8-task step.
// ty = conv(tx; W) + conv(x; tW) + tb, masks applied to the sum
void conv_fwd_t(const Pass& ps, Space s, TS x, TS tx, int cin, int k, long long w_off, long long b_off, int cout, TS ty,
                RowMask rowmask, TS relu_ref = TS{}) {
    ConvOp c = conv_op(tx, cin, k, W(ps, w_off), ty, cout, 0, rowmask);
    c.relu_ref = relu_ref;
    if (Wt(w_off).p) {   // one K-loop over both products (a non-adapted weight has no tangent, and neither has its bias)
        c.x2 = x; c.w2 = Wt(w_off);
        if (b_off >= 0) c.b = Wt(b_off);
    }
    conv_fwd(ps, s, c);
}
// One conv's second-order backward = five products.  The three that start an output (hv(W) = tdy^T x, the primal dgrad,
// tdx = tdy W) are independent, and so are the two that complete one (hv(W) += dy^T tx, tdx += dy tW): two multi-problem
// launches instead of five stand-alone ones.  dx == nullptr: no primal dgrad wanted.
void conv_bwd_t(const Pass& ps, Space s, TS dy, TS tdy, int cout, int k, TS x, TS tx, int cin, long long w_off, long long b_off,
                RowMask bias_mask, TS dx, int dx_flags, TS tdx, bool tdx_accumulate, RowMask rowmask,
                TS relu_ref = TS{}, bool defer_wgrad = false) {
    // each completed output in one dual-source K-loop: ONE multi-problem launch of three problems (defer_wgrad: the hv(W) product is
    // left to hv_wgrad_side, which the caller issues on the side stream once the layer's tangent gradients are all written)
    GemmBatchScope all(gx, stream);
    if (!defer_wgrad) conv_wgrad(ps, s, hv_wgrad_op(x, tx, cin, k, dy, tdy, cout, w_off, b_off, bias_mask));
    ConvOp c = conv_op(dx, cin, k, W(ps, w_off), dy, cout, dx_flags, rowmask);
    c.relu_ref = relu_ref;
    if (dx.p) conv_dgrad(ps, s, c);
    c.x = tdx; c.y = tdy; c.flags = tdx_accumulate ? GEMM_ACCUM : 0;
    if (Wt(w_off).p) { c.y2 = dy; c.w2 = Wt(w_off); }
    conv_dgrad(ps, s, c);
}
// hv(W) = tdy^T x + dy^T tx (one dual-source problem), hv(b) = colsum(tdy)
static ConvOp hv_wgrad_op(TS x, TS tx, int cin, int k, TS dy, TS tdy, int cout, long long w_off, long long b_off, RowMask bias_mask) {
    ConvOp c = wgrad_op(x, cin, k, tdy, cout, w_off, b_off, bias_mask);
    c.y2 = dy; c.x2 = tx;
    return c;
}
// din: dropout applied to ta on load (see ln_jvp_fwd_kernel)
void ln_fwd_t(const Pass& ps, Space s, TS ta, TS tres, TS z, TS st, long long g_off, long long b_off, RowMask mask,
              TS tz_out, TS ty, TS tst, int C, DropSpec din = DropSpec(), DropSpec dout = DropSpec()) {
    const Plan& p = *ps.pl;
    launch_ln_jvp_fwd(on_rows(p, s, stream, mask), ta, tres, z, st, W(ps, g_off), Wt(g_off), Wt(b_off), tz_out, ty, tst, C, din, dout);
}
// the dropout launches of the tangent FFT blocks (two in front of the forward's LayerNorm tangents, four behind the backward's) ride in the LayerNorm
// tangent kernels — the same masks on the same values: bit-identical.  MTTS_SO_FUSE_DROP=0: launches of their own again.
static bool so_fuse_drop() { return knobs().so_fuse_drop != 0; }
// primal dz + tangent tgz, and hv(gamma), hv(beta); dz_drop / tgz_drop (optional): dropout(dz) / dropout(tgz) with the forward site's mask dd
void ln_bwd_t(const Pass& ps, Space s, TS dy, TS tgy, TS z, TS st, TS tz, TS tst, long long g_off, long long b_off,
              RowMask mask, TS dz, TS tgz, int C, int relu_on_z, TS dz_drop = TS{nullptr, 0}, TS tgz_drop = TS{nullptr, 0},
              DropSpec dd = DropSpec(), DropSpec din = DropSpec()) {   // din: dropout applied to dy and tgy on load (both kernels)
    const Plan& p = *ps.pl;
    // stage 1 of hv(gamma) / hv(beta) rides in the tangent kernel (8-row partials, folded by one colfinal launch); MTTS_SO_LN_PART=0: the two-launch
    // reduction over the same arrays in front of it (ColArgs mode 5) — another summation order, equal to fp32 roundoff
    launch_ln_jvp_bwd(on_rows(p, s, stream, mask), dy, tgy, z, st, tz, tst, W(ps, g_off), Wt(g_off), dz, tgz, C, relu_on_z, dz_drop, tgz_drop, dd, din,
                      col_partial, knobs().so_ln_part != 0, col_max_chunks, Gd(g_off), Gd(b_off));
}

// ---- FFT block ----------------------------------------------------------------------------------------
void fft_fwd_t(const Pass& ps, Space s, int heads, const FFTP& P, LayerBuf& b, LayerBuf& t, TS xin, TS txin) {
    TagScope tag_scope(*this, s == SP_P ? 1 : 2);
    const Plan& p = *ps.pl;
    const AttnSide& at = p.at[side_of(s)];
    const int d = cfg.d_model, dk = d / heads;
    const RowMask vm = p.sp[s].valid, im = p.sp[s].inrect, all;
    const float alpha = 1.f / sqrtf((float)dk);
    conv_fwd_t(ps, s, xin, txin, d, 1, P.wqkv, P.bqkv, 3 * d, t.qkv, all);
    attn_gemm(ps, s, TAB_QK, GEMM_NT, t.qkv.p, 3 * d, b.qkv.p, 3 * d, t.P.p, 0, alpha, heads, 0, b.qkv.p, t.qkv.p);
    if (at.groups > 0 && at.maxL > 0)
        launch_softmax_jvp_fwd(at.seqs, at.maxL, at.groups, b.P.p, t.P.p, stream);
    attn_gemm(ps, s, TAB_PV, GEMM_NN, t.P.p, 0, b.qkv.p, 3 * d, t.O.p, d, 1.f, heads, 0, b.P.p, t.qkv.p);
    conv_fwd_t(ps, s, b.O, t.O, d, 1, P.wfc, P.bfc, d, t.z1, all);
    const bool fuse = so_fuse_drop();
    if (!fuse) drop(ps, s, t.z1, t.z1, d, block_dropout(s), site_base);
    ln_fwd_t(ps, s, t.z1, txin, b.z1, b.st1, P.ln1g, P.ln1b, vm, t.z1, t.y1, t.st1, d, fuse ? drop_spec(ps, block_dropout(s), site_base) : DropSpec());
    conv_fwd_t(ps, s, b.y1, t.y1, d, cfg.k1, P.w1, P.b1, cfg.d_ff, t.h, im, b.h);
    conv_fwd_t(ps, s, b.h, t.h, cfg.d_ff, cfg.k2, P.w2, P.b2, d, t.z2, all);
    if (!fuse) drop(ps, s, t.z2, t.z2, d, block_dropout(s), site_base + 1);
    ln_fwd_t(ps, s, t.z2, t.y1, b.z2, b.st2, P.ln2g, P.ln2b, vm, t.z2, t.y2, t.st2, d, fuse ? drop_spec(ps, block_dropout(s), site_base + 1) : DropSpec());
}

// g0_in / tg0: dL/dy2 and its tangent on entry; K.g0 / tg0: dL/dx and its tangent on exit (K: engine.h LayerKeep).
// skip_primal: K holds the primal gradients of this layer from the first sweep's backward (a gradient set of the step's own) — the primal
// input-gradient GEMMs are not repeated; only dP = dO V^T (an L x L x d_k product per head, whose softmax backward rides in the tangent
// kernel) and the row-local LayerNorm backwards are (into the shared scratch sh_g0 / sh_g1).
// tl != null (kept primal gradients + an under-filled plan): deferred hv(W) products, see TLayerGrad
void fft_bwd_t(const Pass& ps, Space s, int heads, const FFTP& P, LayerBuf& b, LayerBuf& t, TS xin, TS txin, TS g0_in, TS tg0,
               const LayerKeep& K, bool skip_primal, TS sh_g0, TS sh_g1, TS tg1, TS tgqkv, TS tgh, TS dS, TS tdS, TLayerGrad* tl = nullptr) {
    TagScope tag_scope(*this, s == SP_P ? 1 : 2);
    const Plan& p = *ps.pl;
    const AttnSide& at = p.at[side_of(s)];
    const int d = cfg.d_model, dk = d / heads, ff = cfg.d_ff;
    const RowMask vm = p.sp[s].valid, im = p.sp[s].inrect, all;
    TS none{nullptr, 0};
    const bool sk = skip_primal;
    const bool df = tl != nullptr && sk;
    TS dz2 = sk ? sh_g1 : K.dy1, dz1 = sk ? sh_g0 : K.g0;
    TS gh = K.gh, gqkv = K.gqkv;
    if (df) { tgh = tl->tgh; tgqkv = tl->tgqkv; }
    TS gm = (s == SP_P) ? gPm : gFm, tgm = (s == SP_P) ? tgPm : tgFm;   // dropout-masked copies (P space: only with an adapted encoder)
    // (the masked copies ride in the LayerNorm tangent kernel when there is a mask to apply: so_fuse_drop)
    const DropSpec dd2 = drop_spec(ps, block_dropout(s), site_base + 1), dd1 = drop_spec(ps, block_dropout(s), site_base);
    const bool fuse2 = so_fuse_drop() && dd2.thr16 != 0 && gm.p != nullptr && tgm.p != nullptr, fuse1 = so_fuse_drop() && dd1.thr16 != 0 && gm.p != nullptr && tgm.p != nullptr;
    ln_bwd_t(ps, s, g0_in, tg0, b.z2, b.st2, t.z2, t.st2, P.ln2g, P.ln2b, vm, dz2, tg1, d, 0, fuse2 ? (df ? tl->dc : gm) : none, fuse2 ? (df ? tl->tdc : tgm) : none, dd2);
    // (deferred: the masked copies — plain copies when dropout is off — go to the layer's own buffers, which outlive the shared scratch)
    auto masked = [&](TS src, TS shared, TS own, int site) {
        if (!df) return drop(ps, s, src, shared, d, block_dropout(s), site);
        if (drop_active(ps) && block_dropout(s) > 0.f) return drop(ps, s, src, own, d, block_dropout(s), site);
        launch_copy_tasks(src, own, (long long)p.sp[s].maxM * d / 4, p.tasks, stream);
        return own;
    };
    TS dc = fuse2 ? (df ? tl->dc : gm) : masked(dz2, gm, df ? tl->dc : gm, site_base + 1), tdc = fuse2 ? (df ? tl->tdc : tgm) : masked(tg1, tgm, df ? tl->tdc : tgm, site_base + 1);
    conv_bwd_t(ps, s, dc, tdc, d, cfg.k2, b.h, t.h, ff, P.w2, P.b2, vm, sk ? none : gh, 0, tgh, false, im, b.h, df);
    conv_bwd_t(ps, s, gh, tgh, ff, cfg.k1, b.y1, t.y1, d, P.w1, P.b1, im, sk ? none : K.dy1, GEMM_ACCUM, tg1, true, im, none, df);   // K.dy1: dz2 + dgrad = dy1
    ln_bwd_t(ps, s, K.dy1, tg1, b.z1, b.st1, t.z1, t.st1, P.ln1g, P.ln1b, vm, dz1, tg0, d, 0, fuse1 ? (df ? tl->da : gm) : none, fuse1 ? (df ? tl->tda : tgm) : none, dd1);
    TS da = fuse1 ? (df ? tl->da : gm) : masked(dz1, gm, df ? tl->da : gm, site_base), tda = fuse1 ? (df ? tl->tda : tgm) : masked(tg0, tgm, df ? tl->tda : tgm, site_base);
    conv_bwd_t(ps, s, da, tda, d, 1, b.O, t.O, d, P.wfc, P.bfc, vm, sk ? none : K.dO, 0, tg1, false, all, none, df);   // K.dO = dO, tg1 = its tangent
    TS g1 = K.dO;
    // dP = dO V^T ; tg_P = tg_O V^T + dO tV^T
    // dV = P^T dO ; tg_V = tP^T dO + P^T tg_O
    {
        GemmBatchScope all(gx, stream);
        attn_gemm(ps, s, TAB_DP, GEMM_NT, g1.p, d, b.qkv.p, 3 * d, dS.p, 0, 1.f, heads);
        attn_gemm(ps, s, TAB_DP, GEMM_NT, tg1.p, d, b.qkv.p, 3 * d, tdS.p, 0, 1.f, heads, 0, g1.p, t.qkv.p);
        if (!sk) attn_gemm(ps, s, TAB_DV, GEMM_TN, b.P.p, 0, g1.p, d, gqkv.p, 3 * d, 1.f, heads);
        attn_gemm(ps, s, TAB_DV, GEMM_TN, t.P.p, 0, g1.p, d, tgqkv.p, 3 * d, 1.f, heads, 0, b.P.p, tg1.p);
    }
    if (at.groups > 0 && at.maxL > 0)
        launch_softmax_jvp_bwd(at.seqs, at.maxL, at.groups, b.P.p, t.P.p, dS.p, tdS.p, 1.f / sqrtf((float)dk), stream);
    // dQ = dS K ; tg_Q = tg_S K + dS tK
    // dK = dS^T Q ; tg_K = tg_S^T Q + dS^T tQ
    {
        GemmBatchScope all(gx, stream);
        if (!sk) attn_gemm(ps, s, TAB_DQ, GEMM_NN, dS.p, 0, b.qkv.p, 3 * d, gqkv.p, 3 * d, 1.f, heads);
        attn_gemm(ps, s, TAB_DQ, GEMM_NN, tdS.p, 0, b.qkv.p, 3 * d, tgqkv.p, 3 * d, 1.f, heads, 0, dS.p, t.qkv.p);
        if (!sk) attn_gemm(ps, s, TAB_DK, GEMM_TN, dS.p, 0, b.qkv.p, 3 * d, gqkv.p, 3 * d, 1.f, heads);
        attn_gemm(ps, s, TAB_DK, GEMM_TN, tdS.p, 0, b.qkv.p, 3 * d, tgqkv.p, 3 * d, 1.f, heads, 0, dS.p, t.qkv.p);
    }
    conv_bwd_t(ps, s, gqkv, tgqkv, 3 * d, 1, xin, txin, d, P.wqkv, P.bqkv, vm, sk ? none : K.g0, GEMM_ACCUM, tg0, true, all, none, df);   // K.g0: dz1 + dgrad = dL/dx
    if (df) {
        // the layer's four hv(W) (+ bias) products, each one dual-source K-loop (hv(W) = tdy^T x + dy^T tx): one multi-problem launch on
        // the side stream, after everything above
        fork_side();
        GemmBatchScope batch(gx_side, side);
        conv_wgrad(ps, s, on_side(hv_wgrad_op(b.y1, t.y1, d, cfg.k1, gh, tgh, ff, P.w1, P.b1, im)));
        conv_wgrad(ps, s, on_side(hv_wgrad_op(b.h, t.h, ff, cfg.k2, dc, tdc, d, P.w2, P.b2, vm)));
        conv_wgrad(ps, s, on_side(hv_wgrad_op(xin, txin, d, 1, gqkv, tgqkv, 3 * d, P.wqkv, P.bqkv, vm)));
        conv_wgrad(ps, s, on_side(hv_wgrad_op(b.O, t.O, d, 1, da, tda, d, P.wfc, P.bfc, vm)));
        defer_live = true;
    }
}

// ---- variance predictor -------------------------------------------------------------------------------
// (s = SP_R: a frame-level predictor on the frame rectangle)
void pred_fwd_t(const Pass& ps, const PredP& P, PredBuf& b, PredBuf& t, TS xin, TS txin, Space s = SP_P) {
    TagScope tag_scope(*this, 4);
    const Plan& p = *ps.pl;
    const int d = cfg.d_model, f = cfg.vp_filter, k = cfg.vp_kernel;
    const RowMask im = p.sp[s].inrect;
    TS none{nullptr, 0};
    conv_fwd_t(ps, s, xin, txin, d, k, P.c1w, P.c1b, f, t.r1, im, b.r1);
    const bool fuse = so_fuse_drop();   // (the dropout behind each LayerNorm rides in its tangent kernel: ln_jvp_fwd_kernel: dout)
    ln_fwd_t(ps, s, t.r1, none, b.r1, b.st1, P.l1g, P.l1b, im, none, t.n1, t.st1, f, DropSpec(), fuse ? drop_spec(ps, cfg.vp_dropout, site_base) : DropSpec());
    if (!fuse) drop(ps, s, t.n1, t.n1, f, cfg.vp_dropout, site_base);
    conv_fwd_t(ps, s, b.n1, t.n1, f, k, P.c2w, P.c2b, f, t.r2, im, b.r2);
    ln_fwd_t(ps, s, t.r2, none, b.r2, b.st2, P.l2g, P.l2b, im, none, t.n2, t.st2, f, DropSpec(), fuse ? drop_spec(ps, cfg.vp_dropout, site_base + 1) : DropSpec());
    if (!fuse) drop(ps, s, t.n2, t.n2, f, cfg.vp_dropout, site_base + 1);
    TS w = W(ps, P.lw), tw = Wt(P.lw), tbb = Wt(P.lb);
    launch_rowdot_jvp(on_rows(p, s, stream, p.sp[s].valid), b.n2, t.n2, w, tw, tbb, t.out, f);
}
// dout / tgout: gradient of the prediction and its tangent; tdx accumulates the tangent of the input gradient, dx (optional: only an
// adapted encoder upstream needs it) the primal input gradient
void pred_bwd_t(const Pass& ps, const PredP& P, PredBuf& b, PredBuf& t, TS xin, TS txin, TS dout, TS tgout, TS tdx,
                TS dx = TS{nullptr, 0}, Space s = SP_P) {
    TagScope tag_scope(*this, 4);
    const Plan& p = *ps.pl;
    const int d = cfg.d_model, f = cfg.vp_filter, k = cfg.vp_kernel;
    const RowMask im = p.sp[s].inrect;
    TS none{nullptr, 0};
    TS g1 = (s == SP_P) ? gPf1 : gRf1, g2 = (s == SP_P) ? gPf2 : gRf2;
    TS tg1 = (s == SP_P) ? tgPf1 : tgRf1, tg2 = (s == SP_P) ? tgPf2 : tgRf2;
    // hv of the 256 -> 1 projection (three reductions over arrays nothing in this pass writes again — the activations n2 / t_n2 and the loss's gradients
    // dout / tgout): on the side stream when there is one (six launches per predictor and reverse step leave the critical stream; joined with the
    // pass's other side-stream work).  MTTS_SO_PRED_SIDE=0: on the critical stream.
    const bool os = knobs().so_pred_side && side != nullptr && col_partial_side != nullptr;
    if (os) fork_side();
    colsum(ps, s, tgout, 1, RowMask(), none, Gd(P.lb), os);
    colsum(ps, s, b.n2, f, RowMask(), tgout, Gd(P.lw), os);
    {   // + sum_m dout[m] * t_n2[m]
        ColArgs a;
        a.X = t.n2.p; a.x_ts = t.n2.ts; a.roww = dout.p; a.roww_ts = dout.ts; a.C = f; a.mode = 0; a.mfield = p.sp[s].mfield; a.accumulate = 1;
        TS o = Gd(P.lw);
        colreduce(p, a, o.p, nullptr, o.ts, s, os);
    }
    TS w = W(ps, P.lw), tw = Wt(P.lw);
    launch_rowdot_jvp_bwd(on_rows(p, s, stream), dout, tgout, w, tw, g1, tg1, f);
    // the dropout behind each LayerNorm masks both incoming gradients: on load in the two kernels of ln_bwd_t (so_fuse_drop), or by launches of their own
    const bool fuse = so_fuse_drop();
    if (!fuse) { drop(ps, s, g1, g1, f, cfg.vp_dropout, site_base + 1); drop(ps, s, tg1, tg1, f, cfg.vp_dropout, site_base + 1); }
    ln_bwd_t(ps, s, g1, tg1, b.r2, b.st2, t.r2, t.st2, P.l2g, P.l2b, im, g2, tg2, f, 1, none, none, DropSpec(), fuse ? drop_spec(ps, cfg.vp_dropout, site_base + 1) : DropSpec());
    conv_bwd_t(ps, s, g2, tg2, f, k, b.n1, t.n1, f, P.c2w, P.c2b, im, g1, 0, tg1, false, im);
    if (!fuse) { drop(ps, s, g1, g1, f, cfg.vp_dropout, site_base); drop(ps, s, tg1, tg1, f, cfg.vp_dropout, site_base); }
    ln_bwd_t(ps, s, g1, tg1, b.r1, b.st1, t.r1, t.st1, P.l1g, P.l1b, im, g2, tg2, f, 1, none, none, DropSpec(), fuse ? drop_spec(ps, cfg.vp_dropout, site_base) : DropSpec());
    conv_bwd_t(ps, s, g2, tg2, f, k, xin, txin, d, P.c1w, P.c1b, im, dx, GEMM_ACCUM, tdx, true, im);
}

// ---- tangent forward of the adapted part (the primal forward of the same batch has just run) ------------
int forward_t(const Pass& ps) {
    const Plan& p = *ps.pl;
    const RowSpace &sP = p.sp[SP_P], &sF = p.sp[SP_F], &sR = p.sp[SP_R];
    set_regime(p);
    const int d = cfg.d_model, nt = p.tasks;
    TS ttab = Wt(spk_table);
    if (ttab.p && !p.ext_spk) {   // external speaker embeddings (speaker_emb: dvec) are inputs of the batch: no tangent
        launch_speaker_vec(on_rows(p, SP_P, stream), p.maxB, ttab, p.spk_ids, (long long)cap_B + 1, cap_B, p.average_spk, t_spk, d);
    } else {
        DEV_CHECK(hipMemsetAsync(t_spk.p, 0, (size_t)t_spk.ts * nt * sizeof(float), stream));
    }
    if (encoder_adapted()) {
        // tangent of the embedding output: the token rows of the word table's tangent (the position table is frozen; invalid rows carry
        // token 0 = the padding row, whose tangent is 0 as its gradient is), then the encoder blocks, then + the speaker vector's tangent
        TS twe = Wt(word_emb);
        launch_embed_add_idx(on_rows(p, SP_P, stream), TS{nullptr, 0}, twe, p.p_tok, t_emb, d);
        TS xe = emb_out, txe = t_emb;
        for (int l = 0; l < cfg.enc_layers; ++l) {
            site_base = 2 * l;
            fft_fwd_t(ps, SP_P, cfg.enc_heads, encP[l], encB[l], tencB[l], xe, txe);
            xe = encB[l].y2; txe = tencB[l].y2;
        }
        launch_add_rowvec(on_rows(p, SP_P, stream, sP.inrect), txe, t_spk, p.p_row_b, t_x0, d);
    } else
    launch_bcast_rowvec(on_rows(p, SP_P, stream, sP.inrect), t_spk, p.p_row_b, t_x0, d);
    // variance adaptor (teacher-forced: the embeddings are looked up at the TARGET buckets, so only the table tangents flow through them);
    // a phoneme-level feature sits on the phoneme rectangle before the length regulator, a frame-level one on the frame rectangle after it
    // (engine.h: forward)
    TS tpe = Wt(pitch_emb), tee = Wt(energy_emb);
    TS xp = x0, txp = t_x0;
    site_base = 128; pred_fwd_t(ps, durP, durB, tdurB, x0, t_x0);
    if (!cfg.pitch_frame) {
        site_base = 132; pred_fwd_t(ps, pitP, pitB, tpitB, xp, txp);
        launch_embed_add_idx(on_rows(p, SP_P, stream), txp, tpe, pidx, t_x1, d);
        xp = x1; txp = t_x1;
    }
    if (!cfg.energy_frame) {
        site_base = 136; pred_fwd_t(ps, eneP, eneB, teneB, xp, txp);
        launch_embed_add_idx(on_rows(p, SP_P, stream), txp, tee, eidx, t_x2, d);
        xp = x2; txp = t_x2;
    }
    if (!any_frame_level()) {
        launch_length_regulate_fwd(on_rows(p, SP_F, stream), txp, p.f_src, p.f_row_b, p.f_row_t, t_spk, nullptr, t_dec_in, d);
    } else {
        launch_length_regulate_rect(on_rows(p, SP_R, stream), txp, p.f_src, sF.ts, p.r2f, t_xr0, d);
        TS xr = xr0, txr = t_xr0;
        if (cfg.pitch_frame) {
            site_base = 132; pred_fwd_t(ps, pitP, pitR, tpitR, xr, txr, SP_R);
            launch_embed_add_idx(on_rows(p, SP_R, stream), txr, tpe, pidx_r, t_xr1, d);
            xr = xr1; txr = t_xr1;
        }
        if (cfg.energy_frame) {
            site_base = 136; pred_fwd_t(ps, eneP, eneR, teneR, xr, txr, SP_R);
            launch_embed_add_idx(on_rows(p, SP_R, stream), txr, tee, eidx_r, t_xr2, d);
            xr = xr2; txr = t_xr2;
        }
        launch_length_regulate_fwd(on_rows(p, SP_F, stream), txr, p.f2r, p.f_row_b, p.f_row_t, t_spk, nullptr, t_dec_in, d);
    }
    TS x = dec_in, tx = t_dec_in;
    for (int l = 0; l < cfg.dec_layers; ++l) {
        site_base = 64 + 2 * l;
        fft_fwd_t(ps, SP_F, cfg.dec_heads, decP[l], decB[l], tdecB[l], x, tx);
        x = decB[l].y2; tx = tdecB[l].y2;
    }
    {   // t_mel = t_dec W^T + dec tW^T + tb on valid frames, tb on padded frames, 0 on guards
        TS w = W(ps, mel_w), tw = Wt(mel_w), tb = Wt(mel_b);
        const bool dual = tw.p != nullptr;
        GemmArgs g = rowgemm(p, SP_F, GEMM_NT);
        g.A = tx.p; g.a_gs = tx.ts; g.lda = d;
        g.B = w.p; g.b_gs = w.ts; g.ldb = d;
        if (dual) { g.A2 = x.p; g.a2_gs = x.ts; g.B2 = tw.p; g.b2_gs = tw.ts; }
        g.C = t_mel.p; g.c_gs = t_mel.ts; g.ldc = cfg.n_mel; g.N = cfg.n_mel; g.K = d;
        if (tb.p) { g.bias = tb.p; g.bias_gs = tb.ts; }
        g.c_rowmap = p.f2r; g.c_rowmap_gs = sF.ts;
        gemm_launch(gx, GEMM_NT, g, sF.maxM, cfg.n_mel, nt, stream, 0, (dual ? 2.0 : 1.0) * 2.0 * sF.alg_rows * cfg.n_mel * d, sF.sumM,
                    4.0 * (sF.alg_rows * ((dual ? 2 : 1) * d + cfg.n_mel) + (dual ? 2.0 : 1.0) * nt * cfg.n_mel * d));
        if (tb.p) {
            launch_fill_padded_rows(on_rows(p, SP_R, stream, sR.inrect), t_mel, tb, sR.valid.m, cfg.n_mel);
        } else {  // zero bias tangent: padded + guard rows are 0 — valid rows were just written
            launch_fill_padded_rows(on_rows(p, SP_R, stream, sR.inrect), t_mel, TS{(float*)tgRz.p, 0}, sR.valid.m, cfg.n_mel);
        }
    }
    TS cur = mel, tcur = t_mel;
    TagScope postnet_tag(*this, 3);
    for (int i = 0; i < cfg.postnet_layers; ++i) {
        const PostP& P = postP[i];
        PostBuf& b = postB[i];
        PostBuf& t = tpostB[i];
        conv_fwd_t(ps, SP_R, cur, tcur, P.cin, cfg.postnet_kernel, P.w, P.b, P.cout, t.c, sR.inrect);
        ColArgs ca = col_args(p, SP_R, sR.inrect, P.cout, 3);  // S1 = sum tc*xhat, S0 = sum tc
        ca.X = t.c.p; ca.x_ts = t.c.ts; ca.Z = b.c.p; ca.z_ts = b.c.ts; ca.stats = b.stats.p; ca.st_ts = b.stats.ts; ca.do_tanh = 0;
        colreduce(p, ca, t.stats.p, t.stats.p + P.cout, t.stats.ts, SP_R);
        TS gm = W(ps, P.g), tgm = Wt(P.g), tbt = Wt(P.beta);
        launch_bn_jvp_apply(on_rows(p, SP_R, stream, sR.inrect), b.c, t.c, b.stats, t.stats, gm, tgm, tbt, b.a, (int)(i < cfg.postnet_layers - 1), t.a, P.cout,
                            drop_active(ps) ? 1.f - cfg.postnet_dropout : 1.f, so_fuse_drop() ? drop_spec(ps, cfg.postnet_dropout, 192 + i) : DropSpec());
        if (!so_fuse_drop()) drop(ps, SP_R, t.a, t.a, P.cout, cfg.postnet_dropout, 192 + i);
        cur = b.a; tcur = t.a;
    }
    return 0;
}

// ---- combined backward: primal activation gradients + tangents; tangent parameter gradients -> Gd() (= hv) ----
// skip_primal: the bound gradient set (engine.h: GK()) holds the primal gradients of this very pass from an earlier backward() — the
// decoder's, the PostNet's and mel_linear's primal input-gradient GEMMs are not repeated (meta_grad_so's reverse sweep).
int backward_t(const Pass& ps, float scale, bool skip_primal = false) {
    const Plan& p = *ps.pl;
    const RowSpace &sP = p.sp[SP_P], &sR = p.sp[SP_R];
    set_regime(p);
    const int d = cfg.d_model, nt = p.tasks, nm = cfg.n_mel;
    TS none{nullptr, 0};
    GradSet& K = GK();
    const bool sk = skip_primal && gs_bound >= 0;
    const TS gRm = K.gRm;                              // final mel gradient (kept, or built below)
    const TS gRm_direct = sk ? this->gRm : K.gRm;      // where the loss kernel puts the direct L1 term (scratch when the final one is kept)
    LossArgs a = loss_args(p);
    launch_loss_grad(p.meta, nt, a, scale, gRm_direct.p, gRp.p, dpred[1].p, dpred[2].p, dpred[0].p, dpred_r[0].p, dpred_r[1].p, stream);
    MTTS_LAUNCH(loss_tangent_kernel, dim3(4, 1, nt), dim3(256), stream, (const int*)p.meta, (const float*)tpitB.out.p,
                (const float*)teneB.out.p, (const float*)tdurB.out.p, tpitB.out.ts, (const unsigned char*)sP.valid.m, sP.ts, scale,
                tdpred[1].p, tdpred[2].p, tdpred[0].p, cfg.pitch_frame, cfg.energy_frame);
    if (any_frame_level())   // MSE over the valid FRAMES (loss.py:54-63): tangent of its gradient = 2 scale / n_frames * tangent of the prediction
        MTTS_LAUNCH(loss_tangent_r_kernel, dim3(16, 1, nt), dim3(256), stream, (const int*)p.meta, (const float*)tpitR.out.p,
                    (const float*)teneR.out.p, tpitR.out.ts, (const unsigned char*)sR.valid.m, sR.ts, scale, tdpred_r[0].p, tdpred_r[1].p,
                    cfg.pitch_frame, cfg.energy_frame);
    // PostNet.  The L1 terms have no second derivative: the gradient tangents of mel_post / mel start at zero (tgRz).
    TS cur = gRp, tcur = tgRz;
    set_tag(3);
    for (int i = cfg.postnet_layers - 1; i >= 0; --i) {
        const PostP& P = postP[i];
        PostBuf& b = postB[i];
        PostBuf& t = tpostB[i];
        const int act = (i < cfg.postnet_layers - 1);
        const float ysc = drop_active(ps) ? 1.f - cfg.postnet_dropout : 1.f;
        // the backward of the layer's dropout masks both incoming gradients: on load in the three kernels that read them (so_fuse_drop), or by two launches
        const DropSpec pdrop = so_fuse_drop() ? drop_spec(ps, cfg.postnet_dropout, 192 + i) : DropSpec();
        if (!so_fuse_drop()) {
            cur = drop(ps, SP_R, cur, gR1, P.cout, cfg.postnet_dropout, 192 + i);
            tcur = drop(ps, SP_R, tcur, tgR1, P.cout, cfg.postnet_dropout, 192 + i);
        }
        ColArgs ca = col_args(p, SP_R, sR.inrect, P.cout, 3);  // primal sums (dgamma, dbeta) -> scratch
        ca.yscale = ysc; ca.xdrop = pdrop;
        ca.X = cur.p; ca.x_ts = cur.ts; ca.Y = b.a.p; ca.y_ts = b.a.ts; ca.Z = b.c.p; ca.z_ts = b.c.ts;
        ca.stats = b.stats.p; ca.st_ts = b.stats.ts; ca.do_tanh = act;
        colreduce(p, ca, b.dgamma_tmp.p, b.dgamma_tmp.p + P.cout, b.dgamma_tmp.ts, SP_R);
        TS hg = Gd(P.g), hb = Gd(P.beta);
        ColArgs cb = col_args(p, SP_R, sR.inrect, P.cout, 6);  // tangent sums = hv(gamma), hv(beta)
        cb.yscale = ysc; cb.xdrop = pdrop;
        cb.X = tcur.p; cb.x_ts = tcur.ts; cb.X2 = cur.p; cb.x2_ts = cur.ts; cb.Y = b.a.p; cb.y_ts = b.a.ts; cb.Y2 = t.a.p; cb.y2_ts = t.a.ts;
        cb.Z = b.c.p; cb.z_ts = b.c.ts; cb.Z2 = t.c.p; cb.z2_ts = t.c.ts; cb.stats = b.stats.p; cb.st_ts = b.stats.ts;
        cb.stats2 = t.stats.p; cb.st2_ts = t.stats.ts; cb.do_tanh = act;
        colreduce(p, cb, hg.p, hb.p, hg.ts, SP_R);
        TS gm = W(ps, P.g), tgm = Wt(P.g);
        // under-filled plans: the layer's hv(W) product leaves the tangent launch for the side stream (as the decoder layers' do: TLayerGrad);
        // the BatchNorm backward then writes into buffers of the layer's own, which outlive the shared scratch the next layer reuses
        const bool dfp = knobs().so_defer_post && !tpostG.empty() && defer_ok(p) && p.tasks <= defer_tasks;
        const TS gR0 = dfp ? TS{tpostG[i].dc.p, tpostG[i].dc.ts} : this->gR0, tgR0 = dfp ? TS{tpostG[i].tdc.p, tpostG[i].tdc.ts} : this->tgR0;
        launch_bn_jvp_bwd(on_rows(p, SP_R, stream, sR.inrect), cur, tcur, b.a, t.a, b.c, t.c, b.stats, t.stats, gm, tgm, b.dgamma_tmp,
                          TS{b.dgamma_tmp.p + P.cout, b.dgamma_tmp.ts}, hg, hb, act, gR0, tgR0, P.cout, ysc, pdrop);
        TS xin = (i == 0) ? mel : postB[i - 1].a, txin = (i == 0) ? t_mel : tpostB[i - 1].a;
        if (i > 0) {
            conv_bwd_t(ps, SP_R, gR0, tgR0, P.cout, cfg.postnet_kernel, xin, txin, P.cin, P.w, P.b, sR.inrect, sk ? none : K.post_cur[i - 1], 0, tgR1, false, sR.inrect,
                       none, dfp);
            cur = K.post_cur[i - 1]; tcur = tgR1;
        } else {
            const long long n4 = (gRm.ts * nt) / 4;
            if (!sk)
                launch_add2(gRm.p - (long long)G * nm, gRp.p - (long long)G * nm, gRm.p - (long long)G * nm, n4, stream);
            conv_bwd_t(ps, SP_R, gR0, tgR0, P.cout, cfg.postnet_kernel, xin, txin, P.cin, P.w, P.b, sR.inrect, sk ? none : gRm, GEMM_ACCUM, tgRm, false, sR.inrect,
                       none, dfp);
        }
        if (dfp) {   // hv(W_i) = tdY^T X + dY^T tX (one dual-source problem) on the side stream, after everything above
            fork_side();
            GemmBatchScope batch(gx_side, side);
            conv_wgrad(ps, SP_R, on_side(hv_wgrad_op(xin, txin, P.cin, cfg.postnet_kernel, gR0, tgR0, P.cout, P.w, P.b, sR.inrect)));
            defer_live = true;
        }
    }
    set_tag(0);
    ar_ready(ar_idx_postnet());   // (overlapped exchange of the last reverse step, engine.h)
    // mel_linear
    colsum(ps, SP_R, tgRm, nm, RowMask(), none, Gd(mel_b));
    launch_gather_rows(on_rows(p, SP_F, stream), gRm, p.f2r, gMelF, nm);
    launch_gather_rows(on_rows(p, SP_F, stream), tgRm, p.f2r, tgMelF, nm);
    TS dec_out = cfg.dec_layers ? decB[cfg.dec_layers - 1].y2 : dec_in;
    TS tdec_out = cfg.dec_layers ? tdecB[cfg.dec_layers - 1].y2 : t_dec_in;
    conv_bwd_t(ps, SP_F, gMelF, tgMelF, nm, 1, dec_out, tdec_out, d, mel_w, -1, RowMask(), sk ? none : K.dec_top, 0, tgF0, false, RowMask());
    for (int l = cfg.dec_layers - 1; l >= 0; --l) {
        TS xin = l == 0 ? dec_in : decB[l - 1].y2, txin = l == 0 ? t_dec_in : tdecB[l - 1].y2;
        site_base = 64 + 2 * l;
        TLayerGrad* tl = (sk && !tdecG.empty() && defer_ok(p)) ? &tdecG[l] : nullptr;
        fft_bwd_t(ps, SP_F, cfg.dec_heads, decP[l], decB[l], tdecB[l], xin, txin, l == cfg.dec_layers - 1 ? K.dec_top : K.dec[l + 1].g0, tgF0,
                  K.dec[l], sk, this->gF0, this->gF1, tgF1, tgFqkv, tgFh, dSf, tdSf, tl);
        ar_ready(ar_idx_dec(l));
    }
    const TS gF0 = cfg.dec_layers ? K.dec[0].g0 : K.dec_top;   // primal gradient of the decoder input
    // length regulator + speaker vector: the tangent always, the primal input gradient only when an adapted encoder sits upstream
    const bool enc_t = encoder_adapted();
    TS dxp = enc_t ? gP0 : none;
    TS gLR = gF0, tgLR = tgF0;
    if (any_frame_level()) {
        // frame-level half of the variance adaptor on the frame rectangle (engine.h: backward_impl), tangent and — for an adapted encoder —
        // primal input gradients
        TS dxr = enc_t ? gRx : none;
        launch_gather_rows(on_rows(p, SP_R, stream), tgF0, p.r2f, tgRx, d);
        if (enc_t)
            launch_gather_rows(on_rows(p, SP_R, stream), gF0, p.r2f, gRx, d);
        if (cfg.energy_frame) {
            launch_table_grad(on_rows(p, SP_R, stream), cfg.n_bins, tgRx, eidx_r, -1, Gd(energy_emb), d);
            site_base = 136;
            pred_bwd_t(ps, eneP, eneR, teneR, cfg.pitch_frame ? xr1 : xr0, cfg.pitch_frame ? t_xr1 : t_xr0, dpred_r[1], tdpred_r[1], tgRx, dxr, SP_R);
        }
        if (cfg.pitch_frame) {
            launch_table_grad(on_rows(p, SP_R, stream), cfg.n_bins, tgRx, pidx_r, -1, Gd(pitch_emb), d);
            site_base = 132;
            pred_bwd_t(ps, pitP, pitR, tpitR, xr0, t_xr0, dpred_r[0], tdpred_r[0], tgRx, dxr, SP_R);
        }
        launch_gather_rows(on_rows(p, SP_F, stream), tgRx, p.f2r, tgFx, d);
        tgLR = tgFx;
        if (enc_t) {
            launch_gather_rows(on_rows(p, SP_F, stream), gRx, p.f2r, gFx, d);
            gLR = gFx;
        }
    }
    launch_length_regulate_bwd(on_rows(p, SP_P, stream), tgLR, p.p_first, p.p_count, tgP0, d, 0);
    if (enc_t)
        launch_length_regulate_bwd(on_rows(p, SP_P, stream), gLR, p.p_first, p.p_count, gP0, d, 0);
    launch_segsum_rows(on_rows(p, SP_F, stream), p.maxB, tgF0, p.f_seg_start, p.f_seg_len, (long long)cap_B, tdspk, d, 0);
    if (!cfg.energy_frame) {
        table_hv(p, tgP0, gPxE, eidx, cfg.n_bins, -1, energy_emb, true);
        site_base = 136;
        pred_bwd_t(ps, eneP, eneB, teneB, cfg.pitch_frame ? x0 : x1, cfg.pitch_frame ? t_x0 : t_x1, dpred[2], tdpred[2], tgP0, dxp);
    }
    if (!cfg.pitch_frame) {
        table_hv(p, tgP0, gPxP, pidx, cfg.n_bins, -1, pitch_emb, true);
        site_base = 132; pred_bwd_t(ps, pitP, pitB, tpitB, x0, t_x0, dpred[1], tdpred[1], tgP0, dxp);
    }
    site_base = 128; pred_bwd_t(ps, durP, durB, tdurB, x0, t_x0, dpred[0], tdpred[0], tgP0, dxp);
    launch_segsum_rows(on_rows(p, SP_P, stream), p.maxB, tgP0, p.p_seg_start, p.p_seg_len, (long long)cap_B, tdspk, d, 1);
    if (!p.ext_spk)
    launch_speaker_table_grad(on_rows(p, SP_P, stream), cfg.n_speaker, tdspk, p.spk_ids, (long long)cap_B + 1, cap_B, p.average_spk, Gd(spk_table), d);
    ar_ready(ar_idx_spk());
    // a non-adapted encoder carries no forward tangent, so the tangent of its gradients is its ordinary backward applied to tgP0; an
    // adapted one goes through the primal + tangent backward like the decoder
    for (int l = cfg.enc_layers - 1; l >= 0; --l) {
        TS xin = l == 0 ? emb_out : encB[l - 1].y2;
        site_base = 2 * l;
        if (enc_t) {
            TS txin = l == 0 ? t_emb : tencB[l - 1].y2;
            fft_bwd_t(ps, SP_P, cfg.enc_heads, encP[l], encB[l], tencB[l], xin, txin, gP0, tgP0, LayerKeep{gP0, gPh, gP1, gP1, gPqkv}, false, gP0, gP1,
                      tgP1, tgPqkv, tgPh, dSp, tdSp);
        } else {
            fft_bwd(ps, SP_P, cfg.enc_heads, encP[l], encB[l], xin, tgP0, LayerKeep{tgP0, gPh, gP1, gP1, gPqkv}, dSp, defer_ok(p) ? &encG[l] : nullptr);
        }
        if (l > 0) ar_ready(ar_idx_enc(l));
    }
    table_hv(p, tgP0, TS{nullptr, 0}, p.p_tok, cfg.vocab, 0, word_emb, false);   // (nothing writes tgP0 after this point: no snapshot)
    join_side();   // (deferred hv(W) products)
    return 0;
}
// hv of an embedding table on the phoneme rectangle: dtable[v] = sum of the rows of `g` whose index is v.  A pure parameter gradient — 44 us of scanning per launch on
// a single-task rank (the bucket of the padded positions is ~100 hits deep) — so it runs on the side stream.  snapshot: `g` is about to be accumulated into by the
// launches that follow on the critical stream (the predictors' input gradients), so the side stream reads a copy (`snap`, a buffer of the early predictor backward,
// idle during the tangent backward; one 5 us copy launch stays on the critical stream).  MTTS_SO_TABLE_SIDE=0: on the critical stream.  Bit-identical either way.
void table_hv(const Plan& p, TS g, TS snap, const int* idx, int n_rows, int skip_row, long long emb_off, bool snapshot) {
    const int d = cfg.d_model, nt = p.tasks;
    if (!knobs().so_table_side || side == nullptr || (snapshot && (arena_pred == nullptr || snap.p == nullptr))) {
        launch_table_grad(on_rows(p, SP_P, stream), n_rows, g, idx, skip_row, Gd(emb_off), d);
        return;
    }
    TS src = g;
    if (snapshot) {
        launch_copy_tasks(g, snap, (long long)p.sp[SP_P].maxM * d / 4, nt, stream);
        src = snap;
    }
    fork_side();
    launch_table_grad(on_rows(p, SP_P, side), n_rows, src, idx, skip_row, Gd(emb_off), d);
}

// ---- second-order meta-gradient ---------------------------------------------------------------------------
int meta_grad_so(int steps, float inner_lr, float grad_scale, float* losses_out, float* sup_losses_out) {
    Plan& sp = plans[0];
    Plan& qp = plans[1];
    if (sp.tasks != qp.tasks || sp.tasks < 1) { set_error("support/query plans not set"); return -1; }
    if (enable_second_order(std::max(steps, 1))) return -1;
    if (inner_prox > 0.f) { set_error("second-order MAML with a proximal inner loss is not defined here (use the iMAML hypergradient)"); return -1; }
    const int nt = sp.tasks;
    const long long hist_ts = n_adapt;             // [step][task][n_adapt]
    if (n_adapt > 0)
        launch_broadcast(theta + adapt_start, TS{fast, n_adapt}, n_adapt / 4, nt, stream);
    Pass ps{&sp, true, true};
    std::vector<unsigned> step_seeds(std::max(steps, 1), 0u);
    unsigned ahead_seeds[kAhead];
    // Inner step s keeps its activations in a set of its own (288 GB of HBM: ~0.65 GB per full-size task and step), so the reverse
    // sweep below goes straight to the tangent passes instead of replaying the forward of every step first (one forward of the eight
    // forward-equivalents a reverse step costs).  MTTS_SO_KEEP_ACT=0, or a device that cannot hold the sets: the replay.
    const bool keep = knobs().so_keep_act && steps >= 1 && ensure_act_sets(steps);
    // ... and the gradients its backward leaves (engine.h: GradSet), so the tangent backward of step s does not repeat the primal
    // input-gradient GEMMs either (another forward-equivalent per step; ~0.3 GB per full-size task and step).  MTTS_SO_KEEP_GRAD=0: recompute.
    const bool keep_grad = keep && knobs().so_keep_grad && ensure_grad_sets(steps);
    struct Rebind { Engine* e; ~Rebind() { e->bind_act(0); e->gs_bound = -1; } } rebind{this};
    unsigned qseed = 0;
    const bool ahead = run_encoder_ahead(sp, steps, ahead_seeds, keep, &qp, &qseed);   // engine.h: the (non-adapted) encoder's forwards of all steps (+ the query pass's), on side2
    for (int s = 0; s < steps; ++s) {
        DEV_CHECK(hipMemcpyAsync(fast_hist + (long long)s * cap_tasks * hist_ts, fast, (size_t)n_adapt * nt * sizeof(float),
                                 hipMemcpyDeviceToDevice, stream));
        if (keep) bind_act(s + 1);
        gs_bound = keep_grad ? s : -1;
        if (ahead) { hipStreamWaitEvent(stream, ev_enc[s], 0); ps.seed_override = ahead_seeds[s]; ps.enc_out = enc_ahead[s]; }
        if (forward(ps)) return -1;
        step_seeds[s] = sp.drop_seed;
        if (sup_losses_out && loss(ps, sup_losses_out + (long long)s * nt * 6)) return -1;
        if (inner_backward_update(ps, nt, inner_lr)) return -1;
    }
    bind_act(0);
    gs_bound = -1;
    Pass pq{&qp, true, true};
    if (ahead && qseed) { hipStreamWaitEvent(stream, ev_enc[steps], 0); pq.seed_override = qseed; pq.enc_out = encB[cfg.enc_layers - 1].y2; }
    if (forward(pq)) return -1;
    if (loss(pq, losses_out ? losses_out : losses)) return -1;
    if (!losses_out || losses_out == losses) { sync_nt = nt; sync_scale = grad_scale; }
    else ar_armed = false;
    if (backward(pq, grad_scale, true)) return -1;          // grad[t] = (e | v_K)
    Pass ph{&sp, true, true};
    ph.update_bn = false;
    for (int s = steps - 1; s >= 0; --s) {
        fast_cur = fast_hist + (long long)s * cap_tasks * hist_ts;
        ph.seed_override = step_seeds[s];  // the dropout masks of inner step s
        int rc = 0;
        if (keep) {
            bind_act(s + 1);               // the activations of inner step s, encoder included (the run-ahead wrote them into this set)
            gs_bound = keep_grad ? s : -1;
            sp.drop_seed = step_seeds[s];
        } else {
            // (the replay runs the encoder again: backward_t applies the encoder's ordinary backward and needs ITS saved activations)
            rc = forward(ph);
        }
        if (!rc) rc = forward_t(ph);
        grad_dst = hv;
        // the LAST reverse step completes the meta-gradient: with the overlapped exchange armed, every bucket gets its update
        // grad -= lr * hv, its task sum and its all-reduce the moment the tangent backward has finished the module (engine.h: ar_ready)
        const bool overlap = s == 0 && ar_begin(nt, -inner_lr);
        if (overlap) ar_tail();
        if (!rc) rc = backward_t(ph, 1.f, keep_grad);
        grad_dst = grad;
        fast_cur = fast;
        gs_bound = -1;
        if (overlap) { if (ar_end() || rc) return -1; return 0; }
        if (rc) return -1;
        launch_axpy(TS{grad, n_total}, TS{hv, n_total}, -inner_lr, n_total / 4, nt, stream);
    }
    ar_armed = false;   // (steps == 0: nothing to overlap with)
    launch_sum_tasks(TS{grad, n_total}, nt, 1.f, outer, n_total / 4, (int)outer_accumulate, stream);
    return 0;
}

// Hessian-vector product of the support loss at the current fast weights (plan 0) in the direction held in the
// per-task gradient buffer (tests): result in hv.
int hvp_support() {
    Plan& sp = plans[0];
    if (sp.tasks < 1) { set_error("support plan not set"); return -1; }
    if (enable_second_order(1)) return -1;
    Pass ph{&sp, true, true};
    ph.update_bn = false;
    int rc = forward(ph);
    if (!rc) rc = forward_t(ph);
    grad_dst = hv;
    if (!rc) rc = backward_t(ph, 1.f);
    grad_dst = grad;
    return rc;
}
