// Kernel-level entry points for the non-GEMM kernels (included by mtts.hip inside extern "C"): each HBM-bound kernel of
// rowops.h can be parity-tested alone against torch through the C ABI (SURVEY.md section 8(b)).  Raw device pointers, caller
// allocated outputs and scratch (`ws`, mtts_kernel_ws_bytes), nothing allocated here, asynchronous on `stream` except for the
// small descriptor upload (one synchronous hipMemcpy of <= 64 bytes / one table).
namespace {
struct KernelWs {            // layout of the caller's scratch
    int* meta;               // META_STRIDE ints (one "task")
    float* col_partial;      // [chunks][3][1024]
    AttnSeq* seqs;           // n_mat descriptors
    GemmGroupDesc* tab[2];
    int chunks;
};
inline long long kernel_ws_bytes(int rows, int n_mat) {
    const long long chunks = (rows + kLnRows - 1) / kLnRows;   // (the LayerNorm backward's 8-row partial chunks: the finer of the two chunkings)
    return 256 + chunks * 3 * 1024 * (long long)sizeof(float) + 256 + (long long)n_mat * (sizeof(AttnSeq) + 2 * sizeof(GemmGroupDesc)) + 256;
}
inline KernelWs carve(void* ws, int rows, int n_mat) {
    KernelWs k;
    char* p = (char*)ws;
    k.meta = (int*)p; p += 256;
    k.chunks = (rows + kRC - 1) / kRC;
    k.col_partial = (float*)p; p += (size_t)((rows + kLnRows - 1) / kLnRows) * 3 * 1024 * sizeof(float);
    p = (char*)(((uintptr_t)p + 255) & ~(uintptr_t)255);
    k.seqs = (AttnSeq*)p; p += (size_t)n_mat * sizeof(AttnSeq);
    k.tab[0] = (GemmGroupDesc*)p; p += (size_t)n_mat * sizeof(GemmGroupDesc);
    k.tab[1] = (GemmGroupDesc*)p;
    return k;
}
// one-task meta table: every row-count field = rows, B * Tcap = n_in (BatchNorm's element count)
inline int put_meta(const KernelWs& k, int rows, int n_in) {
    int m[META_STRIDE];
    m[META_B] = 1; m[META_SMAX] = rows; m[META_TCAP] = n_in; m[META_MP] = rows; m[META_MF] = rows; m[META_MR] = rows; m[META_NP] = rows; m[META_NF] = rows;
    return hipMemcpy(k.meta, m, sizeof(m), hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
// the launchers' view of the scratch block: one task of `rows` rows (every row-count field of the meta table holds it), strides 0
inline RowLaunch one_task(const KernelWs& k, int rows, int mfield, const unsigned char* mask, void* stream) {
    return RowLaunch{k.meta, mfield, rows, 1, mask, 0, (hipStream_t)stream};
}
inline TS T0(const float* p) { return TS{const_cast<float*>(p), 0}; }   // a one-task array
inline void col_reduce(const KernelWs& k, const RowLaunch& r, const ColArgs& a, float* out0, float* out1) {
    launch_colreduce(r, a, k.col_partial, k.chunks, out0, out1, 0);
}
inline bool bad_rows(int rows, int C) { return rows < 1 || C < 4 || (C & 3) || C > 1024; }
}  // namespace

int64_t mtts_kernel_ws_bytes(int rows, int n_mat) { return kernel_ws_bytes(rows < 1 ? 1 : rows, n_mat < 0 ? 0 : n_mat); }

int mtts_layernorm_fwd(int rows, int C, const float* a, const float* res, const float* gamma, const float* beta, const unsigned char* mask,
                       float* z, float* y, float* stats, void* ws, void* stream) {
    if (bad_rows(rows, C) || !a || !gamma || !beta || !y || !stats || !ws) return -1;
    const KernelWs k = carve(ws, rows, 0);
    if (put_meta(k, rows, rows)) return -1;
    launch_layernorm_fwd(one_task(k, rows, META_MP, mask, stream), T0(a), T0(res), T0(gamma), T0(beta), T0(z), T0(y), T0(stats), C);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int mtts_layernorm_bwd(int rows, int C, const float* dy, const float* z, const float* stats, const float* gamma, const unsigned char* mask,
                       float* dz, float* dgamma, float* dbeta, void* ws, void* stream) {
    if (bad_rows(rows, C) || !dy || !z || !stats || !gamma || !dz || !dgamma || !dbeta || !ws) return -1;
    const KernelWs k = carve(ws, rows, 0);
    if (put_meta(k, rows, rows)) return -1;
    // stage 1 of the gamma / beta reduction happens inside the backward kernel (8-row partials), colfinal folds them
    launch_layernorm_bwd(one_task(k, rows, META_MP, mask, stream), T0(dy), T0(z), T0(stats), T0(gamma), T0(dz), C, 0, T0(nullptr), DropSpec(), DropSpec(),
                         k.col_partial, true, T0(dgamma), T0(dbeta));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// S: [n_mat][L][ldS] with ldS = (L + 3) & ~3; softmax over the L valid columns of every row, in place (Modules.py:18-21: the
// padded keys are simply not part of a sequence's score matrix here)
static int put_seqs(const KernelWs& k, int n_mat, int L) {
    const int ldS = (L + 3) & ~3;
    std::vector<AttnSeq> sq(n_mat);
    for (int i = 0; i < n_mat; ++i) sq[i] = AttnSeq{(long long)i * L * ldS, L, ldS};
    return hipMemcpy(k.seqs, sq.data(), sq.size() * sizeof(AttnSeq), hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
int mtts_softmax_fwd(int n_mat, int L, float* S, void* ws, void* stream) {
    if (n_mat < 1 || L < 1 || !S || !ws) return -1;
    const KernelWs k = carve(ws, 1, n_mat);
    if (put_seqs(k, n_mat, L)) return -1;
    launch_softmax_fwd(k.seqs, L, n_mat, S, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// dP -> dS in place: dS = alpha * P o (dP - rowsum(dP o P))
int mtts_softmax_bwd(int n_mat, int L, const float* P, float* dP, float alpha, void* ws, void* stream) {
    if (n_mat < 1 || L < 1 || !P || !dP || !ws) return -1;
    const KernelWs k = carve(ws, 1, n_mat);
    if (put_seqs(k, n_mat, L)) return -1;
    launch_softmax_bwd(k.seqs, L, n_mat, P, dP, alpha, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// ScaledDotProductAttention.forward (transformer/Modules.py:14-25) for n_mat independent (sequence, head) pairs of equal length:
// q, k, v, o [n_mat][L][dk] contiguous; P [n_mat][L][ldS].  Two grouped MFMA GEMMs (descriptor-table mode) around the softmax.
int mtts_sdpa_fwd(int n_mat, int L, int dk, const float* q, const float* kk, const float* v, float* P, float* o, void* ws, void* stream) {
    if (n_mat < 1 || L < 1 || dk < 4 || (dk & 3) || !q || !kk || !v || !P || !o || !ws) return -1;
    const KernelWs k = carve(ws, 1, n_mat);
    if (put_seqs(k, n_mat, L)) return -1;
    const int ldS = (L + 3) & ~3;
    std::vector<GemmGroupDesc> t0(n_mat), t1(n_mat);
    for (int i = 0; i < n_mat; ++i) {
        const long long x = (long long)i * L * dk, s = (long long)i * L * ldS;
        t0[i] = GemmGroupDesc{x, x, s, L, L, dk, dk, dk, ldS};   // S = Q K^T
        t1[i] = GemmGroupDesc{s, x, x, L, dk, L, ldS, dk, dk};   // O = P V
    }
    if (hipMemcpy(k.tab[0], t0.data(), t0.size() * sizeof(GemmGroupDesc), hipMemcpyHostToDevice) != hipSuccess) return -1;
    if (hipMemcpy(k.tab[1], t1.data(), t1.size() * sizeof(GemmGroupDesc), hipMemcpyHostToDevice) != hipSuccess) return -1;
    if (knobs().fused_attn && attn_fused_ok(L, dk)) {   // the fused kernel the engine uses (attention.h)
        AttnFwdArgs fa;
        fa.seqs = (const AttnSeq*)k.seqs; fa.tab_qk = k.tab[0]; fa.tab_pv = k.tab[1];
        fa.Q = q; fa.K = kk; fa.V = v; fa.ld_q = fa.ld_k = fa.ld_v = dk;
        fa.P = P; fa.O = o; fa.ld_o = dk; fa.scale = 1.f / sqrtf((float)dk); fa.dk = dk; fa.rot = 0; fa.prio = 0;
#if defined(MTTS_ATTN_DIAG)
        fa.diag = knobs().attn_diag_mask;
#endif
        attn_fwd_launch(fa, L, n_mat, (hipStream_t)stream);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    GemmCtx& cx = kernel_ctx();
    GemmArgs g;
    g.table = k.tab[0]; g.A = q; g.B = kk; g.C = P; g.alpha = 1.f / sqrtf((float)dk); g.K = dk;
    gemm_launch(cx, GEMM_NT, g, L, L, n_mat, (hipStream_t)stream);
    launch_softmax_fwd(k.seqs, L, n_mat, P, (hipStream_t)stream);
    GemmArgs h;
    h.table = k.tab[1]; h.A = P; h.B = v; h.C = o; h.K = L;
    gemm_launch(cx, GEMM_NN, h, L, dk, n_mat, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Attention in the layout the engine runs (engine.h: fft_fwd / fft_bwd): n_seq sequences of ragged lengths lens[i] at rows row0[i] of one
// packed [rows][3 d] buffer (d = heads * dk; Q | K | V column blocks, a head = dk columns), O / dO in [rows][d]; group n = seq * heads + head,
// its P / dS matrix [L][ldS] at the running sum of L * ldS.  The descriptors are attn_group_descs' — the plan's own.  Contract on buffer
// contents: nothing outside a sequence's rows is read into a result, and the pad columns [L, ldS) of P and dS are WRITTEN (zero) by the
// softmax of either path before any product reads them, so P and dS may hold anything on entry of _fwd / _bwd.
namespace {
struct AttnPackedWs { AttnSeq* seqs; GemmGroupDesc* tab[6]; };
inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
inline long long attn_packed_ws_bytes(long long n) { return (long long)(up256(n * sizeof(AttnSeq)) + 6 * up256(n * sizeof(GemmGroupDesc))); }
struct AttnPacked {
    int n = 0, max_L = 0, d = 0;
    long long sumL = 0;
    double sumL2 = 0.0;
    AttnPackedWs w;
};
// validates, builds the descriptors of every (sequence, head) and uploads them: one synchronous copy
inline int attn_packed_setup(int n_seq, int heads, int dk, const int* lens, const int* row0, void* ws, int64_t ws_bytes, AttnPacked& a) {
    if (n_seq < 1 || heads < 1 || dk < 4 || (dk & 3) || !lens || !row0 || !ws) return -1;
    for (int i = 0; i < n_seq; ++i) if (lens[i] < 1 || row0[i] < 0) return -1;
    a.n = n_seq * heads; a.d = heads * dk;
    const long long need = attn_packed_ws_bytes(a.n);
    if (ws_bytes < need) return -1;
    std::vector<char> img((size_t)need, 0);
    const size_t sb = up256((size_t)a.n * sizeof(AttnSeq)), tb = up256((size_t)a.n * sizeof(GemmGroupDesc));
    AttnSeq* hs = (AttnSeq*)img.data();
    a.w.seqs = (AttnSeq*)ws;
    for (int k = 0; k < 6; ++k) a.w.tab[k] = (GemmGroupDesc*)((char*)ws + sb + k * tb);
    long long so = 0;
    for (int i = 0; i < n_seq; ++i) {
        const int L = lens[i];
        a.max_L = std::max(a.max_L, L);
        a.sumL += (long long)heads * L; a.sumL2 += (double)heads * L * L;
        for (int hh = 0; hh < heads; ++hh) {
            const int n = i * heads + hh;
            GemmGroupDesc gd[6];
            attn_group_descs((long long)row0[i] * 3 * a.d + hh * dk, (long long)row0[i] * a.d + hh * dk, so, L, dk, a.d, hs[n], gd);
            for (int k = 0; k < 6; ++k) ((GemmGroupDesc*)(img.data() + sb + k * tb))[n] = gd[k];
            so += (long long)L * hs[n].ldS;
        }
    }
    return hipMemcpy(ws, img.data(), (size_t)need, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
// one table-mode product with the launch bounds and cost hints of Engine::attn_gemm
inline void attn_packed_gemm(const AttnPacked& a, int which, int form, int dk, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                             float alpha, hipStream_t stream) {
    GemmArgs g;
    g.table = a.w.tab[which];
    g.A = A; g.B = B; g.C = C; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.alpha = alpha;
    const bool sq = which == TAB_QK || which == TAB_DP;
    g.K = sq ? dk : a.max_L;
    gemm_launch(kernel_ctx(), form, g, a.max_L, sq ? a.max_L : dk, a.n, stream, 0, 2.0 * a.sumL2 * dk, a.sumL, 4.0 * (a.sumL2 + 2.0 * (double)a.sumL * dk));
}
}  // namespace

int64_t mtts_attn_packed_ws_bytes(int n_seq, int heads) { return attn_packed_ws_bytes((long long)(n_seq < 1 ? 1 : n_seq) * (heads < 1 ? 1 : heads)); }

// path 0: what fft_fwd launches (the fused kernel when it serves max_L and dk, else the three launches); path 1: the three launches
int mtts_attn_packed_fwd(int n_seq, int heads, int dk, const int* lens, const int* row0, int path, const float* qkv, float* P, float* O, void* ws,
                         int64_t ws_bytes, void* stream) {
    if (!qkv || !P || !O || (path != 0 && path != 1)) return -1;
    AttnPacked a;
    if (attn_packed_setup(n_seq, heads, dk, lens, row0, ws, ws_bytes, a)) return -1;
    const int d = a.d;
    const float scale = 1.f / sqrtf((float)dk);
    if (path == 0 && knobs().fused_attn && attn_fused_ok(a.max_L, dk)) {
        AttnFwdArgs fa;
        fa.seqs = a.w.seqs; fa.tab_qk = a.w.tab[TAB_QK]; fa.tab_pv = a.w.tab[TAB_PV];
        fa.Q = fa.K = fa.V = qkv; fa.ld_q = fa.ld_k = fa.ld_v = 3 * d;
        fa.P = P; fa.O = O; fa.ld_o = d; fa.scale = scale; fa.dk = dk; fa.rot = 0; fa.prio = 0;
#if defined(MTTS_ATTN_DIAG)
        fa.diag = 0;
#endif
        attn_fwd_launch(fa, a.max_L, a.n, (hipStream_t)stream);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    attn_packed_gemm(a, TAB_QK, GEMM_NT, dk, qkv, 3 * d, qkv, 3 * d, P, 0, scale, (hipStream_t)stream);
    launch_softmax_fwd(a.w.seqs, a.max_L, a.n, P, (hipStream_t)stream);
    attn_packed_gemm(a, TAB_PV, GEMM_NN, dk, P, 0, qkv, 3 * d, O, d, 1.f, (hipStream_t)stream);
    return kernel_launch_rc();
}
// fft_bwd's attention part: dP = dO V^T and dV = P^T dO as one batch, dP -> dS in place, dQ = dS K and dK = dS^T Q as one batch;
// gqkv receives dQ | dK | dV in the column blocks of qkv
int mtts_attn_packed_bwd(int n_seq, int heads, int dk, const int* lens, const int* row0, const float* qkv, const float* P, const float* dO, float* dS,
                         float* gqkv, void* ws, int64_t ws_bytes, void* stream) {
    if (!qkv || !P || !dO || !dS || !gqkv) return -1;
    AttnPacked a;
    if (attn_packed_setup(n_seq, heads, dk, lens, row0, ws, ws_bytes, a)) return -1;
    const int d = a.d;
    hipStream_t st = (hipStream_t)stream;
    GemmCtx& cx = kernel_ctx();
    gemm_batch_begin(cx);
    attn_packed_gemm(a, TAB_DP, GEMM_NT, dk, dO, d, qkv, 3 * d, dS, 0, 1.f, st);
    attn_packed_gemm(a, TAB_DV, GEMM_TN, dk, P, 0, dO, d, gqkv, 3 * d, 1.f, st);
    gemm_batch_end(cx, st);
    launch_softmax_bwd(a.w.seqs, a.max_L, a.n, P, dS, 1.f / sqrtf((float)dk), st);
    gemm_batch_begin(cx);
    attn_packed_gemm(a, TAB_DQ, GEMM_NN, dk, dS, 0, qkv, 3 * d, gqkv, 3 * d, 1.f, st);
    attn_packed_gemm(a, TAB_DK, GEMM_TN, dk, dS, 0, qkv, 3 * d, gqkv, 3 * d, 1.f, st);
    gemm_batch_end(cx, st);
    return kernel_launch_rc();
}

// PostNet BatchNorm1d in training mode (transformer/Layers.py:129-137): statistics over the rows with inrect != 0 (the padded
// frames of the rectangle count, as in the reference), y = [tanh](gamma * xhat + beta) on those rows, 0 elsewhere.
// stats [3C] = mean | rstd | unbiased variance (what the running-var update uses).
int mtts_batchnorm_fwd(int rows, int C, const float* x, const unsigned char* inrect, const float* gamma, const float* beta, int do_tanh,
                       float* stats, float* y, void* ws, void* stream) {
    if (bad_rows(rows, C) || !x || !inrect || !gamma || !beta || !stats || !y || !ws) return -1;
    const KernelWs k = carve(ws, rows, 0);
    if (put_meta(k, rows, rows)) return -1;
    ColArgs ca;
    ca.X = x; ca.mask = inrect; ca.C = C; ca.mode = 2; ca.mfield = META_MR;
    const RowLaunch r = one_task(k, rows, META_MR, inrect, stream);
    col_reduce(k, r, ca, stats, nullptr);
    launch_bn_apply(r, T0(x), T0(stats), T0(gamma), T0(beta), do_tanh, T0(y), C);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// backward of the above: dy -> dx, dgamma, dbeta (n_in = number of rows with inrect != 0)
int mtts_batchnorm_bwd(int rows, int n_in, int C, const float* dy, const float* y, const float* x, const float* stats, const unsigned char* inrect,
                       const float* gamma, int do_tanh, float* dx, float* dgamma, float* dbeta, void* ws, void* stream) {
    if (bad_rows(rows, C) || n_in < 1 || !dy || !y || !x || !stats || !inrect || !gamma || !dx || !dgamma || !dbeta || !ws) return -1;
    const KernelWs k = carve(ws, rows, 0);
    if (put_meta(k, rows, n_in)) return -1;
    ColArgs ca;
    ca.X = dy; ca.Y = y; ca.Z = x; ca.stats = stats; ca.mask = inrect; ca.C = C; ca.mode = 3; ca.do_tanh = do_tanh; ca.mfield = META_MR;
    const RowLaunch r = one_task(k, rows, META_MR, inrect, stream);
    col_reduce(k, r, ca, dgamma, dbeta);
    launch_bn_bwd_apply(r, T0(dy), T0(y), T0(x), T0(stats), T0(gamma), T0(dgamma), T0(dbeta), do_tanh, T0(dx), C);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Gradient of an embedding table (nn.Embedding backward; pitch / energy / phoneme tables): dtable[v] = sum over rows with
// idx[row] == v of dx[row], rows summed in ascending order (deterministic, no atomics); every row of dtable is written
// (zero when unused); skip_row (< 0: none) stays zero (padding_idx).
int mtts_table_grad(int rows, int C, int V, const float* dx, const int* idx, int skip_row, float* dtable, void* ws, void* stream) {
    if (bad_rows(rows, C) || V < 1 || !dx || !idx || !dtable || !ws) return -1;
    const KernelWs k = carve(ws, rows, 0);
    if (put_meta(k, rows, rows)) return -1;
    launch_table_grad(one_task(k, rows, META_MP, nullptr, stream), V, T0(dx), idx, skip_row, T0(dtable), C);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Length regulator (modules.py:167-190).  fwd: out[r] = x[src[r]] (+ spk) (+ pos[row_t[r]]) for the n_frames frame rows, 0 where
// src[r] < 0; spk / pos / row_t may be null (plain gather).  bwd: dx[p] = sum of dout over the contiguous frame run
// [first[p], first[p] + count[p]) of every phoneme row — the segment-sum form of the gather's transpose.
int mtts_length_regulate_fwd(int n_frames, int C, const float* x, const int* src, const float* spk, const float* pos, const int* row_t, float* out,
                             void* ws, void* stream) {
    if (bad_rows(n_frames, C) || !x || !src || !out || !ws || (pos && !row_t)) return -1;
    const KernelWs k = carve(ws, n_frames, 0);
    if (put_meta(k, n_frames, n_frames)) return -1;
    // the kernel adds a per-utterance speaker row spk[row_b[r]]: with one utterance row_b is all zero — col_partial is reused as that table
    // (and as the zero speaker row / zero position index when the caller passes none)
    int* zeros_i = (int*)k.col_partial;
    float* zeros_f = k.col_partial + n_frames;   // needs n_frames ints + C floats <= chunks * 3072 floats (chunks = ceil(rows / kRC))
    if ((long long)n_frames + C > (long long)k.chunks * 3 * 1024) return -1;
    if (hipMemsetAsync(k.col_partial, 0, ((size_t)n_frames + C) * sizeof(float), (hipStream_t)stream) != hipSuccess) return -1;
    launch_length_regulate_fwd(one_task(k, n_frames, META_MF, nullptr, stream), T0(x), src, zeros_i, row_t ? row_t : (const int*)zeros_i, T0(spk ? spk : zeros_f),
                               pos, T0(out), C);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int mtts_length_regulate_bwd(int n_phonemes, int C, const float* dout, const int* first, const int* count, float* dx, int accumulate, void* ws,
                             void* stream) {
    if (bad_rows(n_phonemes, C) || !dout || !first || !count || !dx || !ws) return -1;
    const KernelWs k = carve(ws, n_phonemes, 0);
    if (put_meta(k, n_phonemes, n_phonemes)) return -1;
    launch_length_regulate_bwd(one_task(k, n_phonemes, META_MP, nullptr, stream), T0(dout), first, count, T0(dx), C, accumulate);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Forward-mode twins used by the second-order path (tangent.h).  layernorm_jvp: tangent of y = mask * (gamma * xhat + beta) for the
// input tangent ta (+ tres), parameter tangents tgamma / tbeta (null: 0), on the z / stats saved by mtts_layernorm_fwd.
// softmax_jvp: tS -> tP = P (tS - sum_j P_j tS_j), in place.
// layernorm_jvp_full: the same launch with the kernel's two by-products kept — tz_out [rows][C] = ta + tres and tstats_out [rows][2] = (m1, m2),
// what the tangent backward reads (either may be null: tstats then goes to scratch).
int mtts_layernorm_jvp_full(int rows, int C, const float* ta, const float* tres, const float* z, const float* stats, const float* gamma,
                            const float* tgamma, const float* tbeta, const unsigned char* mask, float* ty, float* tz_out, float* tstats_out, void* ws,
                            void* stream) {
    if (bad_rows(rows, C) || !ta || !z || !stats || !gamma || !ty || !ws) return -1;
    const KernelWs k = carve(ws, rows, 0);
    if (put_meta(k, rows, rows)) return -1;
    float* tstats = tstats_out ? tstats_out : k.col_partial;   // per-row (m1, m2), scratch when the caller keeps none
    if (!tstats_out && (long long)rows * 2 > (long long)k.chunks * 3 * 1024) return -1;
    launch_ln_jvp_fwd(one_task(k, rows, META_MP, mask, stream), T0(ta), T0(tres), T0(z), T0(stats), T0(gamma), T0(tgamma), T0(tbeta), T0(tz_out), T0(ty),
                      T0(tstats), C);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int mtts_layernorm_jvp(int rows, int C, const float* ta, const float* tres, const float* z, const float* stats, const float* gamma, const float* tgamma,
                       const float* tbeta, const unsigned char* mask, float* ty, void* ws, void* stream) {
    return mtts_layernorm_jvp_full(rows, C, ta, tres, z, stats, gamma, tgamma, tbeta, mask, ty, nullptr, nullptr, ws, stream);
}
int mtts_softmax_jvp(int n_mat, int L, const float* P, float* tS, void* ws, void* stream) {
    if (n_mat < 1 || L < 1 || !P || !tS || !ws) return -1;
    const KernelWs k = carve(ws, 1, n_mat);
    if (put_seqs(k, n_mat, L)) return -1;
    launch_softmax_jvp_fwd(k.seqs, L, n_mat, P, tS, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Tangent backward twins (tangent.h), primal + tangent in one pass, on what the forward entries above saved.
// layernorm_jvp_bwd: dy / tgy -> dz / tgz and hv(gamma) = sum_rows (tgy xhat + dy t_xhat), hv(beta) = sum_rows tgy over the unmasked rows.
// two_launch = 0: the kernel's own 8-row partials, folded by colfinal (the engine's default); 1: the ColArgs mode-5 reduction in front of
// a kernel launch without partials (the engine under MTTS_SO_LN_PART=0).
int mtts_layernorm_jvp_bwd(int rows, int C, const float* dy, const float* tgy, const float* z, const float* stats, const float* tz, const float* tstats,
                           const float* gamma, const float* tgamma, const unsigned char* mask, int relu_on_z, int two_launch, float* dz, float* tgz,
                           float* hgamma, float* hbeta, void* ws, void* stream) {
    if (bad_rows(rows, C) || !dy || !tgy || !z || !stats || !tz || !tstats || !gamma || !dz || !tgz || !hgamma || !hbeta || !ws) return -1;
    const KernelWs k = carve(ws, rows, 0);
    if (put_meta(k, rows, rows)) return -1;
    launch_ln_jvp_bwd(one_task(k, rows, META_MP, mask, stream), T0(dy), T0(tgy), T0(z), T0(stats), T0(tz), T0(tstats), T0(gamma), T0(tgamma), T0(dz), T0(tgz), C,
                      relu_on_z, T0(nullptr), T0(nullptr), DropSpec(), DropSpec(), k.col_partial, !two_launch, k.chunks, T0(hgamma), T0(hbeta));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// in place: dP -> dS = alpha P (dP - c), tgP -> tg_S = alpha [tP (dP - c) + P (tgP - cdot)]; the pad columns [L, ldS) of both are zeroed
int mtts_softmax_jvp_bwd(int n_mat, int L, const float* P, const float* tP, float* dP, float* tgP, float alpha, void* ws, void* stream) {
    if (n_mat < 1 || L < 1 || !P || !tP || !dP || !tgP || !ws) return -1;
    const KernelWs k = carve(ws, 1, n_mat);
    if (put_seqs(k, n_mat, L)) return -1;
    launch_softmax_jvp_bwd(k.seqs, L, n_mat, P, tP, dP, tgP, alpha, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// batchnorm_jvp: tangent of y = [tanh](gamma xhat + beta) for the input tangent tx on the stats / y of mtts_batchnorm_fwd: tsum [2C] =
// [S1 | S0] = [sum tx xhat | sum tx] over the inrect rows (kept: the backward reads it), then ta; rows outside inrect give 0.
int mtts_batchnorm_jvp(int rows, int n_in, int C, const float* x, const float* tx, const float* stats, const float* gamma, const float* tgamma,
                       const float* tbeta, const float* y, const unsigned char* inrect, int do_tanh, float* tsum, float* ta, void* ws, void* stream) {
    if (bad_rows(rows, C) || n_in < 1 || !x || !tx || !stats || !gamma || !y || !inrect || !tsum || !ta || !ws) return -1;
    const KernelWs k = carve(ws, rows, 0);
    if (put_meta(k, rows, n_in)) return -1;
    ColArgs ca;
    ca.X = tx; ca.Z = x; ca.stats = stats; ca.mask = inrect; ca.C = C; ca.mode = 3; ca.do_tanh = 0; ca.mfield = META_MR;
    const RowLaunch r = one_task(k, rows, META_MR, inrect, stream);
    col_reduce(k, r, ca, tsum, tsum + C);
    launch_bn_jvp_apply(r, T0(x), T0(tx), T0(stats), T0(tsum), T0(gamma), T0(tgamma), T0(tbeta), T0(y), do_tanh, T0(ta), C);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// batchnorm_jvp_bwd: dy / tgy -> dx / tdx and hv(gamma), hv(beta) (the ColArgs mode-6 reduction); dgamma / dbeta are mtts_batchnorm_bwd's
int mtts_batchnorm_jvp_bwd(int rows, int n_in, int C, const float* dy, const float* tgy, const float* y, const float* ta, const float* x, const float* tx,
                           const float* stats, const float* tsum, const float* gamma, const float* tgamma, const float* dgamma, const float* dbeta,
                           const unsigned char* inrect, int do_tanh, float* dx, float* tdx, float* hgamma, float* hbeta, void* ws, void* stream) {
    if (bad_rows(rows, C) || n_in < 1 || !dy || !tgy || !y || !ta || !x || !tx || !stats || !tsum || !gamma || !dgamma || !dbeta || !inrect || !dx ||
        !tdx || !hgamma || !hbeta || !ws)
        return -1;
    const KernelWs k = carve(ws, rows, 0);
    if (put_meta(k, rows, n_in)) return -1;
    ColArgs cb;
    cb.X = tgy; cb.X2 = dy; cb.Y = y; cb.Y2 = ta; cb.Z = x; cb.Z2 = tx; cb.stats = stats; cb.stats2 = tsum; cb.mask = inrect; cb.C = C;
    cb.mode = 6; cb.do_tanh = do_tanh; cb.mfield = META_MR;
    const RowLaunch r = one_task(k, rows, META_MR, inrect, stream);
    col_reduce(k, r, cb, hgamma, hbeta);
    launch_bn_jvp_bwd(r, T0(dy), T0(tgy), T0(y), T0(ta), T0(x), T0(tx), T0(stats), T0(tsum), T0(gamma), T0(tgamma), T0(dgamma), T0(dbeta), T0(hgamma), T0(hbeta),
                      do_tanh, T0(dx), T0(tdx), C);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// rowdot (the variance predictors' 256 -> 1 projection): tout[row] = valid ? dot(tx, w) + dot(x, tw) + tb : 0; bwd: dx = dout w,
// tdx = tgout w + dout tw.  tw / tb may be null (a projection that is not adapted).
int mtts_rowdot_jvp(int rows, int C, const float* x, const float* tx, const float* w, const float* tw, const float* tb, const unsigned char* valid,
                    float* tout, void* ws, void* stream) {
    if (bad_rows(rows, C) || !x || !tx || !w || !valid || !tout || !ws) return -1;
    const KernelWs k = carve(ws, rows, 0);
    if (put_meta(k, rows, rows)) return -1;
    launch_rowdot_jvp(one_task(k, rows, META_MP, valid, stream), T0(x), T0(tx), T0(w), T0(tw), T0(tb), T0(tout), C);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int mtts_rowdot_jvp_bwd(int rows, int C, const float* dout, const float* tgout, const float* w, const float* tw, float* dx, float* tdx, void* ws,
                        void* stream) {
    if (bad_rows(rows, C) || !dout || !tgout || !w || !dx || !tdx || !ws) return -1;
    const KernelWs k = carve(ws, rows, 0);
    if (put_meta(k, rows, rows)) return -1;
    launch_rowdot_jvp_bwd(one_task(k, rows, META_MP, nullptr, stream), T0(dout), T0(tgout), T0(w), T0(tw), T0(dx), T0(tdx), C);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// d-vector speaker encoder kernels (dvector.h), each through the launcher DVector::forward / backward use.  No scratch: `ws` is not needed.
// Shapes: dvec_bad_shape, the predicate of DVector::init (H a multiple of 64 in 64 .. 1024, E a multiple of 4 in 4 .. 256, T, N, B >= 1).
// lstm_recurrent: xp [N][T][4H] gate pre-activations from the input (biases included; gate order i, f, g, o), whhT [H][4H] the TRANSPOSED
// recurrent weight -> hlast [N][H], hseq [N][T][H] (or null) and, for a training pass, gates [N][T][4H] (after their non-linearities),
// cseq [N][T][H], hprev [N][T][H] — all three or none.
int mtts_lstm_recurrent(int N, int T, int H, const float* xp, const float* whhT, float* hseq, float* hlast, float* gates, float* cseq, float* hprev,
                        void* stream) {
    const int kept = (gates != nullptr) + (cseq != nullptr) + (hprev != nullptr);
    if (dvec_bad_shape(H, 4, T, N) || !xp || !whhT || !hlast || (kept != 0 && kept != 3)) return -1;
    launch_lstm_recurrent(N, T, H, xp, whhT, hseq, hlast, gates, cseq, hprev, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// BPTT of one layer on the gates / cseq of the launch above: dh_ext [N][T][H] (gradient reaching every h_t from above, or null), dh_last
// [N][H] (gradient of the final hidden state, or null), whh [4H][H] in torch's layout -> dgates [N][T][4H], the gradient of the gate pre-activations
int mtts_lstm_bptt(int N, int T, int H, const float* gates, const float* cseq, const float* dh_ext, const float* dh_last, const float* whh,
                   float* dgates, void* stream) {
    if (dvec_bad_shape(H, 4, T, N) || !gates || !cseq || !whh || !dgates) return -1;
    launch_lstm_bptt(N, T, H, gates, cseq, dh_ext, dh_last, whh, dgates, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// head: raw = relu(hlast W^T + bias), part = raw / ||raw||  (hlast [N][H], wT [H][E] the TRANSPOSED Linear weight, part [N][E], eraw [N][E] = raw or null)
int mtts_dvec_head(int N, int H, int E, const float* hlast, const float* wT, const float* bias, float* part, float* eraw, void* stream) {
    if (dvec_bad_shape(H, E, 1, N) || !hlast || !wT || !bias || !part) return -1;
    launch_dvec_head(N, H, E, hlast, wT, bias, part, eraw, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// its backward: dpart [N][E] -> dz [N][E] (gradient of the Linear output) and dh_last [N][H] = dz W  (w [E][H] in torch's layout)
int mtts_dvec_head_bwd(int N, int H, int E, const float* eraw, const float* dpart, const float* w, float* dz, float* dh_last, void* stream) {
    if (dvec_bad_shape(H, E, 1, N) || !eraw || !dpart || !w || !dz || !dh_last) return -1;
    launch_dvec_head_bwd(N, H, E, eraw, dpart, w, dz, dh_last, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// utterance b: out[b] = m / max(||m||, 1e-12), m = mean of part[off[b] .. off[b + 1]); off [B + 1] DEVICE ints, non-decreasing (not read
// here: the caller's part / dpart hold off[B] rows)
int mtts_dvec_utterance(int B, int E, const float* part, const int* off, float* out, void* stream) {
    if (dvec_bad_shape(64, E, 1, B) || !part || !off || !out) return -1;
    launch_dvec_utterance(B, E, part, off, out, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// its backward: dout [B][E] -> dpart [off[B]][E] (an utterance without partials writes nothing)
int mtts_dvec_utterance_bwd(int B, int E, const float* part, const int* off, const float* dout, float* dpart, void* stream) {
    if (dvec_bad_shape(64, E, 1, B) || !part || !off || !dout || !dpart) return -1;
    launch_dvec_utterance_bwd(B, E, part, off, dout, dpart, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// GE2E loss and its backward (ge2e.h; the definition: include/mtts.h).  emb [n_spk * n_utt][E] speaker-major, loss3 [3] = L, dL/dw, dL/db,
// demb [n_spk * n_utt][E], sim [n_spk * n_utt][n_spk] or null, ws of mtts_ge2e_ws_bytes bytes — all on the device.  Four launches, nothing
// copied.  A refusal launches nothing and leaves its reason, with the argument named, where mtts_dvector_last_error(NULL) reads it.
size_t mtts_ge2e_ws_bytes(int n_spk, int n_utt, int E) {
    return ge2e_bad_shape(n_spk, n_utt, E, 1.f) ? 0 : ge2e_ws_bytes((long long)n_spk * n_utt, n_spk, E);
}
int mtts_ge2e_loss(int n_spk, int n_utt, int E, const float* emb, float w, float b, float* loss3, float* demb, float* sim, void* ws, size_t ws_bytes,
                   void* stream) {
    const char* bad = ge2e_bad_shape(n_spk, n_utt, E, w);
    if (!bad && !emb) bad = "emb is NULL";
    if (!bad && !loss3) bad = "loss3 is NULL";
    if (!bad && !demb) bad = "demb is NULL";
    if (!bad && !ws) bad = "ws is NULL";
    if (!bad && ws_bytes < ge2e_ws_bytes((long long)n_spk * n_utt, n_spk, E)) bad = "ws_bytes is smaller than mtts_ge2e_ws_bytes";
    if (bad) { g_create_error = std::string("mtts_ge2e_loss: ") + bad; return -1; }
    launch_ge2e_loss(n_spk, n_utt, E, emb, Ge2eScal{nullptr, w, b}, loss3, loss3 + 1, demb, sim, ge2e_carve(ws, (long long)n_spk * n_utt, n_spk, E),
                     (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- Multi-task entries of the loss, optimizer and variance-adaptor row kernels (rowops.h), each through the kernel's one launcher.  What the
// one-task entries above cannot show is pinned here: blockIdx.z * stride addressing and the per-task row count of a ragged launch.  `tasks` in
// 1 .. 8; rows[t] (HOST ints, >= 0, the largest >= 1) is task t's row count; ts[] (HOST int64, elements, >= 0) holds one task stride per array
// in the order each entry documents; per-row arrays (masks, index lists) of one entry share the "row" stride.  `ws` = mtts_kernel_ws_bytes(largest
// row count, 0) bytes.  Nothing is checked against the callers' allocation sizes: task t of an array spans [t * stride, t * stride + its extent).
namespace {
constexpr int kApiTasks = 8;   // the 256-byte meta block of KernelWs holds 8 x META_STRIDE ints
inline int max_of(int tasks, const int* n) { int m = 0; for (int t = 0; t < tasks; ++t) m = std::max(m, n[t]); return m; }
inline bool bad_tasks(int tasks, const int* n) {
    if (tasks < 1 || tasks > kApiTasks || !n) return true;
    for (int t = 0; t < tasks; ++t) if (n[t] < 0) return true;
    return max_of(tasks, n) < 1;
}
inline bool bad_strides(const int64_t* ts, int n) {
    if (!ts) return true;
    for (int i = 0; i < n; ++i) if (ts[i] < 0) return true;
    return false;
}
// per-task meta table from the arguments: B, Mp, Mf, Mr, nP, nF independent per task (Smax = Mp, Tcap = Mr: not read by these kernels)
inline int put_meta_tasks(const KernelWs& k, int tasks, const int* B, const int* Mp, const int* Mf, const int* Mr, const int* nP, const int* nF) {
    int m[kApiTasks * META_STRIDE] = {0};
    for (int t = 0; t < tasks; ++t) {
        int* q = m + t * META_STRIDE;
        q[META_B] = B[t]; q[META_SMAX] = Mp[t]; q[META_TCAP] = Mr[t]; q[META_MP] = Mp[t]; q[META_MF] = Mf[t]; q[META_MR] = Mr[t]; q[META_NP] = nP[t]; q[META_NF] = nF[t];
    }
    return hipMemcpy(k.meta, m, sizeof(m), hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
// every count field of task t = rows[t]
inline int put_meta_rows(const KernelWs& k, int tasks, const int* rows) { return put_meta_tasks(k, tasks, rows, rows, rows, rows, rows, rows); }
inline RowLaunch n_tasks(const KernelWs& k, int tasks, const int* rows, int mfield, const unsigned char* mask, int64_t row_ts, void* stream) {
    return RowLaunch{k.meta, mfield, max_of(tasks, rows), tasks, mask, (long long)row_ts, (hipStream_t)stream};
}
inline TS TT(const float* p, int64_t ts) { return TS{const_cast<float*>(p), (long long)ts}; }
inline bool bad_rows_tasks(int tasks, const int* rows, int C) { return bad_tasks(tasks, rows) || C < 4 || (C & 3) || C > 1024; }
inline int api_rc() { return hipGetLastError() == hipSuccess ? 0 : -1; }
}  // namespace

// out[row] = valid ? emb[tok[row]] + pos[row_t[row]] : 0 (pos shared by the tasks).  ts: emb, row, out
int mtts_rows_embed_pos(int tasks, const int* rows, int C, const float* emb, const float* pos, const int* tok, const int* row_t, const unsigned char* valid,
                        float* out, const int64_t* ts, void* ws, void* stream) {
    if (bad_rows_tasks(tasks, rows, C) || bad_strides(ts, 3) || !emb || !pos || !tok || !row_t || !valid || !out || !ws) return -1;
    const KernelWs k = carve(ws, max_of(tasks, rows), 0);
    if (put_meta_rows(k, tasks, rows)) return -1;
    launch_embed_pos(n_tasks(k, tasks, rows, META_MP, valid, ts[1], stream), TT(out, ts[2]), TT(emb, ts[0]), pos, tok, row_t, C);
    return api_rc();
}
// spk[b] = table[ids[b]] (average 0) or the mean of table[ids[0 .. n)] with n = ids[n_ids_max] (average 1), for b < B[t].  ts: table, ids, spk
int mtts_rows_speaker_vec(int tasks, const int* B, int C, const float* table, const int* ids, int n_ids_max, int average, float* spk, const int64_t* ts,
                          void* ws, void* stream) {
    if (bad_rows_tasks(tasks, B, C) || bad_strides(ts, 3) || n_ids_max < 1 || !table || !ids || !spk || !ws) return -1;
    const KernelWs k = carve(ws, max_of(tasks, B), 0);
    if (put_meta_rows(k, tasks, B)) return -1;
    launch_speaker_vec(n_tasks(k, tasks, B, META_B, nullptr, 0, stream), max_of(tasks, B), TT(table, ts[0]), ids, ts[1], n_ids_max, average, TT(spk, ts[2]), C);
    return api_rc();
}
// its transpose: dtable [n_speaker][C] fully written per task.  ts: dspk, ids, dtable
int mtts_rows_speaker_table_grad(int tasks, const int* B, int C, int n_speaker, const float* dspk, const int* ids, int n_ids_max, int average, float* dtable,
                                 const int64_t* ts, void* ws, void* stream) {
    if (bad_rows_tasks(tasks, B, C) || bad_strides(ts, 3) || n_ids_max < 1 || n_speaker < 1 || !dspk || !ids || !dtable || !ws) return -1;
    const KernelWs k = carve(ws, max_of(tasks, B), 0);
    if (put_meta_rows(k, tasks, B)) return -1;
    launch_speaker_table_grad(n_tasks(k, tasks, B, META_B, nullptr, 0, stream), n_speaker, TT(dspk, ts[0]), ids, ts[1], n_ids_max, average, TT(dtable, ts[2]), C);
    return api_rc();
}
// out[row] = inrect ? x[row] + vec[row_b[row]] : 0.  ts: x, vec, row, out
int mtts_rows_add_rowvec(int tasks, const int* rows, int C, const float* x, const float* vec, const int* row_b, const unsigned char* inrect, float* out,
                         const int64_t* ts, void* ws, void* stream) {
    if (bad_rows_tasks(tasks, rows, C) || bad_strides(ts, 4) || !x || !vec || !row_b || !inrect || !out || !ws) return -1;
    const KernelWs k = carve(ws, max_of(tasks, rows), 0);
    if (put_meta_rows(k, tasks, rows)) return -1;
    launch_add_rowvec(n_tasks(k, tasks, rows, META_MP, inrect, ts[2], stream), TT(x, ts[0]), TT(vec, ts[1]), row_b, TT(out, ts[3]), C);
    return api_rc();
}
// out[row] = inrect ? x[row] + table[bucketize(val[row] * control, bins[nb])] : 0, idx_out[row] = the bucket or -1 (bins shared by the tasks).
// ts: x, val, table, row, out
int mtts_rows_bucket_embed_add(int tasks, const int* rows, int C, const float* x, const float* val, float control, const float* bins, int nb,
                               const float* table, const unsigned char* inrect, int* idx_out, float* out, const int64_t* ts, void* ws, void* stream) {
    if (bad_rows_tasks(tasks, rows, C) || bad_strides(ts, 5) || nb < 1 || !x || !val || !bins || !table || !inrect || !idx_out || !out || !ws) return -1;
    const KernelWs k = carve(ws, max_of(tasks, rows), 0);
    if (put_meta_rows(k, tasks, rows)) return -1;
    launch_bucket_embed_add(n_tasks(k, tasks, rows, META_MP, inrect, ts[3], stream), TT(x, ts[0]), TT(val, ts[1]), control, bins, nb, TT(table, ts[2]), idx_out,
                            TT(out, ts[4]), C);
    return api_rc();
}
// out[row] = valid ? dot(x[row], w) + b : 0; w [C] and b [1] share the "par" stride.  ts: x, par, row, out
int mtts_rows_rowdot(int tasks, const int* rows, int C, const float* x, const float* w, const float* b, const unsigned char* valid, float* out,
                     const int64_t* ts, void* ws, void* stream) {
    if (bad_rows_tasks(tasks, rows, C) || bad_strides(ts, 4) || !x || !w || !b || !valid || !out || !ws) return -1;
    const KernelWs k = carve(ws, max_of(tasks, rows), 0);
    if (put_meta_rows(k, tasks, rows)) return -1;
    launch_rowdot(n_tasks(k, tasks, rows, META_MP, valid, ts[2], stream), TT(x, ts[0]), TT(w, ts[1]), TT(b, ts[1]), TT(out, ts[3]), C);
    return api_rc();
}
// dx[row] = dout[row] * w.  ts: dout, par, dx
int mtts_rows_rowdot_bwd(int tasks, const int* rows, int C, const float* dout, const float* w, float* dx, const int64_t* ts, void* ws, void* stream) {
    if (bad_rows_tasks(tasks, rows, C) || bad_strides(ts, 3) || !dout || !w || !dx || !ws) return -1;
    const KernelWs k = carve(ws, max_of(tasks, rows), 0);
    if (put_meta_rows(k, tasks, rows)) return -1;
    launch_rowdot_bwd(n_tasks(k, tasks, rows, META_MP, nullptr, 0, stream), TT(dout, ts[0]), TT(w, ts[1]), TT(dx, ts[2]), C);
    return api_rc();
}
// out[b] (+)= sum of the rows [start[b], start[b] + len[b]) of X, for b < B[t].  ts: X, seg (start / len), out
int mtts_rows_segsum(int tasks, const int* B, int C, const float* X, const int* start, const int* len, float* out, int accumulate, const int64_t* ts,
                     void* ws, void* stream) {
    if (bad_rows_tasks(tasks, B, C) || bad_strides(ts, 3) || !X || !start || !len || !out || !ws) return -1;
    const KernelWs k = carve(ws, max_of(tasks, B), 0);
    if (put_meta_rows(k, tasks, B)) return -1;
    launch_segsum_rows(n_tasks(k, tasks, B, META_B, nullptr, 0, stream), max_of(tasks, B), TT(X, ts[0]), start, len, ts[1], TT(out, ts[2]), C, accumulate);
    return api_rc();
}
// d_rounded[row] = max(round(exp(logd[row]) - 1) * d_control, 0); logd and d_rounded share the stride.  ts: pred
int mtts_rows_duration_round(int tasks, const int* rows, const float* logd, float d_control, float* d_rounded, const int64_t* ts, void* ws, void* stream) {
    if (bad_tasks(tasks, rows) || bad_strides(ts, 1) || !logd || !d_rounded || !ws) return -1;
    const KernelWs k = carve(ws, max_of(tasks, rows), 0);
    if (put_meta_rows(k, tasks, rows)) return -1;
    launch_duration_round(k.meta, tasks, TT(logd, ts[0]), d_control, nullptr, 0, d_rounded, (hipStream_t)stream);
    return api_rc();
}
// in place on X: rows with valid == 0 become bias (inrect != 0) or 0; valid rows are left alone.  ts: X, bias, row
int mtts_rows_fill_padded(int tasks, const int* rows, int C, float* X, const float* bias, const unsigned char* inrect, const unsigned char* valid,
                          const int64_t* ts, void* ws, void* stream) {
    if (bad_rows_tasks(tasks, rows, C) || bad_strides(ts, 3) || !X || !bias || !inrect || !valid || !ws) return -1;
    const KernelWs k = carve(ws, max_of(tasks, rows), 0);
    if (put_meta_rows(k, tasks, rows)) return -1;
    launch_fill_padded_rows(n_tasks(k, tasks, rows, META_MR, inrect, ts[2], stream), TT(X, ts[0]), TT(bias, ts[1]), valid, C);
    return api_rc();
}
// out[row] = rowmap[row] >= 0 ? src[rowmap[row]] : 0.  ts: src, row (rowmap), out
int mtts_rows_gather(int tasks, const int* rows, int C, const float* src, const int* rowmap, float* out, const int64_t* ts, void* ws, void* stream) {
    if (bad_rows_tasks(tasks, rows, C) || bad_strides(ts, 3) || !src || !rowmap || !out || !ws) return -1;
    const KernelWs k = carve(ws, max_of(tasks, rows), 0);
    if (put_meta_rows(k, tasks, rows)) return -1;
    launch_gather_rows(n_tasks(k, tasks, rows, META_MP, nullptr, ts[1], stream), TT(src, ts[0]), rowmap, TT(out, ts[2]), C);
    return api_rc();
}
// out[row] = x[f_src[r2f[row]]] where r2f[row] >= 0 and f_src[..] >= 0, else 0.  ts: x, f (f_src), row (r2f), out
int mtts_rows_length_regulate_rect(int tasks, const int* rows, int C, const float* x, const int* f_src, const int* r2f, float* out, const int64_t* ts,
                                   void* ws, void* stream) {
    if (bad_rows_tasks(tasks, rows, C) || bad_strides(ts, 4) || !x || !f_src || !r2f || !out || !ws) return -1;
    const KernelWs k = carve(ws, max_of(tasks, rows), 0);
    if (put_meta_rows(k, tasks, rows)) return -1;
    launch_length_regulate_rect(n_tasks(k, tasks, rows, META_MR, nullptr, ts[2], stream), TT(x, ts[0]), f_src, ts[1], r2f, TT(out, ts[3]), C);
    return api_rc();
}

// The 5-term loss (loss.py:19-92) and its gradient.  Per task: Mr mel rows of which nF have rvalid != 0, Mp phoneme rows of which nP have
// pvalid != 0 (the caller states nF / nP: they are the divisors).  ptr[15] (HOST array of device pointers): mel, mel_post, mel_tgt [Mr][n_mel];
// rvalid [Mr] (bytes); pp, ep, logd (predictions [Mp]); p_tgt, e_tgt [Mp]; dur [Mp] (ints); pvalid [Mp] (bytes); pp_r, ep_r (frame-level
// predictions [Mr]), p_tgt_r, e_tgt_r [Mr] — the last four may be NULL unless their level is frame.  ts: mel, rrow (rvalid, *_tgt_r), prow
// (pvalid, dur, p_tgt, e_tgt), pred (pp, ep, logd and their gradients), pred_r (pp_r, ep_r and their gradients).
namespace {
inline bool loss_setup(int tasks, const int* Mr, const int* Mp, const int* nF, const int* nP, int n_mel, int pitch_frame, int energy_frame,
                       const void* const* ptr, const int64_t* ts, void* ws, KernelWs& k, LossArgs& a) {
    if (bad_tasks(tasks, Mr) || bad_tasks(tasks, Mp) || !nF || !nP || n_mel < 4 || (n_mel & 3) || n_mel > 1024 || !ptr || bad_strides(ts, 5) || !ws) return false;
    for (int t = 0; t < tasks; ++t) if (nF[t] < 1 || nF[t] > Mr[t] || nP[t] < 1 || nP[t] > Mp[t]) return false;
    for (int i = 0; i < 11; ++i) if (!ptr[i]) return false;
    if (pitch_frame && (!ptr[11] || !ptr[13])) return false;
    if (energy_frame && (!ptr[12] || !ptr[14])) return false;
    if ((long long)tasks * kLossBlocks * 5 > 3 * 1024) return false;   // the partial sums live in the scratch block's column partials
    k = carve(ws, std::max(max_of(tasks, Mr), max_of(tasks, Mp)), 0);
    if (put_meta_tasks(k, tasks, Mp, Mp, Mr, Mr, nP, nF)) return false;
    a.mel = (const float*)ptr[0]; a.mel_post = (const float*)ptr[1]; a.mel_tgt = (const float*)ptr[2]; a.rvalid = (const unsigned char*)ptr[3];
    a.pp = (const float*)ptr[4]; a.ep = (const float*)ptr[5]; a.logd = (const float*)ptr[6]; a.p_tgt = (const float*)ptr[7]; a.e_tgt = (const float*)ptr[8];
    a.dur = (const int*)ptr[9]; a.pvalid = (const unsigned char*)ptr[10];
    a.pp_r = (const float*)ptr[11]; a.ep_r = (const float*)ptr[12]; a.p_tgt_r = (const float*)ptr[13]; a.e_tgt_r = (const float*)ptr[14];
    a.mel_ts = ts[0]; a.rrow_ts = ts[1]; a.prow_ts = ts[2]; a.pred_ts = ts[3]; a.pred_r_ts = ts[4];
    a.n_mel = n_mel; a.pitch_frame = pitch_frame ? 1 : 0; a.energy_frame = energy_frame ? 1 : 0;
    return true;
}
}  // namespace
// losses [tasks][6] = total, mel, postnet mel, pitch, energy, duration (partial + final)
int mtts_rows_loss(int tasks, const int* Mr, const int* Mp, const int* nF, const int* nP, int n_mel, int pitch_frame, int energy_frame,
                   const void* const* ptr, const int64_t* ts, float* losses, void* ws, void* stream) {
    KernelWs k; LossArgs a;
    if (!losses || !loss_setup(tasks, Mr, Mp, nF, nP, n_mel, pitch_frame, energy_frame, ptr, ts, ws, k, a)) return -1;
    launch_loss_partial(k.meta, tasks, a, k.col_partial, (hipStream_t)stream);
    launch_loss_final(k.meta, tasks, k.col_partial, n_mel, losses, a.pitch_frame, a.energy_frame, (hipStream_t)stream);
    return api_rc();
}
// scale * d(total)/d(prediction): dmel, dpost (mel stride), dpp, dep, dlogd (pred stride), dpp_r, dep_r (pred_r stride; NULL unless frame-level)
int mtts_rows_loss_grad(int tasks, const int* Mr, const int* Mp, const int* nF, const int* nP, int n_mel, int pitch_frame, int energy_frame,
                        const void* const* ptr, const int64_t* ts, float scale, float* dmel, float* dpost, float* dpp, float* dep, float* dlogd, float* dpp_r,
                        float* dep_r, void* ws, void* stream) {
    KernelWs k; LossArgs a;
    if (!dmel || !dpost || !dpp || !dep || !dlogd || (pitch_frame && !dpp_r) || (energy_frame && !dep_r)) return -1;
    if (!loss_setup(tasks, Mr, Mp, nF, nP, n_mel, pitch_frame, energy_frame, ptr, ts, ws, k, a)) return -1;
    launch_loss_grad(k.meta, tasks, a, scale, dmel, dpost, dpp, dep, dlogd, dpp_r, dep_r, (hipStream_t)stream);
    return api_rc();
}

// The flat-array kernels of the optimizer: n4 = number of float4 of one task's array (arrays 16-byte aligned), grid capped by the argument.
// sumsq_norm: out_norm[0] = sqrt(sum g^2 (+ extra[0])) through n_partials (1 .. 4096) workgroup partials [n_partials] (partial + final).
int mtts_sumsq_norm(const float* g, int64_t n4, int n_partials, const float* extra, float* partial, float* out_norm, void* stream) {
    if (!g || n4 < 1 || n_partials < 1 || n_partials > 4096 || !partial || !out_norm) return -1;
    launch_sumsq_partial(g, n4, partial, n_partials, (hipStream_t)stream);
    launch_sumsq_final(partial, n_partials, out_norm, extra, (hipStream_t)stream);
    return api_rc();
}
// clip_grad_norm_(max_norm) (norm[0] on the device; max_norm <= 0: no clip) + torch.optim.Adam step number `step` (>= 1) on w, m, v in place
int mtts_adam_clip(float* w, const float* g, float* m, float* v, int64_t n4, const float* norm, float max_norm, float lr, float b1, float b2, float eps,
                   int step, float weight_decay, int max_blocks, void* stream) {
    if (!w || !g || !m || !v || !norm || n4 < 1 || step < 1 || max_blocks < 1) return -1;
    launch_adam_clip(w, g, m, v, n4, norm, max_norm, lr, b1, b2, eps, adam_bias_correction(b1, step), adam_bias_correction(b2, step), weight_decay,
                     (hipStream_t)stream, (unsigned)max_blocks);
    return api_rc();
}
// w[t] -= lr * g[t] for every task
int mtts_sgd_update(int tasks, float* w, int64_t w_ts, const float* g, int64_t g_ts, int64_t n4, float lr, int max_blocks, void* stream) {
    if (tasks < 1 || tasks > kApiTasks || !w || !g || w_ts < 0 || g_ts < 0 || n4 < 1 || max_blocks < 1) return -1;
    launch_sgd_update(TT(w, w_ts), TT(g, g_ts), n4, lr, tasks, (hipStream_t)stream, (unsigned)max_blocks);
    return api_rc();
}
// out (+)= scale * sum_t g[t], tasks added in ascending order
int mtts_sum_tasks(int tasks, const float* g, int64_t g_ts, float scale, float* out, int64_t n4, int accumulate, int max_blocks, void* stream) {
    if (tasks < 1 || tasks > kApiTasks || !g || !out || g_ts < 0 || n4 < 1 || max_blocks < 1) return -1;
    launch_sum_tasks(TT(g, g_ts), tasks, scale, out, n4, accumulate, (hipStream_t)stream, (unsigned)max_blocks);
    return api_rc();
}
// dst[t] = src for every task
int mtts_broadcast(int tasks, const float* src, float* dst, int64_t dst_ts, int64_t n4, int max_blocks, void* stream) {
    if (tasks < 1 || tasks > kApiTasks || !src || !dst || dst_ts < 0 || n4 < 1 || max_blocks < 1) return -1;
    launch_broadcast(src, TT(dst, dst_ts), n4, tasks, (hipStream_t)stream, (unsigned)max_blocks);
    return api_rc();
}
