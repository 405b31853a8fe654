// d-vector speaker encoder, forward only — the `dvec` speaker mode (config/algorithm/dvec.yaml: `speaker_emb: dvec`, frozen).
//
// Reference: lightning/model/speaker_encoder.py:11-31 (GE2E: nn.LSTM(40, 256, 3, batch_first=True) + nn.Linear(256, 256) + ReLU —
// the architecture of the un-vendored resemblyzer `VoiceEncoder` the `dvec` / `encoder` modes instantiate, :54-60), its forward
// (final hidden state of the last layer -> Linear -> ReLU -> L2 normalisation per partial utterance) and :71-76 (utterance
// embedding = L2-normalised mean of the partial embeddings of that utterance's slice).  The reference runs this encoder on the
// CPU (`VoiceEncoder('cpu')`) in front of every forward of the acoustic model.
//
// MI355X layout: the input projection of a layer is ONE GEMM over all (partial, frame) rows (gemm.h, bias = b_ih + b_hh fused);
// the recurrence runs one workgroup per partial utterance with the hidden state in LDS and the recurrent weights read from L2
// as a transposed image ([H][4H]: thread j of the workgroup owns hidden unit j and reads the four gate columns of every row
// coalesced); all partials advance in parallel, the 1 MB weight image is shared through the L2.  Gate order i, f, g, o (torch).
#pragma once
#include <string>
#include <vector>

#include "ge2e.h"
#include "gemm.h"
#include "params.h"
#include "rowops.h"
#include "tangent.h"

namespace mtts {

__device__ __forceinline__ float dv_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// The shapes the kernels of this file serve: one workgroup of H threads with 2 * 1024 / 4 * 1024 floats of LDS (H a multiple of the wavefront,
// <= 1024), E <= 256 in whole float4 groups (dz_s[256], four wavefront partials; the GEMMs behind dz read rows of E floats as float4),
// T >= 1 frames and n >= 1 workgroups.  DVector::init and the C entries of kernel_api.inc refuse everything else through this one predicate.
inline bool dvec_bad_shape(int H, int E, int T, int n) { return H < 64 || H > 1024 || (H & 63) || E < 4 || E > 256 || (E & 3) || T < 1 || n < 1; }
constexpr int kDvChunk = 32;   // terms per partial sum of the recurrent dot products (H is a multiple of 64)
inline unsigned dvec_emb_block(int E) { return (unsigned)((E + 63) & ~63); }   // workgroup of the head / utterance kernels: E rounded up to whole wavefronts

// xp: [N][T][4H] input projections (biases included); whhT: [H][4H]; hseq: [N][T][H] (all hidden states, the next layer's input);
// hlast: [N][H] final hidden state.  blockDim.x == H.  Training passes also keep what the backward sweep needs: gates [N][T][4H]
// (i, f, g, o AFTER their non-linearities), cseq [N][T][H], hprev [N][T][H] (the hidden state each step started from).
__global__ void lstm_recurrent_kernel(const float* xp, const float* whhT, float* hseq, float* hlast, int T, int H, float* gates, float* cseq,
                                      float* hprev) {
    __shared__ float dv_smem[2 * 1024];   // hidden state, double-buffered (H <= 1024)
    const int n = blockIdx.x, j = threadIdx.x;
    float* h0 = dv_smem;
    float* h1 = dv_smem + H;
    h0[j] = 0.f;
    float c = 0.f, hv = 0.f;
    __syncthreads();
    const float* px = xp + (long long)n * T * 4 * H;
    for (int t = 0; t < T; ++t) {
        const float* hin = (t & 1) ? h1 : h0;
        float* hout = (t & 1) ? h0 : h1;
        float gi = px[(long long)t * 4 * H + j], gf = px[(long long)t * 4 * H + H + j];
        float gg = px[(long long)t * 4 * H + 2 * H + j], go = px[(long long)t * 4 * H + 3 * H + j];
        const float* w = whhT + j;
        // partial sums of kDvChunk terms, added up afterwards: the rounding error grows with kDvChunk + H / kDvChunk terms, not with H
        for (int k0 = 0; k0 < H; k0 += kDvChunk) {
            float si = 0.f, sf = 0.f, sg = 0.f, so = 0.f;
#pragma unroll 4
            for (int k = k0; k < k0 + kDvChunk; ++k) {
                const float hk = hin[k];
                si += w[0] * hk; sf += w[H] * hk; sg += w[2 * H] * hk; so += w[3 * H] * hk;
                w += 4 * H;
            }
            gi += si; gf += sf; gg += sg; go += so;
        }
        gi = dv_sigmoid(gi); gf = dv_sigmoid(gf); gg = tanhf(gg); go = dv_sigmoid(go);
        c = gf * c + gi * gg;
        const long long row = (long long)n * T + t;
        if (gates) {
            float* pg = gates + row * 4 * H;
            pg[j] = gi; pg[H + j] = gf; pg[2 * H + j] = gg; pg[3 * H + j] = go;
            cseq[row * H + j] = c;
            hprev[row * H + j] = hv;
        }
        hv = go * tanhf(c);
        hout[j] = hv;
        if (hseq) hseq[row * H + j] = hv;
        __syncthreads();
    }
    hlast[(long long)n * H + j] = hv;
}
// N partial utterances of T frames; hseq may be null (top layer of an inference pass); gates / cseq / hprev: all three or none
inline void launch_lstm_recurrent(int N, int T, int H, const float* xp, const float* whhT, float* hseq, float* hlast, float* gates, float* cseq,
                                  float* hprev, hipStream_t st) {
    MTTS_LAUNCH(lstm_recurrent_kernel, dim3((unsigned)N), dim3((unsigned)H), st, xp, whhT, hseq, hlast, T, H, gates, cseq, hprev);
}

// Backward sweep of one layer (BPTT), one workgroup per partial utterance, thread j = hidden unit j.  dh_ext [N][T][H]: gradient
// reaching h_t from the layer above (null for the top layer); dh_last [N][H]: gradient of the final hidden state (top layer only,
// else null); whh [4H][H] in torch's layout (row r read coalesced over j).  Writes dgates [N][T][4H]: gradients of the gate
// pre-activations, from which the weight / bias / input gradients are plain GEMMs.
__global__ void lstm_bptt_kernel(const float* gates, const float* cseq, const float* dh_ext, const float* dh_last, const float* whh, float* dgates,
                                 int T, int H) {
    __shared__ float dg_s[4 * 1024];
    const int n = blockIdx.x, j = threadIdx.x;
    float dh_rec = 0.f, dc_next = 0.f;
    for (int t = T - 1; t >= 0; --t) {
        const long long row = (long long)n * T + t;
        const float* pg = gates + row * 4 * H;
        const float gi = pg[j], gf = pg[H + j], gg = pg[2 * H + j], go = pg[3 * H + j];
        const float c = cseq[row * H + j], c_prev = t > 0 ? cseq[(row - 1) * H + j] : 0.f;
        const float tc = tanhf(c);
        float dh = dh_rec;
        if (dh_ext) dh += dh_ext[row * H + j];
        if (dh_last && t == T - 1) dh += dh_last[(long long)n * H + j];
        const float dc = dc_next + dh * go * (1.f - tc * tc);
        const float ai = dc * gg * gi * (1.f - gi), af = dc * c_prev * gf * (1.f - gf);
        const float ag = dc * gi * (1.f - gg * gg), ao = dh * tc * go * (1.f - go);
        dc_next = dc * gf;
        float* po = dgates + row * 4 * H;
        po[j] = ai; po[H + j] = af; po[2 * H + j] = ag; po[3 * H + j] = ao;
        dg_s[j] = ai; dg_s[H + j] = af; dg_s[2 * H + j] = ag; dg_s[3 * H + j] = ao;
        __syncthreads();
        float acc = 0.f;
        const float* w = whh + j;
        for (int r0 = 0; r0 < 4 * H; r0 += kDvChunk) {   // chunked as in the forward: 4H terms
            float sacc = 0.f;
#pragma unroll 4
            for (int r = r0; r < r0 + kDvChunk; ++r) { sacc += dg_s[r] * w[0]; w += H; }
            acc += sacc;
        }
        dh_rec = acc;
        __syncthreads();
    }
}
inline void launch_lstm_bptt(int N, int T, int H, const float* gates, const float* cseq, const float* dh_ext, const float* dh_last, const float* whh,
                             float* dgates, hipStream_t st) {
    MTTS_LAUNCH(lstm_bptt_kernel, dim3((unsigned)N), dim3((unsigned)H), st, gates, cseq, dh_ext, dh_last, whh, dgates, T, H);
}

// e = relu(W h + b), then e / ||e||   (one workgroup per partial utterance, blockDim.x = E rounded up to whole wavefronts; wT: [H][E]);
// eraw (optional): e before the normalisation, for the backward pass
__global__ void dvec_head_kernel(const float* hlast, const float* wT, const float* bias, float* part, int H, int E, float* eraw) {
    __shared__ float dv_smem[1024 + 4];
    const int n = blockIdx.x, j = threadIdx.x;
    for (int k = j; k < H; k += blockDim.x) dv_smem[k] = hlast[(long long)n * H + k];
    __syncthreads();
    float e = 0.f;
    if (j < E) {
        double acc = (double)bias[j];   // (N * E short dot products per launch: float64 accumulation costs nothing here and rounds once)
        for (int k = 0; k < H; ++k) acc += (double)wT[(long long)k * E + j] * (double)dv_smem[k];
        e = acc > 0.0 ? (float)acc : 0.f;
    }
    const float ss = wave_sum(e * e);
    if ((j & 63) == 0) dv_smem[H + (j >> 6)] = ss;   // E <= 256: at most four wavefronts
    __syncthreads();
    float tot = 0.f;
    for (int w = 0; w < (int)(blockDim.x + 63) / 64; ++w) tot += dv_smem[H + w];
    if (j < E) { part[(long long)n * E + j] = e / sqrtf(tot); if (eraw) eraw[(long long)n * E + j] = e; }
}
inline void launch_dvec_head(int N, int H, int E, const float* hlast, const float* wT, const float* bias, float* part, float* eraw, hipStream_t st) {
    MTTS_LAUNCH(dvec_head_kernel, dim3((unsigned)N), dim3(dvec_emb_block(E)), st, hlast, wT, bias, part, H, E, eraw);
}

// backward of the utterance reduction: out_b = m / max(||m||, 1e-12), m = mean of the utterance's partials -> dpart[n] for its partials
__global__ void dvec_utterance_bwd_kernel(const float* part, const int* off, const float* dout, float* dpart, int E) {
    __shared__ float red[2][4];
    const int b = blockIdx.x, j = threadIdx.x;
    const int lo = off[b], hi = off[b + 1];
    if (hi <= lo) return;
    float m = 0.f, d = 0.f;
    if (j < E) {
        for (int n = lo; n < hi; ++n) m += part[(long long)n * E + j];
        m /= (float)(hi - lo);
        d = dout[(long long)b * E + j];
    }
    const float s0 = wave_sum(m * m), s1 = wave_sum(m * d);
    if ((j & 63) == 0) { red[0][j >> 6] = s0; red[1][j >> 6] = s1; }
    __syncthreads();
    float mm = 0.f, md = 0.f;
    for (int w = 0; w < (int)(blockDim.x + 63) / 64; ++w) { mm += red[0][w]; md += red[1][w]; }
    const float nrm = sqrtf(mm);
    float dm;
    if (nrm > 1e-12f) dm = (d - m * md / mm) / nrm;   // d(m / ||m||)
    else dm = d / 1e-12f;                              // clamped branch of F.normalize
    dm /= (float)(hi - lo);
    if (j < E) for (int n = lo; n < hi; ++n) dpart[(long long)n * E + j] = dm;
}
inline void launch_dvec_utterance_bwd(int B, int E, const float* part, const int* off, const float* dout, float* dpart, hipStream_t st) {
    MTTS_LAUNCH(dvec_utterance_bwd_kernel, dim3((unsigned)B), dim3(dvec_emb_block(E)), st, part, off, dout, dpart, E);
}

// backward of the head: y = e / ||e||, e = relu(z): dz [N][E] (gradient of the Linear output) and dh_last [N][H] = dz W  (w: [E][H])
__global__ void dvec_head_bwd_kernel(const float* eraw, const float* dpart, const float* w, float* dz, float* dh_last, int H, int E) {
    __shared__ float dz_s[256];
    __shared__ float red[2][4];
    const int n = blockIdx.x, j = threadIdx.x;
    float e = 0.f, d = 0.f;
    if (j < E) { e = eraw[(long long)n * E + j]; d = dpart[(long long)n * E + j]; }
    const float s0 = wave_sum(e * e), s1 = wave_sum(e * d);
    if ((j & 63) == 0) { red[0][j >> 6] = s0; red[1][j >> 6] = s1; }
    __syncthreads();
    float ee = 0.f, ed = 0.f;
    for (int q = 0; q < (int)(blockDim.x + 63) / 64; ++q) { ee += red[0][q]; ed += red[1][q]; }
    const float nrm = sqrtf(ee);
    float g = 0.f;
    if (j < E) {
        g = (d - e * ed / ee) / nrm;   // through the normalisation
        if (!(e > 0.f)) g = 0.f;       // through the ReLU
        dz[(long long)n * E + j] = g;
        dz_s[j] = g;
    }
    __syncthreads();
    for (int k = j; k < H; k += blockDim.x) {
        float acc = 0.f;
        for (int r = 0; r < E; ++r) acc += dz_s[r] * w[(long long)r * H + k];
        dh_last[(long long)n * H + k] = acc;
    }
}
inline void launch_dvec_head_bwd(int N, int H, int E, const float* eraw, const float* dpart, const float* w, float* dz, float* dh_last, hipStream_t st) {
    MTTS_LAUNCH(dvec_head_bwd_kernel, dim3((unsigned)N), dim3(dvec_emb_block(E)), st, eraw, dpart, w, dz, dh_last, H, E);
}

// utterance b: mean of the partial embeddings [off[b], off[b+1]), then F.normalize (x / max(||x||, 1e-12))
__global__ void dvec_utterance_kernel(const float* part, const int* off, float* out, int E) {
    __shared__ float red[4];
    const int b = blockIdx.x, j = threadIdx.x;
    const int lo = off[b], hi = off[b + 1];
    float m = 0.f;
    if (j < E) {
        for (int n = lo; n < hi; ++n) m += part[(long long)n * E + j];
        m = hi > lo ? m / (float)(hi - lo) : 0.f;
    }
    const float ss = wave_sum(m * m);
    if ((j & 63) == 0) red[j >> 6] = ss;
    __syncthreads();
    float tot = 0.f;
    for (int w = 0; w < (int)(blockDim.x + 63) / 64; ++w) tot += red[w];
    const float nrm = sqrtf(tot);
    if (j < E) out[(long long)b * E + j] = m / (nrm > 1e-12f ? nrm : 1e-12f);
}
inline void launch_dvec_utterance(int B, int E, const float* part, const int* off, float* out, hipStream_t st) {
    MTTS_LAUNCH(dvec_utterance_kernel, dim3((unsigned)B), dim3(dvec_emb_block(E)), st, part, off, out, E);
}

// dst[c][r] = src[r][c]
__global__ void dv_transpose_kernel(const float* src, float* dst, int R, int Cc) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < (long long)R * Cc; i += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(i / Cc), c = (int)(i % Cc);
        dst[(long long)c * R + r] = src[i];
    }
}
inline void launch_dv_transpose(const float* src, float* dst, int R, int Cc, unsigned blocks, hipStream_t st) {   // (grid-stride: any block count)
    MTTS_LAUNCH(dv_transpose_kernel, dim3(blocks), dim3(256), st, src, dst, R, Cc);
}
__global__ void dv_add_kernel(const float* a, const float* b, float* o, int n) {
    for (int i = blockIdx.x * (int)blockDim.x + threadIdx.x; i < n; i += (int)(gridDim.x * blockDim.x)) o[i] = a[i] + b[i];
}
__global__ void dv_fill_kernel(float* o, float v, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) o[i] = v;
}
__global__ void dv_sum_partials_kernel(const float* partial, int n, float* out) {   // out[0] = sum (NOT its root: a term of a joint norm)
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += (double)partial[i];
        out[0] = (float)s;
    }
}

class DVector {
public:
    int n_mels = 40, H = 256, layers = 3, E = 256, cap_N = 0, T = 160, cap_B = 0;
    hipStream_t stream = nullptr;
    std::string last_error;
    GemmCtx gx;
    ParamTable tab;   // grads / adam_m / adam_v mirror its block: the same offsets
    // derived images, rebuilt by load(): transposed recurrent / head weights and the summed biases
    float *whhT = nullptr, *linT = nullptr, *bsum = nullptr;
    float *mels = nullptr, *xp = nullptr, *hseq[2] = {nullptr, nullptr}, *hlast = nullptr, *part = nullptr, *out = nullptr;
    int* off_dev = nullptr;
    bool dirty = true;
    // ---- training state (speaker_emb: encoder / scratch_encoder; allocated by enable_training) ----
    bool train_ready = false;
    std::vector<float*> gates, cseq, hprev, hkeep;   // per layer: [rows][4H], [rows][H], [rows][H], [rows][H] (layer output = next layer's input)
    float *dgates = nullptr, *dxbuf[2] = {nullptr, nullptr}, *eraw = nullptr, *dpart = nullptr, *dz = nullptr, *dh_last = nullptr, *dout = nullptr;
    float *grads = nullptr, *adam_m = nullptr, *adam_v = nullptr, *ones4 = nullptr, *sq_partial = nullptr, *sq_out = nullptr;
    int last_N = 0, last_B = 0, adam_steps = 0;
    bool have_forward = false;
    const float* last_x0 = nullptr;   // the input of the last training forward: the handle's `mels`, or the caller's device stack
    // ---- GE2E training (ge2e.h; allocated by ge2e_enable).  ge2e_wb: four groups of 4 floats — value, gradient, Adam m, Adam v of (w, b, 0, 0):
    // one float4 for launch_adam_clip; NOT entries of `tab`, so the encoder's state dict is what it was ----
    bool ge2e_ready = false, ge2e_have_grad = false;
    void* ge2e_ws = nullptr;
    float *ge2e_wb = nullptr, *ge2e_loss = nullptr, *ge2e_norm = nullptr, *ge2e_sim = nullptr;
    int ge2e_cap_spk = 0;
    std::vector<int> ge2e_off;        // 0 .. max_utts: one partial per utterance

    DevHeap mem;   // every device block of this handle, the scoring workspace included (devres.h)
    int err(const std::string& s) { last_error = s; return -1; }
    void set_error(const std::string& s) { err(s); }
    long long find(const std::string& n) const { return tab.find(n); }
    const float* P(const std::string& n) const { return tab.ptr(n); }
    int in_dim(int l) const { return l == 0 ? n_mels : H; }

    int init(int n_mels_, int hidden, int layers_, int emb, int max_partials, int frames, int max_utts) {
        n_mels = n_mels_; H = hidden; layers = layers_; E = emb; cap_N = max_partials; T = frames; cap_B = max_utts;
        if (n_mels < 4 || (n_mels & 3) || dvec_bad_shape(H, E, T, cap_N < cap_B ? cap_N : cap_B) || layers < 1 || layers > 8) {
            set_error("unsupported d-vector configuration (n_mels % 4, hidden % 64 <= 1024, emb % 4 <= 256)");
            return -1;
        }
        for (int l = 0; l < layers; ++l) {
            const std::string s = std::to_string(l);
            tab.add("lstm.weight_ih_l" + s, 4LL * H * in_dim(l)); tab.add("lstm.weight_hh_l" + s, 4LL * H * H);
            tab.add("lstm.bias_ih_l" + s, 4LL * H); tab.add("lstm.bias_hh_l" + s, 4LL * H);
        }
        tab.add("linear.weight", (long long)E * H); tab.add("linear.bias", E);
        DEV_CHECK(tab.alloc(mem));
        DEV_CHECK(mem.alloc(whhT, (size_t)layers * 4 * H * H * sizeof(float)));
        DEV_CHECK(mem.alloc(linT, (size_t)E * H * sizeof(float)));
        DEV_CHECK(mem.alloc(bsum, (size_t)layers * 4 * H * sizeof(float)));
        const size_t rows = (size_t)cap_N * T;
        DEV_CHECK(mem.alloc(mels, (rows * n_mels + 64) * sizeof(float)));
        DEV_CHECK(mem.alloc(xp, rows * 4 * H * sizeof(float)));
        for (int i = 0; i < 2; ++i) DEV_CHECK(mem.alloc(hseq[i], (rows * H + 64) * sizeof(float)));
        DEV_CHECK(mem.alloc(hlast, (size_t)cap_N * H * sizeof(float)));
        DEV_CHECK(mem.alloc(part, (size_t)cap_N * E * sizeof(float)));
        DEV_CHECK(mem.alloc(out, (size_t)cap_B * E * sizeof(float)));
        DEV_CHECK(mem.alloc(off_dev, (size_t)(cap_B + 1) * sizeof(int)));
        if (gx.alloc_workspace(mem)) return err("out of device memory (split-K workspace)");
        return 0;
    }
    int enable_training() {
        if (train_ready) return 0;
        const size_t rows = (size_t)cap_N * T;
        for (auto* v : {&gates, &cseq, &hprev, &hkeep}) v->resize(layers, nullptr);   // (what an earlier, failed attempt got is taken again below)
        for (int l = 0; l < layers; ++l) {
            DEV_CHECK(mem.alloc(gates[l], (rows * 4 * H + 64) * sizeof(float)));
            DEV_CHECK(mem.alloc(cseq[l], (rows * H + 64) * sizeof(float)));
            DEV_CHECK(mem.alloc(hprev[l], (rows * H + 64) * sizeof(float)));
            DEV_CHECK(mem.alloc(hkeep[l], (rows * H + 64) * sizeof(float)));
        }
        DEV_CHECK(mem.alloc(dgates, (rows * 4 * H + 64) * sizeof(float)));
        for (int i = 0; i < 2; ++i) DEV_CHECK(mem.alloc(dxbuf[i], (rows * H + 64) * sizeof(float)));
        DEV_CHECK(mem.alloc(eraw, (size_t)cap_N * E * sizeof(float)));
        DEV_CHECK(mem.alloc(dpart, (size_t)cap_N * E * sizeof(float)));
        DEV_CHECK(mem.alloc(dz, ((size_t)cap_N * E + 64) * sizeof(float)));
        DEV_CHECK(mem.alloc(dh_last, (size_t)cap_N * H * sizeof(float)));
        DEV_CHECK(mem.alloc(dout, (size_t)cap_B * E * sizeof(float)));
        for (float** p : {&grads, &adam_m, &adam_v}) { DEV_CHECK(mem.alloc(*p, (size_t)tab.n_params * sizeof(float))); DEV_CHECK(hipMemset(*p, 0, (size_t)tab.n_params * sizeof(float))); }
        DEV_CHECK(mem.alloc(ones4, (rows * 4 + 64) * sizeof(float)));
        MTTS_LAUNCH(dv_fill_kernel, dim3(256), dim3(256), stream, ones4, 1.f, (long long)(rows * 4));
        DEV_CHECK(mem.alloc(sq_partial, 512 * sizeof(float)));
        DEV_CHECK(mem.alloc(sq_out, 4 * sizeof(float)));
        DEV_CHECK(hipMemset(sq_out, 0, 4 * sizeof(float)));
        train_ready = true;
        return 0;
    }
    int load(const char* name, const float* host, long long numel) {
        if (!tab.load(name, host, numel, "d-vector", last_error)) return -1;
        dirty = true;
        return 0;
    }
    // transposed images + summed biases, rebuilt on the device whenever the weights changed (load / adam_step)
    int refresh() {
        for (int l = 0; l < layers; ++l) {
            const std::string s = std::to_string(l);
            launch_dv_transpose(P("lstm.weight_hh_l" + s), whhT + (long long)l * 4 * H * H, 4 * H, H, 512, stream);
            MTTS_LAUNCH(dv_add_kernel, dim3(8), dim3(256), stream, P("lstm.bias_ih_l" + s),
                        P("lstm.bias_hh_l" + s), bsum + (long long)l * 4 * H, 4 * H);
        }
        launch_dv_transpose(P("linear.weight"), linT, E, H, 256, stream);
        DEV_CHECK(hipGetLastError());
        dirty = false;
        return 0;
    }
    // mels_host [N][T][n_mels]; utt_off [B+1] partial offsets (utt_off[0] = 0, utt_off[B] = N); out_host [B][E]; part_host [N][E] or null
    int embed(const float* mels_host, int N, const int* utt_off, int B, float* out_host, float* part_host, bool train = false) {
        if (train && !train_ready) { set_error("mtts_dvector_enable_training first"); return -1; }
        if (check_batch(mels_host, N, utt_off, B, out_host) != 0) return -1;
        if (dirty && refresh() != 0) return -1;
        DEV_CHECK(hipMemcpyAsync(mels, mels_host, (size_t)N * T * n_mels * sizeof(float), hipMemcpyHostToDevice, stream));
        if (forward(mels, N, utt_off, B, out_host, part_host, train, 0) != 0) return -1;
        DEV_CHECK(hipStreamSynchronize(stream));
        return 0;
    }
    // The same forward over a partial stack that is already on the device (mels_dev [N][T][n_mels], read in place).  The input
    // projections name their kernel (64x64 tile; no launch queue, no size-dependent choice), so an utterance's d-vector is
    // bit-identical alone, in any batch and under any chunking.  sync = false: the copies to out_host / part_host are only enqueued.
    int forward_device(const float* mels_dev, int N, const int* utt_off, int B, float* out_host, float* part_host, bool sync = true) {
        if (check_batch(mels_dev, N, utt_off, B, out_host) != 0) return -1;
        if (dirty && refresh() != 0) return -1;
        if (forward(mels_dev, N, utt_off, B, out_host, part_host, false, 64) != 0) return -1;
        if (sync) DEV_CHECK(hipStreamSynchronize(stream));
        return 0;
    }
    int check_batch(const float* mels_any, int N, const int* utt_off, int B, const float* out_host) {
        if (!mels_any || !utt_off || !out_host || N < 1 || N > cap_N || B < 1 || B > cap_B) { set_error("bad d-vector arguments"); return -1; }
        if (utt_off[0] != 0 || utt_off[B] != N) { set_error("utterance offsets must cover [0, N)"); return -1; }
        for (int b = 0; b < B; ++b)   // an utterance without partials has no embedding (the reference's mean over an empty slice is NaN)
            if (utt_off[b + 1] <= utt_off[b]) { set_error("every utterance needs at least one partial utterance (offsets must increase)"); return -1; }
        return 0;
    }
    // x0: [N][T][n_mels] on the device; out_host may be null (the GE2E step reads `out` on the device); tile: the input projections' GEMM tile code (0: through the launch queue)
    int forward(const float* x0, int N, const int* utt_off, int B, float* out_host, float* part_host, bool train, int tile) {
        const long long rows = (long long)N * T;
        DEV_CHECK(hipMemcpyAsync(off_dev, utt_off, (size_t)(B + 1) * sizeof(int), hipMemcpyHostToDevice, stream));
        const float* x = x0;
        for (int l = 0; l < layers; ++l) {
            const std::string s = std::to_string(l);
            GemmArgs g;
            g.A = x; g.lda = in_dim(l);
            g.B = P("lstm.weight_ih_l" + s); g.ldb = in_dim(l);
            g.C = xp; g.ldc = 4 * H;
            g.M = (int)rows; g.N = 4 * H; g.K = in_dim(l);
            g.bias = bsum + (long long)l * 4 * H;
            gemm_launch(gx, GEMM_NT, g, (int)rows, 4 * H, 1, stream, tile, 2.0 * rows * 4.0 * H * in_dim(l), 0);
            float* hs = train ? hkeep[l] : ((l + 1 < layers) ? hseq[l & 1] : nullptr);
            launch_lstm_recurrent(N, T, H, xp, whhT + (long long)l * 4 * H * H, hs, hlast, train ? gates[l] : nullptr, train ? cseq[l] : nullptr,
                                  train ? hprev[l] : nullptr, stream);
            x = hs;
        }
        launch_dvec_head(N, H, E, hlast, linT, P("linear.bias"), part, train ? eraw : nullptr, stream);
        if (train) { last_N = N; last_B = B; have_forward = true; last_x0 = x0; }
        launch_dvec_utterance(B, E, part, off_dev, out, stream);
        if (gx.error) { set_error(std::string("GEMM launcher: ") + gx.error); gx.error = nullptr; return -1; }
        DEV_CHECK(hipGetLastError());
        if (out_host) DEV_CHECK(hipMemcpyAsync(out_host, out, (size_t)B * E * sizeof(float), hipMemcpyDeviceToHost, stream));
        if (part_host) DEV_CHECK(hipMemcpyAsync(part_host, part, (size_t)N * E * sizeof(float), hipMemcpyDeviceToHost, stream));
        return 0;
    }

    // ---- training: gradient of the utterance embeddings -> parameter gradients (BPTT), joint-norm term, Adam -------------------
    // TN GEMM dW[M][Ncols] = A[rows][M]^T * B[rows][Ncols]; optional column sums of A (bias gradient) ride along (gemm.h: colsum)
    void wgrad(const float* A, int M, const float* Bm, int Ncols, long long rows, float* dW, float* db) {
        GemmArgs g;
        g.A = A; g.lda = M; g.B = Bm; g.ldb = Ncols; g.C = dW; g.ldc = Ncols;
        g.M = M; g.N = Ncols; g.K = (int)rows;
        if (db) { g.colsum = db; g.colsum_w = ones4; }
        gemm_launch(gx, GEMM_TN, g, M, Ncols, 1, stream, 0, 2.0 * rows * (double)M * Ncols, 0);
    }
    // dout_host [B][E]: gradient of the loss w.r.t. the embeddings returned by the last embed(train = true)
    int backward(const float* dout_host) {
        if (!train_ready || !have_forward || !dout_host) { set_error("d-vector backward without a training forward"); return -1; }
        DEV_CHECK(hipMemcpyAsync(dout, dout_host, (size_t)last_B * E * sizeof(float), hipMemcpyHostToDevice, stream));
        return backward_from_device();
    }
    // the same sweep from the handle's own `dout` [B][E], wherever it was written (the copy above, or the GE2E loss kernels)
    int backward_from_device() {
        if (!train_ready || !have_forward) { set_error("d-vector backward without a training forward"); return -1; }
        const int N = last_N, B = last_B;
        const long long rows = (long long)N * T;
        DEV_CHECK(hipMemsetAsync(grads, 0, (size_t)tab.n_params * sizeof(float), stream));
        launch_dvec_utterance_bwd(B, E, part, off_dev, dout, dpart, stream);
        launch_dvec_head_bwd(N, H, E, eraw, dpart, P("linear.weight"), dz, dh_last, stream);
        wgrad(dz, E, hlast, H, N, grads + find("linear.weight"), grads + find("linear.bias"));
        const float* dh_ext = nullptr;
        for (int l = layers - 1; l >= 0; --l) {
            const std::string s = std::to_string(l);
            launch_lstm_bptt(N, T, H, gates[l], cseq[l], dh_ext, l == layers - 1 ? dh_last : nullptr, P("lstm.weight_hh_l" + s), dgates, stream);
            const float* x = l == 0 ? last_x0 : hkeep[l - 1];
            wgrad(dgates, 4 * H, x, in_dim(l), rows, grads + find("lstm.weight_ih_l" + s), grads + find("lstm.bias_ih_l" + s));
            wgrad(dgates, 4 * H, hprev[l], H, rows, grads + find("lstm.weight_hh_l" + s), nullptr);
            launch_copy_tasks(TS{grads + find("lstm.bias_ih_l" + s), 0}, TS{grads + find("lstm.bias_hh_l" + s), 0}, (long long)H, 1, stream, 4);   // 4H floats = H float4: d b_hh == d b_ih
            if (l > 0) {   // gradient reaching the layer below: dx = dgates W_ih  ([rows][4H] x [4H][H])
                float* dx = dxbuf[l & 1];
                GemmArgs g;
                g.A = dgates; g.lda = 4 * H; g.B = P("lstm.weight_ih_l" + s); g.ldb = H; g.C = dx; g.ldc = H;
                g.M = (int)rows; g.N = H; g.K = 4 * H;
                gemm_launch(gx, GEMM_NN, g, (int)rows, H, 1, stream, 0, 2.0 * rows * 4.0 * H * H, 0);
                dh_ext = dx;
            }
        }
        // (a refused GEMM launch would leave its gradient at the zeros of the memset above: report it, and keep the forward's state for another try)
        if (gx.error) { set_error(std::string("GEMM launcher: ") + gx.error); gx.error = nullptr; return -1; }
        DEV_CHECK(hipGetLastError());
        have_forward = false;
        return 0;
    }
    // device scalar: sum of squares of the parameter gradients (a term of the joint clip_grad_norm_, main.py:61)
    const float* grad_sumsq() {
        launch_sumsq_partial(grads, tab.n_params / 4, sq_partial, 64, stream);
        MTTS_LAUNCH(dv_sum_partials_kernel, dim3(1), dim3(64), stream, (const float*)sq_partial, 64, sq_out);
        return sq_out;
    }
    // norm_dev: device scalar holding the JOINT gradient norm (the engine's, with this encoder's term added); Adam as optimizer.py:9-15
    int adam_step(const float* norm_dev, float max_norm, float lr, float b1, float b2, float eps, float weight_decay) {
        if (!train_ready) { set_error("mtts_dvector_enable_training first"); return -1; }
        ++adam_steps;
        const float bc1 = 1.f - (float)std::pow((double)b1, (double)adam_steps), bc2 = 1.f - (float)std::pow((double)b2, (double)adam_steps);
        launch_adam_clip(tab.data, grads, adam_m, adam_v, tab.n_params / 4, norm_dev, norm_dev ? max_norm : 0.f, lr, b1, b2, eps, bc1, bc2, weight_decay, stream, 256);
        DEV_CHECK(hipGetLastError());
        dirty = true;
        return 0;
    }

    // ---- GE2E: loss + backward + optimizer step without leaving the device (ge2e.h) ---------------------------------------------------
    // needs enable_training; sizes the loss scratch for any N x M <= max_utts (N <= max_utts / 2 at M = 2)
    int ge2e_enable(float w0, float b0) {
        if (!train_ready) return err("mtts_dvector_enable_training first");
        ge2e_cap_spk = cap_B / 2 < GE2E_MAX_SPK ? cap_B / 2 : GE2E_MAX_SPK;
        if (const char* bad = ge2e_bad_shape(ge2e_cap_spk < 2 ? 2 : ge2e_cap_spk, 2, E, w0)) return err(std::string("mtts_dvector_ge2e_enable: ") + bad);
        if (cap_B < 4) return err("mtts_dvector_ge2e_enable: max_utts must hold 2 speakers x 2 utterances");
        if (!ge2e_ready) {
            DEV_CHECK(mem.alloc(ge2e_ws, ge2e_ws_bytes(cap_B, ge2e_cap_spk, E)));
            DEV_CHECK(mem.alloc(ge2e_wb, 16 * sizeof(float)));
            DEV_CHECK(mem.alloc(ge2e_loss, 4 * sizeof(float)));
            DEV_CHECK(mem.alloc(ge2e_norm, 4 * sizeof(float)));
            DEV_CHECK(mem.alloc(ge2e_sim, (size_t)cap_B * ge2e_cap_spk * sizeof(float)));
            ge2e_off.resize(cap_B + 1);
            for (int i = 0; i <= cap_B; ++i) ge2e_off[i] = i;
        }
        const float init[16] = {w0, b0};
        DEV_CHECK(hipStreamSynchronize(stream));
        DEV_CHECK(hipMemcpy(ge2e_wb, init, sizeof(init), hipMemcpyHostToDevice));
        ge2e_ready = true;
        ge2e_have_grad = false;
        return 0;
    }
    // mels_any [N M][T][n_mels], speaker-major, on the host or (on_device) already on the device; one partial per utterance.  Enqueued on the
    // handle's stream; synchronises only when loss_host [1] or sim_host [N M][N] is given.
    int ge2e_forward_backward(const float* mels_any, bool on_device, int N, int M, float* loss_host, float* sim_host) {
        if (!ge2e_ready) return err("mtts_dvector_ge2e_enable first");
        if (!mels_any) return err("mtts_dvector_ge2e_forward_backward: mels is NULL");
        if (const char* bad = ge2e_bad_shape(N, M, E, 1.f)) return err(std::string("mtts_dvector_ge2e_forward_backward: ") + bad);
        const int B = N * M;
        if (B > cap_B) return err("mtts_dvector_ge2e_forward_backward: n_spk * n_utt exceeds max_utts");
        if (B > cap_N) return err("mtts_dvector_ge2e_forward_backward: n_spk * n_utt exceeds max_partials");
        if (dirty && refresh() != 0) return -1;
        const float* x0 = mels_any;
        if (!on_device) {
            DEV_CHECK(hipMemcpyAsync(mels, mels_any, (size_t)B * T * n_mels * sizeof(float), hipMemcpyHostToDevice, stream));
            x0 = mels;
        }
        if (forward(x0, B, ge2e_off.data(), B, nullptr, nullptr, true, 0) != 0) return -1;
        launch_ge2e_loss(N, M, E, out, Ge2eScal{ge2e_wb, 0.f, 0.f}, ge2e_loss, ge2e_wb + 4, dout, sim_host ? ge2e_sim : nullptr, ge2e_carve(ge2e_ws, B, N, E), stream);
        if (backward_from_device() != 0) return -1;
        ge2e_have_grad = true;
        if (loss_host) DEV_CHECK(hipMemcpyAsync(loss_host, ge2e_loss, sizeof(float), hipMemcpyDeviceToHost, stream));
        if (sim_host) DEV_CHECK(hipMemcpyAsync(sim_host, ge2e_sim, (size_t)B * N * sizeof(float), hipMemcpyDeviceToHost, stream));
        if (loss_host || sim_host) DEV_CHECK(hipStreamSynchronize(stream));
        return 0;
    }
    // scale dw / db, joint norm of every gradient on the device, clip + Adam on the encoder and on (w, b) with the same step count
    int ge2e_step(float lr, float b1, float b2, float eps, float max_norm, float scalar_grad_scale) {
        if (!ge2e_ready) return err("mtts_dvector_ge2e_enable first");
        if (!ge2e_have_grad) return err("mtts_dvector_ge2e_step without mtts_dvector_ge2e_forward_backward");
        const float* sumsq = grad_sumsq();
        float *gwb = ge2e_wb + 4, *norm = ge2e_norm;
        MTTS_LAUNCH(ge2e_joint_norm_kernel, dim3(1), dim3(64), stream, sumsq, gwb, scalar_grad_scale, norm);
        if (adam_step(ge2e_norm, max_norm, lr, b1, b2, eps, 0.f) != 0) return -1;
        const float bc1 = 1.f - (float)std::pow((double)b1, (double)adam_steps), bc2 = 1.f - (float)std::pow((double)b2, (double)adam_steps);
        launch_adam_clip(ge2e_wb, ge2e_wb + 4, ge2e_wb + 8, ge2e_wb + 12, 1, ge2e_norm, max_norm, lr, b1, b2, eps, bc1, bc2, 0.f, stream, 1);
        DEV_CHECK(hipGetLastError());
        ge2e_have_grad = false;
        return 0;
    }
    // which: 0 value, 1 gradient, 2 Adam m, 3 Adam v of (w, b)
    int ge2e_get(int which, float* wb2_host) {
        if (!ge2e_ready) return err("mtts_dvector_ge2e_enable first");
        if (which < 0 || which > 3 || !wb2_host) return err("mtts_dvector_ge2e_get: which must be 0 .. 3 and the output not NULL");
        DEV_CHECK(hipStreamSynchronize(stream));
        DEV_CHECK(hipMemcpy(wb2_host, ge2e_wb + 4 * which, 2 * sizeof(float), hipMemcpyDeviceToHost));
        return 0;
    }
    int ge2e_set(int which, const float* wb2_host) {
        if (!ge2e_ready) return err("mtts_dvector_ge2e_enable first");
        if (which < 0 || which > 3 || !wb2_host) return err("mtts_dvector_ge2e_set: which must be 0 .. 3 and the input not NULL");
        if (which == 0)
            if (const char* bad = ge2e_bad_shape(2, 2, E, wb2_host[0])) return err(std::string("mtts_dvector_ge2e_set: ") + bad);
        DEV_CHECK(hipStreamSynchronize(stream));
        DEV_CHECK(hipMemcpy(ge2e_wb + 4 * which, wb2_host, 2 * sizeof(float), hipMemcpyHostToDevice));
        return 0;
    }
    // which: 0 parameter, 1 gradient, 2 Adam m, 3 Adam v
    float* state_ptr(int which) { return which == 0 ? tab.data : which == 1 ? grads : which == 2 ? adam_m : which == 3 ? adam_v : nullptr; }
    int export_state(const char* name, int which, float* out_host, long long numel) {
        float* base = state_ptr(which);
        if (!base) return err("state not available (enable training first)");
        const ParamTable::Tensor* t = tab.check(name, numel, "d-vector", last_error);
        if (!t) return -1;
        DEV_CHECK(hipStreamSynchronize(stream));
        DEV_CHECK(hipMemcpy(out_host, base + t->off, (size_t)numel * sizeof(float), hipMemcpyDeviceToHost));
        return 0;
    }
    int import_state(const char* name, int which, const float* host, long long numel) {
        if (which == 0) return load(name, host, numel);
        float* base = state_ptr(which);
        if (!base) return err("state not available (enable training first)");
        const ParamTable::Tensor* t = tab.check(name, numel, "d-vector", last_error);
        if (!t) return -1;
        DEV_CHECK(hipMemcpy(base + t->off, host, (size_t)numel * sizeof(float), hipMemcpyHostToDevice));
        return 0;
    }
};

}  // namespace mtts
