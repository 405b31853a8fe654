// MOSNet (CNN-BLSTM; Lo et al. 2019) in inference mode: magnitude spectrograms -> frame scores and utterance scores — DESIGN.md
// section 1 row f13, the naturalness score of the evaluation stage.
//
// Reference call site: evaluation/compute_mos.py (NeuralMOS.compute_mosnet: speechmetrics' MOSNet on one wav file at a time on the
// CPU).  Neither speechmetrics, its TensorFlow model code nor cnn_blstm.h5 is in the reference tree: the network below is the published
// one, stated in full in include/mtts.h (mtts_mosnet_*), and parity with the published weights is UNPINNED — the pinned object is that
// definition, restated in torch by tests/mosnet_oracle.py.
//     twelve 3x3 convolutions (time x frequency) in four blocks of C = 16, 32, 64, 128, bias + ReLU each, TensorFlow "same" padding,
//     the third of a block with stride 3 along frequency;  BLSTM(128 per direction) over the [F4 * 128] features of a frame
//     (frequency-major, then channel);  Dense(256 -> 128) + ReLU;  Dense(128 -> 1) = frame score;  utterance score = mean over frames.
//
// MI355X mapping.  Activations are channels-last [sum T][F][C], compact over the utterances of a call; a table (MosUtt) gives every
// utterance's first frame and T, and every grid takes the utterance from a grid dimension of its own, so no tile straddles two
// utterances and an utterance's numbers do not depend on what else is in the call.
//   mos_conv_first_kernel     CIN = 1: K = 9 is no matrix product; one lane per (frame, column), 144 FMAs, four float4 stores.
//   mos_conv3x3_kernel        a whole 3x3 convolution as an implicit GEMM, M = output positions, N = COUT, K = 9 CIN, no padded copy and no
//                             im2col in HBM.  A workgroup (4 wavefronts) owns TT time rows x TFO output columns (<= 128 positions, a
//                             wavefront 32 of them x all COUT: COUT / 32 accumulator tiles); it stages the input patch — TT + 2 rows x
//                             (TFO - 1) SF + 3 columns x CK channels, zeros outside the utterance's frames and outside [0, F_in) — in LDS
//                             (position stride CK + 4 floats: the 16 lanes of a ds_read_b128 group fall on 16 distinct 4-bank slots for
//                             position strides 1 and 3) and runs the product on v_mfma_f32_32x32x2_f32, CK input channels at a time
//                             (K-loop over chunks: static LDS 29 KB, 45 KB for the stride-3 instances).  TFO / TT are chosen per layer on
//                             the host (mos_plan) so that narrow layers (F = 29, 10, 4) still fill the 128 positions: position m of a
//                             tile is (m / TFO, m % TFO).  Stride-3 instances compute the kept columns only.  The weight image is
//                             [tap][cin / 8][cout][8]: the (column, k-half) lanes of a wavefront read one contiguous 1 KB block per
//                             accumulator tile and k-step.  Epilogue: bias + ReLU in registers, 128-byte row stores.
//   input projection          ONE gemm.h launch for both directions over all frames, [sum T][IN] x [IN][2 * 512], biases in the epilogue;
//                             the kernel is named (64x64 tile, no split-K), so a frame's row does not depend on the call.
//   mos_blstm_kernel          grid (utterance, direction), 512 threads: thread g owns gate column g with its 128 recurrent weights in
//                             registers; h double-buffered in LDS (broadcast ds_read_b128), the cell update on the first 128 threads.
//   head                      Dense + ReLU as a named gemm.h launch, then mos_head_kernel: one workgroup per utterance, a wavefront per
//                             frame for the 128-long dot, the mean from four per-wavefront sums in a fixed order.  No atomics anywhere.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "gemm.h"
#include "melfront.h"
#include "params.h"
#include "resample.h"

namespace mtts {

constexpr int kMosH = 128;          // LSTM units per direction
constexpr int kMosBlocks = 4;
constexpr int kMosMaxPos = 128;     // output positions of a convolution workgroup (4 wavefronts x 32)

struct MosUtt { int frame0, T; };

// TensorFlow "same" padding along frequency for a 3-wide kernel: F_in -> F_out = ceil(F_in / stride), and the zero columns on the left
inline void mos_same_pad(int F_in, int stride, int* F_out, int* left, int* right) {
    const int fo = (F_in + stride - 1) / stride;
    const int total = std::max((fo - 1) * stride + 3 - F_in, 0);
    *F_out = fo; *left = total / 2; *right = total - total / 2;
}

template <int CIN, int SF>
struct MosConvCfg {
    static constexpr int CK = SF == 3 ? 16 : (CIN < 32 ? CIN : 32);   // input channels staged per chunk
    static constexpr int LDP = CK + 4;                                // floats between two positions of the patch
    static constexpr int CAP = SF == 3 ? 11520 : 7424;                // floats of LDS (46080 / 29696 bytes)
};
// The tile of a layer: TFO output columns x TT time rows per workgroup, nft column tiles.  The columns are spread evenly over the fewest
// tiles of at most 32, the rows fill the 128 positions and shrink until the patch fits the LDS array.
struct MosPlan { int TFO, TT, nft; };
inline MosPlan mos_plan(int F_out, int SF, int ldp, int cap) {
    MosPlan p;
    p.nft = (F_out + 31) / 32;
    p.TFO = (F_out + p.nft - 1) / p.nft;
    p.TT = kMosMaxPos / p.TFO;
    const int W = (p.TFO - 1) * SF + 3;
    while (p.TT > 1 && (p.TT + 2) * W * ldp > cap) --p.TT;
    return p;
}

// y[frame][f][0..16) = relu(b + sum_{dt, df} w[dt * 3 + df][.] * mag[frame + dt - 1][f + df - 1]), zeros outside the utterance and [0, F)
__global__ __launch_bounds__(256) void mos_conv_first_kernel(const MosUtt* utts, const float* mag, int ld, int F, const float* w, const float* b, float* y) {
    const MosUtt u = utts[blockIdx.z];
    const long long idx = (long long)blockIdx.x * 256 + (int)threadIdx.x;
    if (idx >= (long long)u.T * F) return;
    const int t = (int)(idx / F), f = (int)(idx - (long long)t * F);
    float in[9];
#pragma unroll
    for (int dt = 0; dt < 3; ++dt)
#pragma unroll
        for (int df = 0; df < 3; ++df) {
            const int tt = t + dt - 1, ff = f + df - 1;
            in[dt * 3 + df] = (tt >= 0 && tt < u.T && ff >= 0 && ff < F) ? mag[(long long)(u.frame0 + tt) * ld + ff] : 0.f;
        }
    float acc[16];
#pragma unroll
    for (int n = 0; n < 16; ++n) acc[n] = b[n];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int n = 0; n < 16; ++n) acc[n] = fmaf(in[tap], w[tap * 16 + n], acc[n]);
    float* py = y + ((long long)(u.frame0 + t) * F + f) * 16;
#pragma unroll
    for (int n = 0; n < 16; n += 4)
        st4(py + n, make_float4(fmaxf(acc[n], 0.f), fmaxf(acc[n + 1], 0.f), fmaxf(acc[n + 2], 0.f), fmaxf(acc[n + 3], 0.f)));
}

// x [sum T][F_in][CIN] -> y [sum T][F_out][COUT]: y[t][f][n] = relu(b[n] + sum_{dt, df, c} w[dt][df][c][n] x[t + dt - 1][f SF + df - pad_left][c]).
// w: [9][CIN / 8][COUT][8] (k = 8 q + 4 h + e at ((tap * CIN / 8 + q) * COUT + n) * 8 + 4 h + e).  Grid (time tiles of the longest utterance,
// column tiles, utterance); TT * TFO <= 128 and the patch fits CAP (mos_plan).
struct MosConvArgs {
    const MosUtt* utts = nullptr;
    const float* x = nullptr; const float* w = nullptr; const float* bias = nullptr;
    float* y = nullptr;
    int F_in = 0, F_out = 0, pad_left = 0, TT = 0, TFO = 0;
};
template <int CIN, int COUT, int SF>
__global__ __launch_bounds__(256) void mos_conv3x3_kernel(MosConvArgs a) {
    using Cfg = MosConvCfg<CIN, SF>;
    constexpr int CK = Cfg::CK, LDP = Cfg::LDP, C4 = CK / 4, TN = (COUT + 31) / 32;
    __shared__ float Ps[Cfg::CAP];
    const MosUtt u = a.utts[blockIdx.z];
    const int t0 = (int)blockIdx.x * a.TT;
    if (t0 >= u.T) return;   // (uniform over the workgroup, before any barrier)
    const int f0 = (int)blockIdx.y * a.TFO;
    const int W = (a.TFO - 1) * SF + 3, rows = a.TT + 2, npos = a.TT * a.TFO;
    const int fin0 = f0 * SF - a.pad_left;   // input column of patch column 0
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const bool live = wave * 32 < npos;      // (wave-uniform)
    int ma = wave * 32 + l31;
    if (ma >= npos) ma = 0;                  // an idle lane reads position 0 and stores nothing
    const int tla = ma / a.TFO, fla = ma - tla * a.TFO;
    const int pbase = (tla * W + fla * SF) * LDP + 4 * h;
    f32x16 acc[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    for (int c0 = 0; c0 < CIN; c0 += CK) {
        if (c0) __syncthreads();   // the previous chunk has been read
        for (int i = tid; i < rows * W * C4; i += 256) {
            const int pos = i / C4, c4 = i - pos * C4;
            const int row = pos / W, col = pos - row * W;
            const int t = t0 - 1 + row, fin = fin0 + col;
            float4 v = zero4();
            if (t >= 0 && t < u.T && fin >= 0 && fin < a.F_in) v = ld4(a.x + ((long long)(u.frame0 + t) * a.F_in + fin) * CIN + c0 + 4 * c4);
            st4(Ps + pos * LDP + 4 * c4, v);
        }
        __syncthreads();
        if (!live) continue;
#if defined(MTTS_EMU)
        for (int j = 0; j < TN; ++j)
            for (int r = 0; r < 16; ++r) {
                const int m = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h, n = j * 32 + l31;
                if (m >= npos || n >= COUT) continue;
                const int tl = m / a.TFO, fl = m - tl * a.TFO;
                float s = acc[j][r];
                for (int tap = 0; tap < 9; ++tap) {
                    const float* pa = Ps + ((tl + tap / 3) * W + fl * SF + tap % 3) * LDP;
                    for (int c = 0; c < CK; ++c)
                        s = fmaf(pa[c], a.w[((long long)(tap * (CIN / 8) + (c0 + c) / 8) * COUT + n) * 8 + ((c0 + c) & 7)], s);
                }
                acc[j][r] = s;
            }
#else
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
            const int dt = tap / 3, df = tap - 3 * dt;
            const float* pa = Ps + pbase + (dt * W + df) * LDP;
            const float* pw = a.w + ((long long)(tap * (CIN / 8) + c0 / 8) * COUT + l31) * 8 + 4 * h;
#pragma unroll
            for (int q = 0; q < CK / 8; ++q) {
                const float4 av = ld4(pa + 8 * q);
                float4 bv[TN];
#pragma unroll
                for (int j = 0; j < TN; ++j) bv[j] = (COUT >= 32 || l31 < COUT) ? ld4(pw + (long long)(q * COUT + j * 32) * 8) : zero4();
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv[j].x, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv[j].y, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv[j].z, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv[j].w, acc[j], 0, 0, 0);
                }
            }
        }
#endif
    }
    if (!live) return;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = j * 32 + l31;
        if (n >= COUT) continue;
        const float bn = a.bias[n];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (m >= npos) continue;
            const int tl = m / a.TFO, fl = m - tl * a.TFO;
            const int t = t0 + tl, f = f0 + fl;
            if (t >= u.T || f >= a.F_out) continue;
            a.y[((long long)(u.frame0 + t) * a.F_out + f) * COUT + n] = fmaxf(acc[j][r] + bn, 0.f);
        }
    }
}

__device__ __forceinline__ float mos_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// The recurrence of both directions of every utterance.  xproj [sum T][2][4H]: W_ih x + b of the frame, gate order i, f, g, o; whh
// [2][H / 4][4H][4]: recurrent weight of gate column g and hidden unit 4 k4 + e at ((dir * H / 4 + k4) * 4H + g) * 4 + e; hout [sum T][2 H] =
// [forward | backward].  Direction 1 starts at the utterance's own last frame.  Zero initial state.
__global__ __launch_bounds__(512) void mos_blstm_kernel(const MosUtt* utts, const float* xproj, const float* whh, float* hout) {
    constexpr int H = kMosH, G = 4 * kMosH;
    __shared__ float hs[2][H];
    __shared__ float gs[G];
    const MosUtt u = utts[blockIdx.x];
    const int dir = (int)blockIdx.y, g = (int)threadIdx.x;
    float w[H];
#pragma unroll
    for (int k4 = 0; k4 < H / 4; ++k4) {
        const float4 v = ld4(whh + (((long long)dir * (H / 4) + k4) * G + g) * 4);
        w[4 * k4] = v.x; w[4 * k4 + 1] = v.y; w[4 * k4 + 2] = v.z; w[4 * k4 + 3] = v.w;
    }
    if (g < H) hs[0][g] = 0.f;
    float c = 0.f;
    __syncthreads();
    const float* px = xproj + (long long)u.frame0 * (2 * G) + dir * G + g;
    const int step = dir ? -1 : 1;
    int t = dir ? u.T - 1 : 0;
    float xv = px[(long long)t * (2 * G)];
    for (int s = 0; s < u.T; ++s, t += step) {
        const float* hin = hs[s & 1];
        const float x_t = xv;
        if (s + 1 < u.T) xv = px[(long long)(t + step) * (2 * G)];   // the next step's input, in flight across the barriers
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
        for (int k4 = 0; k4 < H / 4; ++k4) {
            const float4 hv = ld4(hin + 4 * k4);
            a0 = fmaf(w[4 * k4], hv.x, a0); a1 = fmaf(w[4 * k4 + 1], hv.y, a1); a2 = fmaf(w[4 * k4 + 2], hv.z, a2); a3 = fmaf(w[4 * k4 + 3], hv.w, a3);
        }
        const float pre = x_t + ((a0 + a1) + (a2 + a3));
        gs[g] = (g >= 2 * H && g < 3 * H) ? tanhf(pre) : mos_sigmoid(pre);
        __syncthreads();
        if (g < H) {
            c = gs[H + g] * c + gs[g] * gs[2 * H + g];
            const float hv = gs[3 * H + g] * tanhf(c);
            hs[(s + 1) & 1][g] = hv;
            hout[(long long)(u.frame0 + t) * (2 * H) + dir * H + g] = hv;
        }
        __syncthreads();
    }
}

// frame_scores[frame] = <d[frame], w> + b;  utt_scores[utterance] = mean of its frame scores.  One workgroup per utterance; wavefront v
// takes frames v, v + 4, ... and adds their scores in that order; the four sums are combined as (s0 + s1) + (s2 + s3).
__global__ __launch_bounds__(256) void mos_head_kernel(const MosUtt* utts, const float* d, const float* w, const float* b, float* frame_scores, float* utt_scores) {
    __shared__ float red[4];
    const MosUtt u = utts[blockIdx.x];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const float w0 = w[lane], w1 = w[64 + lane], b0 = b[0];
    float part = 0.f;
    for (int t = wave; t < u.T; t += 4) {
        const float* p = d + (long long)(u.frame0 + t) * kMosH;
        const float s = wave_sum(p[lane] * w0 + p[64 + lane] * w1) + b0;
        if (lane == 0) frame_scores[u.frame0 + t] = s;
        part += s;
    }
    if (lane == 0) red[wave] = part;
    __syncthreads();
    if (threadIdx.x == 0) utt_scores[blockIdx.x] = ((red[0] + red[1]) + (red[2] + red[3])) / (float)u.T;
}

class MosNet {
public:
    int n_freq = 257, cap_frames = 0, cap_utts = 0;
    int F[kMosBlocks + 1] = {0}, padl[kMosBlocks] = {0};   // widths before block b (F[4]: after the last), left pad of block b's stride-3 convolution
    int IN = 0;                                            // BLSTM input features: 128 * F[4]
    hipStream_t stream = nullptr;
    std::string last_error;

    ParamTable tab;   // (plan_call refuses a call while a tensor has not been loaded)
    float *act0 = nullptr, *act1 = nullptr, *mag_dev = nullptr, *xproj = nullptr, *hseq = nullptr, *dense = nullptr, *fs_dev = nullptr, *us_dev = nullptr;
    MosUtt* utts_dev = nullptr;
    std::vector<MosUtt> h_utts;
    long long total = 0;
    int max_T = 0;
    GemmCtx gx;
    DevHeap mem;

    int err(const std::string& s) { last_error = s; return -1; }
    void set_error(const std::string& s) { err(s); }
    static int chan(int b) { return 16 << b; }
    const float* P(const std::string& n) const { return tab.ptr(n); }

    static std::string check_cfg(int n_freq_, int max_frames, int max_utts) {
        if (n_freq_ < 2 || n_freq_ > 4097) return "n_freq must be 2..4097";
        if (max_frames < 1 || max_frames > (1 << 20)) return "max_frames_per_call must be 1..1048576";
        if (max_utts < 1 || max_utts > 65535) return "max_utts must be 1..65535";
        return "";
    }

    int init(int n_freq_, int max_frames, int max_utts) {
        const std::string why = check_cfg(n_freq_, max_frames, max_utts);
        if (!why.empty()) return err("mtts_mosnet_create: " + why);
        n_freq = n_freq_; cap_frames = max_frames; cap_utts = max_utts;
        F[0] = n_freq;
        long long widest = 16LL * n_freq;
        for (int b = 0; b < kMosBlocks; ++b) {
            int right;
            mos_same_pad(F[b], 3, &F[b + 1], &padl[b], &right);
            widest = std::max(widest, (long long)chan(b) * F[b]);
        }
        IN = chan(kMosBlocks - 1) * F[kMosBlocks];
        for (int l = 0; l < 3 * kMosBlocks; ++l) {
            const int b = l / 3, cout = chan(b), cin = l % 3 ? cout : (b ? chan(b - 1) : 1);
            tab.add("conv." + std::to_string(l) + ".w", 9LL * cin * cout);   // conv.0: [9][16]; else [9][cin / 8][cout][8]
            tab.add("conv." + std::to_string(l) + ".b", cout);
        }
        tab.add("blstm.w_ih", 2LL * 4 * kMosH * IN);      // [2][4H][IN]: forward rows, then backward
        tab.add("blstm.b", 2LL * 4 * kMosH);
        tab.add("blstm.w_hh", 2LL * 4 * kMosH * kMosH);   // [2][H / 4][4H][4]
        tab.add("dense.w", 2LL * kMosH * kMosH);          // [128][256]
        tab.add("dense.b", kMosH);
        tab.add("frame_score.w", kMosH);
        tab.add("frame_score.b", 1);
        if (gx.alloc_workspace(mem)) return err("out of device memory (split-K workspace)");
        DEV_CHECK(tab.alloc(mem));
        const size_t fr = (size_t)cap_frames;
        DEV_CHECK(mem.alloc(act0, fr * (size_t)widest * sizeof(float)));
        DEV_CHECK(mem.alloc(act1, fr * (size_t)widest * sizeof(float)));
        DEV_CHECK(mem.alloc(mag_dev, fr * (size_t)n_freq * sizeof(float)));
        DEV_CHECK(mem.alloc(xproj, fr * 8 * kMosH * sizeof(float)));
        DEV_CHECK(mem.alloc(hseq, fr * 2 * kMosH * sizeof(float)));
        DEV_CHECK(mem.alloc(dense, fr * kMosH * sizeof(float)));
        DEV_CHECK(mem.alloc(fs_dev, fr * sizeof(float)));
        DEV_CHECK(mem.alloc(us_dev, (size_t)cap_utts * sizeof(float)));
        DEV_CHECK(mem.alloc(utts_dev, (size_t)cap_utts * sizeof(MosUtt)));
        return 0;
    }
    int load(const char* name, const float* host, long long numel) { return tab.load(name, host, numel, "MOSNet", last_error) ? 0 : -1; }

    // what both entries refuse about the frame counts before any launch; fills the utterance table
    int plan_call(const std::string& who, int n_utts, const int* n_frames) {
        for (auto& t : tab.tensors)
            if (!t.loaded) return err(who + "tensor " + t.name + " has not been loaded (mtts_mosnet_load)");
        if (n_utts < 1) return err(who + "n_utts < 1");
        if (n_utts > 65535) return err(who + "more than 65535 utterances in one call");
        if (n_utts > cap_utts) return err(who + std::to_string(n_utts) + " utterances exceed max_utts = " + std::to_string(cap_utts));
        h_utts.clear();
        total = 0; max_T = 0;
        for (int i = 0; i < n_utts; ++i) {
            if (n_frames[i] < 1) return err(who + "utterance " + std::to_string(i) + ": n_frames < 1");
            if (total + n_frames[i] > cap_frames)
                return err(who + "more than max_frames_per_call = " + std::to_string(cap_frames) + " frames in one call (utterance " + std::to_string(i) + ")");
            h_utts.push_back(MosUtt{(int)total, n_frames[i]});
            total += n_frames[i];
            max_T = std::max(max_T, n_frames[i]);
        }
        return 0;
    }

    template <int CIN, int COUT, int SF>
    void conv_launch(MosConvArgs a, int n_utts, hipStream_t st) {
        using Cfg = MosConvCfg<CIN, SF>;
        const MosPlan p = mos_plan(a.F_out, SF, Cfg::LDP, Cfg::CAP);
        a.TT = p.TT; a.TFO = p.TFO;
        const dim3 grid((unsigned)((max_T + p.TT - 1) / p.TT), (unsigned)p.nft, (unsigned)n_utts);
        MTTS_LAUNCH((mos_conv3x3_kernel<CIN, COUT, SF>), grid, dim3(256), st, a);
    }
    void conv(int cin, int cout, int sf, const MosConvArgs& a, int n_utts, hipStream_t st) {
#define MOS_CONV_CASE(CI, CO, S) if (cin == CI && cout == CO && sf == S) return conv_launch<CI, CO, S>(a, n_utts, st);
        MOS_CONV_CASE(16, 16, 1) MOS_CONV_CASE(16, 16, 3) MOS_CONV_CASE(16, 32, 1) MOS_CONV_CASE(32, 32, 1) MOS_CONV_CASE(32, 32, 3)
        MOS_CONV_CASE(32, 64, 1) MOS_CONV_CASE(64, 64, 1) MOS_CONV_CASE(64, 64, 3) MOS_CONV_CASE(64, 128, 1) MOS_CONV_CASE(128, 128, 1)
        MOS_CONV_CASE(128, 128, 3)
#undef MOS_CONV_CASE
    }

    // The planned call's magnitudes at mag (device, row stride ld) -> fs_dev [sum T], us_dev [n_utts]; asynchronous on st.
    int network(const float* mag, int ld, hipStream_t st) {
        const int n_utts = (int)h_utts.size(), M = (int)total;
        DEV_CHECK(hipMemcpyAsync(utts_dev, h_utts.data(), h_utts.size() * sizeof(MosUtt), hipMemcpyHostToDevice, st));
        MTTS_LAUNCH(mos_conv_first_kernel, dim3((unsigned)(((long long)max_T * n_freq + 255) / 256), 1, (unsigned)n_utts), dim3(256), st,
                    (const MosUtt*)utts_dev, mag, ld, n_freq, P("conv.0.w"), P("conv.0.b"), act0);
        float *src = act0, *dst = act1;
        for (int l = 1; l < 3 * kMosBlocks; ++l) {
            const int b = l / 3, cout = chan(b), cin = l % 3 ? cout : chan(b - 1), sf = l % 3 == 2 ? 3 : 1;
            MosConvArgs a;
            a.utts = utts_dev; a.x = src; a.y = dst;
            a.w = P("conv." + std::to_string(l) + ".w"); a.bias = P("conv." + std::to_string(l) + ".b");
            a.F_in = F[b]; a.F_out = sf == 3 ? F[b + 1] : F[b]; a.pad_left = sf == 3 ? padl[b] : 1;
            conv(cin, cout, sf, a, n_utts, st);
            std::swap(src, dst);
        }
        {   // both directions' input projections: xproj [sum T][2 * 4H] = x [sum T][IN] * w_ih [2 * 4H][IN]^T + b
            GemmArgs g;
            g.A = src; g.lda = IN; g.B = P("blstm.w_ih"); g.ldb = IN; g.C = xproj; g.ldc = 8 * kMosH;
            g.M = M; g.N = 8 * kMosH; g.K = IN; g.bias = P("blstm.b");
            gemm_launch(gx, GEMM_NT, g, M, 8 * kMosH, 1, st, 64, 2.0 * M * 8.0 * kMosH * IN, 0);
        }
        MTTS_LAUNCH(mos_blstm_kernel, dim3((unsigned)n_utts, 2), dim3(4 * kMosH), st, (const MosUtt*)utts_dev, (const float*)xproj, P("blstm.w_hh"), hseq);
        {   // dense [sum T][128] = relu(h [sum T][256] * W [128][256]^T + b)
            GemmArgs g;
            g.A = hseq; g.lda = 2 * kMosH; g.B = P("dense.w"); g.ldb = 2 * kMosH; g.C = dense; g.ldc = kMosH;
            g.M = M; g.N = kMosH; g.K = 2 * kMosH; g.bias = P("dense.b"); g.flags = GEMM_RELU;
            gemm_launch(gx, GEMM_NT, g, M, kMosH, 1, st, 64, 2.0 * M * 2.0 * kMosH * kMosH, 0);
        }
        MTTS_LAUNCH(mos_head_kernel, dim3((unsigned)n_utts), dim3(256), st, (const MosUtt*)utts_dev, (const float*)dense, P("frame_score.w"),
                    P("frame_score.b"), fs_dev, us_dev);
        if (gx.error) { const std::string e = std::string("GEMM launcher: ") + gx.error; gx.error = nullptr; return err(e); }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return err(std::string("kernel launch failed: ") + hipGetErrorString(e));
        return 0;
    }
    int download(hipStream_t st, float* utt_scores, float* frame_scores) {
        DEV_CHECK(hipMemcpyAsync(utt_scores, us_dev, h_utts.size() * sizeof(float), hipMemcpyDeviceToHost, st));
        if (frame_scores) DEV_CHECK(hipMemcpyAsync(frame_scores, fs_dev, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, st));
        DEV_CHECK(hipStreamSynchronize(st));
        return 0;
    }

    // mag_host [sum T][n_freq] -> utt_scores [n_utts], frame_scores [sum T] (or NULL)
    int score(int n_utts, const int* n_frames, const float* mag_host, float* utt_scores, float* frame_scores) {
        const std::string who = "mtts_mosnet_score: ";
        if (!n_frames || !mag_host || !utt_scores) return err(who + "NULL argument");
        if (plan_call(who, n_utts, n_frames)) return -1;
        for (long long i = 0; i < total * n_freq; ++i)
            if (!std::isfinite(mag_host[i]))
                return err(who + "non-finite magnitude at frame " + std::to_string(i / n_freq) + ", column " + std::to_string(i % n_freq));
        DEV_CHECK(hipMemcpyAsync(mag_dev, mag_host, (size_t)total * n_freq * sizeof(float), hipMemcpyHostToDevice, stream));
        if (network(mag_dev, n_freq, stream)) return -1;
        return download(stream, utt_scores, frame_scores);
    }

    // Waveforms -> scores through front's MelFront (pack, upload, reflect pad, forward STFT per utterance, magnitude), behind front's resampler when
    // `resampled`; the network reads MelFront::mag where it lies.  The whole chain runs on the front-end's stream.  A refusal is left
    // on this handle (and, where a front-end check made it, on the front-end too).
    int score_wavs(MelFront& mf, Resample& rs, int n_utts, const int* n_samples, const float* wavs_host, bool resampled, float* utt_scores, int* n_frames_out,
                   float* frame_scores) {
        const std::string who = "mtts_mosnet_score_wavs: ";
        if (!n_samples || !wavs_host || !utt_scores || !n_frames_out) return err(who + "NULL argument");
        if (mf.n_fft != 2 * (n_freq - 1))
            return err(who + "the STFT handle has filter_length " + std::to_string(mf.n_fft) + ", n_freq = " + std::to_string(n_freq) + " needs " +
                       std::to_string(2 * (n_freq - 1)));
        if (!mf.have_basis) return err(who + "STFT forward basis not loaded (mtts_stft_load)");
        if (n_utts < 1) return err(who + "n_utts < 1");
        if (resampled && rs.check_lengths(who, n_utts, n_samples)) return err(mf.last_error);
        std::vector<long long> n16((size_t)n_utts);
        for (int u = 0; u < n_utts; ++u) n16[(size_t)u] = resampled ? rs.out_len(n_samples[u]) : n_samples[u];
        if (mf.check_utterances(who, n_utts, [&](int u) { return n16[(size_t)u]; }, MelFront::UTT_GRID | MelFront::UTT_CAP | MelFront::UTT_PAD, resampled))
            return err(mf.last_error);
        for (int u = 0; u < n_utts; ++u) n_frames_out[u] = mf.frames_of((int)n16[(size_t)u]);
        if (plan_call(who, n_utts, n_frames_out)) return -1;
        hipStream_t st = mf.stream;
        mf.pack_begin();
        for (int u = 0; u < n_utts; ++u) mf.pack_add(n16[(size_t)u], n_frames_out[u]);
        if (mf.stage("mtts_mosnet_score_wavs", true)) return err(mf.last_error);
        if (resampled) {
            rs.table_begin();
            for (int u = 0; u < n_utts; ++u) rs.table_add(n_samples[u], mf.h_utts[(size_t)u].wav0);
            if (rs.n_src > (1LL << 31) - 1) return err(who + "too many samples in one call");
            if (rs.reserve(rs.n_src, rs.n_slots, (size_t)n_utts) || rs.launch(wavs_host, std::nan(""), false) || mf.pad_staged(false, true)) return err(mf.last_error);
        } else if (mf.pad_waveforms(wavs_host, false, true))
            return err(mf.last_error);
        // One forward-STFT launch per utterance, with the launcher's own choice for its T rows: exactly the launch mtts_stft_transform
        // makes for that waveform.  So the magnitudes are those of mtts_stft_transform bit for bit, and they depend on the utterance alone
        // (the choice is a function of T), not on what shares the call.  The product is 4 % of the network's work.
        for (const StftUtt& u : mf.h_utts) {
            GemmArgs g;
            g.A = mf.xp.p + u.xp0; g.lda = mf.hop; g.B = mf.basis; g.ldb = mf.n_fft; g.C = mf.spec.p + (long long)u.frame0 * mf.ld_spec; g.ldc = mf.ld_spec;
            g.M = u.T; g.N = 2 * mf.F; g.K = mf.n_fft;
            gemm_launch(mf.gx, GEMM_NT, g, u.T, 2 * mf.F, 1, st, 0, 2.0 * u.T * 2.0 * mf.F * mf.n_fft, 0);
        }
        const float* spec = mf.spec;
        float *mag = mf.mag, *energy = mf.energy;
        const int ld_spec = mf.ld_spec, ld_mag = mf.ld_mag, rows = (int)mf.n_frames, bins = mf.F;
        MTTS_LAUNCH(stft_magnitude_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), st, spec, ld_spec, rows, bins, mag, ld_mag, energy);
        if (mf.check_launch()) return err(mf.last_error);
        if (network(mag, ld_mag, st)) return -1;
        return download(st, utt_scores, frame_scores);
    }
};

}  // namespace mtts
