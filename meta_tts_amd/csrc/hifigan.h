// HiFi-GAN generator (mel -> waveform), ResBlock type "1" — DESIGN.md section 1 row a24, the second neural vocoder beside vocoder.h.
//
// Reference call site: utils/model.py:32-50 (vocoder_infer, branch name == "HiFi-GAN": vocoder(mels).squeeze(1), x max_wav_value ->
// int16, cut to lengths).  The generator itself is NOT in the reference tree (its hifigan/ package and generator_universal.pth.tar are
// absent): the architecture below is the published one (Kong et al. 2020, Generator with resblock "1"):
//     x = conv_pre(mel)                                  Conv1d(n_mel -> C0, k 7, zero pad 3)
//     for i in 0..n_up-1:
//         x = leaky_relu(x, 0.1);  x = ups[i](x)         ConvTranspose1d(C_i -> C_i/2, k = 2 r_i, stride r_i, pad r_i/2)
//         x = (1/n_k) * sum_j resblocks[i*n_k + j](x)    ("MRF": mean over the n_k kernel sizes)
//     x = leaky_relu(x, 0.01);  x = conv_post(x)         Conv1d(C_last -> 1, k 7, zero pad 3);  tanh
//     ResBlock1(k, (d_0..d_{m-1})): for each d:  t = leaky_relu(x, 0.1);  t = conv(k, dilation d, zero pad d(k-1)/2)(t)
//                                                t = leaky_relu(t, 0.1);  t = conv(k, dilation 1, zero pad (k-1)/2)(t);  x = t + x
// with weight normalisation folded on the host (meta_tts_amd/hifigan.py).  Parity with published weights is UNPINNED: checked against
// tests/hifigan_oracle.py, a torch restatement of the same definition.  Padding is zero padding at each utterance's own ends.
//
// MI355X mapping: activations are channels-last row matrices [time][C] per utterance, row counts through GemmArgs::dimptr, as in vocoder.h.
//   GEMM route (every channel count): conv_pre, the r polyphase GEMMs of a transposed convolution (one multi-problem launch) and the
//   residual convolutions go through gemm_launch.  A pair costs three launches: hg_pad_kernel writes the zero-padded LeakyReLU image of
//   x and clears the guard rows of the buffer conv1 writes into; conv1 (dilated taps inside the K-loop when C % 32 == 0, else one
//   accumulate pass per tap) puts LeakyReLU(. + b) between those guard rows; conv2 (K = k C over contiguous rows) accumulates onto x
//   in place (GEMM_ACCUM) — the residual add.  The MRF mean rides in the pad pass: the first pad of block j > 0 folds block j-1's result
//   into the sum and restarts x from the stage input; the pad that feeds the next stage reads sum + x / n_k.
//   Direct route (C in {32, 64}, C <= direct_max_channels): hg_conv_direct_kernel does a whole dilated convolution without a padded
//   copy — a workgroup stages 128 + (k-1) d rows in LDS (LeakyReLU on the way in, zeros outside the utterance), runs the k C deep product
//   on the fp32 MFMA pipe with the weights streamed from L2, and ends with bias + LeakyReLU, bias + residual, or bias + residual + MRF
//   accumulation.  A pair costs two launches and no pad pass.
//   bf16-operand mode (set_numerics(1, .); include/mtts.h): the same graph with every convolution but conv_post multiplying operands
//   rounded to bf16 — the GEMM route on the bf16 family of gemm_bf16.h through this handle's GemmCtx (rounding in its staging pass, no
//   split-K), the direct route (C in {32, 64, 128}) on hg_conv_direct_bf16_kernel over weight images packed once per tensor.  Everything
//   between the convolutions, every tensor in HBM and conv_post + tanh stay fp32.
#pragma once
#include <string>
#include <vector>

#include "gemm_bf16.h"
#include "vocoder.h"

namespace mtts {

constexpr int kHgMaxUps = 8, kHgMaxKernels = 4, kHgMaxDil = 4, kHgMaxResKernel = 11, kHgMaxDilation = 5;
constexpr int kHgTileRows = 128;                                             // output rows of a direct-route workgroup
constexpr int kHgMaxHalo = (kHgMaxResKernel - 1) * kHgMaxDilation;           // 50 rows (both sides together)

struct HifiGanCfg {
    int n_mel = 80, c0 = 512, n_up = 4, n_k = 3, n_dil = 3, resblock = 1, direct_max = 0;
    int rates[kHgMaxUps] = {8, 8, 2, 2, 0, 0, 0, 0};
    int kernels[kHgMaxKernels] = {3, 7, 11, 0};
    int dil[kHgMaxKernels][kHgMaxDil] = {{1, 3, 5, 0}, {1, 3, 5, 0}, {1, 3, 5, 0}, {0, 0, 0, 0}};
};

// empty: supported; else the refusal, naming the argument
inline std::string hifigan_check_cfg(const HifiGanCfg& c, int max_B, int max_T) {
    if (c.resblock != 1) return "resblock_type " + std::to_string(c.resblock) + " is not supported (only ResBlock \"1\")";
    if (c.n_mel < 16 || c.n_mel % 16) return "n_mel must be a positive multiple of 16";
    if (c.n_up < 1 || c.n_up > kHgMaxUps) return "n_rates must be 1.." + std::to_string(kHgMaxUps);
    if (c.n_k < 1 || c.n_k > kHgMaxKernels) return "n_res_kernels must be 1.." + std::to_string(kHgMaxKernels);
    if (c.n_dil < 1 || c.n_dil > kHgMaxDil) return "n_dil must be 1.." + std::to_string(kHgMaxDil);
    if (c.c0 < 16 || c.c0 % (16 << c.n_up)) return "initial_channels must halve per stage and stay a multiple of 16 (need a multiple of " + std::to_string(16 << c.n_up) + ")";
    for (int i = 0; i < c.n_up; ++i)
        if (c.rates[i] < 2 || (c.rates[i] & 1)) return "rates[" + std::to_string(i) + "] = " + std::to_string(c.rates[i]) + ": every rate must be even and >= 2";
    for (int j = 0; j < c.n_k; ++j) {
        if (c.kernels[j] < 1 || !(c.kernels[j] & 1) || c.kernels[j] > kHgMaxResKernel)
            return "res_kernels[" + std::to_string(j) + "] = " + std::to_string(c.kernels[j]) + ": residual kernel sizes must be odd and <= " + std::to_string(kHgMaxResKernel);
        for (int m = 0; m < c.n_dil; ++m)
            if (c.dil[j][m] < 1 || c.dil[j][m] > kHgMaxDilation)
                return "res_dilations[" + std::to_string(j) + "][" + std::to_string(m) + "] = " + std::to_string(c.dil[j][m]) + ": dilations must be 1.." + std::to_string(kHgMaxDilation);
    }
    if (c.direct_max != 0 && c.direct_max != 32 && c.direct_max != 64) return "direct_max_channels must be 0, 32 or 64";
    if (max_B < 1) return "max_B must be >= 1";
    if (max_T < 4) return "max_T must be >= 4";
    return "";
}

// One pass over the rows of x (T = lens[z] * len_mult rows of C floats per utterance z):  v = xs * x[row] (+ add[row])
//   y rows [0, T + 2d):  y[d + row] = leaky_relu(v, slope), zero rows outside       (the padded operand of the next convolution)
//   mrf[row] = (fold_init ? 0 : mrf[row]) + fs * fold[row]                           (MRF sum; read BEFORE copy is written: fold may be copy)
//   copy[row] = v                                                                     (restart of x from the stage input)
//   guard rows [0, gp) and [gp + T, 2 gp + T) = 0                                     (zero padding of the buffer conv1 writes between them)
struct HgPadArgs {
    const int* lens = nullptr; int len_mult = 1, C = 0;
    const float* x = nullptr; long long x_gs = 0; float xs = 1.f;
    const float* add = nullptr; long long add_gs = 0;
    float* y = nullptr; long long y_gs = 0; int d = 0; float slope = 1.f;
    const float* fold = nullptr; long long fold_gs = 0; float fs = 0.f; int fold_init = 0;
    float* mrf = nullptr; long long mrf_gs = 0;
    float* copy = nullptr; long long copy_gs = 0;
    float* guard = nullptr; long long guard_gs = 0; int gp = 0;
};
__device__ __forceinline__ float hg_lrelu(float v, float slope) { return v > 0.f ? v : slope * v; }
__global__ void hg_pad_kernel(HgPadArgs a) {
    const int z = blockIdx.z;
    const int T = a.lens[z] * a.len_mult, C4 = a.C >> 2;
    const long long idx = (long long)blockIdx.x * 256 + (int)threadIdx.x;
    if (a.guard && idx < 2LL * a.gp * C4) {
        const int g = (int)(idx / C4), c = (int)(idx - (long long)g * C4) * 4;
        st4(a.guard + (long long)z * a.guard_gs + (long long)(g < a.gp ? g : T + g) * a.C + c, zero4());
    }
    const long long prow = idx / C4;
    if (prow >= (long long)T + 2 * a.d) return;
    const int c = (int)(idx - prow * C4) * 4;
    const long long row = prow - a.d;
    float4 v = zero4();
    if (row >= 0 && row < T) {
        const long long o = row * a.C + c;
        v = ld4(a.x + (long long)z * a.x_gs + o);
        v.x *= a.xs; v.y *= a.xs; v.z *= a.xs; v.w *= a.xs;
        if (a.add) { const float4 s = ld4(a.add + (long long)z * a.add_gs + o); v.x += s.x; v.y += s.y; v.z += s.z; v.w += s.w; }
        if (a.fold) {
            const float4 f = ld4(a.fold + (long long)z * a.fold_gs + o);
            float* pm = a.mrf + (long long)z * a.mrf_gs + o;
            const float4 m = a.fold_init ? zero4() : ld4(pm);
            st4(pm, make_float4(m.x + a.fs * f.x, m.y + a.fs * f.y, m.z + a.fs * f.z, m.w + a.fs * f.w));
        }
        if (a.copy) st4(a.copy + (long long)z * a.copy_gs + o, v);
        v.x = hg_lrelu(v.x, a.slope); v.y = hg_lrelu(v.y, a.slope); v.z = hg_lrelu(v.z, a.slope); v.w = hg_lrelu(v.w, a.slope);
    }
    st4(a.y + (long long)z * a.y_gs + prow * a.C + c, v);
}

// Direct route: out = epilogue(bias + conv(k, dilation d, zero pad d (k-1)/2)(leaky_relu(x, in_slope))) for one utterance's 128-row tile.
//   mode 0: out = leaky_relu(., 0.1)                          (first convolution of a pair; the second then reads with in_slope 1)
//   mode 1: out = . + res                                     (second convolution: the residual add; out may be res)
//   mode 2: mrf = (mrf_init ? 0 : mrf) + inv_nk * (. + res)   (last pair of a block: the block's result goes to the MRF sum only)
// w: [C][k][C] (the GEMM route's image).  LDS: (128 + (k-1) d) rows of C + 4 floats (<= 48.4 KB at C = 64: three workgroups per CU).
// Wave w owns rows [32 w, 32 w + 32) x all C columns: C / 32 MFMA tiles; fragments as in gemm.h (lane half h feeds k = 8 q + 4 h + e).
struct HgConvArgs {
    const int* lens = nullptr; int len_mult = 1;
    const float* x = nullptr; long long x_gs = 0; float in_slope = 1.f;
    const float* w = nullptr; const float* bias = nullptr; int k = 3, d = 1;
    const float* res = nullptr; long long res_gs = 0;
    float* out = nullptr; long long out_gs = 0;
    float* mrf = nullptr; long long mrf_gs = 0; float inv_nk = 1.f; int mrf_init = 0;
    int mode = 0;
};
template <int C>
__global__ __launch_bounds__(256) void hg_conv_direct_kernel(HgConvArgs a) {
    constexpr int LDA = C + 4, TN = C / 32;
    __shared__ float As[(kHgTileRows + kHgMaxHalo) * LDA];
    const int z = blockIdx.z, tid = (int)threadIdx.x;
    const int T = a.lens[z] * a.len_mult, m0 = (int)blockIdx.x * kHgTileRows;
    if (m0 >= T) return;   // (uniform over the workgroup, before the barrier)
    const int halo = (a.k - 1) * a.d, pad = halo >> 1, nrows = kHgTileRows + halo;
    const float* px = a.x + (long long)z * a.x_gs;
    for (int i = tid; i < nrows * (C / 4); i += 256) {
        const int lr = i / (C / 4), c = (i - lr * (C / 4)) * 4;
        const int row = m0 - pad + lr;
        float4 v = zero4();
        if (row >= 0 && row < T) {
            v = ld4(px + (long long)row * C + c);
            v.x = hg_lrelu(v.x, a.in_slope); v.y = hg_lrelu(v.y, a.in_slope); v.z = hg_lrelu(v.z, a.in_slope); v.w = hg_lrelu(v.w, a.in_slope);
        }
        st4(As + lr * LDA + c, v);
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int KW = a.k * C;   // floats per output channel of w
    f32x16 acc[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
#if defined(MTTS_EMU)
    for (int j = 0; j < TN; ++j)
        for (int r = 0; r < 16; ++r) {
            const int lr = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            const float* pw = a.w + (long long)(j * 32 + l31) * KW;
            float s = 0.f;
            for (int t = 0; t < a.k; ++t)
                for (int c = 0; c < C; ++c) s = fmaf(As[(lr + t * a.d) * LDA + c], pw[t * C + c], s);
            acc[j][r] = s;
        }
#else
    for (int t = 0; t < a.k; ++t) {
        const float* pa = As + (wave * 32 + l31 + t * a.d) * LDA + 4 * h;
        const float* pw = a.w + (long long)l31 * KW + t * C + 4 * h;
#pragma unroll
        for (int q = 0; q < C / 8; ++q) {
            const float4 av = ld4(pa + 8 * q);
            float4 bv[TN];
#pragma unroll
            for (int j = 0; j < TN; ++j) bv[j] = ld4(pw + (long long)j * 32 * KW + 8 * q);
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
    const float* pres = a.res ? a.res + (long long)z * a.res_gs : nullptr;
    float* pout = a.out ? a.out + (long long)z * a.out_gs : nullptr;
    float* pmrf = a.mrf ? a.mrf + (long long)z * a.mrf_gs : nullptr;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = j * 32 + l31;
        const float bv = a.bias[n];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (m >= T) continue;
            const long long o = (long long)m * C + n;
            float v = acc[j][r] + bv;
            if (a.mode == 0) pout[o] = hg_lrelu(v, 0.1f);
            else {
                v += pres[o];
                if (a.mode == 1) pout[o] = v;
                else pmrf[o] = (a.mrf_init ? 0.f : pmrf[o]) + a.inv_nk * v;
            }
        }
    }
}

// ---- bf16-operand mode (numerics mode 1; definition in include/mtts.h) -----------------------------------------------------------------
// Weight image of the direct bf16 kernel: [tap][cin / 16][cout / 32][half][cout % 32][8] bf16 — the B fragment of one wavefront for one
// (tap, 16-deep k-step, 32-column tile) is 64 lanes x 16 bytes = ONE contiguous KB (lane l = half * 32 + column reads bytes [16 l, 16 l + 16)),
// against the 32-byte pieces the fp32 kernel gathers from the [C][k][C] image.  Rounded here, once (round to nearest even).
// One thread per 8 elements: 8 consecutive cin of one (cout, tap).
__global__ void hg_pack_bf16_kernel(const float* __restrict__ w, bf16_t* __restrict__ out, int C, int k) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;   // one 16-byte piece of the image
    if (i >= C * k * (C / 8)) return;
    const int TN = C / 32, KS = C / 16;
    const int n32 = i & 31, h = (i >> 5) & 1, j = (i >> 6) % TN, q = ((i >> 6) / TN) % KS, t = (i >> 6) / (TN * KS);
    const float* src = w + ((long long)(j * 32 + n32) * k + t) * C + 16 * q + 8 * h;
    const float4 lo = ld4(src), hi = ld4(src + 4);
    u32x4 v;
    v.x = pack2_bf16(lo.x, lo.y); v.y = pack2_bf16(lo.z, lo.w); v.z = pack2_bf16(hi.x, hi.y); v.w = pack2_bf16(hi.z, hi.w);
    *reinterpret_cast<u32x4*>(out + (long long)i * 8) = v;
}

// Direct route of the bf16 mode: the convolution of hg_conv_direct_kernel with both operands rounded to bf16, exact products, fp32
// accumulation (v_mfma_f32_32x32x16_bf16).  Same tile contract (128 output rows per workgroup, wave w owns rows [32 w, 32 w + 32) x all C
// columns) and the same three epilogues in fp32 registers.  wpk: the image of hg_pack_bf16_kernel, streamed from L2 (not staged in LDS: at
// C = 128 a tap's slab is 32 KB beside 48.4 KB of activations).  LDS: (128 + (k-1) d) rows of C + 8 bf16, LeakyReLU and the utterance-end
// zeros applied on the way in, one packed convert per two elements: 48.4 KB at C = 128, 25.6 KB at C = 64, 14.2 KB at C = 32.  Fragments as in
// bf16_compute_slice: lane l feeds row / column l & 31 and the 8 consecutive k of half l >> 5; a dilated tap is a row offset t d.
struct HgConvBf16Args {
    HgConvArgs a;
    const bf16_t* wpk = nullptr;
};
template <int C>
__global__ __launch_bounds__(256) void hg_conv_direct_bf16_kernel(HgConvBf16Args p) {
    constexpr int LDA = C + 8, TN = C / 32, KS = C / 16;
    __shared__ __attribute__((aligned(16))) bf16_t As[(kHgTileRows + kHgMaxHalo) * LDA];
    const HgConvArgs& a = p.a;
    const int z = blockIdx.z, tid = (int)threadIdx.x;
    const int T = a.lens[z] * a.len_mult, m0 = (int)blockIdx.x * kHgTileRows;
    if (m0 >= T) return;   // (uniform over the workgroup, before the barrier)
    const int halo = (a.k - 1) * a.d, pad = halo >> 1, nrows = kHgTileRows + halo;
    const float* px = a.x + (long long)z * a.x_gs;
    for (int i = tid; i < nrows * (C / 8); i += 256) {
        const int lr = i / (C / 8), c = (i - lr * (C / 8)) * 8;
        const int row = m0 - pad + lr;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (row >= 0 && row < T) {
            const float4 lo = ld4(px + (long long)row * C + c), hi = ld4(px + (long long)row * C + c + 4);
            v.x = pack2_bf16(hg_lrelu(lo.x, a.in_slope), hg_lrelu(lo.y, a.in_slope));
            v.y = pack2_bf16(hg_lrelu(lo.z, a.in_slope), hg_lrelu(lo.w, a.in_slope));
            v.z = pack2_bf16(hg_lrelu(hi.x, a.in_slope), hg_lrelu(hi.y, a.in_slope));
            v.w = pack2_bf16(hg_lrelu(hi.z, a.in_slope), hg_lrelu(hi.w, a.in_slope));
        }
        *reinterpret_cast<u32x4*>(As + lr * LDA + c) = v;
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    f32x16 acc[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
#if defined(MTTS_EMU)
    for (int j = 0; j < TN; ++j)
        for (int r = 0; r < 16; ++r) {
            const int lr = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            float s = 0.f;
            for (int t = 0; t < a.k; ++t)
                for (int c = 0; c < C; ++c) {
                    const long long wi = ((((long long)(t * KS + (c >> 4)) * TN + j) * 2 + ((c >> 3) & 1)) * 32 + l31) * 8 + (c & 7);
                    s = fmaf(bf16_to_f32(As[(lr + t * a.d) * LDA + c]), bf16_to_f32(p.wpk[wi]), s);
                }
            acc[j][r] = s;
        }
#else
    for (int t = 0; t < a.k; ++t) {
        const bf16_t* pa = As + (wave * 32 + l31 + t * a.d) * LDA + 8 * h;
        const bf16_t* pw = p.wpk + (long long)t * KS * TN * 512 + lane * 8;
#pragma unroll
        for (int q = 0; q < KS; ++q) {
            const bf16x8 av = *reinterpret_cast<const bf16x8*>(pa + 16 * q);
            bf16x8 bv[TN];
#pragma unroll
            for (int j = 0; j < TN; ++j) bv[j] = *reinterpret_cast<const bf16x8*>(pw + (q * TN + j) * 512);
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv[j], acc[j], 0, 0, 0);
        }
    }
#endif
    const float* pres = a.res ? a.res + (long long)z * a.res_gs : nullptr;
    float* pout = a.out ? a.out + (long long)z * a.out_gs : nullptr;
    float* pmrf = a.mrf ? a.mrf + (long long)z * a.mrf_gs : nullptr;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = j * 32 + l31;
        const float bv = a.bias[n];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (m >= T) continue;
            const long long o = (long long)m * C + n;
            float v = acc[j][r] + bv;
            if (a.mode == 0) pout[o] = hg_lrelu(v, 0.1f);
            else {
                v += pres[o];
                if (a.mode == 1) pout[o] = v;
                else pmrf[o] = (a.mrf_init ? 0.f : pmrf[o]) + a.inv_nk * v;
            }
        }
    }
}
constexpr bool hg_direct_bf16_channels(int C) { return C == 32 || C == 64 || C == 128; }   // (C = 256 is not built: 94 KB of activations)

class HifiGan : public WaveGen {
public:
    HifiGanCfg cfg;
    int numerics = 0;           // 0: fp32 (the default); 1: bf16 operands (set_numerics)
    bf16_t* wpk = nullptr;      // bf16 mode: the direct kernel's weight images, at the offsets of the tensor table (residual convolutions of 32 / 64 / 128 channels)
    Buf b_up, b_xj, b_pad, b_h, b_mrf;   // stage input, running x of a block, padded operand, t of a pair, MRF sum
    using Tensor = ParamTable::Tensor;

    HifiGan() { kind = "HiFi-GAN"; act_slope = 0.1f; }
    int ch(int stage) const { return cfg.c0 >> stage; }   // channels after `stage` upsamples
    bool direct(int C) const { return (numerics ? hg_direct_bf16_channels(C) : (C == 32 || C == 64)) && C <= cfg.direct_max; }

    // bf16 mode: (re)build the direct kernel's image of one tensor, if it is a residual convolution of a channel count the kernel is built for
    void pack_tensor(const Tensor& t) {
        if (t.name.compare(0, 10, "resblocks.") != 0 || t.name.size() < 2 || t.name.compare(t.name.size() - 2, 2, ".w") != 0) return;
        for (int s = 0; s < cfg.n_up; ++s) {
            const int C = ch(s + 1);
            if (!hg_direct_bf16_channels(C)) continue;
            for (int j = 0; j < cfg.n_k; ++j) {
                const std::string pre = "resblocks." + std::to_string(s * cfg.n_k + j) + ".";
                if (t.name.compare(0, pre.size(), pre) != 0) continue;
                const int k = cfg.kernels[j], pieces = C * k * (C / 8);
                MTTS_LAUNCH(hg_pack_bf16_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), stream, (const float*)(tab.data + t.off), wpk + t.off, C, k);
                return;
            }
        }
    }
    // mode 0: fp32, direct_max in {0, 32, 64} — what create built; mode 1: bf16 operands, direct_max in {0, 32, 64, 128}.  Refused before any launch.
    int set_numerics(int mode, int direct_max) {
        if (mode != 0 && mode != 1) return err("mtts_hifigan_set_numerics: mode = " + std::to_string(mode) + " (0: fp32, 1: bf16 operands)");
        const bool ok = direct_max == 0 || direct_max == 32 || direct_max == 64 || (mode == 1 && direct_max == 128);
        if (!ok) return err("mtts_hifigan_set_numerics: direct_max_channels = " + std::to_string(direct_max) + (mode ? " (bf16 operands: 0, 32, 64 or 128)" : " (fp32: 0, 32 or 64)"));
        if (mode == 1) {
            if (!wpk) {
                for (const Tensor& t : tab.tensors) if (t.off % 8) return err("mtts_hifigan_set_numerics: tensor " + t.name + " is not 16-byte aligned in the bf16 image");
                DEV_CHECK(mem.alloc(wpk, (size_t)tab.n_params * sizeof(bf16_t)));
            }
            numerics = 1;   // (pack_tensor needs no mode; set first so that a failure below leaves a consistent handle)
            for (const Tensor& t : tab.tensors) pack_tensor(t);
            DEV_CHECK(hipStreamSynchronize(stream));
        }
        numerics = mode; cfg.direct_max = direct_max;
        gx.bf16 = mode == 1; gx.no_splitk = mode == 1;   // (no split-K: the split factor follows the batch, and an utterance must not)
        return 0;
    }

    int init(const HifiGanCfg& c, int max_B, int max_T) {
        cfg = c; cap_B = max_B; cap_T = max_T;
        const std::string why = hifigan_check_cfg(c, max_B, max_T);
        if (!why.empty()) return err("mtts_hifigan_create: " + why);
        hop = 1;
        for (int s = 0; s < cfg.n_up; ++s) hop *= cfg.rates[s];
        tab.add("conv_pre.w", (long long)cfg.c0 * 7 * cfg.n_mel); tab.add("conv_pre.b", cfg.c0);
        for (int s = 0; s < cfg.n_up; ++s) {
            const int cin = ch(s), cout = ch(s + 1), r = cfg.rates[s];
            tab.add("ups." + std::to_string(s) + ".w", (long long)r * cout * 2 * cin);   // [phase][C_out][x[q-1] | x[q]]
            tab.add("ups." + std::to_string(s) + ".b", cout);
            for (int j = 0; j < cfg.n_k; ++j)
                for (int m = 0; m < cfg.n_dil; ++m)
                    for (int half = 1; half <= 2; ++half) {
                        const std::string p = "resblocks." + std::to_string(s * cfg.n_k + j) + ".convs" + std::to_string(half) + "." + std::to_string(m);
                        tab.add(p + ".w", (long long)cout * cfg.kernels[j] * cout); tab.add(p + ".b", cout);   // [C][k][C]
                    }
        }
        tab.add("conv_post.w", 7LL * ch(cfg.n_up)); tab.add("conv_post.b", 1);
        long long worst = (long long)(cap_T + 32) * std::max(cfg.n_mel, cfg.c0);
        long long mult = 1;
        for (int s = 0; s < cfg.n_up; ++s) { mult *= cfg.rates[s]; worst = std::max(worst, ((long long)cap_T * mult + kHgMaxHalo + 32) * ch(s + 1)); }
        if (alloc_common(5, (worst + 63) & ~63LL, cfg.n_mel) != 0) return -1;
        b_up = buf(0); b_xj = buf(1); b_pad = buf(2); b_h = buf(3); b_mrf = buf(4);
        return 0;
    }
    int load(const char* name, const float* host, long long numel) {
        const Tensor* t = tab.load(name, host, numel, kind, last_error);
        if (!t) return -1;
        if (numerics == 1) { pack_tensor(*t); DEV_CHECK(hipStreamSynchronize(stream)); }   // a tensor loaded after the mode was set
        return 0;
    }

    void pad(HgPadArgs a, int B, int max_rows, int len_mult, int C) {
        a.lens = lens_dev; a.len_mult = len_mult; a.C = C;
        const long long n = std::max<long long>((long long)(max_rows + 2 * a.d) * (C / 4), 2LL * a.gp * (C / 4));
        MTTS_LAUNCH(hg_pad_kernel, dim3((unsigned)((n + 255) / 256), 1, (unsigned)B), dim3(256), stream, a);
    }
    void conv_direct(HgConvArgs a, int B, int max_rows, int len_mult, int C, const bf16_t* image = nullptr) {
        a.lens = lens_dev; a.len_mult = len_mult;
        const dim3 grid((unsigned)((max_rows + kHgTileRows - 1) / kHgTileRows), 1, (unsigned)B);
        if (numerics == 1) {
            HgConvBf16Args p;
            p.a = a; p.wpk = image ? image : wpk + (a.w - tab.data);   // (a.w names the tensor: its image sits at the same offset)
            if (C == 128) MTTS_LAUNCH(hg_conv_direct_bf16_kernel<128>, grid, dim3(256), stream, p);
            else if (C == 64) MTTS_LAUNCH(hg_conv_direct_bf16_kernel<64>, grid, dim3(256), stream, p);
            else MTTS_LAUNCH(hg_conv_direct_bf16_kernel<32>, grid, dim3(256), stream, p);
            return;
        }
        if (C == 64) MTTS_LAUNCH(hg_conv_direct_kernel<64>, grid, dim3(256), stream, a);
        else MTTS_LAUNCH(hg_conv_direct_kernel<32>, grid, dim3(256), stream, a);
    }

    // mel: device pointer [B][T_max][n_mel]; wav: device [B][wav_gs]; mel_gs: floats between utterances of `mel` (0: T_max * n_mel)
    int run(const float* mel, int B, int T_max, const int* lens_host, float mel_scale, float* wav, long long wav_gs, long long mel_gs = 0) {
        if (check_batch(B, T_max, lens_host) != 0) return -1;
        DEV_CHECK(hipMemcpyAsync(lens_dev, lens_host, B * sizeof(int), hipMemcpyHostToDevice, stream));
        const int nm = cfg.n_mel;
        {   // conv_pre: zero pad 3 of the scaled mel, k = 7
            HgPadArgs p;
            p.x = mel; p.x_gs = mel_gs > 0 ? mel_gs : (long long)T_max * nm; p.xs = mel_scale; p.y = at(b_pad); p.y_gs = b_pad.gs; p.d = 3; p.slope = 1.f;
            pad(p, B, T_max, 1, nm);
            gemm(at(b_pad), b_pad.gs, nm, P("conv_pre.w"), 7 * nm, 7 * nm, P("conv_pre.b"), at(b_up), b_up.gs, ch(0), ch(0), B, T_max, 1, 0);
        }
        // what the next stage reads: xs * src (+ add)
        HgPadArgs next;
        next.x = at(b_up); next.x_gs = b_up.gs;
        int mult = 1;
        const float inv_nk = 1.f / (float)cfg.n_k;
        for (int s = 0; s < cfg.n_up; ++s) {
            const int cin = ch(s), C = ch(s + 1), r = cfg.rates[s];
            const int rows_in = T_max * mult;
            {   // LeakyReLU + one zero row each side, then r polyphase GEMMs into the stage input
                HgPadArgs a = next;
                a.y = at(b_pad); a.y_gs = b_pad.gs; a.d = 1; a.slope = 0.1f;
                pad(a, B, rows_in, mult, cin);
                upsample_polyphase(b_pad, P("ups." + std::to_string(s) + ".w"), P("ups." + std::to_string(s) + ".b"), b_up, cin, C, r, B, rows_in, mult);
            }
            mult *= r;
            const int rows = T_max * mult;
            const bool dir = direct(C);
            for (int j = 0; j < cfg.n_k; ++j) {
                const int k = cfg.kernels[j], p2 = (k - 1) / 2;
                for (int m = 0; m < cfg.n_dil; ++m) {
                    const int d = cfg.dil[j][m];
                    const std::string pre = "resblocks." + std::to_string(s * cfg.n_k + j);
                    const float* w1 = P(pre + ".convs1." + std::to_string(m) + ".w");
                    const float* b1 = P(pre + ".convs1." + std::to_string(m) + ".b");
                    const float* w2 = P(pre + ".convs2." + std::to_string(m) + ".w");
                    const float* b2 = P(pre + ".convs2." + std::to_string(m) + ".b");
                    const Buf& src = m == 0 ? b_up : b_xj;
                    if (dir) {
                        HgConvArgs c1;
                        c1.x = at(src); c1.x_gs = src.gs; c1.in_slope = 0.1f; c1.w = w1; c1.bias = b1; c1.k = k; c1.d = d;
                        c1.out = at(b_h); c1.out_gs = b_h.gs; c1.mode = 0;
                        conv_direct(c1, B, rows, mult, C);
                        HgConvArgs c2;
                        c2.x = at(b_h); c2.x_gs = b_h.gs; c2.in_slope = 1.f; c2.w = w2; c2.bias = b2; c2.k = k; c2.d = 1;
                        c2.res = at(src); c2.res_gs = src.gs;
                        if (m == cfg.n_dil - 1) { c2.mode = 2; c2.mrf = at(b_mrf); c2.mrf_gs = b_mrf.gs; c2.inv_nk = inv_nk; c2.mrf_init = j == 0; }
                        else { c2.mode = 1; c2.out = at(b_xj); c2.out_gs = b_xj.gs; }
                        conv_direct(c2, B, rows, mult, C);
                    } else {
                        HgPadArgs a;
                        a.x = at(src); a.x_gs = src.gs; a.y = at(b_pad); a.y_gs = b_pad.gs; a.d = d * p2; a.slope = 0.1f;
                        a.guard = at(b_h); a.guard_gs = b_h.gs; a.gp = p2;
                        if (m == 0) {
                            if (j > 0) { a.fold = at(b_xj); a.fold_gs = b_xj.gs; a.fs = inv_nk; a.fold_init = j == 1; a.mrf = at(b_mrf); a.mrf_gs = b_mrf.gs; }
                            a.copy = at(b_xj); a.copy_gs = b_xj.gs;
                        }
                        pad(a, B, rows, mult, C);
                        conv_gemm(at(b_pad), b_pad.gs, w1, b1, at(b_h) + (long long)p2 * C, b_h.gs, C, k, d, B, rows, mult, GEMM_LRELU);
                        conv_gemm(at(b_h), b_h.gs, w2, b2, at(b_xj), b_xj.gs, C, k, 1, B, rows, mult, GEMM_ACCUM);
                    }
                }
            }
            next = HgPadArgs();
            if (dir) { next.x = at(b_mrf); next.x_gs = b_mrf.gs; }
            else {
                next.x = at(b_xj); next.x_gs = b_xj.gs; next.xs = inv_nk;
                if (cfg.n_k > 1) { next.add = at(b_mrf); next.add_gs = b_mrf.gs; }
            }
        }
        // LeakyReLU(0.01), zero pad 3, k = 7 conv to one channel, tanh
        const int cl = ch(cfg.n_up), rows = T_max * mult;
        next.y = at(b_pad); next.y_gs = b_pad.gs; next.d = 3; next.slope = 0.01f;
        pad(next, B, rows, mult, cl);
        MTTS_LAUNCH(dot_tanh_kernel, dim3((unsigned)((rows + 3) / 4), 1, (unsigned)B), dim3(256), stream, (const int*)lens_dev, mult,
                    (const float*)at(b_pad), b_pad.gs, P("conv_post.w"), P("conv_post.b"),
                    wav, wav_gs, cl, 7 * cl);
        return 0;
    }

    // Kernel-level entry (mtts_hifigan_conv_bf16): ONE convolution of the bf16 mode on host arrays, without the network around it.
    //   out / mrf = epilogue(bias + conv(k, dilation d, zero pad d (k-1)/2)(bf16(leaky_relu(x, in_slope))) with bf16(w)), modes as HgConvArgs.
    // x, res, out, mrf: [B][T_max][C]; w: [C][k][C]; rows >= lens[b] of out / mrf are left as the caller filled them.
    // route 0: hg_conv_direct_bf16_kernel; route 1: the GEMM route of the same convolution (hg_pad_kernel, the bf16 GEMM family through
    // this handle's GemmCtx, accumulate epilogue for the residual, the pad pass's fold for the MRF sum).
    int conv_bf16_host(int route, int C, int k, int d, int B, int T_max, const int* lens_host, const float* x, const float* w, const float* bias,
                       float in_slope, int mode, const float* res, float* mrf, float inv_nk, int mrf_init, float* out) {
        const std::string e = "mtts_hifigan_conv_bf16: ";
        if (route != 0 && route != 1) return err(e + "route = " + std::to_string(route) + " (0: direct kernel, 1: GEMM route)");
        if (!hg_direct_bf16_channels(C)) return err(e + "C = " + std::to_string(C) + " (32, 64 or 128)");
        if (k < 1 || !(k & 1) || k > kHgMaxResKernel) return err(e + "k = " + std::to_string(k) + " (odd, <= " + std::to_string(kHgMaxResKernel) + ")");
        if (d < 1 || d > kHgMaxDilation) return err(e + "d = " + std::to_string(d) + " (1.." + std::to_string(kHgMaxDilation) + ")");
        if (mode < 0 || mode > 2) return err(e + "mode = " + std::to_string(mode) + " (0, 1 or 2)");
        if (B < 1 || B > cap_B) return err(e + "B = " + std::to_string(B) + " exceeds max_B = " + std::to_string(cap_B));
        if (T_max < 1 || !lens_host || !x || !w || !bias) return err(e + "NULL argument or T_max < 1");
        for (int b = 0; b < B; ++b)
            if (lens_host[b] < 1 || lens_host[b] > T_max) return err(e + "lens[" + std::to_string(b) + "] = " + std::to_string(lens_host[b]) + " out of range (1..T_max)");
        if ((mode == 0 || mode == 1) && !out) return err(e + "out is NULL");
        if (mode >= 1 && !res) return err(e + "res is NULL");
        if (mode == 2 && !mrf) return err(e + "mrf is NULL");
        const int p2 = (k - 1) / 2, hp = d * p2;
        const long long gs = (long long)T_max * C, pgs = (long long)(T_max + 2 * hp + 8) * C, nw = (long long)C * k * C;
        const size_t bytes = (size_t)gs * B * sizeof(float);
        float *dx = nullptr, *dres = nullptr, *dout = nullptr, *dmrf = nullptr, *dpad = nullptr, *dw = nullptr, *db = nullptr;
        bf16_t* dimg = nullptr;
        struct Saved { HifiGan& h; int num; bool b, s; ~Saved() { h.numerics = num; h.gx.bf16 = b; h.gx.no_splitk = s; } } saved{*this, numerics, gx.bf16, gx.no_splitk};
        auto done = [&](int rc) { mem.give_back(dx); mem.give_back(dres); mem.give_back(dout); mem.give_back(dmrf); mem.give_back(dpad); mem.give_back(dw); mem.give_back(db); mem.give_back(dimg); return rc; };
#define HG_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return done(err(std::string(#x) + ": " + hipGetErrorString(e_))); } while (0)
        HG_TRY(hipStreamSynchronize(stream));   // (lens_dev may still be read by an earlier run)
        HG_TRY(mem.alloc(dx, bytes)); HG_TRY(mem.alloc(dres, bytes)); HG_TRY(mem.alloc(dout, bytes)); HG_TRY(mem.alloc(dmrf, bytes));
        HG_TRY(mem.alloc(dpad, (size_t)pgs * B * sizeof(float))); HG_TRY(mem.alloc(dw, (size_t)nw * sizeof(float))); HG_TRY(mem.alloc(db, C * sizeof(float)));
        HG_TRY(mem.alloc(dimg, (size_t)nw * sizeof(bf16_t)));
        HG_TRY(hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice));
        HG_TRY(hipMemcpy(dw, w, (size_t)nw * sizeof(float), hipMemcpyHostToDevice));
        HG_TRY(hipMemcpy(db, bias, C * sizeof(float), hipMemcpyHostToDevice));
        if (res) HG_TRY(hipMemcpy(dres, res, bytes, hipMemcpyHostToDevice));
        if (mrf) HG_TRY(hipMemcpy(dmrf, mrf, bytes, hipMemcpyHostToDevice));
        if (out) HG_TRY(hipMemcpy(dout, out, bytes, hipMemcpyHostToDevice));
        HG_TRY(hipMemcpy(lens_dev, lens_host, B * sizeof(int), hipMemcpyHostToDevice));
        numerics = 1; gx.bf16 = true; gx.no_splitk = true;
        if (route == 0) {
            MTTS_LAUNCH(hg_pack_bf16_kernel, dim3((unsigned)((nw / 8 + 255) / 256)), dim3(256), stream, (const float*)dw, dimg, C, k);
            HgConvArgs c;
            c.x = dx; c.x_gs = gs; c.in_slope = in_slope; c.w = dw; c.bias = db; c.k = k; c.d = d; c.mode = mode;
            c.res = dres; c.res_gs = gs; c.out = dout; c.out_gs = gs; c.mrf = dmrf; c.mrf_gs = gs; c.inv_nk = inv_nk; c.mrf_init = mrf_init;
            conv_direct(c, B, T_max, 1, C, dimg);
        } else {
            HgPadArgs a;
            a.x = dx; a.x_gs = gs; a.y = dpad; a.y_gs = pgs; a.d = hp; a.slope = in_slope;
            pad(a, B, T_max, 1, C);
            // the residual add is the accumulate epilogue: the valid rows of the target start as res
            float* acc_to = mode == 1 ? dout : dx;   // (mode 2: x has been consumed by the pad pass)
            if (mode >= 1)
                for (int b = 0; b < B; ++b)
                    HG_TRY(hipMemcpyAsync(acc_to + b * gs, dres + b * gs, (size_t)lens_host[b] * C * sizeof(float), hipMemcpyDeviceToDevice, stream));
            conv_gemm(dpad, pgs, dw, db, mode == 0 ? dout : acc_to, gs, C, k, d, B, T_max, 1, mode == 0 ? GEMM_LRELU : GEMM_ACCUM);
            if (mode == 2) {
                HgPadArgs f;
                f.x = acc_to; f.x_gs = gs; f.y = dpad; f.y_gs = pgs; f.d = 0; f.slope = 1.f;
                f.fold = acc_to; f.fold_gs = gs; f.fs = inv_nk; f.fold_init = mrf_init; f.mrf = dmrf; f.mrf_gs = gs;
                pad(f, B, T_max, 1, C);
            }
        }
        if (gx.error) { const std::string m = std::string("GEMM launcher: ") + gx.error; gx.error = nullptr; return done(err(e + m)); }
        HG_TRY(hipGetLastError());
        HG_TRY(hipStreamSynchronize(stream));
        if (mode <= 1) HG_TRY(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
        else HG_TRY(hipMemcpy(mrf, dmrf, bytes, hipMemcpyDeviceToHost));
#undef HG_TRY
        return done(0);
    }
};

}  // namespace mtts
