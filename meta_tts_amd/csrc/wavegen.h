// What the two mel-to-waveform generators (Vocoder: MelGAN, vocoder.h; HifiGan: hifigan.h) share on the host: capacities, the tensor
// table, the activation arena and I/O buffers, the grouped GEMM over ragged utterances with its convolution and transposed-convolution
// forms, the batch checks and the host entry.  A plain base class: nothing is virtual, the subclass's `run` is reached through a template.
// No kernel lives here; the subclasses keep theirs.
#pragma once
#include <string>

#include "gemm.h"
#include "params.h"

namespace mtts {

class WaveGen {
public:
    const char* kind = "";      // the network's name in messages (set by the subclass)
    float act_slope = 0.f;      // LeakyReLU slope of the GEMM epilogue (GEMM_LRELU)
    int n_mel = 0, cap_B = 0, cap_T = 0, hop = 1;
    hipStream_t stream = nullptr;
    std::string last_error;
    ParamTable tab;
    GemmCtx gx;                 // this handle's launcher state (gemm.h)
    DevHeap mem;                // every device block of this handle (devres.h)
    // per-stage scratch: element offsets into the arena, per-utterance strides
    struct Buf { long long off, gs; };
    float* arena = nullptr;
    long long per_utt = 0;
    int* lens_dev = nullptr;
    float* mel_dev = nullptr;
    float* wav_dev = nullptr;

    int err(const std::string& s) { last_error = s; return -1; }
    void set_error(const std::string& s) { err(s); }
    float* at(const Buf& b) const { return arena + b.off; }
    Buf buf(int i) const { return Buf{i * per_utt * cap_B, per_utt}; }
    const float* P(const std::string& n) const { return tab.ptr(n); }

    // split-K workspace, the (filled) tensor table, n_bufs zeroed arena buffers of per_utt_floats per utterance, lengths, mel and waveform
    int alloc_common(int n_bufs, long long per_utt_floats, int n_mel_) {
        n_mel = n_mel_; per_utt = per_utt_floats;
        if (gx.alloc_workspace(mem)) return err("out of device memory (split-K workspace)");
        DEV_CHECK(tab.alloc(mem));
        DEV_CHECK(mem.alloc_zeroed(arena, (size_t)per_utt * cap_B * n_bufs * sizeof(float)));
        DEV_CHECK(mem.alloc(lens_dev, cap_B * sizeof(int)));
        DEV_CHECK(mem.alloc(mel_dev, (size_t)cap_B * cap_T * n_mel * sizeof(float)));
        DEV_CHECK(mem.alloc(wav_dev, (size_t)cap_B * cap_T * hop * sizeof(float)));
        return 0;
    }

    // one grouped GEMM: C[z][M_z, N] (+)= A[z][M_z, K] * W[N, K]^T + bias; M_z = lens[z] * len_mult
    void gemm(const float* A, long long a_gs, int lda, const float* W, int ldb, int K, const float* bias, float* C, long long c_gs,
              int ldc, int N, int B, int max_rows, int len_mult, int flags, int a_tap_k = 0, int a_tap_rows = 0) {
        GemmArgs g;
        if (a_tap_k > 0) { g.a_tap_k = a_tap_k; g.a_tap_rows = a_tap_rows; }
        g.A = A; g.a_gs = a_gs; g.lda = lda;
        g.B = W; g.b_gs = 0; g.ldb = ldb;
        g.C = C; g.c_gs = c_gs; g.ldc = ldc;
        g.M = max_rows; g.N = N; g.K = K;
        g.dimptr = lens_dev; g.dim_stride = 1; g.dim_sel = 0; g.dim_mult = len_mult;
        g.bias = bias; g.flags = flags; g.act_slope = act_slope;
        gemm_launch(gx, GEMM_NT, g, max_rows, N, B, stream, 0, 2.0 * max_rows * B * (double)N * K, 0);
    }
    // a convolution of k taps, dilation d, over the padded rows at A (row 0 = the first pad row), w [C][k][C]: out (+)= conv + bias.
    // d == 1: the implicit GEMM over overlapping rows; C % 32 == 0: the taps inside the K-loop (k = t * C + c reads row m + t * d);
    // else one accumulate pass per tap: bias on tap 0, GEMM_ACCUM on taps > 0, the caller's GEMM_LRELU on the last.
    void conv_gemm(const float* A, long long a_gs, const float* w, const float* bias, float* out, long long out_gs, int C, int k, int d, int B, int rows,
                   int mult, int flags) {
        if (d == 1) gemm(A, a_gs, C, w, k * C, k * C, bias, out, out_gs, C, C, B, rows, mult, flags);
        else if (C % 32 == 0) gemm(A, a_gs, C, w, k * C, k * C, bias, out, out_gs, C, C, B, rows, mult, flags, C, d);
        else
            for (int t = 0; t < k; ++t)
                gemm(A + (long long)t * d * C, a_gs, C, w + (long long)t * C, k * C, C, t == 0 ? bias : nullptr, out, out_gs, C, C, B, rows, mult,
                     (t ? GEMM_ACCUM : (flags & GEMM_ACCUM)) | (t == k - 1 ? (flags & GEMM_LRELU) : 0));
    }
    // ConvTranspose1d (k = 2r, stride r, pad r / 2; r even) as r polyphase GEMMs in one multi-problem launch: output o = q r + ph - r / 2
    // reads the contiguous pair [x[q-1] | x[q]] of `src` (the activated input with one zero row each side); W [phase][cout][2 cin].
    void upsample_polyphase(const Buf& src, const float* W, const float* bias, const Buf& dst, int cin, int cout, int r, int B, int rows_in, int mult) {
        const int p = r / 2;
        gemm_batch_begin(gx);
        for (int ph = 0; ph < r; ++ph) {
            const int q0 = ph >= p ? 0 : 1;
            gemm(at(src) + (long long)q0 * cin, src.gs, cin, W + (long long)ph * cout * 2 * cin, 2 * cin, 2 * cin, bias,
                 at(dst) + (long long)(q0 * r + ph - p) * cout, dst.gs, r * cout, cout, B, rows_in, mult, 0);
        }
        gemm_batch_end(gx, stream);
    }

    int load(const char* name, const float* host, long long numel) { return tab.load(name, host, numel, kind, last_error) ? 0 : -1; }
    int check_batch(int B, int T_max, const int* lens_host) {
        const std::string k = std::string(kind) + ": ";
        if (B < 1 || B > cap_B) return err(k + "B = " + std::to_string(B) + " exceeds max_B = " + std::to_string(cap_B));
        if (T_max < 4 || T_max > cap_T) return err(k + "T_max = " + std::to_string(T_max) + " out of range (need 4 <= T_max <= max_T = " + std::to_string(cap_T) + ")");
        for (int b = 0; b < B; ++b)
            if (lens_host[b] < 4 || lens_host[b] > T_max)
                return err(k + "mel_lens[" + std::to_string(b) + "] = " + std::to_string(lens_host[b]) + " out of range (need 4 <= len <= T_max = " + std::to_string(T_max) + ")");
        return 0;
    }
    // host entry: mel_host [B][T_max][n_mel] -> wav_host [B][T_max * hop] (samples beyond len * hop are left untouched)
    template <class Gen>
    static int infer_host(Gen& g, const float* mel_host, int B, int T_max, const int* lens_host, float mel_scale, float* wav_host) {
        auto err = [&g](const std::string& s) { return g.err(s); };   // (for DEV_CHECK)
        if (g.check_batch(B, T_max, lens_host) != 0) return -1;
        const long long gs = (long long)T_max * g.hop;
        DEV_CHECK(hipMemcpyAsync(g.mel_dev, mel_host, (size_t)B * T_max * g.n_mel * sizeof(float), hipMemcpyHostToDevice, g.stream));
        if (g.run(g.mel_dev, B, T_max, lens_host, mel_scale, g.wav_dev, gs) != 0) return -1;
        DEV_CHECK(hipStreamSynchronize(g.stream));
        for (int b = 0; b < B; ++b)
            DEV_CHECK(hipMemcpy(wav_host + b * gs, g.wav_dev + b * gs, (size_t)lens_host[b] * g.hop * sizeof(float), hipMemcpyDeviceToHost));
        return 0;
    }
    // Launches are asynchronous: a launcher refusal or a rejected launch shows only here.  Every compute entry ends with it.
    int launched(int rc) {
        if (rc) return rc;
        if (gx.error) { set_error(std::string("GEMM launcher: ") + gx.error); gx.error = nullptr; return -1; }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return err(std::string("kernel launch failed: ") + hipGetErrorString(e));
        return 0;
    }
};

}  // namespace mtts
