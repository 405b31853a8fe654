// Spectrogram -> waveform on the device: the inverse half of the reference's `audio` package.
//
// Reference: audio/stft.py:52-77 (STFT.transform: reflect padding by n_fft/2 WITHOUT the [-1, 1] clip of get_mel_from_wav, strided Conv1d
// against the windowed Fourier basis, magnitude and atan2 phase), :79-119 (STFT.inverse: conv_transpose1d of [M cos p | M sin p] against
// the windowed pseudo-inverse basis, division by the window's sum-square envelope where it exceeds float32 `tiny`, x n_fft / hop, trim
// n_fft / 2 at both ends), audio/audio_processing.py:7-80 (window_sumsquare, griffin_lim) and audio/tools.py:18-37 (inv_mel_spec:
// exp(mel)^T @ mel_basis x 1000, last frame dropped, Griffin-Lim).
//
// MI355X layout.  Every utterance of a call goes through the same launches; frames are rows ([frame][bin], the engine's layout).
//   * R [sum T][ld_spec] = [M cos p | M sin p | 0 pad] — the recombined spectrum, zero padded to the GEMM's K alignment;
//   * inverse GEMM (NT against the stored transpose of the inverse basis, [n_fft][ld_spec], zero padded columns):
//     frames [sum T][n_fft] = R * inverse_basis;
//   * overlap-add (gl_overlap_add_kernel): a deterministic gather of the <= ceil(n_fft / hop) frames that cover a sample, the envelope
//     derived from the squared window in the same loop, and the next transform's reflect-padded input written directly (the trimmed
//     waveform on the last pass);
//   * forward GEMM: melfront.h's MelFront::forward_stft over the packed padded signals (MelFront's packing: one NT launch covers all
//     utterances, the straddling rows are dropped through the row map and the spectrum lands compact in R's buffer);
//   * phasor (gl_phasor_kernel, in place): R = M * (re, im) / |z| = (M cos atan2, M sin atan2) without the transcendentals.
// One Griffin-Lim iteration is these four launches on the handle's stream.  The packed waveforms, the padded signals, R, the magnitude,
// the log-mel, the row map and the utterance table live in MelFront's workspace; this file owns the frames, the angles, exp(mel), the
// mel GEMM's row map, the inverse basis and the squared window.
#pragma once
#include <cfloat>
#include <string>
#include <vector>

#include "melfront.h"

namespace mtts {

// spec [T][ld] = [re | im] -> magnitude [T][F] = sqrt(re^2 + im^2), phase [T][F] = atan2(im, re)   (stft.py:71-75)
__global__ void gl_mag_phase_kernel(const float* spec, int ld, int T, int F, float* mag, float* phase) {
    const long long total = (long long)T * F;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long t = i / F;
        const int f = (int)(i - t * F);
        const float re = spec[t * ld + f], im = spec[t * ld + F + f];
        mag[i] = sqrtf(re * re + im * im);
        phase[i] = atan2f(im, re);
    }
}

// out [rows][ldo] = exp(log_mel [rows][n_mel]), columns n_mel .. ldo zeroed (TacotronSTFT.spectral_de_normalize, C = 1)
__global__ void gl_exp_rows_kernel(const float* x, int rows, int n_mel, float* out, int ldo) {
    const long long total = (long long)rows * ldo;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / ldo;
        const int c = (int)(i - r * ldo);
        out[i] = c < n_mel ? expf(x[r * n_mel + c]) : 0.f;
    }
}

// First pass: R[t] = [M cos a | M sin a | 0] from the host-drawn angles a [T][F]   (stft.py:80-82)
__global__ void gl_phasor_init_kernel(const float* mag, int ldm, const float* ang, int T, int F, float* R, int ldr) {
    const long long total = (long long)T * ldr;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long t = i / ldr;
        const int c = (int)(i - t * ldr);
        float v = 0.f;
        if (c < 2 * F) {
            const int f = c < F ? c : c - F;
            const float m = mag[t * ldm + f], a = ang[t * F + f];
            v = c < F ? m * cosf(a) : m * sinf(a);
        }
        R[i] = v;
    }
}

// In place: R[t] = [re | im | pad] -> [M re / |z| | M im / |z| | 0]  =  (M cos atan2(im, re), M sin atan2(im, re)).
// |z| == 0 follows atan2's signs: re = +0 -> (M, 0), re = -0 -> (-M, 0).  A pair whose squares underflow is rescaled first.
__global__ void gl_phasor_kernel(float* R, int ldr, const float* mag, int ldm, int T, int F) {
    const long long total = (long long)T * (ldr - F);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long t = i / (ldr - F);
        const int f = (int)(i - t * (ldr - F));
        float* row = R + t * ldr;
        if (f >= F) {                         // padding columns 2F .. ldr
            if (F + f < ldr) row[F + f] = 0.f;
            continue;
        }
        float re = row[f], im = row[F + f];
        const float m = mag[t * ldm + f];
        float r = sqrtf(re * re + im * im);
        if (!(r > 0.f)) {
            const float s = fmaxf(fabsf(re), fabsf(im));
            if (s > 0.f) { re /= s; im /= s; r = sqrtf(re * re + im * im); }
        }
        float c, sn;
        if (r > 0.f) { c = re / r; sn = im / r; }
        else { c = copysignf(1.f, re); sn = 0.f; }
        row[f] = m * c;
        row[F + f] = m * sn;
    }
}

// Overlap-add of the inverse transform (conv_transpose1d with stride hop), envelope division, hop-ratio scale and trim, per sample a
// gather of the frames that cover it (no atomics).  blockIdx.y = utterance.  mode 0: write the next transform's reflect-padded input
// at xp0 (n + n_fft samples); mode 1: write the trimmed waveform at wav0 (n = hop * (T - 1) samples).
__global__ void gl_overlap_add_kernel(const float* frames, const StftUtt* utts, const float* win2, int n_fft, int hop, float scale, float* dst,
                                      int mode) {
    const StftUtt u = utts[blockIdx.y];
    const long long n = (long long)hop * (u.T - 1), half = n_fft / 2;
    const long long total = mode == 0 ? n + n_fft : n;
    const float* fr = frames + (long long)u.frame0 * n_fft;
    for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < total; j += (long long)gridDim.x * blockDim.x) {
        long long s = j;
        if (mode == 0) {
            s = j - half;
            if (s < 0) s = -s;
            else if (s >= n) s = 2 * (n - 1) - s;
        }
        const long long p = s + half;                                 // position in the untrimmed overlap-add
        long long t_lo = p - n_fft + 1 <= 0 ? 0 : (p - n_fft + hop) / hop;
        long long t_hi = p / hop;
        if (t_hi > u.T - 1) t_hi = u.T - 1;
        float acc = 0.f, env = 0.f;
        for (long long t = t_lo; t <= t_hi; ++t) {
            const int k = (int)(p - t * hop);
            acc += fr[t * n_fft + k];
            env += win2[k];                                           // window_sumsquare: frames added in order
        }
        if (env > FLT_MIN) acc /= env;                                // np.finfo(float32).tiny
        acc *= scale;
        dst[(mode == 0 ? u.xp0 : u.wav0) + j] = acc;
    }
}

class GriffinLim {
public:
    MelFront* mf = nullptr;
    float* invT = nullptr;        // [n_fft][ld_spec]: transpose of the windowed inverse basis, columns 2F .. ld_spec zero
    float* win2 = nullptr;        // [n_fft] squared, centre-padded window
    bool have_inverse = false;
    DevBuf<float> frames, ang, emel;   // inverse GEMM's output [sum T][n_fft]; angles / phase [sum T][F]; exp(log-mel) [sum Tm][ldm]
    DevBuf<int> melmap;                // inv_mel's row map: the last mel frame of every utterance dropped
    std::vector<int> h_melmap;

    int err(const std::string& s) { return mf->err(s); }   // (DEV_CHECK)

    // inverse_basis: [2F][n_fft] (stft.py:33-45: pinv(scale * fourier_basis).T, float32, x window); window_sq: [n_fft] (window_sumsquare)
    int load(const float* inverse_basis, const float* window_sq) {
        const int n_fft = mf->n_fft, F = mf->F, ld = mf->ld_spec;
        if (!inverse_basis || !window_sq) return err("mtts_stft_load_inverse: NULL inverse basis or squared window");
        if (!invT && mf->mem.alloc(invT, (size_t)n_fft * ld * sizeof(float)) != hipSuccess) return err("out of device memory (inverse basis)");
        if (!win2 && mf->mem.alloc(win2, (size_t)n_fft * sizeof(float)) != hipSuccess) return err("out of device memory (window)");
        std::vector<float> t((size_t)n_fft * ld, 0.f);
        for (int c = 0; c < 2 * F; ++c)
            for (int k = 0; k < n_fft; ++k) t[(size_t)k * ld + c] = inverse_basis[(size_t)c * n_fft + k];
        if (hipMemcpy(invT, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(win2, window_sq, (size_t)n_fft * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            return err("hipMemcpy failed (inverse basis)");
        have_inverse = true;
        return 0;
    }

    // STFT.transform of one waveform (no clip, no max_samples bound): magnitude / phase [T][F]; returns T
    int transform(const float* wav_host, int n, float* mag_host, float* phase_host) {
        const int F = mf->F;
        if (!mf->have_basis) return err("STFT forward basis not loaded");
        if (!wav_host || !mag_host || !phase_host) return err("mtts_stft_transform: NULL argument");
        if (n <= mf->n_fft / 2) return err("waveform too short for the reflection padding (need n_samples > filter_length / 2)");
        const int T = mf->frames_of(n);
        mf->pack_begin();
        mf->pack_add(n, T);
        if (mf->stage("mtts_stft_transform", false) || mf->grow(ang, (size_t)T * F, "phase") || mf->pad_waveforms(wav_host, false, false)) return -1;
        hipStream_t st = mf->stream;
        mf->forward_stft(T, nullptr, 0);
        MTTS_LAUNCH(gl_mag_phase_kernel, dim3(512), dim3(256), st, (const float*)mf->spec, mf->ld_spec, T, F, mf->mag.p, ang.p);
        if (mf->check_launch()) return -1;
        DEV_CHECK(hipMemcpyAsync(mag_host, mf->mag, (size_t)T * F * sizeof(float), hipMemcpyDeviceToHost, st));
        DEV_CHECK(hipMemcpyAsync(phase_host, ang, (size_t)T * F * sizeof(float), hipMemcpyDeviceToHost, st));
        DEV_CHECK(hipStreamSynchronize(st));
        return T;
    }

    // griffin_lim (audio_processing.py:66-80) of n_utts spectrograms: magnitude / angles [sum T][F] frame-major, waveforms packed
    // (hop * (T_u - 1) samples each).  n_iters = 0 is STFT.inverse(magnitude, angles).  Returns the total number of samples.
    long long griffin_lim(int n_utts, const int* n_frames, const float* mag_host, const float* ang_host, int n_iters, float* out_host) {
        if (!mag_host) return err("mtts_stft_griffin_lim: NULL magnitude");
        if (prepare(n_utts, n_frames, ang_host, n_iters, out_host)) return -1;
        const int F = mf->F;
        DEV_CHECK(hipMemcpyAsync(mf->mag, mag_host, (size_t)mf->n_frames * F * sizeof(float), hipMemcpyHostToDevice, mf->stream));
        return run(mf->mag, F, n_iters, out_host);
    }

    // inv_mel_spec (tools.py:18-37): log_mel [sum Tm][n_mel] frame-major; angles [sum (Tm - 1)][F]
    long long inv_mel(int n_utts, const int* n_mel_frames, const float* log_mel, const float* ang_host, int n_iters, float* out_host) {
        if (!mf->have_mel) return err("mel basis not loaded");
        if (!log_mel || !n_mel_frames || n_utts < 1) return err("mtts_stft_inv_mel: bad arguments");
        std::vector<int> T(n_utts);
        for (int u = 0; u < n_utts; ++u) T[u] = n_mel_frames[u] - 1;            // spec_from_mel[:, :, :-1]
        if (prepare(n_utts, T.data(), ang_host, n_iters, out_host)) return -1;
        const int F = mf->F, n_mel = mf->n_mel, ldm = (n_mel + 3) & ~3, ld_mag = mf->ld_mag;
        const long long mrows = mf->n_frames + n_utts;
        h_melmap.resize((size_t)mrows);
        for (int u = 0, r = 0, o = 0; u < n_utts; ++u) {
            for (int t = 0; t <= T[u]; ++t) h_melmap[(size_t)r++] = t < T[u] ? o + t : -1;   // the last frame of every utterance is dropped
            o += T[u];
        }
        if (mf->grow(mf->mel, (size_t)mrows * n_mel, "log-mel") || mf->grow(emel, (size_t)mrows * ldm + 64, "exp(mel)") || mf->grow(melmap, (size_t)mrows, "mel row map"))
            return -1;
        hipStream_t st = mf->stream;
        DEV_CHECK(hipMemcpyAsync(mf->mel, log_mel, (size_t)mrows * n_mel * sizeof(float), hipMemcpyHostToDevice, st));
        DEV_CHECK(hipMemcpyAsync(melmap, h_melmap.data(), (size_t)mrows * sizeof(int), hipMemcpyHostToDevice, st));
        MTTS_LAUNCH(gl_exp_rows_kernel, dim3(512), dim3(256), st, (const float*)mf->mel, (int)mrows, n_mel, emel.p, ldm);
        {   // magnitude [sum T][F] = 1000 * exp(mel)[sum Tm][n_mel] * mel_basis[n_mel][F], the last frame of each utterance dropped
            GemmArgs g;
            g.A = emel; g.lda = ldm; g.B = mf->melb; g.ldb = ld_mag; g.C = mf->mag; g.ldc = ld_mag;
            g.M = (int)mrows; g.N = F; g.K = n_mel; g.alpha = 1000.f; g.c_rowmap = melmap;
            gemm_launch(mf->gx, GEMM_NN, g, (int)mrows, F, 1, st, 0, 2.0 * mrows * F * n_mel, 0);
        }
        if (mf->check_launch()) return -1;
        return run(mf->mag, ld_mag, n_iters, out_host);
    }

private:
    // validation (before any launch), MelFront's packing and workspace, upload of the angles
    int prepare(int n_utts, const int* T, const float* ang_host, int n_iters, float* out_host) {
        const int n_fft = mf->n_fft, hop = mf->hop, F = mf->F;
        if (!have_inverse) return err("inverse basis not loaded (mtts_stft_load_inverse)");
        if (!mf->have_basis) return err("STFT forward basis not loaded");
        if (n_utts < 1 || !T || !ang_host || !out_host) return err("Griffin-Lim: bad arguments (n_utts < 1 or NULL pointer)");
        if (n_iters < 0) return err("Griffin-Lim: n_iters < 0");
        mf->pack_begin();
        for (int u = 0; u < n_utts; ++u) {
            if (T[u] < 1 || (n_iters > 0 && (long long)hop * (T[u] - 1) <= n_fft / 2))
                return err("spectrogram too short: the waveform of T frames has hop * (T - 1) samples and must exceed filter_length / 2 "
                           "for the reflection padding of the next transform (inv_mel: T = mel frames - 1)");
            mf->pack_add((long long)hop * (T[u] - 1), T[u]);
        }
        const size_t rows = (size_t)mf->n_frames;
        if (mf->stage("Griffin-Lim", true) || mf->grow(frames, rows * n_fft + 64, "frames") || mf->grow(ang, rows * F, "angles")) return -1;
        DEV_CHECK(hipMemcpyAsync(ang, ang_host, rows * F * sizeof(float), hipMemcpyHostToDevice, mf->stream));
        return 0;
    }

    // the prepared call: M [sum T][ldm] magnitudes on the device -> out_host, the packed waveforms
    long long run(const float* M, int ldm, int n_iters, float* out_host) {
        const int n_fft = mf->n_fft, hop = mf->hop, F = mf->F, ld = mf->ld_spec, n_utts = (int)mf->h_utts.size();
        const long long rows = mf->n_frames;
        float* R = mf->spec;
        hipStream_t st = mf->stream;
        const dim3 ola_grid((unsigned)std::min<long long>((mf->max_span + 255) / 256, 4096), (unsigned)n_utts);
        const float scale = (float)((double)n_fft / hop);
        MTTS_LAUNCH(gl_phasor_init_kernel, dim3(1024), dim3(256), st, M, ldm, (const float*)ang, (int)rows, F, R, ld);
        for (int it = 0;; ++it) {
            {   // frames [rows][n_fft] = R [rows][2F] * inverse_basis [2F][n_fft]
                GemmArgs g;
                g.A = R; g.lda = ld; g.B = invT; g.ldb = ld; g.C = frames; g.ldc = n_fft;
                g.M = (int)rows; g.N = n_fft; g.K = 2 * F;
                gemm_launch(mf->gx, GEMM_NT, g, (int)rows, n_fft, 1, st, 0, 2.0 * rows * 2.0 * F * n_fft, 0);
            }
            const bool last = it == n_iters;
            MTTS_LAUNCH(gl_overlap_add_kernel, ola_grid, dim3(256), st, (const float*)frames, (const StftUtt*)mf->utts, (const float*)win2, n_fft, hop, scale,
                        last ? mf->wav.p : mf->xp.p, last ? 1 : 0);
            if (last) break;
            mf->forward_stft(mf->xp_rows, mf->rowmap, 0);
            MTTS_LAUNCH(gl_phasor_kernel, dim3(1024), dim3(256), st, R, ld, M, ldm, (int)rows, F);
        }
        if (mf->check_launch()) return -1;
        DEV_CHECK(hipMemcpyAsync(out_host, mf->wav, (size_t)mf->n_samples * sizeof(float), hipMemcpyDeviceToHost, st));
        DEV_CHECK(hipStreamSynchronize(st));
        return mf->n_samples;
    }
};

}  // namespace mtts
