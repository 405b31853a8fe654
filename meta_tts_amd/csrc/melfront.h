// The STFT front-end every audio stage of an mtts_stft handle shares, and waveform -> log-mel spectrogram + frame energy on top of it.
//
// Reference: audio/stft.py:15-77 (STFT.transform: reflect padding by n_fft/2, a strided Conv1d against the windowed real / imaginary
// Fourier basis, magnitude) and :128-178 (TacotronSTFT.mel_spectrogram: mel_basis @ magnitude, log(clamp(., 1e-5)), energy = L2 norm
// of the magnitudes over frequency), called by audio/tools.py:8-15 (get_mel_from_wav: clip to [-1, 1] first) from the preprocessor.
//
// MI355X layout: the strided Conv1d is an implicit GEMM over OVERLAPPING rows of the padded waveform — frame t is the contiguous
// span x[t*hop .. t*hop + n_fft), i.e. an A operand with lda = hop < K = n_fft, no framing copy — against the [2*(n_fft/2+1)][n_fft]
// basis on the fp32 matrix cores (gemm.h); magnitude and energy are one wavefront-per-frame pass; the mel projection is a second
// GEMM whose epilogue-side log/clamp runs as a small row kernel.  Output rows are [frame][n_mel] (the engine's mel layout).
//
// What is shared (MelFront; griffin.h and preprocess.h build on it and keep only the buffers that are theirs):
//   * packing (pack_begin / pack_add / stage): the utterances of a call are described by StftUtt; every reflect-padded signal starts
//     at a multiple of hop, so ONE forward GEMM covers all of them, and the rows that straddle two signals are dropped through
//     GemmArgs::c_rowmap (the spectrum lands compact, [sum T] rows).  A single-utterance entry stages without the map;
//   * stft_reflect_pad_kernel (clip on or off), forward_stft (the overlapping-row GEMM), mel_from_spectrum (magnitude + energy, mel
//     GEMM, log-clamp, download), check_launch, and the grow-on-demand workspace (DevBuf, devres.h): one set of wav / padded signal / spectrum /
//     magnitude / mel / energy buffers per handle, which every entry point may use because each is synchronous on the handle's stream.
// The workspace is allocated by the first call that needs it, not at create: max_samples only bounds mel_spectrogram's input, and a
// create with an absurd max_samples succeeds where it used to fail in hipMalloc (the first call that large fails instead).
#pragma once
#include <string>
#include <vector>

#include "gemm.h"
#include "rowops.h"

namespace mtts {

struct StftUtt {
    int n;            // samples of the waveform (Griffin-Lim: hop * (T - 1))
    int T;            // frames kept (<= n / hop + 1)
    int frame0;       // first row of this utterance in the compact spectrum / frames
    int pad_;
    long long wav0;   // first sample of its waveform in the packed waveforms
    long long xp0;    // first sample of its reflect-padded signal (a multiple of hop)
};

// xp[xp0 + j] = wav[wav0 + reflect(j - n_fft / 2)], clipped to [-1, 1] when `clip` (tools.py:9; STFT.transform itself does not clip),
// for the hop * (T - 1) + n_fft samples the kept frames read (F.pad(..., mode="reflect") of stft.py:60-65).  blockIdx.y = utterance
// of the table `utts`; utts == nullptr: the one utterance passed by value.
__global__ void stft_reflect_pad_kernel(const float* wav, const StftUtt* utts, StftUtt one, int n_fft, int hop, int clip, float* xp) {
    const StftUtt u = utts ? utts[blockIdx.y] : one;
    const long long total = (long long)hop * (u.T - 1) + n_fft, pad = n_fft / 2;
    for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < total; j += (long long)gridDim.x * blockDim.x) {
        long long s = j - pad;
        if (s < 0) s = -s;
        else if (s >= u.n) s = 2LL * (u.n - 1) - s;
        float v = wav[u.wav0 + s];
        if (clip) v = v < -1.f ? -1.f : (v > 1.f ? 1.f : v);
        xp[u.xp0 + j] = v;
    }
}

// spec: [T][ld_spec] = [re(0..F) | im(0..F)] per frame  ->  mag [T][ld_mag] (columns >= F zeroed), energy[t] = ||mag[t]||_2
__global__ void stft_magnitude_kernel(const float* spec, int ld_spec, int T, int F, float* mag, int ld_mag, float* energy) {
    const int row = blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    if (row >= T) return;
    const float* p = spec + (long long)row * ld_spec;
    float* m = mag + (long long)row * ld_mag;
    float ss = 0.f;
    for (int f = lane; f < ld_mag; f += 64) {
        float v = 0.f;
        if (f < F) {
            const float re = p[f], im = p[F + f];
            const float sq = re * re + im * im;
            v = sqrtf(sq);
            ss += sq;
        }
        m[f] = v;
    }
    ss = wave_sum(ss);
    if (lane == 0) energy[row] = sqrtf(ss);
}

// in place: x = log(max(x, clip))   (audio_processing.py:85-91, C = 1)
__global__ void log_clamp_kernel(float* x, long long n, float clip) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float v = x[i];
        x[i] = logf(v > clip ? v : clip);
    }
}

class MelFront {
public:
    int n_fft = 1024, hop = 256, n_mel = 80, F = 513, cap_samples = 0;
    int ld_spec = 0, ld_mag = 0;
    hipStream_t stream = nullptr;
    std::string last_error;
    DevHeap mem;   // every device block and event of the mtts_stft handle: this front-end's and those of the stages built on it (devres.h)
    GemmCtx gx;
    float *basis = nullptr, *melb = nullptr;   // [2F][n_fft] windowed Fourier basis; [n_mel][ld_mag] mel filter bank (zero padded)
    bool have_basis = false, have_mel = false;
    // the handle's workspace: packed waveforms, packed reflect-padded signals, spectrum [sum T][ld_spec] (Griffin-Lim's recombined
    // spectrum R), magnitude [sum T][ld_mag], (log-)mel [sum T][n_mel], energy [sum T], the forward GEMM's row map, the utterance table
    DevBuf<float> wav, xp, spec, mag, mel, energy;
    DevBuf<int> rowmap;
    DevBuf<StftUtt> utts;
    // the packed call (pack_begin / pack_add): totals over its utterances
    std::vector<StftUtt> h_utts;
    std::vector<int> h_rowmap;
    long long n_frames = 0, xp_rows = 0, n_samples = 0, max_span = 0;   // sum T, forward-GEMM rows, sum n, longest padded span

    int err(const std::string& s) { last_error = s; return -1; }

    int init(int filter_length, int hop_length, int n_mel_channels, int max_samples) {
        n_fft = filter_length; hop = hop_length; n_mel = n_mel_channels; cap_samples = max_samples;
        if (n_fft < 16 || (n_fft & 3) || hop < 4 || (hop & 3) || hop > n_fft || n_mel < 1 || n_mel > 1024 || max_samples <= n_fft / 2)
            return err("unsupported STFT configuration (filter_length % 4, hop_length % 4 <= filter_length, max_samples > filter_length / 2)");
        F = n_fft / 2 + 1;
        ld_spec = (2 * F + 3) & ~3;
        ld_mag = (F + 3) & ~3;
        DEV_CHECK(mem.alloc(basis, (size_t)2 * F * n_fft * sizeof(float)));
        DEV_CHECK(mem.alloc_zeroed(melb, (size_t)n_mel * ld_mag * sizeof(float)));
        if (gx.alloc_workspace(mem)) return err("out of device memory (split-K workspace)");
        return 0;
    }
    // forward_basis: [2F][n_fft] (stft.py:27-46, window applied); mel_basis: [n_mel][F] (stft.py:143-147)
    int load(const float* forward_basis, const float* mel_basis) {
        if (forward_basis) { DEV_CHECK(hipMemcpy(basis, forward_basis, (size_t)2 * F * n_fft * sizeof(float), hipMemcpyHostToDevice)); have_basis = true; }
        if (mel_basis) {
            std::vector<float> padded((size_t)n_mel * ld_mag, 0.f);
            for (int m = 0; m < n_mel; ++m)
                for (int f = 0; f < F; ++f) padded[(size_t)m * ld_mag + f] = mel_basis[(size_t)m * F + f];
            DEV_CHECK(hipMemcpy(melb, padded.data(), padded.size() * sizeof(float), hipMemcpyHostToDevice));
            have_mel = true;
        }
        return 0;
    }

    template <class T>
    int grow(DevBuf<T>& b, size_t need, const char* what) { return mtts::grow(mem, b, need, stream, what, last_error); }
    // Launches are asynchronous: what the GEMM launcher refused is in gx.error, what the runtime refused in hipGetLastError().
    int check_launch() {
        if (gx.error) { const std::string e = std::string("GEMM launcher: ") + gx.error; gx.error = nullptr; return err(e); }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return err(std::string("kernel launch failed: ") + hipGetErrorString(e));
        return 0;
    }

    int frames_of(int n_samples) const { return n_samples / hop + 1; }   // conv1d over the padded signal: (n + n_fft - n_fft) / hop + 1

    // What the batched entries refuse about their utterances before any launch, each asking for the conditions that are its own.
    // UTT_GRID: more than 65535 utterances (its kernels take the utterance from gridDim.y).  UTT_CAP: a length below 1 or beyond
    // max_samples.  UTT_PAD: a length the reflection padding cannot read (n <= n_fft / 2).  len_of(u) = samples of utterance u;
    // resampled: they are counted behind a resampler (of n_in source samples each), and the texts say so.
    enum { UTT_GRID = 1, UTT_CAP = 2, UTT_PAD = 4 };
    template <class LenOf>
    int check_utterances(const std::string& who, int n_utts, LenOf len_of, int checks, bool resampled = false) {
        if ((checks & UTT_GRID) && n_utts > 65535) return err(who + "more than 65535 utterances in one call");
        for (int u = 0; u < n_utts; ++u) {
            const std::string utt = who + "utterance " + std::to_string(u) + ": ";
            const long long n = len_of(u);
            if ((checks & UTT_CAP) && n < 1) return err(utt + (resampled ? "n_in < 1" : "n_samples < 1"));
            if ((checks & UTT_CAP) && n > cap_samples)
                return err(utt + std::to_string(n) + (resampled ? " resampled" : "") + " samples exceed max_samples = " + std::to_string(cap_samples));
            if ((checks & UTT_PAD) && n <= n_fft / 2)
                return err(utt + "waveform too short for the reflection padding (need n_samples > filter_length / 2 = " + std::to_string(n_fft / 2) + ")");
        }
        return 0;
    }

    // ---- packing: host only, so a caller validates utterance by utterance before anything is launched ------------------------------
    void pack_begin() { h_utts.clear(); n_frames = xp_rows = n_samples = max_span = 0; }
    // one more utterance of n samples of which T frames are kept; its padded signal starts at the next free multiple of hop
    // (a count beyond what StftUtt's ints hold is refused by stage)
    void pack_add(long long n, int T) {
        h_utts.push_back(StftUtt{(int)n, T, (int)n_frames, 0, n_samples, xp_rows * hop});
        n_frames += T;
        n_samples += n;
        xp_rows += T + (n_fft + hop - 1) / hop - 1;   // + the rows that straddle into the next padded signal
        max_span = std::max(max_span, (long long)hop * (T - 1) + n_fft);
    }
    // Workspace for the packed call.  mapped: also the row map (forward-GEMM row -> compact row, -1 for a straddling row) and the
    // utterance table on the device, and the padded signals zeroed (the gaps are read only by dropped rows).
    int stage(const char* who, bool mapped) {
        if (n_frames > (1LL << 30) / std::max(ld_spec, n_fft) || xp_rows > (1LL << 30) || n_samples > (1LL << 31) - 1)
            return err(std::string(who) + ": too many frames in one call");
        const size_t rows = (size_t)n_frames, xp_len = (size_t)xp_rows * hop + n_fft + 64;
        if (grow(wav, (size_t)n_samples + 64, "waveforms") || grow(xp, xp_len, "padded signals") || grow(spec, rows * ld_spec + 64, "spectrum") ||
            grow(mag, rows * ld_mag + 64, "magnitude") || grow(mel, rows * n_mel + 64, "mel") || grow(energy, rows, "energy"))
            return -1;
        if (!mapped) return 0;
        h_rowmap.assign((size_t)xp_rows, -1);
        for (const StftUtt& u : h_utts)
            for (int t = 0; t < u.T; ++t) h_rowmap[(size_t)(u.xp0 / hop + t)] = u.frame0 + t;
        if (grow(rowmap, (size_t)xp_rows, "row map") || grow(utts, h_utts.size(), "utterances")) return -1;
        DEV_CHECK(hipMemcpyAsync(utts, h_utts.data(), h_utts.size() * sizeof(StftUtt), hipMemcpyHostToDevice, stream));
        DEV_CHECK(hipMemcpyAsync(rowmap, h_rowmap.data(), (size_t)xp_rows * sizeof(int), hipMemcpyHostToDevice, stream));
        DEV_CHECK(hipMemsetAsync(xp, 0, xp_len * sizeof(float), stream));
        return 0;
    }
    // wav_host (the staged call's waveforms one after another) -> the reflect-padded signals
    int pad_waveforms(const float* wav_host, bool clip, bool mapped) {
        DEV_CHECK(hipMemcpyAsync(wav, wav_host, (size_t)n_samples * sizeof(float), hipMemcpyHostToDevice, stream));
        return pad_staged(clip, mapped);
    }
    // the same for waveforms an earlier launch on this stream has left in `wav` (resample.h): no upload
    int pad_staged(bool clip, bool mapped) {
        const dim3 grid((unsigned)std::min<long long>((max_span + 255) / 256, 1024), (unsigned)h_utts.size());
        MTTS_LAUNCH(stft_reflect_pad_kernel, grid, dim3(256), stream, (const float*)wav, (const StftUtt*)(mapped ? utts.p : nullptr), h_utts[0], n_fft, hop,
                    clip ? 1 : 0, xp.p);
        return 0;
    }
    // spec rows (compact through `map`, or rows 0 .. M when map == nullptr) = overlapping frames of xp (lda = hop) * basis[2F][n_fft]^T
    void forward_stft(long long M, const int* map, int tile) {
        GemmArgs g;
        g.A = xp; g.lda = hop; g.B = basis; g.ldb = n_fft; g.C = spec; g.ldc = ld_spec;
        g.M = (int)M; g.N = 2 * F; g.K = n_fft; g.c_rowmap = map;
        gemm_launch(gx, GEMM_NT, g, (int)M, 2 * F, 1, stream, tile, 2.0 * M * 2.0 * F * n_fft, 0);
    }
    // spectrum of the staged call -> mel_host [sum T][n_mel] (log-mel), energy_host [sum T]
    int mel_from_spectrum(int tile, float* mel_host, float* energy_host) {
        const long long T = n_frames;
        MTTS_LAUNCH(stft_magnitude_kernel, dim3((unsigned)((T + 3) / 4)), dim3(256), stream, (const float*)spec, ld_spec, (int)T, F, mag.p, ld_mag, energy.p);
        {   // mel[T][n_mel] = mag[T][F] * mel_basis[n_mel][F]^T   (both zero padded to ld_mag columns)
            GemmArgs g;
            g.A = mag; g.lda = ld_mag; g.B = melb; g.ldb = ld_mag; g.C = mel; g.ldc = n_mel;
            g.M = (int)T; g.N = n_mel; g.K = ld_mag;
            gemm_launch(gx, GEMM_NT, g, (int)T, n_mel, 1, stream, tile, 2.0 * T * (double)n_mel * F, 0);
        }
        MTTS_LAUNCH(log_clamp_kernel, dim3((unsigned)std::min<long long>((T * n_mel + 255) / 256, 1024)), dim3(256), stream, mel.p, T * n_mel, 1e-5f);
        if (check_launch()) return -1;
        DEV_CHECK(hipMemcpyAsync(mel_host, mel, (size_t)T * n_mel * sizeof(float), hipMemcpyDeviceToHost, stream));
        DEV_CHECK(hipMemcpyAsync(energy_host, energy, (size_t)T * sizeof(float), hipMemcpyDeviceToHost, stream));
        DEV_CHECK(hipStreamSynchronize(stream));
        return 0;
    }

    // wav_host [n_samples] -> mel_host [T][n_mel] (log-mel), energy_host [T]; returns T, < 0 on error
    int mel_spectrogram(const float* wav_host, int n_samples_, float* mel_host, float* energy_host) {
        if (!have_basis || !have_mel) return err("STFT bases not loaded");
        if (!wav_host || !mel_host || !energy_host || n_samples_ <= n_fft / 2 || n_samples_ > cap_samples)
            return err("bad waveform length (need filter_length / 2 < n_samples <= max_samples: reflection padding reads n_fft / 2 samples)");
        const int T = frames_of(n_samples_);
        pack_begin();
        pack_add(n_samples_, T);
        if (stage("mtts_stft_mel_spectrogram", false) || pad_waveforms(wav_host, true, false)) return -1;
        forward_stft(T, nullptr, 0);
        return mel_from_spectrum(0, mel_host, energy_host) ? -1 : T;
    }
};

}  // namespace mtts
