// Fundamental frequency of waveform batches on the device: YIN (de Cheveigné & Kawahara 2002) on MelFront's packed waveform buffer.
//
// Reference: preprocessor/preprocessor.py:214-220 calls pyworld's DIO + StoneMask at a frame period of one hop.  pyworld is not
// vendored and is NOT restated; parity with it is UNPINNED.  What is built is stated in include/mtts.h (and, in float64 numpy, in
// tests/f0_oracle.py): per frame t of an utterance (T = n / hop + 1 frames, DIO's and mel_batch's count), over the span
// s = x[t * hop - L / 2 .. + L) with zeros outside the utterance, L = W + tau_max,
//     d(tau)  = sum_{j < W} (s[j] - s[j + tau])^2,  tau = 0 .. tau_max          (fp32 FMAs in ascending j; the direct form, which does not cancel)
//     d'(tau) = d(tau) tau / sum_{k = 1 .. tau} d(k)   (1 at tau = 0 and where the running sum is 0; fp32, the sum in ascending k)
// the smallest tau in [tau_min, tau_max) with d'(tau) < threshold, walked forward while d' falls, a parabola through its neighbours
// (fp64), f0 = sr / (tau + offset); 0 when no lag is below the threshold or when mean(s[0 : W]^2) < silence_rms^2.
//
// MI355X layout.  A workgroup takes F consecutive frames of ONE utterance (blockIdx.y = utterance through MelFront's table, as the
// reflect-pad and the resampling kernels do) and stages the union of their spans, (F - 1) hop + L floats, in LDS once.  The work is
// W (tau_max + 1) subtract + FMA pairs per frame (160 k at 22 050 Hz) on data that never leaves LDS, so LDS reads per FMA decide the
// speed.  A lane owns FOUR consecutive lags of one frame and walks j in steps of four: per step one ds_read_b128 of s[j .. j + 4)
// (the same address in every lane of a frame: a broadcast) and one of the next four samples of its sliding window s[j + 4 b + 4 ..)
// (lane b reads 16 bytes at 16 b: consecutive, conflict-free) feed 16 subtract + FMA pairs, which hipcc packs two lags at a time
// (v_pk_add_f32 / v_pk_fma_f32).  As compiled, the window is re-read at odd offsets rather than permuted in registers, which leaves
// the LDS port about as busy as the VALUs.  The (frame, lag block) items of a workgroup are dealt to its 256 lanes
// densely, so wavefronts are full whatever tau_max is (F * ceil((tau_max + 1) / 4) items: 1248 = 4.9 passes at 22 050 Hz).
// d lands in a second LDS array; one lane per frame then forms d' in place (a running sum is serial by definition), searches, descends
// and refines.  No wavefront intrinsics and no atomics: LDS and barriers only, so the SIMT emulator runs the same source.
//
// Determinism.  Every (frame, lag) sum is one lane's chain of FMAs over j = 0 .. W - 1; which lane, which workgroup and which F do not
// enter.  F is fixed when the configuration is loaded (from hop, L and the LDS arrays below, at most 16), never by the batch.
// LDS: 4736 + 5056 + 256 floats = 40 192 B per workgroup -> 4 workgroups (16 wavefronts) per CU.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "melfront.h"

namespace mtts {

constexpr int PT_THREADS = 256;
constexpr int PT_SPAN = 4736;     // floats of waveform one workgroup may stage
constexpr int PT_DP = 5056;       // floats of d / d' one workgroup holds: F rows of 4 * nb
constexpr int PT_MAX_F = 16;      // frames per workgroup, at most
constexpr int PT_ESPLIT = 16;     // lanes that share a frame's energy sum (PT_MAX_F * PT_ESPLIT <= PT_THREADS)

struct PitchCfg {
    int hop, W, L, tau_min, tau_max;
    int nb, F;               // lag blocks of four per frame: ceil((tau_max + 1) / 4); frames per workgroup
    float threshold;
    double sr, silence_ms;   // silence_rms^2
};

// f0[frame0 + t], ap[frame0 + t] of the utterances of the table `utts` (n, T, frame0, wav0 are read).  gridDim.x covers the longest
// utterance; a workgroup past its utterance's last frame does nothing.
__global__ __launch_bounds__(PT_THREADS) void pitch_yin_kernel(const float* wav, const StftUtt* utts, PitchCfg c, double* f0, float* ap) {
    __shared__ __attribute__((aligned(16))) float xs[PT_SPAN];
    __shared__ __attribute__((aligned(16))) float dp[PT_DP];
    __shared__ float part[PT_THREADS];
    const StftUtt u = utts[blockIdx.y];
    const int t0 = (int)blockIdx.x * c.F;
    if (t0 >= u.T) return;   // (the whole workgroup: no barrier is left waiting)
    const int nf = u.T - t0 < c.F ? u.T - t0 : c.F;
    const int tid = (int)threadIdx.x;
    const int row = 4 * c.nb;
    // the lag blocks are padded to a multiple of four lags, and a window runs one step ahead: row + 4 floats past W are read (the
    // lags above tau_max are computed and dropped); <= PT_SPAN: F was chosen for it
    const int span = (nf - 1) * c.hop + c.W + row + 4;
    const long long m0 = (long long)t0 * c.hop - c.L / 2;
    for (int i = tid; i < span; i += PT_THREADS) {
        const long long m = m0 + i;
        xs[i] = (m >= 0 && m < u.n) ? wav[u.wav0 + m] : 0.f;
    }
    __syncthreads();
    // energy of s[0 : W]: PT_ESPLIT interleaved partial sums per frame, added in order by the frame's lane below
    if (tid < nf * PT_ESPLIT) {
        const float* s = xs + (tid / PT_ESPLIT) * c.hop;
        float e = 0.f;
        for (int j = tid % PT_ESPLIT; j < c.W; j += PT_ESPLIT) e = fmaf(s[j], s[j], e);
        part[tid] = e;
    }
    // d(4 b + k) = sum_j (s[j] - s[j + 4 b + k])^2 for k = 0 .. 3: lo = s[j + 4 b ..), hi the four after
    const int items = nf * c.nb;
    for (int it = tid; it < items; it += PT_THREADS) {
        const int f = it / c.nb, b = it - f * c.nb;
        const float* s = xs + f * c.hop;   // 16-byte aligned: hop % 4 == 0 (MelFront::init)
        const float* w = s + 4 * b;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, d;
        float4 lo = ld4(w);
        for (int j = 0; j < c.W; j += 4) {
            const float4 x = ld4(s + j);
            const float4 hi = ld4(w + j + 4);
            d = x.x - lo.x; a0 = fmaf(d, d, a0);
            d = x.x - lo.y; a1 = fmaf(d, d, a1);
            d = x.x - lo.z; a2 = fmaf(d, d, a2);
            d = x.x - lo.w; a3 = fmaf(d, d, a3);
            d = x.y - lo.y; a0 = fmaf(d, d, a0);
            d = x.y - lo.z; a1 = fmaf(d, d, a1);
            d = x.y - lo.w; a2 = fmaf(d, d, a2);
            d = x.y - hi.x; a3 = fmaf(d, d, a3);
            d = x.z - lo.z; a0 = fmaf(d, d, a0);
            d = x.z - lo.w; a1 = fmaf(d, d, a1);
            d = x.z - hi.x; a2 = fmaf(d, d, a2);
            d = x.z - hi.y; a3 = fmaf(d, d, a3);
            d = x.w - lo.w; a0 = fmaf(d, d, a0);
            d = x.w - hi.x; a1 = fmaf(d, d, a1);
            d = x.w - hi.y; a2 = fmaf(d, d, a2);
            d = x.w - hi.z; a3 = fmaf(d, d, a3);
            lo = hi;
        }
        st4(dp + f * row + 4 * b, make_float4(a0, a1, a2, a3));
    }
    __syncthreads();
    if (tid >= nf) return;
    // one lane per frame: d -> d' in place, silence, first lag below the threshold, descent, parabola
    float* dn = dp + tid * row;
    float e = 0.f;
    for (int p = 0; p < PT_ESPLIT; ++p) e += part[tid * PT_ESPLIT + p];
    float run = 0.f;
    dn[0] = 1.f;
    for (int tau = 1; tau <= c.tau_max; ++tau) {
        const float v = dn[tau];
        run += v;
        dn[tau] = run > 0.f ? v * (float)tau / run : 1.f;
    }
    double hz = 0.0;
    float conf = 1.f;
    if (!((double)e / (double)c.W < c.silence_ms)) {
        int tau = c.tau_min;
        while (tau < c.tau_max && !(dn[tau] < c.threshold)) ++tau;
        if (tau < c.tau_max) {
            while (tau + 1 < c.tau_max && dn[tau + 1] < dn[tau]) ++tau;
            double off = 0.0;
            if (tau > c.tau_min && tau < c.tau_max - 1) {
                const double y0 = dn[tau - 1], y1 = dn[tau], y2 = dn[tau + 1];
                const double den = y0 - 2.0 * y1 + y2;
                if (den != 0.0) off = 0.5 * (y0 - y2) / den;
            }
            hz = c.sr / ((double)tau + off);
            conf = dn[tau];
        }
    }
    f0[u.frame0 + t0 + tid] = hz;
    ap[u.frame0 + t0 + tid] = conf;
}

class Pitch {
public:
    MelFront* mf = nullptr;
    PitchCfg c{};
    bool loaded = false;
    DevBuf<double> f0;
    DevBuf<float> ap;

    int err(const std::string& s) { return mf->err(s); }

    int load(int sampling_rate, double f0_floor, double f0_ceil, double threshold, double silence_rms) {
        const char* who = "mtts_stft_load_pitch: ";
        if (sampling_rate < 1 || !(f0_floor > 0.0) || !std::isfinite(f0_ceil) || !(threshold > 0.0) || !std::isfinite(threshold) || !(silence_rms >= 0.0) ||
            !std::isfinite(silence_rms))
            return err(std::string(who) + "bad arguments (need sampling_rate >= 1, f0_floor > 0, threshold > 0, silence_rms >= 0, all finite)");
        if (!(f0_ceil > f0_floor)) return err(std::string(who) + "f0_ceil <= f0_floor");
        const double tmax = std::ceil(sampling_rate / f0_floor), tmin = std::floor(sampling_rate / f0_ceil);
        if (tmin < 2.0) return err(std::string(who) + "tau_min = floor(sampling_rate / f0_ceil) = " + std::to_string((int)tmin) + " < 2: f0_ceil is too close to the sampling rate");
        if (tmax > 1e6) return err(std::string(who) + "f0_floor is too low for this sampling rate");
        PitchCfg n{};
        n.hop = mf->hop;
        n.tau_min = (int)tmin;
        n.tau_max = (int)tmax;
        if (n.tau_max - n.tau_min < 2) return err(std::string(who) + "fewer than two lags between f0_ceil and f0_floor");
        n.W = ((3 * n.tau_max + 1) / 2 + 63) / 64 * 64;
        n.L = n.W + n.tau_max;
        n.nb = (n.tau_max + 4) / 4;
        const int row = 4 * n.nb;
        int F = PT_MAX_F;
        while (F >= 1 && ((long long)(F - 1) * n.hop + n.W + row + 4 > PT_SPAN || F * row > PT_DP)) --F;
        if (F < 1) return err(std::string(who) + "a frame's span of " + std::to_string(n.W + row + 4) + " samples (lags up to " + std::to_string(n.tau_max) +
                              ") exceeds what a workgroup stages: raise f0_floor or lower the sampling rate");
        n.F = F;
        n.threshold = (float)threshold;
        n.sr = (double)sampling_rate;
        n.silence_ms = silence_rms * silence_rms;
        c = n;
        loaded = true;
        return 0;
    }

    // host in, host out: wavs = the utterances one after another; f0_out, ap_out [sum T_u], T_u = n_samples[u] / hop + 1.  Returns sum T_u.
    long long f0_batch(int n_utts, const int* n_samples, const float* wavs, double* f0_out, float* ap_out) {
        const char* who = "mtts_stft_f0_batch: ";
        if (!loaded) return err(std::string(who) + "no pitch configuration loaded (mtts_stft_load_pitch)");
        if (n_utts < 1 || !n_samples || !wavs || !f0_out) return err(std::string(who) + "bad arguments (n_utts < 1 or NULL pointer)");
        if (mf->check_utterances(who, n_utts, [&](int u) { return n_samples[u]; }, MelFront::UTT_GRID | MelFront::UTT_CAP)) return -1;
        mf->pack_begin();
        int max_T = 0;
        for (int u = 0; u < n_utts; ++u) {
            const int T = mf->frames_of(n_samples[u]);
            mf->pack_add(n_samples[u], T);
            max_T = std::max(max_T, T);
        }
        if (mf->n_samples > (1LL << 31) - 1 || mf->n_frames > (1LL << 31) - 1) return err(std::string(who) + "too many samples in one call");
        const size_t rows = (size_t)mf->n_frames;
        if (mf->grow(mf->wav, (size_t)mf->n_samples + 64, "waveforms") || mf->grow(mf->utts, mf->h_utts.size(), "utterances") || mf->grow(f0, rows, "f0") ||
            mf->grow(ap, rows, "aperiodicity"))
            return -1;
        DEV_CHECK(hipMemcpyAsync(mf->wav.p, wavs, (size_t)mf->n_samples * sizeof(float), hipMemcpyHostToDevice, mf->stream));
        DEV_CHECK(hipMemcpyAsync(mf->utts.p, mf->h_utts.data(), mf->h_utts.size() * sizeof(StftUtt), hipMemcpyHostToDevice, mf->stream));
        MTTS_LAUNCH(pitch_yin_kernel, dim3((unsigned)((max_T + c.F - 1) / c.F), (unsigned)n_utts), dim3(PT_THREADS), mf->stream, (const float*)mf->wav.p,
                    (const StftUtt*)mf->utts.p, c, f0.p, ap.p);
        if (mf->check_launch()) return -1;
        DEV_CHECK(hipMemcpyAsync(f0_out, f0.p, rows * sizeof(double), hipMemcpyDeviceToHost, mf->stream));
        if (ap_out) DEV_CHECK(hipMemcpyAsync(ap_out, ap.p, rows * sizeof(float), hipMemcpyDeviceToHost, mf->stream));
        DEV_CHECK(hipStreamSynchronize(mf->stream));
        return mf->n_frames;
    }
};

}  // namespace mtts
