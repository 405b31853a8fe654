// Waveform batches -> the preprocessed feature tree's values on the device: the wav -> features half of the preprocessing stage.
//
// Reference: preprocessor/preprocessor.py:188-306 (Preprocessor.process_utterance: get_mel_from_wav truncated to sum(duration) frames,
// interp1d over the unvoiced pitch frames, the in-place phoneme-level segment mean of pitch (float64) and energy (float32)), :348-356
// (remove_outlier: np.percentile 25 / 75 with linear interpolation, 1.5 IQR fences, strict inequalities), :60-185 (build_from_path:
// StandardScaler.partial_fit over the kept values utterance by utterance) and :358-369 (normalize: (x - mean) / std and the global
// minimum / maximum of the normalised values).
//
// MI355X layout.  Every utterance of a call goes through the same launches; only descriptor tables are built by a host loop.
//   * front-end (Preprocess::mel_batch): melfront.h's shared pieces with every utterance packed into one call — the clip +
//     reflect-pad kernel, ONE forward-STFT GEMM whose rows between two utterances are dropped, the magnitude + energy pass, the mel
//     GEMM and the log-clamp over the compact [sum T] rows, all in MelFront's workspace.  Both GEMMs name their kernel explicitly (no
//     split-K, no size-dependent choice), so an utterance's rows do not depend on what else is in the call.
//   * pp_segment_kernel<T>: one workgroup per utterance; interpolation by nearest-voiced-left / right walks, the duration prefix sum,
//     and the segment means (T = double for pitch, float for energy).  The reference's loop writes pitch[i] while later means read
//     pitch[pos : pos + d]; when some pos < i (more zero durations than frames so far) a later mean reads an already overwritten
//     entry.  Such an utterance takes the sequential in-place loop on one lane and gets the reference's answer.
//   * pp_outlier_stats_kernel<T>: one workgroup per utterance; bitonic sort in LDS, numpy's linear percentiles, the keep mask and
//     the kept values' (count, mean, M2) in fp64 by the two-pass sums StandardScaler uses.  No floating-point atomics: the block
//     reductions are fixed trees and the partials are merged on the host in utterance order (Preprocess::merge_stats).
//   * pp_normalize_kernel<T>: (x - mean) / std in fp64 over the packed values of a call, one min / max pair per workgroup.
#pragma once
#include <cfloat>
#include <cmath>
#include <string>
#include <vector>

#include "melfront.h"

namespace mtts {

constexpr int kPpMaxValues = 4096;   // values of one utterance the outlier kernel sorts in LDS (32 KiB of doubles)
constexpr int kPpThreads = 256;

struct PpSeq { int T; int S; long long x0; long long d0; };      // frames at x0 of the packed values, phones at d0 of the packed durations
struct PpVal { int n; int pad_; long long x0; };                 // values of one utterance of the outlier step

// Block-wide fixed-tree reductions through LDS (deterministic; fp64 has no wave_sum).  `red` holds blockDim.x doubles.
__device__ __forceinline__ double pp_block_sum(double v, double* red) {
    const int tid = (int)threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = (int)blockDim.x >> 1; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double pp_block_min(double v, double* red) {
    const int tid = (int)threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = (int)blockDim.x >> 1; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid + s] < red[tid] ? red[tid + s] : red[tid];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// preprocessor.py:231-261 for one utterance per workgroup.  x: packed frame values; work: same size (interpolated copy, and the array
// the aliased loop rewrites in place); dur / pos: packed durations and their exclusive prefix sums (written here); out: packed [sum S].
template <class T>
__global__ void pp_segment_kernel(const T* x, T* work, const int* dur, int* pos, const PpSeq* seqs, T* out, int interpolate) {
    __shared__ int aliased;
    const PpSeq q = seqs[blockIdx.x];
    const T* xi = x + q.x0;
    T* w = work + q.x0;
    const int* d = dur + q.d0;
    int* p = pos + q.d0;
    T* o = out + q.d0;
    const int tid = (int)threadIdx.x, nth = (int)blockDim.x;
    if (tid == 0) {   // duration prefix sum (S is of max_seq_len order) and the aliasing test: iteration i reads an entry j < i iff pos_i < i
        int acc = 0, al = 0;
        for (int i = 0; i < q.S; ++i) {
            p[i] = acc;
            if (d[i] > 0 && acc < i) al = 1;
            acc += d[i];
        }
        aliased = al;
    }
    for (int t = tid; t < q.T; t += nth) {
        T v = xi[t];
        if (interpolate && v == (T)0) {   // interp1d(kind="linear", fill_value=(first voiced, last voiced)) at an unvoiced frame
            int a = t - 1, b = t + 1;
            while (a >= 0 && xi[a] == (T)0) --a;
            while (b < q.T && xi[b] == (T)0) ++b;
            if (a < 0) v = b < q.T ? xi[b] : (T)0;
            else if (b >= q.T) v = xi[a];
            else {
                const T slope = (xi[b] - xi[a]) / (T)(b - a);
                v = slope * (T)(t - a) + xi[a];
            }
        }
        w[t] = v;
    }
    __syncthreads();
    if (!aliased) {
        for (int i = tid; i < q.S; i += nth) {
            T m = (T)0;
            if (d[i] > 0) {
                const int lo = p[i] < q.T ? p[i] : q.T, hi = p[i] + d[i] < q.T ? p[i] + d[i] : q.T;   // a numpy slice clips at the end
                T s = (T)0;
                for (int k = lo; k < hi; ++k) s += w[k];
                m = s / (T)(hi - lo);                                                                  // (np.mean of an empty slice: nan)
            }
            o[i] = m;
        }
    } else if (tid == 0) {   // the reference's loop as written: w[i] is overwritten while later means still read w[pos : pos + d]
        for (int i = 0; i < q.S; ++i) {
            T m = (T)0;
            if (d[i] > 0) {
                const int lo = p[i] < q.T ? p[i] : q.T, hi = p[i] + d[i] < q.T ? p[i] + d[i] : q.T;
                T s = (T)0;
                for (int k = lo; k < hi; ++k) s += w[k];
                m = s / (T)(hi - lo);
            }
            w[i] = m;
            o[i] = m;
        }
    }
}

// remove_outlier (preprocessor.py:348-356) + the kept values' (count, mean, M2) for one utterance per workgroup.
// keep: packed bytes (1 = lower < v < upper); partials: [n_utts][3] doubles.
template <class T>
__global__ void pp_outlier_stats_kernel(const T* x, const PpVal* vals, unsigned char* keep, double* partials) {
    __shared__ double s[kPpMaxValues];
    __shared__ double red[kPpThreads];
    __shared__ double fence[2];
    const PpVal q = vals[blockIdx.x];
    const T* xi = x + q.x0;
    const int n = q.n, tid = (int)threadIdx.x, nth = (int)blockDim.x;
    double* out = partials + 3LL * blockIdx.x;
    if (n <= 0) {
        if (tid == 0) { out[0] = 0.0; out[1] = 0.0; out[2] = 0.0; }
        return;
    }
    int P = 2;
    while (P < n) P <<= 1;
    for (int i = tid; i < P; i += nth) s[i] = i < n ? (double)xi[i] : HUGE_VAL;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)          // bitonic sort, ascending
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += nth) {
                const int l = i ^ j;
                if (l > i) {
                    const double a = s[i], b = s[l];
                    const bool up = (i & k) == 0;
                    if (up ? a > b : a < b) { s[i] = b; s[l] = a; }
                }
            }
            __syncthreads();
        }
    if (tid == 0) {   // np.percentile(method="linear"): virtual index q (n - 1), numpy's two-sided lerp
        double pc[2];
        for (int h = 0; h < 2; ++h) {
            const double vi = (h == 0 ? 0.25 : 0.75) * (double)(n - 1);
            const double fl = floor(vi);
            int i0 = (int)fl, i1 = i0 + 1;
            if (i0 > n - 1) i0 = n - 1;
            if (i1 > n - 1) i1 = n - 1;
            const double a = s[i0], b = s[i1], t = vi - fl, diff = b - a;
            pc[h] = t >= 0.5 ? b - diff * (1.0 - t) : a + diff * t;
        }
        fence[0] = pc[0] - 1.5 * (pc[1] - pc[0]);
        fence[1] = pc[1] + 1.5 * (pc[1] - pc[0]);
    }
    __syncthreads();
    const double lower = fence[0], upper = fence[1];
    double sum = 0.0, cnt = 0.0;
    for (int i = tid; i < n; i += nth) {
        const double v = (double)xi[i];
        const bool k = v > lower && v < upper;
        keep[q.x0 + i] = k ? 1 : 0;
        if (k) { sum += v; cnt += 1.0; }
    }
    sum = pp_block_sum(sum, red);
    cnt = pp_block_sum(cnt, red);
    const double mean = cnt > 0.0 ? sum / cnt : 0.0;
    double corr = 0.0, sq = 0.0;   // sklearn's _incremental_mean_and_var: sum((x - mean)^2) - sum(x - mean)^2 / n
    for (int i = tid; i < n; i += nth) {
        const double v = (double)xi[i];
        if (v > lower && v < upper) { const double c = v - mean; corr += c; sq += c * c; }
    }
    corr = pp_block_sum(corr, red);
    sq = pp_block_sum(sq, red);
    if (tid == 0) {
        out[0] = cnt;
        out[1] = mean;
        out[2] = cnt > 0.0 ? sq - corr * corr / cnt : 0.0;
    }
}

// out = (x - mean) / std in fp64 (preprocessor.py:363); minmax[2 b], [2 b + 1] = this workgroup's minimum / maximum
template <class T>
__global__ void pp_normalize_kernel(const T* x, long long n, double mean, double stdv, double* out, double* minmax) {
    __shared__ double red[kPpThreads];
    double lo = DBL_MAX, hi = -DBL_MAX;   // np.finfo(np.float64).max / .min, the reference's starting values
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const double v = ((double)x[i] - mean) / stdv;
        out[i] = v;
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    lo = pp_block_min(lo, red);
    hi = -pp_block_min(-hi, red);
    if (threadIdx.x == 0) { minmax[2 * blockIdx.x] = lo; minmax[2 * blockIdx.x + 1] = hi; }
}

class Preprocess {
public:
    MelFront* mf = nullptr;
    // sized in bytes (values are float or double): values, interpolated copy, durations and their prefix sums, segment means or
    // normalised values, keep mask, per-utterance or per-workgroup partials, the PpSeq / PpVal table
    DevBuf<unsigned char> vals, work, durs, pos, outb, keepb, parts, descs;
    std::vector<PpSeq> h_seq;
    std::vector<PpVal> h_val;
    std::vector<double> h_minmax;

    int err(const std::string& s) { return mf->err(s); }   // (DEV_CHECK)

    // get_mel_from_wav of n_utts waveforms (packed in wav_host), each truncated to keep_frames[u] frames (< 0: all):
    // mel_host [sum T][n_mel] log-mel, energy_host [sum T]; T_u = min(n_u / hop + 1, keep_u)   (preprocessor.py:227-229)
    int mel_batch(int n_utts, const int* n_samples, const int* keep_frames, const float* wav_host, float* mel_host, float* energy_host) {
        const int n_fft = mf->n_fft;
        if (!mf->have_basis || !mf->have_mel) return err("STFT bases not loaded");
        if (n_utts < 1 || !n_samples || !wav_host || !mel_host || !energy_host) return err("mtts_stft_mel_batch: bad arguments (n_utts < 1 or NULL pointer)");
        mf->pack_begin();
        for (int u = 0; u < n_utts; ++u) {
            const int n = n_samples[u], keep = keep_frames ? keep_frames[u] : -1;
            if (n <= n_fft / 2)
                return err("mtts_stft_mel_batch: utterance " + std::to_string(u) + ": waveform too short for the reflection padding (need n_samples > filter_length / 2)");
            if (keep == 0) return err("mtts_stft_mel_batch: utterance " + std::to_string(u) + ": keep_frames == 0 (sum(duration) == 0: nothing to keep)");
            mf->pack_add(n, keep < 0 ? mf->frames_of(n) : std::min(mf->frames_of(n), keep));
        }
        if (mf->stage("mtts_stft_mel_batch", true) || mf->pad_waveforms(wav_host, true, true)) return -1;
        mf->forward_stft(mf->xp_rows, mf->rowmap, n_fft >= 1024 ? 3064 : 64);
        return mf->mel_from_spectrum(64, mel_host, energy_host);
    }

    // preprocessor.py:231-261.  values: packed [sum T] (dtype 0: float32, 1: float64); durations: packed [sum S]; out: packed [sum S]
    int phoneme_average(int n_utts, const int* n_frames, const int* n_phones, const int* durations, const void* values, int dtype, int interpolate,
                        void* out_host) {
        if (n_utts < 1 || !n_frames || !n_phones || !durations || !values || !out_host || (dtype != 0 && dtype != 1))
            return err("mtts_stft_phoneme_average: bad arguments (n_utts < 1, NULL pointer or dtype not 0 / 1)");
        h_seq.resize((size_t)n_utts);
        long long nx = 0, nd = 0;
        for (int u = 0; u < n_utts; ++u) {
            const int T = n_frames[u], S = n_phones[u];
            const std::string who = "mtts_stft_phoneme_average: utterance " + std::to_string(u) + ": ";
            if (T < 1 || S < 1) return err(who + "no frames or no phones");
            if (S > T) return err(who + "more phones than frames (S > T: the reference's in-place loop indexes past the end)");
            for (int i = 0; i < S; ++i)
                if (durations[nd + i] < 0) return err(who + "negative duration");
            if (interpolate) {
                int voiced = 0;
                for (int t = 0; t < T && voiced < 2; ++t)
                    voiced += dtype ? ((const double*)values)[nx + t] != 0.0 : ((const float*)values)[nx + t] != 0.f;
                if (voiced < 2) return err(who + "no voiced frame to interpolate between (fewer than two non-zero values; the reference drops the utterance)");
            }
            h_seq[(size_t)u] = PpSeq{T, S, nx, nd};
            nx += T;
            nd += S;
        }
        if (nx > (1LL << 30)) return err("mtts_stft_phoneme_average: too many frames in one call");
        const size_t esz = dtype ? sizeof(double) : sizeof(float);
        if (mf->grow(vals, (size_t)nx * esz, "values") || mf->grow(work, (size_t)nx * esz, "interpolated values") || mf->grow(durs, (size_t)nd * sizeof(int), "durations") ||
            mf->grow(pos, (size_t)nd * sizeof(int), "duration prefix sums") || mf->grow(outb, (size_t)nd * esz, "segment means") ||
            mf->grow(descs, (size_t)n_utts * sizeof(PpSeq), "utterances"))
            return -1;
        hipStream_t st = mf->stream;
        DEV_CHECK(hipMemcpyAsync(vals.p, values, (size_t)nx * esz, hipMemcpyHostToDevice, st));
        DEV_CHECK(hipMemcpyAsync(durs.p, durations, (size_t)nd * sizeof(int), hipMemcpyHostToDevice, st));
        DEV_CHECK(hipMemcpyAsync(descs.p, h_seq.data(), (size_t)n_utts * sizeof(PpSeq), hipMemcpyHostToDevice, st));
        if (dtype)
            MTTS_LAUNCH(pp_segment_kernel<double>, dim3((unsigned)n_utts), dim3(kPpThreads), st, (const double*)vals.p, (double*)work.p, (const int*)durs.p,
                        (int*)pos.p, (const PpSeq*)descs.p, (double*)outb.p, interpolate);
        else
            MTTS_LAUNCH(pp_segment_kernel<float>, dim3((unsigned)n_utts), dim3(kPpThreads), st, (const float*)vals.p, (float*)work.p, (const int*)durs.p,
                        (int*)pos.p, (const PpSeq*)descs.p, (float*)outb.p, interpolate);
        if (mf->check_launch()) return -1;
        DEV_CHECK(hipMemcpyAsync(out_host, outb.p, (size_t)nd * esz, hipMemcpyDeviceToHost, st));
        DEV_CHECK(hipStreamSynchronize(st));
        return 0;
    }

    // preprocessor.py:348-356 + the statistics of what it keeps.  values: packed [sum n]; keep_host: packed bytes; partials_host: [n_utts][3]
    int outlier_stats(int n_utts, const int* n_values, const void* values, int dtype, unsigned char* keep_host, double* partials_host) {
        if (n_utts < 1 || !n_values || !values || !keep_host || !partials_host || (dtype != 0 && dtype != 1))
            return err("mtts_stft_outlier_stats: bad arguments (n_utts < 1, NULL pointer or dtype not 0 / 1)");
        h_val.resize((size_t)n_utts);
        long long nx = 0;
        for (int u = 0; u < n_utts; ++u) {
            if (n_values[u] < 0 || n_values[u] > kPpMaxValues)
                return err("mtts_stft_outlier_stats: utterance " + std::to_string(u) + ": value count outside 0 .. " + std::to_string(kPpMaxValues) +
                           " (the per-utterance sort runs in LDS)");
            h_val[(size_t)u] = PpVal{n_values[u], 0, nx};
            nx += n_values[u];
        }
        const size_t esz = dtype ? sizeof(double) : sizeof(float);
        if (mf->grow(vals, (size_t)std::max<long long>(nx, 1) * esz, "values") || mf->grow(keepb, (size_t)std::max<long long>(nx, 1), "keep mask") ||
            mf->grow(parts, (size_t)n_utts * 3 * sizeof(double), "partial statistics") || mf->grow(descs, (size_t)n_utts * sizeof(PpVal), "utterances"))
            return -1;
        hipStream_t st = mf->stream;
        DEV_CHECK(hipMemcpyAsync(vals.p, values, (size_t)nx * esz, hipMemcpyHostToDevice, st));
        DEV_CHECK(hipMemcpyAsync(descs.p, h_val.data(), (size_t)n_utts * sizeof(PpVal), hipMemcpyHostToDevice, st));
        if (dtype)
            MTTS_LAUNCH(pp_outlier_stats_kernel<double>, dim3((unsigned)n_utts), dim3(kPpThreads), st, (const double*)vals.p, (const PpVal*)descs.p,
                        (unsigned char*)keepb.p, (double*)parts.p);
        else
            MTTS_LAUNCH(pp_outlier_stats_kernel<float>, dim3((unsigned)n_utts), dim3(kPpThreads), st, (const float*)vals.p, (const PpVal*)descs.p,
                        (unsigned char*)keepb.p, (double*)parts.p);
        if (mf->check_launch()) return -1;
        DEV_CHECK(hipMemcpyAsync(keep_host, keepb.p, (size_t)nx, hipMemcpyDeviceToHost, st));
        DEV_CHECK(hipMemcpyAsync(partials_host, parts.p, (size_t)n_utts * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
        DEV_CHECK(hipStreamSynchronize(st));
        return 0;
    }

    // StandardScaler.partial_fit's update (sklearn _incremental_mean_and_var), one (count, mean, M2) partial after the other in the
    // order given: a scalar recurrence over utterances, so it runs on the host.  state: (count, mean, M2), all zero to start.
    int merge_stats(double* state, int n, const double* partials) {
        if (!state || n < 0 || (n > 0 && !partials)) return err("mtts_stft_merge_stats: bad arguments");
        for (int u = 0; u < n; ++u) {
            const double nb = partials[3 * u], mb = partials[3 * u + 1], M2b = partials[3 * u + 2];
            if (nb < 0.0) return err("mtts_stft_merge_stats: negative count");
            if (nb == 0.0) continue;   // (build_from_path skips empty kept sets)
            const double na = state[0], last_sum = state[1] * na, new_sum = mb * nb, tot = na + nb;
            double M2 = M2b;
            if (na > 0.0) {
                const double r = na / nb, dlt = last_sum / r - new_sum;
                M2 = state[2] + M2b + r / tot * dlt * dlt;
            }
            state[0] = tot;
            state[1] = (last_sum + new_sum) / tot;
            state[2] = M2;
        }
        return 0;
    }

    // preprocessor.py:358-369 over the packed values of a call: out_host [n] float64, minmax_host = (min, max) of the normalised values
    int normalize(long long n, const void* values, int dtype, double mean, double stdv, double* out_host, double* minmax_host) {
        if (n < 1 || !values || !out_host || !minmax_host || (dtype != 0 && dtype != 1)) return err("mtts_stft_normalize: bad arguments (n < 1, NULL pointer or dtype not 0 / 1)");
        if (!(stdv != 0.0)) return err("mtts_stft_normalize: std == 0");
        const size_t esz = dtype ? sizeof(double) : sizeof(float);
        const int blocks = (int)std::min<long long>((n + kPpThreads - 1) / kPpThreads, 256);
        if (mf->grow(vals, (size_t)n * esz, "values") || mf->grow(outb, (size_t)n * sizeof(double), "normalised values") ||
            mf->grow(parts, (size_t)blocks * 2 * sizeof(double), "min / max partials"))
            return -1;
        hipStream_t st = mf->stream;
        DEV_CHECK(hipMemcpyAsync(vals.p, values, (size_t)n * esz, hipMemcpyHostToDevice, st));
        if (dtype)
            MTTS_LAUNCH(pp_normalize_kernel<double>, dim3((unsigned)blocks), dim3(kPpThreads), st, (const double*)vals.p, n, mean, stdv, (double*)outb.p, (double*)parts.p);
        else
            MTTS_LAUNCH(pp_normalize_kernel<float>, dim3((unsigned)blocks), dim3(kPpThreads), st, (const float*)vals.p, n, mean, stdv, (double*)outb.p, (double*)parts.p);
        if (mf->check_launch()) return -1;
        h_minmax.resize((size_t)blocks * 2);
        DEV_CHECK(hipMemcpyAsync(out_host, outb.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
        DEV_CHECK(hipMemcpyAsync(h_minmax.data(), parts.p, (size_t)blocks * 2 * sizeof(double), hipMemcpyDeviceToHost, st));
        DEV_CHECK(hipStreamSynchronize(st));
        double lo = h_minmax[0], hi = h_minmax[1];
        for (int b = 1; b < blocks; ++b) { lo = std::min(lo, h_minmax[(size_t)2 * b]); hi = std::max(hi, h_minmax[(size_t)2 * b + 1]); }
        minmax_host[0] = lo;
        minmax_host[1] = hi;
        return 0;
    }
};

}  // namespace mtts
