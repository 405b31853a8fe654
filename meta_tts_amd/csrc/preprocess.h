// Waveform batches -> the preprocessed feature tree's values on the device: the wav -> features half of the preprocessing stage.
//
// Reference: preprocessor/preprocessor.py:188-306 (Preprocessor.process_utterance: get_mel_from_wav truncated to sum(duration) frames,
// interp1d over the unvoiced pitch frames, the in-place phoneme-level segment mean of pitch (float64) and energy (float32)), :348-356
// (remove_outlier: np.percentile 25 / 75 with linear interpolation, 1.5 IQR fences, strict inequalities), :60-185 (build_from_path:
// StandardScaler.partial_fit over the kept values utterance by utterance) and :358-369 (normalize: (x - mean) / std and the global
// minimum / maximum of the normalised values).
//
// MI355X layout.  Every utterance of a call goes through the same launches; only descriptor tables are built by a host loop.
//   * front-end (Preprocess::mel_batch): one clip + reflect-pad kernel writes every utterance's padded signal at a multiple of hop
//     (griffin.h's packing), the forward STFT is ONE implicit GEMM over overlapping rows (lda = hop) whose rows between two utterances
//     are dropped through GemmArgs::c_rowmap, then melfront.h's magnitude + energy pass, the mel GEMM and the log-clamp over the
//     compact [sum T] rows.  Both GEMMs name their kernel explicitly (no split-K, no size-dependent choice), so an utterance's rows
//     do not depend on what else is in the call.
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

#include "griffin.h"

namespace mtts {

constexpr int kPpMaxValues = 4096;   // values of one utterance the outlier kernel sorts in LDS (32 KiB of doubles)
constexpr int kPpThreads = 256;

struct PpWav { int n; int T; long long wav0; long long xp0; };   // samples, kept frames, first sample (packed input / padded signal)
struct PpSeq { int T; int S; long long x0; long long d0; };      // frames at x0 of the packed values, phones at d0 of the packed durations
struct PpVal { int n; int pad_; long long x0; };                 // values of one utterance of the outlier step

// xp[xp0 + j] = clip(wav[wav0 + reflect(j - pad)], -1, 1) for the hop * (T - 1) + n_fft samples the kept frames read
// (tools.py:9 + stft.py:60-65).  blockIdx.y = utterance.
__global__ void pp_clip_pad_kernel(const float* wav, const PpWav* utts, int pad, int hop, int n_fft, float* xp) {
    const PpWav u = utts[blockIdx.y];
    const long long total = (long long)hop * (u.T - 1) + n_fft;
    for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < total; j += (long long)gridDim.x * blockDim.x) {
        long long s = j - pad;
        if (s < 0) s = -s;
        else if (s >= u.n) s = 2LL * (u.n - 1) - s;
        float v = wav[u.wav0 + s];
        v = v < -1.f ? -1.f : (v > 1.f ? 1.f : v);
        xp[u.xp0 + j] = v;
    }
}

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
    struct Buf { void* p = nullptr; size_t cap = 0; };
    Buf wav, xp, spec, mag, mel, energy, rowmap, descs, vals, work, durs, pos, outb, keepb, parts;
    std::vector<int> h_rowmap;
    std::vector<PpWav> h_wav;
    std::vector<PpSeq> h_seq;
    std::vector<PpVal> h_val;
    std::vector<double> h_minmax;

    void set_error(const std::string& s) { mf->set_error(s); }   // (MF_CHECK)
    int err(const std::string& s) { set_error(s); return -1; }
    void destroy() {
        for (Buf* b : {&wav, &xp, &spec, &mag, &mel, &energy, &rowmap, &descs, &vals, &work, &durs, &pos, &outb, &keepb, &parts})
            if (b->p) { hipFree(b->p); b->p = nullptr; b->cap = 0; }
    }
    int grow(Buf& b, size_t bytes, const char* what) {   // the workspace grows on demand, as Griffin-Lim's does
        if (bytes <= b.cap) return 0;
        const size_t n = std::max(bytes + bytes / 4, (size_t)4096);
        if (b.p) { hipStreamSynchronize(mf->stream); hipFree(b.p); b.p = nullptr; b.cap = 0; }
        if (hipMalloc(&b.p, n) != hipSuccess) { b.p = nullptr; return err(std::string("hipMalloc failed (preprocessing workspace: ") + what + ")"); }
        b.cap = n;
        return 0;
    }
    int check_launch() {
        if (mf->gx.error) { std::string e = std::string("GEMM launcher: ") + mf->gx.error; mf->gx.error = nullptr; return err(e); }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return err(std::string("kernel launch failed: ") + hipGetErrorString(e));
        return 0;
    }

    // get_mel_from_wav of n_utts waveforms (packed in wav_host), each truncated to keep_frames[u] frames (< 0: all):
    // mel_host [sum T][n_mel] log-mel, energy_host [sum T]; T_u = min(n_u / hop + 1, keep_u)   (preprocessor.py:227-229)
    int mel_batch(int n_utts, const int* n_samples, const int* keep_frames, const float* wav_host, float* mel_host, float* energy_host) {
        const int n_fft = mf->n_fft, hop = mf->hop, F = mf->F, ld = mf->ld_spec, ld_mag = mf->ld_mag, n_mel = mf->n_mel;
        if (!mf->have_basis || !mf->have_mel) return err("STFT bases not loaded");
        if (n_utts < 1 || !n_samples || !wav_host || !mel_host || !energy_host) return err("mtts_stft_mel_batch: bad arguments (n_utts < 1 or NULL pointer)");
        h_wav.resize((size_t)n_utts);
        long long samples = 0, rows = 0, xp_rows = 0, max_span = 0;
        const int extra = (n_fft + hop - 1) / hop - 1;   // rows that straddle two packed padded signals
        for (int u = 0; u < n_utts; ++u) {
            const int n = n_samples[u], keep = keep_frames ? keep_frames[u] : -1;
            if (n <= n_fft / 2)
                return err("mtts_stft_mel_batch: utterance " + std::to_string(u) + ": waveform too short for the reflection padding (need n_samples > filter_length / 2)");
            if (keep == 0) return err("mtts_stft_mel_batch: utterance " + std::to_string(u) + ": keep_frames == 0 (sum(duration) == 0: nothing to keep)");
            const int full = n / hop + 1, T = keep < 0 ? full : std::min(full, keep);
            h_wav[(size_t)u] = PpWav{n, T, samples, xp_rows * hop};
            samples += n;
            rows += T;
            xp_rows += T + extra;
            max_span = std::max(max_span, (long long)hop * (T - 1) + n_fft);
        }
        if (rows > (1LL << 30) / std::max(ld, n_fft) || xp_rows > (1LL << 30) || samples > (1LL << 31) - 1)
            return err("mtts_stft_mel_batch: too many frames in one call");
        h_rowmap.assign((size_t)xp_rows, -1);
        for (int u = 0, r = 0; u < n_utts; ++u)
            for (int t = 0; t < h_wav[(size_t)u].T; ++t) h_rowmap[(size_t)(h_wav[(size_t)u].xp0 / hop + t)] = r++;
        const size_t xp_len = (size_t)xp_rows * hop + n_fft + 64;
        if (grow(wav, (size_t)samples * sizeof(float), "waveforms") || grow(xp, xp_len * sizeof(float), "padded signals") ||
            grow(spec, ((size_t)rows * ld + 64) * sizeof(float), "spectrum") || grow(mag, ((size_t)rows * ld_mag + 64) * sizeof(float), "magnitude") ||
            grow(mel, ((size_t)rows * n_mel + 64) * sizeof(float), "mel") || grow(energy, (size_t)rows * sizeof(float), "energy") ||
            grow(rowmap, (size_t)xp_rows * sizeof(int), "row map") || grow(descs, (size_t)n_utts * sizeof(PpWav), "utterances"))
            return -1;
        hipStream_t st = mf->stream;
        MF_CHECK(hipMemcpyAsync(wav.p, wav_host, (size_t)samples * sizeof(float), hipMemcpyHostToDevice, st));
        MF_CHECK(hipMemcpyAsync(descs.p, h_wav.data(), (size_t)n_utts * sizeof(PpWav), hipMemcpyHostToDevice, st));
        MF_CHECK(hipMemcpyAsync(rowmap.p, h_rowmap.data(), (size_t)xp_rows * sizeof(int), hipMemcpyHostToDevice, st));
        MF_CHECK(hipMemsetAsync(xp.p, 0, xp_len * sizeof(float), st));   // (gaps are read only by dropped rows)
        const dim3 pad_grid((unsigned)std::min<long long>((max_span + 255) / 256, 1024), (unsigned)n_utts);
        MTTS_LAUNCH(pp_clip_pad_kernel, pad_grid, dim3(256), st, (const float*)wav.p, (const PpWav*)descs.p, n_fft / 2, hop, n_fft, (float*)xp.p);
        {   // spec [sum T][2F] = overlapping frames of the packed padded signals * basis^T, rows between utterances dropped
            GemmArgs g;
            g.A = (const float*)xp.p; g.lda = hop; g.B = mf->basis; g.ldb = n_fft; g.C = (float*)spec.p; g.ldc = ld;
            g.M = (int)xp_rows; g.N = 2 * F; g.K = n_fft; g.c_rowmap = (const int*)rowmap.p;
            gemm_launch(mf->gx, GEMM_NT, g, (int)xp_rows, 2 * F, 1, st, n_fft >= 1024 ? 3064 : 64, 2.0 * xp_rows * 2.0 * F * n_fft, 0);
        }
        MTTS_LAUNCH(stft_magnitude_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), st, (const float*)spec.p, ld, (int)rows, F, (float*)mag.p, ld_mag,
                    (float*)energy.p);
        {   // mel [sum T][n_mel] = mag * mel_basis^T (both zero padded to ld_mag columns)
            GemmArgs g;
            g.A = (const float*)mag.p; g.lda = ld_mag; g.B = mf->melb; g.ldb = ld_mag; g.C = (float*)mel.p; g.ldc = n_mel;
            g.M = (int)rows; g.N = n_mel; g.K = ld_mag;
            gemm_launch(mf->gx, GEMM_NT, g, (int)rows, n_mel, 1, st, 64, 2.0 * rows * (double)n_mel * F, 0);
        }
        MTTS_LAUNCH(log_clamp_kernel, dim3(1024), dim3(256), st, (float*)mel.p, rows * n_mel, 1e-5f);
        if (check_launch()) return -1;
        MF_CHECK(hipMemcpyAsync(mel_host, mel.p, (size_t)rows * n_mel * sizeof(float), hipMemcpyDeviceToHost, st));
        MF_CHECK(hipMemcpyAsync(energy_host, energy.p, (size_t)rows * sizeof(float), hipMemcpyDeviceToHost, st));
        MF_CHECK(hipStreamSynchronize(st));
        return 0;
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
        if (grow(vals, (size_t)nx * esz, "values") || grow(work, (size_t)nx * esz, "interpolated values") || grow(durs, (size_t)nd * sizeof(int), "durations") ||
            grow(pos, (size_t)nd * sizeof(int), "duration prefix sums") || grow(outb, (size_t)nd * esz, "segment means") ||
            grow(descs, (size_t)n_utts * sizeof(PpSeq), "utterances"))
            return -1;
        hipStream_t st = mf->stream;
        MF_CHECK(hipMemcpyAsync(vals.p, values, (size_t)nx * esz, hipMemcpyHostToDevice, st));
        MF_CHECK(hipMemcpyAsync(durs.p, durations, (size_t)nd * sizeof(int), hipMemcpyHostToDevice, st));
        MF_CHECK(hipMemcpyAsync(descs.p, h_seq.data(), (size_t)n_utts * sizeof(PpSeq), hipMemcpyHostToDevice, st));
        if (dtype)
            MTTS_LAUNCH(pp_segment_kernel<double>, dim3((unsigned)n_utts), dim3(kPpThreads), st, (const double*)vals.p, (double*)work.p, (const int*)durs.p,
                        (int*)pos.p, (const PpSeq*)descs.p, (double*)outb.p, interpolate);
        else
            MTTS_LAUNCH(pp_segment_kernel<float>, dim3((unsigned)n_utts), dim3(kPpThreads), st, (const float*)vals.p, (float*)work.p, (const int*)durs.p,
                        (int*)pos.p, (const PpSeq*)descs.p, (float*)outb.p, interpolate);
        if (check_launch()) return -1;
        MF_CHECK(hipMemcpyAsync(out_host, outb.p, (size_t)nd * esz, hipMemcpyDeviceToHost, st));
        MF_CHECK(hipStreamSynchronize(st));
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
        if (grow(vals, (size_t)std::max<long long>(nx, 1) * esz, "values") || grow(keepb, (size_t)std::max<long long>(nx, 1), "keep mask") ||
            grow(parts, (size_t)n_utts * 3 * sizeof(double), "partial statistics") || grow(descs, (size_t)n_utts * sizeof(PpVal), "utterances"))
            return -1;
        hipStream_t st = mf->stream;
        MF_CHECK(hipMemcpyAsync(vals.p, values, (size_t)nx * esz, hipMemcpyHostToDevice, st));
        MF_CHECK(hipMemcpyAsync(descs.p, h_val.data(), (size_t)n_utts * sizeof(PpVal), hipMemcpyHostToDevice, st));
        if (dtype)
            MTTS_LAUNCH(pp_outlier_stats_kernel<double>, dim3((unsigned)n_utts), dim3(kPpThreads), st, (const double*)vals.p, (const PpVal*)descs.p,
                        (unsigned char*)keepb.p, (double*)parts.p);
        else
            MTTS_LAUNCH(pp_outlier_stats_kernel<float>, dim3((unsigned)n_utts), dim3(kPpThreads), st, (const float*)vals.p, (const PpVal*)descs.p,
                        (unsigned char*)keepb.p, (double*)parts.p);
        if (check_launch()) return -1;
        MF_CHECK(hipMemcpyAsync(keep_host, keepb.p, (size_t)nx, hipMemcpyDeviceToHost, st));
        MF_CHECK(hipMemcpyAsync(partials_host, parts.p, (size_t)n_utts * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
        MF_CHECK(hipStreamSynchronize(st));
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
        if (grow(vals, (size_t)n * esz, "values") || grow(outb, (size_t)n * sizeof(double), "normalised values") ||
            grow(parts, (size_t)blocks * 2 * sizeof(double), "min / max partials"))
            return -1;
        hipStream_t st = mf->stream;
        MF_CHECK(hipMemcpyAsync(vals.p, values, (size_t)n * esz, hipMemcpyHostToDevice, st));
        if (dtype)
            MTTS_LAUNCH(pp_normalize_kernel<double>, dim3((unsigned)blocks), dim3(kPpThreads), st, (const double*)vals.p, n, mean, stdv, (double*)outb.p, (double*)parts.p);
        else
            MTTS_LAUNCH(pp_normalize_kernel<float>, dim3((unsigned)blocks), dim3(kPpThreads), st, (const float*)vals.p, n, mean, stdv, (double*)outb.p, (double*)parts.p);
        if (check_launch()) return -1;
        h_minmax.resize((size_t)blocks * 2);
        MF_CHECK(hipMemcpyAsync(out_host, outb.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
        MF_CHECK(hipMemcpyAsync(h_minmax.data(), parts.p, (size_t)blocks * 2 * sizeof(double), hipMemcpyDeviceToHost, st));
        MF_CHECK(hipStreamSynchronize(st));
        double lo = h_minmax[0], hi = h_minmax[1];
        for (int b = 1; b < blocks; ++b) { lo = std::min(lo, h_minmax[(size_t)2 * b]); hi = std::max(hi, h_minmax[(size_t)2 * b + 1]); }
        minmax_host[0] = lo;
        minmax_host[1] = hi;
        return 0;
    }
};

}  // namespace mtts
