// Silence trimming of waveform batches on the device: the last step of resemblyzer's `preprocess_wav`, behind resample.h's two.
//
// Reference: every speaker-encoder entry calls `preprocess_wav` (evaluation/wavs_to_dvector.py:206-296, preprocessor/preprocessor.py:265,
// dataset.py:8), whose third step is `trim_long_silences`: webrtcvad's voiced / unvoiced decision per 30 ms window, a moving average
// of width 8 rounded to bool, a binary dilation by 7 windows, and the samples of the windows kept.  webrtcvad's GMM decision is third
// party and NOT restated; parity with it is UNPINNED.  What stands in its place is stated in include/mtts.h (and, in float64 numpy,
// in tests/vad_oracle.py): per utterance of n samples, W = window_ms * sampling_rate / 1000, n_w = floor(n / W) windows (the last
// n mod W samples are dropped, as resemblyzer drops them),
//     e[w]   = mean of x^2 over window w                                  (float64; see below)
//     noise  = the k-th smallest e[w], k = floor(noise_quantile * (n_w - 1))   (an order statistic, no interpolation)
//     raw[w] = e[w] >= max(10^(floor_db / 10), noise * 10^(margin_db / 10))    (or the caller's flags, one byte per window)
// and then resemblyzer's post-processing, restated exactly:
//     smooth[w] = round(mean(raw[w - (ma_width - 1) / 2 .. w + ma_width / 2]))   zeros outside, numpy's round: 2 * count > ma_width
//     mask[w]   = any smooth[w - max_silence / 2 .. w + (max_silence + 1) / 2]   the centred structure of max_silence + 1 ones
//     out       = the samples of the windows kept, in order; when none is kept the utterance passes through as it is (all n samples).
//
// MI355X layout.  The data volume is tiny (64 x 5 s at 16 kHz = 20 MB), so the stage is three launches and one read-back of lengths:
//   * vad_energy_kernel: one wavefront per window (blockIdx.y = utterance through a small table, as the resampling and pitch kernels
//     do), coalesced dword loads — a window of a packed buffer starts at any sample, so no wider load is assumed.  A lane adds the
//     squares of its samples (lane, lane + 64, ...) in ascending order in fp64 — the product of two fp32 values is exact there — and
//     a fixed tree over the 64 lanes follows (LDS and barriers, no wavefront intrinsic, so the SIMT emulator runs the same source).
//   * vad_mask_kernel: one 256-thread workgroup per utterance with its at most 4096 energies (about 122 s) in LDS as fp64 (32 KB):
//     a bitonic sort for the order statistic, the flags, the smoothing count in integers, the dilation, and an inclusive scan of the
//     kept windows that gives every kept window its destination; then n_out and n_voiced.
//   * vad_compact_kernel: one wavefront per window copies the kept windows to their destinations in ANOTHER buffer (a parallel
//     left-shift in place would race): the source is this stage's staging buffer, the destination MelFront::wav.
// No atomics anywhere: an utterance's energies, mask and output depend on its samples and the configuration only, so they are
// bit-identical alone, in any batch, at any position.  The host reads the lengths once between the mask and the compaction (the
// packed destinations follow from them), which is the stage's only synchronisation.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "melfront.h"

namespace mtts {

constexpr int VAD_THREADS = 256;
constexpr int VAD_MAX_W = 4096;   // windows of one utterance, at most (fp64 in LDS: 32 KB)

struct VadCfg {
    int W;                 // samples per window
    int ma_width, ma_l;    // moving average: raw[w - ma_l .. w - ma_l + ma_width)
    int dil_l, dil_r;      // dilation: smooth[w - dil_l .. w + dil_r]
    int pad_;
    double quantile, floor_lin, margin_lin;   // 10^(floor_db / 10), 10^(margin_db / 10)
};

struct VadUtt {
    int n, n_w;          // samples, floor(n / W)
    int win0, pad_;      // first window of this utterance in the packed per-window arrays
    long long src0;      // first sample in the staging buffer
    long long dst0;      // first output sample in the destination buffer (known once the lengths have been read back)
};

// e[win0 + w] = mean of src[src0 + w W .. + W)^2.  gridDim.x covers the longest utterance, four windows per workgroup.
__global__ __launch_bounds__(VAD_THREADS) void vad_energy_kernel(const float* src, const VadUtt* utts, int W, double* e) {
    __shared__ double red[VAD_THREADS];
    const VadUtt u = utts[blockIdx.y];
    if ((int)blockIdx.x * 4 >= u.n_w) return;   // (the whole workgroup: no barrier is left waiting)
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int w = (int)blockIdx.x * 4 + (tid >> 6);
    double s = 0.0;
    if (w < u.n_w) {
        const float* x = src + u.src0 + (long long)w * W;
        for (int i = lane; i < W; i += 64) {
            const double v = (double)x[i];
            s += v * v;
        }
    }
    red[tid] = s;
    __syncthreads();
    for (int h = 32; h > 0; h >>= 1) {
        if (lane < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (lane == 0 && w < u.n_w) e[u.win0 + w] = red[tid] / (double)W;
}

// One workgroup per utterance (blockIdx.x): raw flags (from e, or flags_in when given), smoothing, dilation, scan.
// mask[win0 + w] = 1 for a kept window; woff[win0 + w] = how many kept windows precede it (-1 for a dropped one);
// nout[2 u] = samples out (W * kept, or n when nothing is kept: the pass-through), nout[2 u + 1] = kept windows.
__global__ __launch_bounds__(VAD_THREADS) void vad_mask_kernel(const VadUtt* utts, VadCfg c, const double* e, const unsigned char* flags_in, unsigned char* mask,
                                                               int* woff, int* nout) {
    __shared__ double es[VAD_MAX_W];
    __shared__ unsigned char fa[VAD_MAX_W], fb[VAD_MAX_W];
    __shared__ int cnt[VAD_THREADS];
    const VadUtt u = utts[blockIdx.x];
    const int tid = (int)threadIdx.x, n_w = u.n_w;   // n_w <= VAD_MAX_W: refused on the host otherwise
    if (!flags_in) {
        int P = 1;
        while (P < n_w) P <<= 1;
        for (int i = tid; i < P; i += VAD_THREADS) es[i] = i < n_w ? e[u.win0 + i] : __builtin_huge_val();
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < P; i += VAD_THREADS) {
                    const int l = i ^ j;
                    if (l > i) {
                        const double a = es[i], b = es[l];
                        if (((i & k) == 0) ? (a > b) : (a < b)) { es[i] = b; es[l] = a; }
                    }
                }
                __syncthreads();
            }
        if (n_w > 0) {
            int k = (int)floor(c.quantile * (double)(n_w - 1));
            k = k < 0 ? 0 : (k > n_w - 1 ? n_w - 1 : k);
            const double t = es[k] * c.margin_lin;
            const double thr = c.floor_lin > t ? c.floor_lin : t;
            for (int i = tid; i < n_w; i += VAD_THREADS) fa[i] = e[u.win0 + i] >= thr ? 1 : 0;
        }
    } else {
        for (int i = tid; i < n_w; i += VAD_THREADS) fa[i] = flags_in[u.win0 + i] ? 1 : 0;
    }
    __syncthreads();
    for (int i = tid; i < n_w; i += VAD_THREADS) {
        int s = 0;
        for (int j = 0; j < c.ma_width; ++j) {
            const int q = i - c.ma_l + j;
            if (q >= 0 && q < n_w) s += fa[q];
        }
        fb[i] = 2 * s > c.ma_width ? 1 : 0;
    }
    __syncthreads();
    for (int i = tid; i < n_w; i += VAD_THREADS) {
        int any = 0;
        for (int q = i - c.dil_l; q <= i + c.dil_r; ++q)
            if (q >= 0 && q < n_w) any |= fb[q];
        fa[i] = (unsigned char)any;
    }
    __syncthreads();
    // a lane owns VAD_MAX_W / VAD_THREADS consecutive windows; an inclusive scan of the lanes' counts gives its first destination
    constexpr int PER = VAD_MAX_W / VAD_THREADS;
    const int lo = tid * PER, hi = lo + PER < n_w ? lo + PER : n_w;
    int mine = 0;
    for (int i = lo; i < hi; ++i) mine += fa[i];
    cnt[tid] = mine;
    __syncthreads();
    for (int off = 1; off < VAD_THREADS; off <<= 1) {
        const int v = tid >= off ? cnt[tid - off] : 0;
        __syncthreads();
        cnt[tid] += v;
        __syncthreads();
    }
    int at = cnt[tid] - mine;
    for (int i = lo; i < hi; ++i) {
        mask[u.win0 + i] = fa[i];
        woff[u.win0 + i] = fa[i] ? at++ : -1;
    }
    if (tid == 0) {
        const int kept = cnt[VAD_THREADS - 1];
        nout[2 * blockIdx.x] = kept > 0 ? kept * c.W : u.n;
        nout[2 * blockIdx.x + 1] = kept;
    }
}

// dst[dst0 + woff W ..] = src[src0 + w W ..) for every kept window w, one wavefront per window slot; an utterance that keeps nothing is
// copied whole (slot n_w is its tail of n mod W samples).  blockIdx.y = utterance; src and dst are different buffers.
__global__ __launch_bounds__(VAD_THREADS) void vad_compact_kernel(const float* src, const VadUtt* utts, int W, const int* woff, const int* nout, float* dst) {
    const VadUtt u = utts[blockIdx.y];
    const int lane = (int)threadIdx.x & 63;
    const int s = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (s > u.n_w) return;
    long long to = (long long)s * W;
    int len = W;
    if (nout[2 * blockIdx.y + 1] == 0) {
        if (s == u.n_w) len = u.n - u.n_w * W;
    } else {
        if (s == u.n_w) return;
        const int o = woff[u.win0 + s];
        if (o < 0) return;
        to = (long long)o * W;
    }
    const float* x = src + u.src0 + (long long)s * W;
    float* y = dst + u.dst0 + to;
    for (int i = lane; i < len; i += 64) y[i] = x[i];
}

class Vad {
public:
    MelFront* mf = nullptr;
    VadCfg c{};
    bool loaded = false;
    DevBuf<float> stage;            // the untrimmed waveforms of a call (or of a chunk of one): the compaction's source
    DevBuf<double> e;               // [sum n_w]
    DevBuf<unsigned char> mask, flags;
    DevBuf<int> woff, nout;         // [sum n_w]; [n_utts][2]
    DevBuf<VadUtt> utts;
    std::vector<VadUtt> h_utts;
    std::vector<int> h_nout;
    long long n_src = 0;
    int n_win = 0, max_nw = 0;

    int err(const std::string& s) { return mf->err(s); }

    int load(int sampling_rate, int window_ms, int ma_width, int max_silence, double floor_db, double noise_quantile, double margin_db) {
        const char* who = "mtts_stft_load_vad: ";
        if (sampling_rate < 1 || window_ms < 1) return err(std::string(who) + "bad arguments (need sampling_rate >= 1, window_ms >= 1)");
        const long long ws = (long long)window_ms * sampling_rate;
        if (ws % 1000 != 0) return err(std::string(who) + "window_ms * sampling_rate = " + std::to_string(ws) + " is not a multiple of 1000");
        if (ws / 1000 > (1 << 24)) return err(std::string(who) + "window too long");
        if (ma_width < 1 || ma_width > 64) return err(std::string(who) + "ma_width outside 1 .. 64");
        if (max_silence < 1 || max_silence > 64) return err(std::string(who) + "max_silence outside 1 .. 64");
        if (!(noise_quantile >= 0.0 && noise_quantile <= 1.0)) return err(std::string(who) + "noise_quantile outside [0, 1]");
        if (!std::isfinite(floor_db) || !std::isfinite(margin_db)) return err(std::string(who) + "non-finite threshold (floor_db, margin_db)");
        VadCfg n{};
        n.W = (int)(ws / 1000);
        n.ma_width = ma_width;
        n.ma_l = (ma_width - 1) / 2;
        n.dil_l = max_silence / 2;          // a centred structure of L = max_silence + 1 ones: (L - 1) / 2 to the left, L / 2 to the right
        n.dil_r = (max_silence + 1) / 2;
        n.quantile = noise_quantile;
        n.floor_lin = std::pow(10.0, floor_db / 10.0);
        n.margin_lin = std::pow(10.0, margin_db / 10.0);
        if (!std::isfinite(n.floor_lin) || !std::isfinite(n.margin_lin)) return err(std::string(who) + "non-finite threshold (floor_db, margin_db)");
        c = n;
        loaded = true;
        return 0;
    }

    // what both entries refuse before any launch; n[u] = samples at the rate the detector runs at
    template <class Len>
    int check_lengths(const std::string& who, int n_utts, const Len* n) {
        if (!loaded) return err(who + "no VAD configuration loaded (mtts_stft_load_vad)");
        if (mf->check_utterances(who, n_utts, [&](int u) { return n[u]; }, MelFront::UTT_GRID | MelFront::UTT_CAP)) return -1;
        for (int u = 0; u < n_utts; ++u)
            if (n[u] / c.W > VAD_MAX_W)
                return err(who + "utterance " + std::to_string(u) + ": " + std::to_string(n[u] / c.W) + " windows of " + std::to_string(c.W) + " samples exceed the " +
                           std::to_string(VAD_MAX_W) + " a workgroup holds");
        return 0;
    }

    // ---- the table of a launch: host only ------------------------------------------------------------------------------------------------
    void table_begin() { h_utts.clear(); n_src = 0; n_win = 0; max_nw = 0; }
    void table_add(long long n) {
        const int n_w = (int)(n / c.W);
        h_utts.push_back(VadUtt{(int)n, n_w, n_win, 0, n_src, 0});
        n_src += n;
        n_win += n_w;
        max_nw = std::max(max_nw, n_w);
    }
    // room for a launch of at most n_src_ samples, n_win_ windows and n_utts_ utterances
    int reserve(long long n_src_, long long n_win_, size_t n_utts_, bool with_flags) {
        const size_t nw = (size_t)n_win_ + 1;
        return mf->grow(stage, (size_t)n_src_ + 64, "untrimmed waveforms") || mf->grow(e, nw, "window energies") || mf->grow(mask, nw, "window mask") ||
               mf->grow(woff, nw, "window destinations") || (with_flags && mf->grow(flags, nw, "window flags")) || mf->grow(nout, 2 * n_utts_, "trimmed lengths") ||
               mf->grow(utts, n_utts_, "VAD utterances") ? -1 : 0;
    }
    // The tabled utterances, already in `stage` at their src0 (enqueued on mf->stream): energies, mask, and the lengths read back into
    // h_nout [n_utts][2] = (samples out, windows kept).  Synchronises mf->stream.
    int detect(const unsigned char* flags_host) {
        const unsigned n_utts = (unsigned)h_utts.size();
        DEV_CHECK(hipMemcpyAsync(utts.p, h_utts.data(), h_utts.size() * sizeof(VadUtt), hipMemcpyHostToDevice, mf->stream));
        if (flags_host) {
            if (n_win > 0) DEV_CHECK(hipMemcpyAsync(flags.p, flags_host, (size_t)n_win, hipMemcpyHostToDevice, mf->stream));
        } else if (max_nw > 0)
            MTTS_LAUNCH(vad_energy_kernel, dim3((unsigned)((max_nw + 3) / 4), n_utts), dim3(VAD_THREADS), mf->stream, (const float*)stage.p, (const VadUtt*)utts.p, c.W,
                        e.p);
        MTTS_LAUNCH(vad_mask_kernel, dim3(n_utts), dim3(VAD_THREADS), mf->stream, (const VadUtt*)utts.p, c, (const double*)e.p,
                    (const unsigned char*)(flags_host ? flags.p : nullptr), mask.p, woff.p, nout.p);
        if (mf->check_launch()) return -1;
        h_nout.resize(2 * (size_t)n_utts);
        DEV_CHECK(hipMemcpyAsync(h_nout.data(), nout.p, h_nout.size() * sizeof(int), hipMemcpyDeviceToHost, mf->stream));
        DEV_CHECK(hipStreamSynchronize(mf->stream));
        return 0;
    }
    // The kept windows -> dst at the dst0 the caller has written into h_utts (after detect).  Asynchronous on mf->stream; h_utts must
    // stay as it is until the stream has been synchronised.
    int compact(float* dst) {
        DEV_CHECK(hipMemcpyAsync(utts.p, h_utts.data(), h_utts.size() * sizeof(VadUtt), hipMemcpyHostToDevice, mf->stream));
        MTTS_LAUNCH(vad_compact_kernel, dim3((unsigned)((max_nw + 1 + 3) / 4), (unsigned)h_utts.size()), dim3(VAD_THREADS), mf->stream, (const float*)stage.p,
                    (const VadUtt*)utts.p, c.W, (const int*)woff.p, (const int*)nout.p, dst);
        return 0;
    }

    // host in, host out: wavs = the utterances one after another; out = the trimmed ones one after another.  Returns the samples out.
    long long trim_batch(int n_utts, const int* n_samples, const float* wavs, const unsigned char* flags_in, float* out, int* n_out, int* n_voiced_out,
                         unsigned char* mask_out, double* energy_out) {
        const char* who = "mtts_stft_trim_batch: ";
        if (n_utts < 1 || !n_samples || !wavs || !out || !n_out) return err(std::string(who) + "bad arguments (n_utts < 1 or NULL n_samples / wavs / out / n_out)");
        if (check_lengths(who, n_utts, n_samples)) return -1;
        table_begin();
        for (int u = 0; u < n_utts; ++u) table_add(n_samples[u]);
        if (n_src > (1LL << 31) - 1) return err(std::string(who) + "too many samples in one call");
        if (reserve(n_src, n_win, (size_t)n_utts, flags_in != nullptr) || mf->grow(mf->wav, (size_t)n_src + 64, "waveforms")) return -1;
        DEV_CHECK(hipMemcpyAsync(stage.p, wavs, (size_t)n_src * sizeof(float), hipMemcpyHostToDevice, mf->stream));
        if (detect(flags_in)) return -1;
        long long total = 0;
        for (int u = 0; u < n_utts; ++u) {
            h_utts[(size_t)u].dst0 = total;
            total += h_nout[2 * (size_t)u];
        }
        if (compact(mf->wav.p) || mf->check_launch()) return -1;
        DEV_CHECK(hipMemcpyAsync(out, mf->wav.p, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, mf->stream));
        if (mask_out && n_win > 0) DEV_CHECK(hipMemcpyAsync(mask_out, mask.p, (size_t)n_win, hipMemcpyDeviceToHost, mf->stream));
        if (energy_out && !flags_in && n_win > 0) DEV_CHECK(hipMemcpyAsync(energy_out, e.p, (size_t)n_win * sizeof(double), hipMemcpyDeviceToHost, mf->stream));
        DEV_CHECK(hipStreamSynchronize(mf->stream));
        for (int u = 0; u < n_utts; ++u) {
            n_out[u] = h_nout[2 * (size_t)u];
            if (n_voiced_out) n_voiced_out[u] = h_nout[2 * (size_t)u + 1];
        }
        return total;
    }
};

}  // namespace mtts
