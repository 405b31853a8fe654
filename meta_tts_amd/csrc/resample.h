// Rate conversion and volume normalisation of waveform batches on the device, in front of MelFront's packed waveform buffer.
//
// Reference: every loader resamples — `librosa.load(path, sampling_rate)` (preprocessor/libritts.py:37, vctk.py:35,
// preprocessor.py:205) — and every speaker-encoder entry calls resemblyzer's `preprocess_wav` (evaluation/wavs_to_dvector.py:206-296,
// preprocessor.py:265, dataset.py:8): resample to 16 kHz, normalise to -30 dBFS (increase only), webrtcvad trimming.  Neither library
// is vendored; what is built is stated in include/mtts.h: an exact polyphase evaluation of
//     y[n] = sum_m h[n * down - m * up] x[m],   |n * down - m * up| <= H,  0 <= m < n_in,   n_out = ceil(n_in * up / down)
// for a Kaiser-windowed sinc h designed on the host in float64 (meta_tts_amd/audio/resample.py), and
// normalize_volume(wav, target, increase_only): gain = 10^((target - 10 log10(mean(y^2))) / 20).  Silence trimming follows in vad.h.
//
// MI355X layout.  The phase of output n is (n * down) mod up, which has period `up` in n, so the fp32 coefficient bank is stored
// [tap][n mod up]: the 64 lanes of a wavefront, which hold consecutive outputs, read consecutive addresses for every tap (the bank is
// at most a few hundred KB and stays in L2).  Tap t of output n multiplies x[floor(n * down / up) + lead - t]; a workgroup takes `run`
// consecutive outputs of ONE utterance (blockIdx.y = utterance through a small table, as the reflect-pad kernel does) and stages the
// input span they read — run * down / up + taps samples, zeros outside the utterance — in LDS once.  One output per lane per pass,
// taps FMAs in fp32 in tap order: an output depends on its utterance's samples and the bank only, so it is bit-identical alone, in any
// batch, at any position.  `run` is fixed when the bank is loaded (the largest multiple of 256, at most 1024, whose span fits the LDS
// array), never by the batch.  The kernel writes straight into MelFront::wav, the packed buffer every later stage reads.
//
// Sum of squares: every workgroup adds the squares of its outputs in fp64 (per lane in output order, then a fixed tree over the 256
// lanes) into the slot (utterance, workgroup); resample_gain_kernel adds an utterance's slots in slot order, forms the gain in fp64
// and scales in place, rounding the fp64 product once.  No atomics: the gain depends on the utterance and `run` only.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "melfront.h"

namespace mtts {

constexpr int RS_THREADS = 256;
constexpr int RS_SPAN = 4096;      // floats of input one workgroup may stage (16 KB of LDS)
constexpr int RS_MAX_RUN = 1024;   // outputs per workgroup, at most

struct RsUtt {
    int n_in, n_out;     // samples at the source rate, ceil(n_in * up / down)
    int slot0, pad_;     // first sum-of-squares slot of this utterance (one per workgroup: ceil(n_out / run))
    long long src0;      // first sample in the packed source-rate buffer
    long long dst0;      // first output sample in MelFront::wav
};

// dst[dst0 + n] = sum_t bank[t][n mod up] * x[floor(n * down / up) + lead - t]  (x = 0 outside [0, n_in)), and
// partials[slot0 + blockIdx.x] = the fp64 sum of the squares of this workgroup's outputs.  gridDim.x covers the longest utterance of
// the table; a workgroup past its utterance's end stages and writes nothing.
__global__ void resample_polyphase_kernel(const float* src, const RsUtt* utts, const float* bank, int up, int down, int taps, int lead, int run, float* dst,
                                          double* partials) {
    __shared__ float xs[RS_SPAN];
    __shared__ double red[RS_THREADS];
    const RsUtt u = utts[blockIdx.y];
    const int tid = (int)threadIdx.x;
    const long long n0 = (long long)blockIdx.x * run;
    const bool live = n0 < u.n_out;
    const int cnt = !live ? 0 : (u.n_out - n0 < run ? (int)(u.n_out - n0) : run);
    // the lowest input index read is tap taps - 1 of output n0, the highest tap 0 of output n0 + cnt - 1
    const long long m_base = n0 * down / up + lead - (taps - 1);
    const int span = live ? (int)((n0 + cnt - 1) * down / up + lead - m_base) + 1 : 0;   // <= RS_SPAN: `run` was chosen for it
    for (int i = tid; i < span; i += RS_THREADS) {
        const long long m = m_base + i;
        xs[i] = (m >= 0 && m < u.n_in) ? src[u.src0 + m] : 0.f;
    }
    __syncthreads();
    double ss = 0.0;
    for (int i = tid; i < cnt; i += RS_THREADS) {
        const long long n = n0 + i;
        const float* b = bank + (int)(n % up);
        const float* x = xs + (int)(n * down / up + lead - m_base);
        float acc = 0.f;
        for (int t = 0; t < taps; ++t) acc = fmaf(b[(long long)t * up], x[-t], acc);
        dst[u.dst0 + n] = acc;
        ss += (double)acc * (double)acc;
    }
    red[tid] = ss;
    __syncthreads();
    for (int h = RS_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (live && tid == 0) partials[u.slot0 + (int)blockIdx.x] = red[0];
}

// resemblyzer's normalize_volume on the resampled utterances, in place: dBFS = 10 log10(mean(y^2)), change = target - dBFS, left as it
// is when change < 0 and increase_only (and when the utterance is all zeros, where the reference divides by zero), else y *= gain =
// 10^(change / 20) — the fp64 product rounded once.  gains[utterance] = the gain applied (1 where left).  blockIdx.y = utterance.
__global__ void resample_gain_kernel(const RsUtt* utts, const double* partials, int run, double target_dbfs, int increase_only, float* dst, double* gains) {
    __shared__ double g_s;
    const RsUtt u = utts[blockIdx.y];
    if (threadIdx.x == 0) {
        const int slots = (u.n_out + run - 1) / run;
        double ss = 0.0;
        for (int s = 0; s < slots; ++s) ss += partials[u.slot0 + s];
        double g = 1.0;
        if (ss > 0.0) {
            const double change = target_dbfs - 10.0 * log10(ss / (double)u.n_out);
            if (!(change < 0.0 && increase_only)) g = pow(10.0, change / 20.0);
        }
        g_s = g;
        if (blockIdx.x == 0) gains[blockIdx.y] = g;
    }
    __syncthreads();
    const double g = g_s;
    if (g == 1.0) return;
    float* y = dst + u.dst0;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < u.n_out; i += (long long)gridDim.x * blockDim.x) y[i] = (float)((double)y[i] * g);
}

class Resample {
public:
    MelFront* mf = nullptr;
    int up = 0, down = 0, taps = 0, lead = 0, run = 0;   // up == 0: no resampler loaded
    float* bank = nullptr;                                // [taps][up]
    DevBuf<float> src;                                    // the source-rate samples of a call (or of a chunk of one)
    DevBuf<double> partials, gains;
    DevBuf<RsUtt> utts;
    std::vector<RsUtt> h_utts;
    int n_slots = 0, max_out = 0;
    long long n_src = 0;

    int err(const std::string& s) { return mf->err(s); }
    bool loaded() const { return up > 0; }
    long long out_len(long long n_in) const { return (n_in * up + down - 1) / down; }

    // bank_host [taps][up]: bank_host[t][p] = h[((p * down) mod up) + (t - lead) * up + H], zero outside the filter
    int load(int up_, int down_, int taps_, int lead_, const float* bank_host) {
        const char* who = "mtts_stft_load_resampler: ";
        if (up_ < 1 || down_ < 1 || taps_ < 1 || lead_ < 0 || lead_ >= taps_ || !bank_host) return err(std::string(who) + "bad arguments (need up, down, taps >= 1, 0 <= lead < taps, a bank)");
        if ((long long)taps_ * up_ > (1LL << 22)) return err(std::string(who) + "coefficient bank larger than 16 MB");
        // the span of `run` outputs: floor((run - 1) * down / up) + taps input samples, + 1 for where floor() falls
        int r = RS_MAX_RUN;
        while (r >= RS_THREADS && (long long)(r - 1) * down_ / up_ + taps_ + 1 > RS_SPAN) r -= RS_THREADS;
        if (r < RS_THREADS) return err(std::string(who) + "ratio " + std::to_string(up_) + " / " + std::to_string(down_) + " with " + std::to_string(taps_) +
                                       " taps: the input span of 256 outputs exceeds the " + std::to_string(RS_SPAN) + " samples a workgroup stages");
        hipStreamSynchronize(mf->stream);   // (a bank still in use by an earlier call)
        up = 0;
        DEV_CHECK(mf->mem.alloc(bank, (size_t)taps_ * up_ * sizeof(float)));
        DEV_CHECK(hipMemcpy(bank, bank_host, (size_t)taps_ * up_ * sizeof(float), hipMemcpyHostToDevice));
        up = up_; down = down_; taps = taps_; lead = lead_; run = r;
        return 0;
    }

    // ---- the table of a launch: host only --------------------------------------------------------------------------------------------
    void table_begin() { h_utts.clear(); n_slots = 0; max_out = 0; n_src = 0; }
    void table_add(int n_in, long long dst0) {
        const int n_out = (int)out_len(n_in);
        h_utts.push_back(RsUtt{n_in, n_out, n_slots, 0, n_src, dst0});
        n_slots += (n_out + run - 1) / run;
        max_out = std::max(max_out, n_out);
        n_src += n_in;
    }
    // room for a launch of at most n_src_ source samples, n_slots_ slots and n_utts_ utterances
    int reserve(long long n_src_, long long n_slots_, size_t n_utts_) {
        return mf->grow(src, (size_t)n_src_ + 64, "source-rate waveforms") || mf->grow(partials, (size_t)n_slots_, "sum-of-squares slots") ||
               mf->grow(gains, n_utts_, "gains") || mf->grow(utts, n_utts_, "resampler utterances") ? -1 : 0;
    }
    // The tabled utterances, packed in src_host, -> mf->wav at their dst0 (the caller has sized mf->wav), then the gain.  Asynchronous on
    // mf->stream; h_utts and src_host must stay as they are until the stream has been synchronised.  dst: another buffer than mf->wav
    // (vad.h's staging buffer, when silence trimming follows and fills mf->wav itself).
    int launch(const float* src_host, double target_dbfs, bool increase_only, float* dst = nullptr) {
        DEV_CHECK(hipMemcpyAsync(src.p, src_host, (size_t)n_src * sizeof(float), hipMemcpyHostToDevice, mf->stream));
        return convert(target_dbfs, increase_only, dst);
    }
    // the same for source-rate samples an earlier launch on mf->stream has left in `src` at the table's src0 (wavsource.h): no upload
    int convert(double target_dbfs, bool increase_only, float* dst = nullptr) {
        if (!dst) dst = mf->wav.p;
        DEV_CHECK(hipMemcpyAsync(utts.p, h_utts.data(), h_utts.size() * sizeof(RsUtt), hipMemcpyHostToDevice, mf->stream));
        const unsigned n_utts = (unsigned)h_utts.size();
        MTTS_LAUNCH(resample_polyphase_kernel, dim3((unsigned)((max_out + run - 1) / run), n_utts), dim3(RS_THREADS), mf->stream, (const float*)src.p,
                    (const RsUtt*)utts.p, (const float*)bank, up, down, taps, lead, run, dst, partials.p);
        if (!std::isnan(target_dbfs))
            MTTS_LAUNCH(resample_gain_kernel, dim3((unsigned)std::min((max_out + 1023) / 1024, 64), n_utts), dim3(256), mf->stream, (const RsUtt*)utts.p,
                        (const double*)partials.p, run, target_dbfs, increase_only ? 1 : 0, dst, gains.p);
        return 0;
    }

    // what both entries refuse before any launch (out_len(n_in) < 1 exactly when n_in < 1); checks: MelFront::UTT_GRID where the
    // whole call is one launch
    int check_lengths(const std::string& who, int n_utts, const int* n_in, int checks = 0) {
        if (!loaded()) return err(who + "no resampler loaded (mtts_stft_load_resampler)");
        return mf->check_utterances(who, n_utts, [&](int u) { return out_len(n_in[u]); }, checks | MelFront::UTT_CAP, true);
    }

    // host in, host out: wavs = the utterances one after another (n_in[u] samples each), out = the resampled ones one after another
    int resample_batch(int n_utts, const int* n_in, const float* wavs, double target_dbfs, int increase_only, float* out, double* gains_out) {
        const char* who = "mtts_stft_resample_batch: ";
        if (n_utts < 1 || !n_in || !wavs || !out) return err(std::string(who) + "bad arguments (n_utts < 1 or NULL pointer)");
        if (check_lengths(who, n_utts, n_in, MelFront::UTT_GRID)) return -1;
        table_begin();
        long long total = 0;
        for (int u = 0; u < n_utts; ++u) { table_add(n_in[u], total); total += out_len(n_in[u]); }
        if (total > (1LL << 31) - 1 || n_src > (1LL << 31) - 1) return err(std::string(who) + "too many samples in one call");
        if (mf->grow(mf->wav, (size_t)total + 64, "waveforms") || reserve(n_src, n_slots, (size_t)n_utts)) return -1;
        if (launch(wavs, target_dbfs, increase_only != 0) || mf->check_launch()) return -1;
        DEV_CHECK(hipMemcpyAsync(out, mf->wav.p, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, mf->stream));
        if (gains_out && !std::isnan(target_dbfs)) DEV_CHECK(hipMemcpyAsync(gains_out, gains.p, (size_t)n_utts * sizeof(double), hipMemcpyDeviceToHost, mf->stream));
        DEV_CHECK(hipStreamSynchronize(mf->stream));
        if (gains_out && std::isnan(target_dbfs)) std::fill(gains_out, gains_out + n_utts, 1.0);
        return 0;
    }
};

}  // namespace mtts
