// Speaker-similarity evaluation on the device: 16 kHz waveforms -> speaker-encoder mels -> partial utterances -> d-vectors, and the
// scoring of those d-vectors (indexed cosine similarity, speaker centroids).
//
// Reference: evaluation/wavs_to_dvector.py:202-209,216-301 (`encoder.embed_utterance(preprocess_wav(path))`, one wav at a time on the
// CPU), :176-183 (centroids), evaluation/pair_similarity.py:68-88 and centroid_similarity.py:47-118 (nn.CosineSimilarity(dim=1,
// eps=1e-6) over np.repeat-expanded copies), preprocessor/preprocessor.py:263-299 (`spk_ref_mel_slices`).  The un-vendored
// resemblyzer behind them is restated from its published recipe: `wav_to_mel_spectrogram` = librosa.feature.melspectrogram(wav, 16000,
// n_fft=400, hop_length=160, n_mels=40).T — centred frames over the reflect-padded signal, POWER spectrum re^2 + im^2, mel
// projection, no log, no clamp — and `compute_partial_slices`: 160-frame windows every frame_step = round(16000 / rate / 160) frames
// over ceil((n + 1) / 160) frames, the last one dropped when it covers less than min_coverage of its span and is not the only one,
// the waveform zero-extended to the end of the last window kept.  Of `preprocess_wav`, resampling and -30 dBFS normalisation are
// resample.h's (embed_wavs with a Resample: the chained entry) and silence trimming is vad.h's (embed_wavs with a Vad: all of
// `preprocess_wav` chained; the detector is this project's, parity with webrtcvad is UNPINNED).  Without either, inputs are 16 kHz
// waveforms as they are.
//
// MI355X layout.  All utterances of a chunk share every launch (melfront.h's packing): the reflect-pad kernel, ONE forward-STFT GEMM
// with the rows between utterances dropped, stft_power_kernel (one wavefront per frame, HBM-bound: 2F floats in, F out), the mel GEMM,
// and spk_gather_kernel, which copies the windows of every utterance from the packed mel [sum T][n_mel] into the encoder's partial
// stack [N][frames][n_mel] — a window is ONE contiguous span of frames * n_mel floats of the packed mel, so the gather is float4
// copies of 25.6 KB spans, never leaving HBM — then DVector::forward on that stack.  Every GEMM names its kernel (64x64 tile, no
// split-K, no size-dependent choice), so the mel rows, the slices and the d-vector of an utterance do not depend on what else is in
// the call nor on how the call was cut into chunks (a chunk = consecutive utterances whose partials fit the encoder's max_partials).
// No host synchronisation stands between the chunks of a call: every chunk keeps packing tables of its own on the host until the
// call's final synchronise, and the partial stack is sized once, for the largest chunk, before the first launch — so the host packs
// chunk k + 1 while the device works on chunk k (only a chunk that outgrows MelFront's workspace waits, inside MelFront::grow).  With
// the two handles on different streams the stages are ordered by events, and the front-end kernels of chunk k + 1 also overlap the
// recurrence of chunk k.
//
// Scoring: spk_cosine_kernel (one wavefront per pair, operands picked through index arrays, so the reference's np.repeat expansions
// are never materialised) and spk_centroid_kernel (one workgroup per speaker over its ragged list).  Both accumulate in fp64 in a
// fixed order and round once: deterministic (no atomics), and within half an ulp of the float64 result.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "dvector.h"
#include "melfront.h"
#include "resample.h"
#include "vad.h"

namespace mtts {

// spec: [T][ld_spec] = [re(0..F) | im(0..F)] per frame  ->  pw [T][ld_pw] = re^2 + im^2 (columns >= F zeroed: the mel GEMM's K padding)
__global__ void stft_power_kernel(const float* spec, int ld_spec, int T, int F, float* pw, int ld_pw) {
    const int row = blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    if (row >= T) return;
    const float* p = spec + (long long)row * ld_spec;
    float* o = pw + (long long)row * ld_pw;
    for (int f = lane; f < ld_pw; f += 64) {
        float v = 0.f;
        if (f < F) {
            const float re = p[f], im = p[F + f];
            v = re * re + im * im;
        }
        o[f] = v;
    }
}

// stack[p][0 .. span4) = mel[win_row[p] * n_mel / 4 + (0 .. span4)] as float4 (span4 = frames * n_mel / 4; n_mel % 4 == 0, so every
// window starts on a 16-byte boundary).  `per` consecutive workgroups share one partial utterance (gridDim.x = N * per: the partial
// count of a front-end-only call is not bounded by the 65535 of gridDim.y).
__global__ void spk_gather_kernel(const float* mel, const int* win_row, int n_mel, int span4, int per, float* stack) {
    const int p = (int)(blockIdx.x / (unsigned)per), b = (int)(blockIdx.x % (unsigned)per);
    const float* src = mel + (long long)win_row[p] * n_mel;
    float* dst = stack + (long long)p * span4 * 4;
    for (int i = b * (int)blockDim.x + (int)threadIdx.x; i < span4; i += per * (int)blockDim.x) st4(dst + 4LL * i, ld4(src + 4LL * i));
}

// sim[i] = cos(A[ia[i]], B[ib[i]]) = <a, b> / (max(||a||, eps) * max(||b||, eps))   (nn.CosineSimilarity(dim=1, eps)); one wavefront
// per i, fp64 accumulation, the 64 lane partials added in lane order.
__global__ void spk_cosine_kernel(const float* A, const float* B, const int* ia, const int* ib, int n, int dim, double eps, float* sim) {
    __shared__ double red[3][256];
    const int tid = (int)threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int i = blockIdx.x * 4 + w;
    double dot = 0.0, na = 0.0, nb = 0.0;
    if (i < n) {
        const float* a = A + (long long)ia[i] * dim;
        const float* b = B + (long long)ib[i] * dim;
        for (int k = lane; k < dim; k += 64) {
            const double x = (double)a[k], y = (double)b[k];
            dot += x * y; na += x * x; nb += y * y;
        }
    }
    red[0][tid] = dot; red[1][tid] = na; red[2][tid] = nb;
    __syncthreads();
    if (lane == 0 && i < n) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int k = 0; k < 64; ++k) { s0 += red[0][w * 64 + k]; s1 += red[1][w * 64 + k]; s2 += red[2][w * 64 + k]; }
        const double x = sqrt(s1), y = sqrt(s2);
        sim[i] = (float)(s0 / ((x > eps ? x : eps) * (y > eps ? y : eps)));
    }
}

// centroid[s] = m / ||m||_2, m = mean of vecs[off[s] .. off[s + 1])   (wavs_to_dvector.py:180-181; an empty list gives NaN, as np.mean
// does).  One workgroup of 256 threads per speaker, dim <= 1024; the rows are added in list order, the squares by a fixed tree.
__global__ void spk_centroid_kernel(const float* vecs, const int* off, int dim, float* out) {
    __shared__ double m_s[1024];
    __shared__ double red[256];
    const int s = blockIdx.x, tid = (int)threadIdx.x;
    const int lo = off[s], hi = off[s + 1];
    double ss = 0.0;
    for (int j = tid; j < dim; j += 256) {
        double m = 0.0;
        for (int r = lo; r < hi; ++r) m += (double)vecs[(long long)r * dim + j];
        m /= (double)(hi - lo);
        m_s[j] = m;
        ss += m * m;
    }
    red[tid] = ss;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    const double nrm = sqrt(red[0]);
    for (int j = tid; j < dim; j += 256) out[(long long)s * dim + j] = (float)(m_s[j] / nrm);
}

// resemblyzer's compute_partial_slices for one utterance of n samples: the number of windows kept, and through n_ext the length the
// waveform is zero-extended to (preprocessor.py:272-274).  Window p covers mel frames [p * step, p * step + frames).
inline int spk_partial_count(long long n, int hop, int frames, int step, double min_coverage, long long* n_ext) {
    const long long n_frames = (n + 1 + hop - 1) / hop;                                  // ceil((n + 1) / samples_per_frame)
    const long long steps = std::max<long long>(1, n_frames - frames + step + 1);
    long long cnt = (steps + step - 1) / step;                                           // len(range(0, steps, step))
    const double coverage = (double)(n - (cnt - 1) * step * hop) / (double)((long long)frames * hop);
    if (coverage < min_coverage && cnt > 1) --cnt;
    if (n_ext) *n_ext = std::max(n, ((cnt - 1) * step + frames) * (long long)hop);
    return (int)std::min<long long>(cnt, 0x7fffffff);
}

class SpeakerEval {
public:
    MelFront* mf = nullptr;
    int device = 0;
    DevBuf<float> stack;    // [N][frames][n_mel]: the partial utterances of a chunk
    DevBuf<int> win;        // first packed mel row of every partial
    hipEvent_t ev_front = nullptr, ev_enc = nullptr;
    std::vector<float> h_wav;                  // the call's waveforms, zero-extended
    std::vector<long long> h_ext;
    std::vector<int> h_cnt;
    std::vector<std::vector<int>> h_win, h_off;   // per chunk (alive until the call's last copy has been enqueued and waited for)
    std::vector<std::vector<StftUtt>> keep_utts;  // MelFront's packing tables of the chunks already enqueued, kept for the same reason
    std::vector<std::vector<int>> keep_maps;
    std::vector<std::vector<RsUtt>> keep_rs;      // and the resampler's tables (embed_wavs with a resampler)
    std::vector<std::vector<VadUtt>> keep_vad;    // and the trimmer's (embed_wavs with a Vad)
    std::vector<long long> h_n;                   // samples per utterance at the front-end's rate
    struct Chunk { int u0, u1, N; };
    std::vector<Chunk> chunks;

    int err(const std::string& s) { return mf->err(s); }

    // Speaker-encoder mel of the staged call into mf->mel [sum T][n_mel]: forward STFT, power, mel projection (no log, no clamp).
    void power_mel() {
        const long long T = mf->n_frames;
        mf->forward_stft(mf->xp_rows, mf->rowmap, 64);
        MTTS_LAUNCH(stft_power_kernel, dim3((unsigned)((T + 3) / 4)), dim3(256), mf->stream, (const float*)mf->spec, mf->ld_spec, (int)T, mf->F, mf->mag.p,
                    mf->ld_mag);
        GemmArgs g;
        g.A = mf->mag; g.lda = mf->ld_mag; g.B = mf->melb; g.ldb = mf->ld_mag; g.C = mf->mel; g.ldc = mf->n_mel;
        g.M = (int)T; g.N = mf->n_mel; g.K = mf->ld_mag;
        gemm_launch(mf->gx, GEMM_NT, g, (int)T, mf->n_mel, 1, mf->stream, 64, 2.0 * T * (double)mf->n_mel * mf->F, 0);
    }

    // wav_to_mel_spectrogram of n_utts waveforms as they are (no zero-extension): mel_host [sum T][n_mel], T_u = n_u / hop + 1
    int power_mel_batch(int n_utts, const int* n_samples, const float* wavs, float* mel_host) {
        const char* who = "mtts_stft_power_mel_batch: ";
        if (!mf->have_basis || !mf->have_mel) return err(std::string(who) + "STFT bases not loaded");
        if (n_utts < 1 || !n_samples || !wavs || !mel_host) return err(std::string(who) + "bad arguments (n_utts < 1 or NULL pointer)");
        if (n_utts > 65535) return err(std::string(who) + "more than 65535 utterances in one call");
        for (int u = 0; u < n_utts; ++u)
            if (n_samples[u] <= mf->n_fft / 2)
                return err(std::string(who) + "utterance " + std::to_string(u) + ": waveform too short for the reflection padding (need n_samples > filter_length / 2 = " +
                           std::to_string(mf->n_fft / 2) + ")");
        mf->pack_begin();
        for (int u = 0; u < n_utts; ++u) mf->pack_add(n_samples[u], mf->frames_of(n_samples[u]));
        if (mf->stage("mtts_stft_power_mel_batch", true) || mf->pad_waveforms(wavs, false, true)) return -1;
        power_mel();
        if (mf->check_launch()) return -1;
        DEV_CHECK(hipMemcpyAsync(mel_host, mf->mel, (size_t)mf->n_frames * mf->n_mel * sizeof(float), hipMemcpyDeviceToHost, mf->stream));
        DEV_CHECK(hipStreamSynchronize(mf->stream));
        return 0;
    }

    // dv != nullptr: out [n_utts][E] d-vectors.  slices_out != nullptr: the partial stacks [sum N][frames][n_mel] (all utterances one
    // after another).  n_partials_out [n_utts].  Everything that can be refused is refused before the first launch.
    // rs != nullptr (mtts_dvector_embed_wavs_resampled): n_samples counts SOURCE-rate samples; every chunk is resampled (and normalised
    // to target_dbfs unless that is NaN) by rs straight into mf->wav, zero-extended there, and the front-end rate's signal never
    // visits the host.  The chunking, the launches behind the waveform buffer and the results are those of the plain entry on the
    // resampled waveforms.
    // vad != nullptr (mtts_dvector_embed_wavs_preprocessed): every chunk's waveforms go (through rs when given, else as they are) into
    // vad's staging buffer, are trimmed there, and the kept windows are compacted into mf->wav over zeros.  Chunks and capacities are
    // planned from the untrimmed lengths (trimming only shortens, and the partial count never grows as a waveform shrinks); the partial
    // rule then applies to the trimmed lengths, which the host reads back once per chunk (Vad::detect).  n_trimmed_out (or nullptr):
    // the trimmed lengths.  slices_out holds the partials of the trimmed utterances one after another.
    int embed_wavs(DVector* dv, int dv_device, int n_utts, const int* n_samples, const float* wavs, int frames, int step, double min_coverage, float* out,
                   int* n_partials_out, float* slices_out, Resample* rs = nullptr, double target_dbfs = 0.0, int increase_only = 0, Vad* vad = nullptr,
                   int* n_trimmed_out = nullptr) {
        const char* who = vad ? "mtts_dvector_embed_wavs_preprocessed: " : rs ? "mtts_dvector_embed_wavs_resampled: " : "mtts_dvector_embed_wavs: ";
        const int hop = mf->hop, n_mel = mf->n_mel;
        if (!mf->have_basis || !mf->have_mel) return err(std::string(who) + "STFT bases not loaded");
        if (n_utts < 1 || !n_samples || !wavs || !n_partials_out) return err(std::string(who) + "bad arguments (n_utts < 1 or NULL n_samples / wavs / n_partials_out)");
        if (dv ? !out : !slices_out) return err(std::string(who) + "NULL output (out with an encoder, slices_out without one)");
        if (frames < 1 || step < 1 || step > frames || !(min_coverage > 0.0 && min_coverage <= 1.0))
            return err(std::string(who) + "bad partial rule (need 1 <= frame_step <= partial_frames, 0 < min_coverage <= 1)");
        if (n_mel & 3) return err(std::string(who) + "n_mel % 4 != 0");
        if (dv) {
            if (dv_device != device) return err(std::string(who) + "the encoder and the STFT handle are on different devices");
            if (dv->n_mels != n_mel || dv->T != frames)
                return err(std::string(who) + "the encoder expects partials of " + std::to_string(dv->T) + " x " + std::to_string(dv->n_mels) + ", the front-end makes " +
                           std::to_string(frames) + " x " + std::to_string(n_mel));
        }
        if (rs && rs->check_lengths(who, n_utts, n_samples)) return -1;
        h_ext.resize((size_t)n_utts);
        h_cnt.resize((size_t)n_utts);
        h_n.resize((size_t)n_utts);
        if (vad) {
            if (!rs && !std::isnan(target_dbfs))
                return err(std::string(who) + "volume normalisation needs a resampler (mtts_stft_load_resampler; the identity bank for waveforms at the front-end's rate)");
            for (int u = 0; u < n_utts; ++u) h_n[(size_t)u] = rs ? rs->out_len(n_samples[u]) : n_samples[u];
            if (vad->check_lengths(who, n_utts, h_n.data())) return -1;
            if (vad->c.W <= mf->n_fft / 2)
                return err(std::string(who) + "a VAD window of " + std::to_string(vad->c.W) + " samples is too short for the reflection padding (need more than filter_length / 2 = " +
                           std::to_string(mf->n_fft / 2) + ")");
        }
        long long total = 0, total_parts = 0;
        for (int u = 0; u < n_utts; ++u) {
            const std::string utt = std::string(who) + "utterance " + std::to_string(u) + ": ";
            const long long n = h_n[(size_t)u] = rs ? rs->out_len(n_samples[u]) : n_samples[u];
            if (n <= mf->n_fft / 2)
                return err(utt + "waveform too short for the reflection padding (need n_samples > filter_length / 2 = " + std::to_string(mf->n_fft / 2) + ")");
            h_cnt[(size_t)u] = spk_partial_count(n, hop, frames, step, min_coverage, &h_ext[(size_t)u]);
            if (dv && h_cnt[(size_t)u] > dv->cap_N)
                return err(utt + std::to_string(h_cnt[(size_t)u]) + " partial utterances exceed the encoder's max_partials = " + std::to_string(dv->cap_N));
            if (h_ext[(size_t)u] > 0x7fffffffLL - hop) return err(utt + "too long");
            total += h_ext[(size_t)u];
            total_parts += h_cnt[(size_t)u];
        }
        if (total_parts > (1LL << 30) / ((long long)frames * n_mel)) return err(std::string(who) + "too many partial utterances in one call");
        if (dv && dv->dirty && dv->refresh() != 0) return err(std::string(who) + dv->last_error);
        const bool two_streams = dv && dv->stream != mf->stream;
        if (two_streams) { DEV_CHECK(mf->mem.event(ev_front)); DEV_CHECK(mf->mem.event(ev_enc)); }
        if (!rs && !vad) {
            h_wav.assign((size_t)total, 0.f);
            long long src = 0, dst = 0;
            for (int u = 0; u < n_utts; ++u) {
                std::copy(wavs + src, wavs + src + n_samples[u], h_wav.begin() + dst);
                src += n_samples[u];
                dst += h_ext[(size_t)u];
            }
        }
        for (int u = 0; u < n_utts; ++u) n_partials_out[u] = h_cnt[(size_t)u];
        h_win.clear();
        h_off.clear();
        keep_utts.clear();
        keep_maps.clear();
        keep_rs.clear();
        keep_vad.clear();
        chunks.clear();
        int max_N = 0;
        for (int u0 = 0; u0 < n_utts;) {   // a chunk: consecutive utterances within the encoder's capacity (front-end only: the whole call)
            int u1 = u0, N = 0;
            while (u1 < n_utts && u1 - u0 < 65535 && (!dv || (N + h_cnt[(size_t)u1] <= dv->cap_N && u1 - u0 < dv->cap_B))) N += h_cnt[(size_t)u1++];   // (65535: the pad kernel's gridDim.y)
            chunks.push_back(Chunk{u0, u1, N});
            max_N = std::max(max_N, N);
            u0 = u1;
        }
        const int span4 = frames * n_mel / 4, per = std::min((span4 + 255) / 256, 8);
        // sized once for the largest chunk, before the first launch: a later, larger chunk must not free the stack the previous chunk's
        // encoder still reads on the other stream
        if (mf->grow(stack, (size_t)max_N * span4 * 4 + 64, "partial utterances") || mf->grow(win, (size_t)max_N, "windows")) return -1;
        if (rs) {   // the same for the resampler's buffers: the largest chunk's source samples, slots and utterances
            long long max_src = 0, max_slots = 0;
            size_t max_utts = 0;
            for (const Chunk& c : chunks) {
                long long n_src = 0, slots = 0;
                for (int u = c.u0; u < c.u1; ++u) { n_src += n_samples[u]; slots += (h_n[(size_t)u] + rs->run - 1) / rs->run; }
                max_src = std::max(max_src, n_src);
                max_slots = std::max(max_slots, slots);
                max_utts = std::max(max_utts, (size_t)(c.u1 - c.u0));
            }
            if (max_src > (1LL << 31) - 1) return err(std::string(who) + "too many samples in one chunk");
            if (rs->reserve(max_src, max_slots, max_utts)) return -1;
        }
        if (vad) {   // and for the trimmer's: the largest chunk's untrimmed samples, windows and utterances
            long long max_n = 0, max_win = 0;
            size_t max_utts = 0;
            for (const Chunk& c : chunks) {
                long long n = 0, nw = 0;
                for (int u = c.u0; u < c.u1; ++u) { n += h_n[(size_t)u]; nw += h_n[(size_t)u] / vad->c.W; }
                max_n = std::max(max_n, n);
                max_win = std::max(max_win, nw);
                max_utts = std::max(max_utts, (size_t)(c.u1 - c.u0));
            }
            if (max_n > (1LL << 31) - 1) return err(std::string(who) + "too many samples in one chunk");
            if (vad->reserve(max_n, max_win, max_utts, false)) return -1;
        }
        long long wav0 = 0, src0 = 0, part0 = 0;
        for (size_t c = 0; c < chunks.size(); ++c) {
            const int u0 = chunks[c].u0, u1 = chunks[c].u1;
            int N = chunks[c].N;
            if (vad) {   // untrimmed waveforms into the staging buffer, the mask, and the trimmed lengths back: the partial rule is theirs
                vad->table_begin();
                for (int u = u0; u < u1; ++u) vad->table_add(h_n[(size_t)u]);
                if (rs) {
                    rs->table_begin();
                    for (int u = u0; u < u1; ++u) rs->table_add(n_samples[u], vad->h_utts[(size_t)(u - u0)].src0);
                    if (rs->launch(wavs + src0, target_dbfs, increase_only != 0, vad->stage.p)) return -1;
                    src0 += rs->n_src;
                } else {
                    DEV_CHECK(hipMemcpyAsync(vad->stage.p, wavs + src0, (size_t)vad->n_src * sizeof(float), hipMemcpyHostToDevice, mf->stream));
                    src0 += vad->n_src;
                }
                if (vad->detect(nullptr)) return -1;   // (synchronises mf->stream: the resampler's table is free again)
                N = 0;
                for (int u = u0; u < u1; ++u) {
                    const int n = vad->h_nout[2 * (size_t)(u - u0)];
                    n_partials_out[u] = h_cnt[(size_t)u] = spk_partial_count(n, hop, frames, step, min_coverage, &h_ext[(size_t)u]);
                    if (n_trimmed_out) n_trimmed_out[u] = n;
                    N += h_cnt[(size_t)u];
                }
            }
            mf->pack_begin();
            for (int u = u0; u < u1; ++u) mf->pack_add(h_ext[(size_t)u], mf->frames_of((int)h_ext[(size_t)u]));
            if (mf->stage("mtts_dvector_embed_wavs", true)) return -1;
            if (vad) {   // the kept windows into mf->wav over zeros (the zero-extension to the last partial window's end)
                DEV_CHECK(hipMemsetAsync(mf->wav.p, 0, (size_t)mf->n_samples * sizeof(float), mf->stream));
                for (int u = u0; u < u1; ++u) vad->h_utts[(size_t)(u - u0)].dst0 = mf->h_utts[(size_t)(u - u0)].wav0;
                if (vad->compact(mf->wav.p) || mf->pad_staged(false, true)) return -1;
                keep_vad.emplace_back(std::move(vad->h_utts));
                vad->h_utts.clear();
            } else if (rs) {   // source-rate samples up, resampled into mf->wav over zeros (the zero-extension to the last window's end)
                DEV_CHECK(hipMemsetAsync(mf->wav.p, 0, (size_t)mf->n_samples * sizeof(float), mf->stream));
                rs->table_begin();
                for (int u = u0; u < u1; ++u) rs->table_add(n_samples[u], mf->h_utts[(size_t)(u - u0)].wav0);
                if (rs->launch(wavs + src0, target_dbfs, increase_only != 0) || mf->pad_staged(false, true)) return -1;
                keep_rs.emplace_back(std::move(rs->h_utts));
                rs->h_utts.clear();
                src0 += rs->n_src;
            } else if (mf->pad_waveforms(h_wav.data() + wav0, false, true)) return -1;
            power_mel();
            h_win.emplace_back();
            h_off.emplace_back(1, 0);
            std::vector<int>& wv = h_win.back();
            std::vector<int>& off = h_off.back();
            for (int u = u0; u < u1; ++u) {
                const StftUtt& q = mf->h_utts[(size_t)(u - u0)];
                for (int p = 0; p < h_cnt[(size_t)u]; ++p) {
                    if (p * step + frames > q.T) return err(std::string(who) + "internal: a window ends past its utterance's frames");
                    wv.push_back(q.frame0 + p * step);
                }
                off.push_back((int)wv.size());
            }
            // the tables stage() has just enqueued for upload stay alive (a moved vector keeps its storage); MelFront packs the next chunk into fresh ones
            keep_utts.emplace_back(std::move(mf->h_utts));
            keep_maps.emplace_back(std::move(mf->h_rowmap));
            mf->h_utts.clear();
            mf->h_rowmap.clear();
            DEV_CHECK(hipMemcpyAsync(win.p, wv.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, mf->stream));
            if (two_streams && c > 0) DEV_CHECK(hipStreamWaitEvent(mf->stream, ev_enc, 0));   // the previous chunk's encoder still reads the stack
            MTTS_LAUNCH(spk_gather_kernel, dim3((unsigned)N * (unsigned)per), dim3(256), mf->stream, (const float*)mf->mel, (const int*)win.p, n_mel, span4, per,
                        stack.p);
            if (mf->check_launch()) return -1;
            if (slices_out)
                DEV_CHECK(hipMemcpyAsync(slices_out + part0 * span4 * 4, stack.p, (size_t)N * span4 * 4 * sizeof(float), hipMemcpyDeviceToHost, mf->stream));
            if (dv) {
                if (two_streams) { DEV_CHECK(hipEventRecord(ev_front, mf->stream)); DEV_CHECK(hipStreamWaitEvent(dv->stream, ev_front, 0)); }
                if (dv->forward_device(stack.p, N, off.data(), u1 - u0, out + (long long)u0 * dv->E, nullptr, false) != 0) return err(std::string(who) + dv->last_error);
                if (two_streams) DEV_CHECK(hipEventRecord(ev_enc, dv->stream));
            }
            for (int u = u0; u < u1; ++u) wav0 += h_ext[(size_t)u];
            part0 += N;
        }
        if (dv) DEV_CHECK(hipStreamSynchronize(dv->stream));
        DEV_CHECK(hipStreamSynchronize(mf->stream));
        return 0;
    }
};

// Scoring on an mtts_dvector handle's stream: host arrays in and out, grow-on-demand device scratch.
class SpeakerScore {
public:
    DevBuf<float> a, b, o;
    DevBuf<int> ia, ib;
    DVector* dv = nullptr;   // the handle it scores on: its stream, its heap, its error string

    int err(const std::string& s) { return dv->err(s); }
    template <class T>
    int grow(DevBuf<T>& buf, size_t need) { return mtts::grow(dv->mem, buf, need, dv->stream, "scoring workspace", dv->last_error); }

    int cosine_indexed(const float* A, int n_a, const float* B, int n_b, int dim, int n, const int* idx_a, const int* idx_b, double eps, float* sim) {
        const char* who = "mtts_dvector_cosine_indexed: ";
        if (!A || !B || !idx_a || !idx_b || !sim || n_a < 1 || n_b < 1 || dim < 1 || n < 1) return err(std::string(who) + "bad arguments (NULL pointer or a count < 1)");
        for (int i = 0; i < n; ++i)
            if (idx_a[i] < 0 || idx_a[i] >= n_a || idx_b[i] < 0 || idx_b[i] >= n_b) return err(std::string(who) + "pair " + std::to_string(i) + ": index out of range");
        if (grow(a, (size_t)n_a * dim) || grow(b, (size_t)n_b * dim) || grow(o, (size_t)n) || grow(ia, (size_t)n) || grow(ib, (size_t)n)) return -1;
        hipStream_t st = dv->stream;
        DEV_CHECK(hipMemcpyAsync(a.p, A, (size_t)n_a * dim * sizeof(float), hipMemcpyHostToDevice, st));
        DEV_CHECK(hipMemcpyAsync(b.p, B, (size_t)n_b * dim * sizeof(float), hipMemcpyHostToDevice, st));
        DEV_CHECK(hipMemcpyAsync(ia.p, idx_a, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
        DEV_CHECK(hipMemcpyAsync(ib.p, idx_b, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
        MTTS_LAUNCH(spk_cosine_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), st, (const float*)a.p, (const float*)b.p, (const int*)ia.p, (const int*)ib.p, n, dim,
                    eps, o.p);
        DEV_CHECK(hipGetLastError());
        DEV_CHECK(hipMemcpyAsync(sim, o.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, st));
        DEV_CHECK(hipStreamSynchronize(st));
        return 0;
    }

    int centroids(const float* vecs, const int* offsets, int n_spk, int dim, float* out) {
        const char* who = "mtts_dvector_centroids: ";
        if (!vecs || !offsets || !out || n_spk < 1 || dim < 1 || dim > 1024) return err(std::string(who) + "bad arguments (NULL pointer, n_speakers < 1 or dim outside 1 .. 1024)");
        if (offsets[0] != 0) return err(std::string(who) + "offsets must start at 0");
        for (int s = 0; s < n_spk; ++s)
            if (offsets[s + 1] < offsets[s]) return err(std::string(who) + "speaker " + std::to_string(s) + ": offsets must not decrease");
        const size_t rows = (size_t)offsets[n_spk];
        if (grow(a, std::max(rows, (size_t)1) * dim) || grow(o, (size_t)n_spk * dim) || grow(ia, (size_t)n_spk + 1)) return -1;
        hipStream_t st = dv->stream;
        DEV_CHECK(hipMemcpyAsync(a.p, vecs, rows * dim * sizeof(float), hipMemcpyHostToDevice, st));
        DEV_CHECK(hipMemcpyAsync(ia.p, offsets, ((size_t)n_spk + 1) * sizeof(int), hipMemcpyHostToDevice, st));
        MTTS_LAUNCH(spk_centroid_kernel, dim3((unsigned)n_spk), dim3(256), st, (const float*)a.p, (const int*)ia.p, dim, o.p);
        DEV_CHECK(hipGetLastError());
        DEV_CHECK(hipMemcpyAsync(out, o.p, (size_t)n_spk * dim * sizeof(float), hipMemcpyDeviceToHost, st));
        DEV_CHECK(hipStreamSynchronize(st));
        return 0;
    }
};

}  // namespace mtts
