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
// resample.h's and silence trimming is vad.h's (the detector is this project's, parity with webrtcvad is UNPINNED).  Without either,
// inputs are 16 kHz waveforms as they are.
//
// embed_wavs is one function behind three entries, in three parts.  The plan: validate, cut the call into chunks, reserve every
// buffer for the largest chunk.  The source (WavPrep): how a chunk's waveforms reach MelFront::wav — uploaded, resampled there, or
// resampled / uploaded into the trimmer's staging buffer, trimmed and compacted there; it is the only place that knows which entry was
// called, and (mtts_dvector_embed_wavs_source, wavsource.h) where the waveforms live: packed host float32 as in the three entries, host
// int16, or device float32 rows.  The tail, shared: power mel, the partial windows, the gather, the encoder.
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
#include "wavsource.h"

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

// The partial rule and the outputs of an embed_wavs call.  out (with an encoder): [n_utts][E] d-vectors.  n_partials [n_utts].  slices
// (or nullptr; required without an encoder): the partial stacks [sum N][frames][n_mel], all utterances one after another.  n_trimmed
// (or nullptr; written with a Vad): the trimmed lengths.
struct PartialRule { int frames, step; double min_coverage; };
struct EmbedOut { float* out; int* n_partials; float* slices; int* n_trimmed; };

// A chunk of a call: utterances [u0, u1) with N partials; src0 = its first sample in the waveforms WavPrep reads.
struct Chunk { int u0, u1, N; long long src0; };

// The host tables of one chunk.  Every one of them is the source of an asynchronous upload, so it stays alive, one ChunkTables per
// chunk, until the call's final synchronise.
struct ChunkTables {
    std::vector<StftUtt> utts;   // MelFront's packing tables
    std::vector<int> rowmap;
    std::vector<int> win, off;   // first packed mel row of every partial; partials before every utterance
    std::vector<RsUtt> rs;       // the resampler's table (WavPrep with a resampler and no trimmer)
    std::vector<VadUtt> vad;     // the trimmer's
    std::vector<WavUtt> ingest;  // the source's (WavPrep with a source that is not host float32, outside the trimmer's lengths())
    // the table a stage has just enqueued for upload moves here (a moved vector keeps its storage); the stage packs its next chunk into a fresh one
    template <class T>
    static void keep(std::vector<T>& kept, std::vector<T>& staged) { kept = std::move(staged); staged.clear(); }
};

// How a chunk's waveforms reach mf->wav: all that the three embed_wavs entries differ in.
//   neither (mtts_dvector_embed_wavs): the waveforms are at the front-end's rate and are uploaded, zero-extended on the host.
//   rs (.._resampled): n_samples counts SOURCE-rate samples; every chunk is resampled (and normalised to target_dbfs unless that is NaN)
//     by rs straight into mf->wav over zeros, and the front-end rate's signal never visits the host.
//   vad (.._preprocessed): every chunk's waveforms go (through rs when given, else as they are) into vad's staging buffer, are trimmed
//     there, and the kept windows are compacted into mf->wav over zeros.  Chunks and capacities are planned from the untrimmed lengths
//     (trimming only shortens, and the partial count never grows as a waveform shrinks); the partial rule then applies to the trimmed
//     lengths, which the host reads back once per chunk (Vad::detect).
// The chunking, the launches behind the waveform buffer and the results are those of the plain entry on the prepared waveforms.
//
// src (mtts_dvector_embed_wavs_source; wavsource.h) says where the waveforms are.  Host float32, the three entries' form, is uploaded
// as above.  Host int16 and device float32 reach the first stage's input — the resampler's source buffer, the trimmer's staging
// buffer, or mf->wav over zeros at the packed wav0 offsets — through ing's kernel instead of that upload; every launch behind that
// buffer is the same, so the results are those of the host float32 route on the same sample values.
struct WavPrep {
    MelFront* mf;
    Resample* rs;
    Vad* vad;
    double target_dbfs;
    bool increase_only;
    WavSource src;
    WavIngest* ing;

    int err(const std::string& s) const { return mf->err(s); }
    bool plain() const { return !rs && !vad; }
    bool host_f32() const { return src.kind == WAV_HOST_F32; }
    bool extended() const { return plain() && host_f32(); }   // the host zero-extends and one upload fills mf->wav
    const float* f32(const Chunk& c) const { return (const float*)src.data + c.src0; }

    // a chunk's utterances through the source's kernel into dst, utterance k of the chunk at dst0_of(k)
    template <class Dst0>
    int ingest(const Chunk& c, const int* n_samples, float* dst, Dst0 dst0_of) const {
        ing->table_begin();
        for (int u = c.u0; u < c.u1; ++u) ing->table_add(src, u, n_samples[u], dst0_of((size_t)(u - c.u0)));
        return ing->launch(src, c.src0, dst);
    }

    // The refusals that are the stages' own, and h_n [n_utts]: every utterance's samples at the front-end's rate (before trimming).
    int check(const std::string& who, int n_utts, const int* n_samples, std::vector<long long>& h_n) const {
        if (ing->check(who, src, n_utts, n_samples)) return -1;
        if (rs && rs->check_lengths(who, n_utts, n_samples)) return -1;
        if (vad && !rs && !std::isnan(target_dbfs))
            return err(who + "volume normalisation needs a resampler (mtts_stft_load_resampler; the identity bank for waveforms at the front-end's rate)");
        h_n.resize((size_t)n_utts);
        for (int u = 0; u < n_utts; ++u) h_n[(size_t)u] = rs ? rs->out_len(n_samples[u]) : n_samples[u];
        if (vad) {
            if (vad->check_lengths(who, n_utts, h_n.data())) return -1;
            if (vad->c.W <= mf->n_fft / 2)
                return err(who + "a VAD window of " + std::to_string(vad->c.W) + " samples is too short for the reflection padding (need more than filter_length / 2 = " +
                           std::to_string(mf->n_fft / 2) + ")");
        }
        return mf->check_utterances(who, n_utts, [&](int u) { return h_n[(size_t)u]; }, MelFront::UTT_PAD);
    }

    // The stages' buffers for the largest chunk: its source samples, its samples at the front-end's rate, slots, windows and utterances.
    int reserve(const std::string& who, const std::vector<Chunk>& chunks, const int* n_samples, const long long* h_n) const {
        if (extended()) return 0;
        long long max_src = 0, max_n = 0, max_slots = 0, max_win = 0;
        size_t max_utts = 0;
        for (const Chunk& c : chunks) {
            long long n_src = 0, n = 0, slots = 0, nw = 0;
            for (int u = c.u0; u < c.u1; ++u) {
                n_src += n_samples[u];
                n += h_n[u];
                if (rs) slots += (h_n[u] + rs->run - 1) / rs->run;
                if (vad) nw += h_n[u] / vad->c.W;
            }
            max_src = std::max(max_src, n_src);
            max_n = std::max(max_n, n);
            max_slots = std::max(max_slots, slots);
            max_win = std::max(max_win, nw);
            max_utts = std::max(max_utts, (size_t)(c.u1 - c.u0));
        }
        if (max_src > (1LL << 31) - 1 || (vad && max_n > (1LL << 31) - 1)) return err(who + "too many samples in one chunk");
        return (!host_f32() && ing->reserve(src, max_src, max_utts)) || (rs && rs->reserve(max_src, max_slots, max_utts)) ||
               (vad && vad->reserve(max_n, max_win, max_utts, false)) ? -1 : 0;
    }
    // before the first launch: a device source's producer
    int begin() const { return ing->after_producer(src); }

    // Before packing.  With a trimmer: the untrimmed waveforms into its staging buffer, the mask, and the chunk's trimmed lengths back
    // into h_n (synchronises mf->stream: the resampler's table is free again).  Without one the lengths stand.
    int lengths(const Chunk& c, const int* n_samples, long long* h_n) const {
        if (!vad) return 0;
        vad->table_begin();
        for (int u = c.u0; u < c.u1; ++u) vad->table_add(h_n[u]);
        if (rs) {
            rs->table_begin();
            for (int u = c.u0; u < c.u1; ++u) rs->table_add(n_samples[u], vad->h_utts[(size_t)(u - c.u0)].src0);
            if (host_f32() ? rs->launch(f32(c), target_dbfs, increase_only, vad->stage.p)
                           : ingest(c, n_samples, rs->src.p, [&](size_t k) { return rs->h_utts[k].src0; }) || rs->convert(target_dbfs, increase_only, vad->stage.p))
                return -1;
        } else if (host_f32())
            DEV_CHECK(hipMemcpyAsync(vad->stage.p, f32(c), (size_t)vad->n_src * sizeof(float), hipMemcpyHostToDevice, mf->stream));
        else if (ingest(c, n_samples, vad->stage.p, [&](size_t k) { return vad->h_utts[k].src0; }))
            return -1;
        if (vad->detect(nullptr)) return -1;
        for (int u = c.u0; u < c.u1; ++u) h_n[u] = vad->h_nout[2 * (size_t)(u - c.u0)];
        return 0;
    }

    // After packing: the chunk's waveforms into mf->wav at the places MelFront has packed, and the reflect-padded signals.  The stages
    // write over zeros: the zero-extension to the last partial window's end.
    int fill(const Chunk& c, const int* n_samples, ChunkTables& t) const {
        if (extended()) return mf->pad_waveforms(f32(c), false, true);
        DEV_CHECK(hipMemsetAsync(mf->wav.p, 0, (size_t)mf->n_samples * sizeof(float), mf->stream));
        if (vad) {   // the kept windows
            for (int u = c.u0; u < c.u1; ++u) vad->h_utts[(size_t)(u - c.u0)].dst0 = mf->h_utts[(size_t)(u - c.u0)].wav0;
            if (vad->compact(mf->wav.p)) return -1;
            ChunkTables::keep(t.vad, vad->h_utts);
        } else if (rs) {   // source-rate samples up, resampled
            rs->table_begin();
            for (int u = c.u0; u < c.u1; ++u) rs->table_add(n_samples[u], mf->h_utts[(size_t)(u - c.u0)].wav0);
            if (host_f32() ? rs->launch(f32(c), target_dbfs, increase_only)
                           : ingest(c, n_samples, rs->src.p, [&](size_t k) { return rs->h_utts[k].src0; }) || rs->convert(target_dbfs, increase_only))
                return -1;
            ChunkTables::keep(t.rs, rs->h_utts);
        } else if (ingest(c, n_samples, mf->wav.p, [&](size_t k) { return mf->h_utts[k].wav0; }))   // the source's samples as they are
            return -1;
        if (!host_f32() && !vad) ChunkTables::keep(t.ingest, ing->h_utts);
        return mf->pad_staged(false, true);
    }
};

class SpeakerEval {
public:
    MelFront* mf = nullptr;
    int device = 0;
    DevBuf<float> stack;    // [N][frames][n_mel]: the partial utterances of a chunk
    DevBuf<int> win;        // first packed mel row of every partial
    hipEvent_t ev_front = nullptr, ev_enc = nullptr;
    std::vector<float> h_wav;       // the plain entry's waveforms, zero-extended
    std::vector<long long> h_n;     // per utterance: samples at the front-end's rate,
    std::vector<long long> h_ext;   // the length it is zero-extended to,
    std::vector<int> h_cnt;         // and its partials
    std::vector<Chunk> chunks;
    std::vector<ChunkTables> tables;

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
        if (mf->check_utterances(who, n_utts, [&](int u) { return n_samples[u]; }, MelFront::UTT_GRID | MelFront::UTT_PAD)) return -1;
        mf->pack_begin();
        for (int u = 0; u < n_utts; ++u) mf->pack_add(n_samples[u], mf->frames_of(n_samples[u]));
        if (mf->stage("mtts_stft_power_mel_batch", true) || mf->pad_waveforms(wavs, false, true)) return -1;
        power_mel();
        if (mf->check_launch()) return -1;
        DEV_CHECK(hipMemcpyAsync(mel_host, mf->mel, (size_t)mf->n_frames * mf->n_mel * sizeof(float), hipMemcpyDeviceToHost, mf->stream));
        DEV_CHECK(hipStreamSynchronize(mf->stream));
        return 0;
    }

    // The three mtts_dvector_embed_wavs* entries (name: the one called; prep: what tells them apart).  dv == nullptr: the front-end only.
    // Everything that can be refused is refused before the first launch.
    int embed_wavs(const char* name, const WavPrep& prep, DVector* dv, int dv_device, int n_utts, const int* n_samples, const float* wavs, const PartialRule& r,
                   const EmbedOut& o) {
        const std::string who = std::string(name) + ": ";
        if (validate(who, prep, dv, dv_device, n_utts, n_samples, wavs, r, o)) return -1;
        const bool two_streams = dv && dv->stream != mf->stream;
        if (two_streams) { DEV_CHECK(mf->mem.event(ev_front)); DEV_CHECK(mf->mem.event(ev_enc)); }
        WavPrep fed = prep;   // what front() reads from: the plain chain's host float32 is zero-extended here, everything else is as the caller holds it
        fed.src.data = prep.extended() ? zero_extended(n_utts, n_samples, wavs) : (const void*)wavs;
        for (int u = 0; u < n_utts; ++u) o.n_partials[u] = h_cnt[(size_t)u];
        const int max_N = plan(dv, n_utts, n_samples, prep.extended());
        // sized once for the largest chunk, before the first launch: a later, larger chunk must not free the stack the previous chunk's
        // encoder still reads on the other stream (and the same for the stages' buffers)
        if (mf->grow(stack, (size_t)max_N * span4(r) * 4 + 64, "partial utterances") || mf->grow(win, (size_t)max_N, "windows") ||
            prep.reserve(who, chunks, n_samples, h_n.data()) || prep.begin())
            return -1;
        tables.clear();
        tables.resize(chunks.size());
        long long part0 = 0;
        for (size_t c = 0; c < chunks.size(); ++c) {
            if (front(name, fed, chunks[c], n_samples, r, o, tables[c]) || tail(who, chunks[c], tables[c], dv, c > 0, part0, r, o)) return -1;
            part0 += chunks[c].N;
        }
        if (dv) DEV_CHECK(hipStreamSynchronize(dv->stream));
        DEV_CHECK(hipStreamSynchronize(mf->stream));
        return 0;
    }

    int span4(const PartialRule& r) const { return r.frames * mf->n_mel / 4; }

    // the arguments, the stages' refusals, and per utterance the partial count and the zero-extended length (h_n, h_cnt, h_ext)
    int validate(const std::string& who, const WavPrep& prep, DVector* dv, int dv_device, int n_utts, const int* n_samples, const float* wavs, const PartialRule& r,
                 const EmbedOut& o) {
        const int n_mel = mf->n_mel;
        if (!mf->have_basis || !mf->have_mel) return err(who + "STFT bases not loaded");
        if (n_utts < 1 || !n_samples || !wavs || !o.n_partials) return err(who + "bad arguments (n_utts < 1 or NULL n_samples / wavs / n_partials_out)");
        if (dv ? !o.out : !o.slices) return err(who + "NULL output (out with an encoder, slices_out without one)");
        if (r.frames < 1 || r.step < 1 || r.step > r.frames || !(r.min_coverage > 0.0 && r.min_coverage <= 1.0))
            return err(who + "bad partial rule (need 1 <= frame_step <= partial_frames, 0 < min_coverage <= 1)");
        if (n_mel & 3) return err(who + "n_mel % 4 != 0");
        if (dv) {
            if (dv_device != device) return err(who + "the encoder and the STFT handle are on different devices");
            if (dv->n_mels != n_mel || dv->T != r.frames)
                return err(who + "the encoder expects partials of " + std::to_string(dv->T) + " x " + std::to_string(dv->n_mels) + ", the front-end makes " +
                           std::to_string(r.frames) + " x " + std::to_string(n_mel));
        }
        if (prep.check(who, n_utts, n_samples, h_n)) return -1;
        h_ext.resize((size_t)n_utts);
        h_cnt.resize((size_t)n_utts);
        long long total_parts = 0;
        for (int u = 0; u < n_utts; ++u) {
            const std::string utt = who + "utterance " + std::to_string(u) + ": ";
            h_cnt[(size_t)u] = spk_partial_count(h_n[(size_t)u], mf->hop, r.frames, r.step, r.min_coverage, &h_ext[(size_t)u]);
            if (dv && h_cnt[(size_t)u] > dv->cap_N)
                return err(utt + std::to_string(h_cnt[(size_t)u]) + " partial utterances exceed the encoder's max_partials = " + std::to_string(dv->cap_N));
            if (h_ext[(size_t)u] > 0x7fffffffLL - mf->hop) return err(utt + "too long");
            total_parts += h_cnt[(size_t)u];
        }
        if (total_parts > (1LL << 30) / ((long long)r.frames * n_mel)) return err(who + "too many partial utterances in one call");
        if (dv && dv->dirty && dv->refresh() != 0) return err(who + dv->last_error);
        return 0;
    }

    // the plain entry's waveforms, every one zero-extended to the end of its last partial window
    const float* zero_extended(int n_utts, const int* n_samples, const float* wavs) {
        long long total = 0, src = 0, dst = 0;
        for (int u = 0; u < n_utts; ++u) total += h_ext[(size_t)u];
        h_wav.assign((size_t)total, 0.f);
        for (int u = 0; u < n_utts; ++u) {
            std::copy(wavs + src, wavs + src + n_samples[u], h_wav.begin() + dst);
            src += n_samples[u];
            dst += h_ext[(size_t)u];
        }
        return h_wav.data();
    }

    // A chunk: consecutive utterances within the encoder's capacity (front-end only: the whole call; 65535: the pad kernel's gridDim.y).
    // Returns the partials of the largest.
    int plan(const DVector* dv, int n_utts, const int* n_samples, bool plain) {
        chunks.clear();
        int max_N = 0;
        long long src0 = 0;
        for (int u0 = 0; u0 < n_utts;) {
            Chunk c{u0, u0, 0, src0};
            while (c.u1 < n_utts && c.u1 - u0 < 65535 && (!dv || (c.N + h_cnt[(size_t)c.u1] <= dv->cap_N && c.u1 - u0 < dv->cap_B))) {
                src0 += plain ? h_ext[(size_t)c.u1] : n_samples[c.u1];
                c.N += h_cnt[(size_t)c.u1++];
            }
            chunks.push_back(c);
            max_N = std::max(max_N, c.N);
            u0 = c.u1;
        }
        return max_N;
    }

    // One chunk up to its mel: the lengths (with a trimmer: the trimmed ones, and the partial rule on them), packing, waveforms, front-end.
    int front(const char* name, const WavPrep& prep, Chunk& c, const int* n_samples, const PartialRule& r, const EmbedOut& o, ChunkTables& t) {
        if (prep.lengths(c, n_samples, h_n.data())) return -1;
        if (prep.vad) {
            c.N = 0;
            for (int u = c.u0; u < c.u1; ++u) {
                o.n_partials[u] = h_cnt[(size_t)u] = spk_partial_count(h_n[(size_t)u], mf->hop, r.frames, r.step, r.min_coverage, &h_ext[(size_t)u]);
                if (o.n_trimmed) o.n_trimmed[u] = (int)h_n[(size_t)u];
                c.N += h_cnt[(size_t)u];
            }
        }
        mf->pack_begin();
        for (int u = c.u0; u < c.u1; ++u) mf->pack_add(h_ext[(size_t)u], mf->frames_of((int)h_ext[(size_t)u]));
        if (mf->stage(name, true) || prep.fill(c, n_samples, t)) return -1;
        power_mel();
        return 0;
    }

    // The shared tail: the chunk's windows out of the packed mel into the partial stack, and the encoder on it.  With the two handles
    // on different streams, every chunk but the first waits for the previous chunk's encoder, which still reads the stack.
    int tail(const std::string& who, const Chunk& c, ChunkTables& t, DVector* dv, bool wait_enc, long long part0, const PartialRule& r, const EmbedOut& o) {
        const bool two_streams = dv && dv->stream != mf->stream;
        const int s4 = span4(r), per = std::min((s4 + 255) / 256, 8);
        t.off.assign(1, 0);
        for (int u = c.u0; u < c.u1; ++u) {
            const StftUtt& q = mf->h_utts[(size_t)(u - c.u0)];
            for (int p = 0; p < h_cnt[(size_t)u]; ++p) {
                if (p * r.step + r.frames > q.T) return err(who + "internal: a window ends past its utterance's frames");
                t.win.push_back(q.frame0 + p * r.step);
            }
            t.off.push_back((int)t.win.size());
        }
        ChunkTables::keep(t.utts, mf->h_utts);
        ChunkTables::keep(t.rowmap, mf->h_rowmap);
        DEV_CHECK(hipMemcpyAsync(win.p, t.win.data(), (size_t)c.N * sizeof(int), hipMemcpyHostToDevice, mf->stream));
        if (two_streams && wait_enc) DEV_CHECK(hipStreamWaitEvent(mf->stream, ev_enc, 0));
        MTTS_LAUNCH(spk_gather_kernel, dim3((unsigned)c.N * (unsigned)per), dim3(256), mf->stream, (const float*)mf->mel, (const int*)win.p, mf->n_mel, s4, per, stack.p);
        if (mf->check_launch()) return -1;
        if (o.slices) DEV_CHECK(hipMemcpyAsync(o.slices + part0 * s4 * 4, stack.p, (size_t)c.N * s4 * 4 * sizeof(float), hipMemcpyDeviceToHost, mf->stream));
        if (!dv) return 0;
        if (two_streams) { DEV_CHECK(hipEventRecord(ev_front, mf->stream)); DEV_CHECK(hipStreamWaitEvent(dv->stream, ev_front, 0)); }
        if (dv->forward_device(stack.p, c.N, t.off.data(), c.u1 - c.u0, o.out + (long long)c.u0 * dv->E, nullptr, false) != 0) return err(who + dv->last_error);
        if (two_streams) DEV_CHECK(hipEventRecord(ev_enc, dv->stream));
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
