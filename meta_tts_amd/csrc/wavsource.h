// Where the waveforms of an embed_wavs call live, and the one kernel that brings a chunk of them into the float32 buffer the next stage
// reads (the resampler's source buffer, the trimmer's staging buffer, or MelFront::wav at the packed wav0 offsets).
//
// Reference: evaluation/wavs_to_dvector.py reads 16-bit PCM files (widened to float on the host, `int16 / 2^15`), and the test stage's
// waveform is cut to int16 on its way to such a file (lightning/utils.py:20-30, `(wav * max_wav_value).astype("int16")`).  Both
// conversions are exact in fp32 — a 16-bit integer times a power of two, and a truncation — so they can run behind the upload at no
// numerical cost: a PCM16 source uploads 2 bytes per sample, and a device source (the vocoder's output) is never downloaded at all.
//
//   WAV_HOST_F32    host float32, packed back to back: today's form.  It does not come through here: speakereval.h uploads it as before.
//   WAV_HOST_PCM16  host int16, packed back to back.  A chunk's raw samples are uploaded into `pcm` and widened: x = v / 32768.
//   WAV_DEVICE_F32  device float32, utterance u at data + u * row_stride, n_samples[u] <= row_stride; what lies beyond n_samples[u] in
//                   a row is never read.  `producer`: the stream that writes it (the front-end's stream waits for an event recorded on
//                   it; no host synchronisation).  quantize_scale s > 0: every sample goes through a 16-bit file's round trip,
//                   q = trunc(x * s) clamped to [-32768, 32767], x' = q / 32768 (s = max_wav_value; |x * s| >= 32768 is outside the
//                   contract — numpy's cast is undefined there — and the clamp only keeps the device defined); 0: as they are.
//
// MI355X layout.  Pure streaming, 2 or 4 bytes in and 4 bytes out per sample, no reuse: nothing to stage in LDS, a handful of VGPRs, and
// the grid is (groups of the longest utterance, utterances) through a small table, as resample.h and vad.h drive theirs.  A lane owns
// one group of 16 source bytes (8 int16 or 4 floats) whose DESTINATION starts on a 16-byte boundary: the stores, two thirds or half of
// the traffic, are always whole float4s on the body.  Packed int16 utterances start at any 2-byte offset, so source and destination
// alignment differ from utterance to utterance: where the group's source is 16-byte aligned too it is one 16-byte load, elsewhere the
// lane reads its own samples one by one (consecutive lanes still read consecutive addresses).  The at most 3 samples before the first
// boundary and the ragged end are scalar.  A lane reads and writes samples of its own utterance only, within [0, n): no atomics, no
// wavefront intrinsics, and an output depends on its own input sample alone, so it is bit-identical alone, in any batch, at any position.
// Nothing is written beyond an utterance's length: the zero extension stays the memset or the padding that provides it.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "melfront.h"

namespace mtts {

enum { WAV_HOST_F32 = 0, WAV_HOST_PCM16 = 1, WAV_DEVICE_F32 = 2 };
constexpr int WI_THREADS = 256;

struct WavSource {
    int kind = WAV_HOST_F32;
    const void* data = nullptr;
    long long row_stride = 0;          // WAV_DEVICE_F32: floats between utterances
    hipStream_t producer = nullptr;    // WAV_DEVICE_F32: the stream that writes `data`
    float quantize_scale = 0.f;        // WAV_DEVICE_F32: max_wav_value of the 16-bit round trip, 0 for none
};

struct WavUtt {
    long long src0;   // first sample in the source (the chunk's staged int16, or the caller's device rows)
    long long dst0;   // first sample in the destination buffer
    int n, pad_;
};

struct alignas(16) Pcm8 { short v[8]; };

__device__ __forceinline__ float wav_sample(short v, float) { return (float)v * (1.f / 32768.f); }
__device__ __forceinline__ float wav_sample(float x, float scale) {
    if (!(scale > 0.f)) return x;
    const float q = fminf(fmaxf(truncf(x * scale), -32768.f), 32767.f);
    return q * (1.f / 32768.f);
}
// G samples from a 16-byte aligned address
__device__ __forceinline__ void wav_load16(const short* p, float scale, float* v) {
    const Pcm8 r = *reinterpret_cast<const Pcm8*>(p);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = wav_sample(r.v[k], scale);
}
__device__ __forceinline__ void wav_load16(const float* p, float scale, float* v) {
    const float4 r = ld4(p);
    v[0] = wav_sample(r.x, scale); v[1] = wav_sample(r.y, scale); v[2] = wav_sample(r.z, scale); v[3] = wav_sample(r.w, scale);
}

// dst[dst0 + i] = sample(src[src0 + i]) for 0 <= i < n of utterance blockIdx.y.  `head` = the samples before the destination's first
// 16-byte boundary; group g (one per lane, gridDim.x covers the longest utterance) is samples [head + G (g - 1), head + G g), cut to
// [0, n): group 0 is the head, a whole group inside the utterance is the aligned body, the last one the ragged end.
template <class Src>
__global__ __launch_bounds__(WI_THREADS) void wav_ingest_kernel(const Src* src, const WavUtt* utts, float scale, float* dst) {
    constexpr int G = 16 / (int)sizeof(Src);
    const WavUtt u = utts[blockIdx.y];
    const Src* x = src + u.src0;
    float* y = dst + u.dst0;
    const int head = (int)((0u - (unsigned)(reinterpret_cast<uintptr_t>(y) >> 2)) & 3u);
    const long long g = (long long)blockIdx.x * WI_THREADS + (long long)threadIdx.x;
    const long long lo = head + G * (g - 1), hi = lo + G;
    if (lo >= u.n) return;
    if (lo >= 0 && hi <= u.n) {
        float v[G];
        if ((reinterpret_cast<uintptr_t>(x + lo) & 15u) == 0)
            wav_load16(x + lo, scale, v);
        else {
#pragma unroll
            for (int k = 0; k < G; ++k) v[k] = wav_sample(x[lo + k], scale);
        }
#pragma unroll
        for (int k = 0; k < G; k += 4) st4(y + lo + k, make_float4(v[k], v[k + 1], v[k + 2], v[k + 3]));
    } else {
        const long long a = lo < 0 ? 0 : lo, b = hi < u.n ? hi : u.n;
        for (long long i = a; i < b; ++i) y[i] = wav_sample(x[i], scale);
    }
}

// The device side of a source that is not host float32: the int16 staging buffer, the table, the event behind the producer.
class WavIngest {
public:
    MelFront* mf = nullptr;
    DevBuf<short> pcm;               // a chunk's raw int16 samples (WAV_HOST_PCM16)
    DevBuf<WavUtt> utts;
    hipEvent_t ev_src = nullptr;
    std::vector<WavUtt> h_utts;
    long long n_src = 0;
    int max_n = 0;

    int err(const std::string& s) { return mf->err(s); }

    // what the entry refuses about the source itself, before any launch
    int check(const std::string& who, const WavSource& s, int n_utts, const int* n_samples) {
        if (s.kind != WAV_HOST_F32 && s.kind != WAV_HOST_PCM16 && s.kind != WAV_DEVICE_F32)
            return err(who + "unknown source kind " + std::to_string(s.kind) + " (0: host float32, 1: host int16, 2: device float32)");
        if (!(s.quantize_scale >= 0.f)) return err(who + "negative quantize_scale (0: none, > 0: max_wav_value)");
        if (s.quantize_scale > 0.f && s.kind != WAV_DEVICE_F32) return err(who + "quantize_scale on a host source (only a device float32 source is quantised)");
        if (s.kind == WAV_DEVICE_F32)
            for (int u = 0; u < n_utts; ++u)
                if (n_samples[u] > s.row_stride)
                    return err(who + "utterance " + std::to_string(u) + ": " + std::to_string(n_samples[u]) + " samples exceed row_stride = " + std::to_string(s.row_stride));
        return 0;
    }

    // ---- the table of a launch: host only ----------------------------------------------------------------------------------------------
    void table_begin() { h_utts.clear(); n_src = 0; max_n = 0; }
    // utterance u of the call, n samples, to dst0 of the destination buffer
    void table_add(const WavSource& s, int u, int n, long long dst0) {
        h_utts.push_back(WavUtt{s.kind == WAV_DEVICE_F32 ? (long long)u * s.row_stride : n_src, dst0, n, 0});
        n_src += n;
        max_n = std::max(max_n, n);
    }
    // room for a launch of at most n_src_ source samples and n_utts_ utterances
    int reserve(const WavSource& s, long long n_src_, size_t n_utts_) {
        return (s.kind == WAV_HOST_PCM16 && mf->grow(pcm, (size_t)n_src_ + 64, "16-bit waveforms")) || mf->grow(utts, n_utts_, "source utterances") ? -1 : 0;
    }
    // once per call, before its first launch: the front-end's stream waits for what the producer has enqueued so far
    int after_producer(const WavSource& s) {
        if (s.kind != WAV_DEVICE_F32 || s.producer == mf->stream) return 0;
        DEV_CHECK(mf->mem.event(ev_src));
        DEV_CHECK(hipEventRecord(ev_src, s.producer));
        DEV_CHECK(hipStreamWaitEvent(mf->stream, ev_src, 0));
        return 0;
    }
    // The tabled utterances -> dst at their dst0.  chunk0: the chunk's first sample in a packed host source.  Asynchronous on mf->stream;
    // h_utts and the host samples must stay as they are until the stream has been synchronised.
    int launch(const WavSource& s, long long chunk0, float* dst) {
        const int G = s.kind == WAV_HOST_PCM16 ? 8 : 4;
        const dim3 grid((unsigned)((((long long)max_n + G - 1) / G + 1 + WI_THREADS - 1) / WI_THREADS), (unsigned)h_utts.size());   // + 1: the head's group
        DEV_CHECK(hipMemcpyAsync(utts.p, h_utts.data(), h_utts.size() * sizeof(WavUtt), hipMemcpyHostToDevice, mf->stream));
        if (s.kind == WAV_HOST_PCM16) {
            DEV_CHECK(hipMemcpyAsync(pcm.p, (const short*)s.data + chunk0, (size_t)n_src * sizeof(short), hipMemcpyHostToDevice, mf->stream));
            MTTS_LAUNCH(wav_ingest_kernel<short>, grid, dim3(WI_THREADS), mf->stream, (const short*)pcm.p, (const WavUtt*)utts.p, 0.f, dst);
        } else
            MTTS_LAUNCH(wav_ingest_kernel<float>, grid, dim3(WI_THREADS), mf->stream, (const float*)s.data, (const WavUtt*)utts.p, s.quantize_scale, dst);
        return 0;
    }
};

}  // namespace mtts
