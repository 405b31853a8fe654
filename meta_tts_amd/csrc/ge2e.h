// GE2E loss (generalized end-to-end loss, Wan et al. 2018, softmax variant) and its hand-derived backward: the objective the reference's
// from-scratch encoder class is named after (lightning/model/speaker_encoder.py:11-31) and does not contain.  No GE2E loss code exists in the
// reference tree: the definition is the one stated in include/mtts.h, restated in float64 torch by tests/ge2e_oracle.py; parity with any
// published GE2E trainer is UNPINNED.
//
// Input e [N speakers][M utterances][E], speaker-major rows r = j M + i.  With S_k = sum_i e[k][i]:
//   c_k = S_k / |S_k|                                     inclusive centroid
//   chat_r = u / |u|,  u = (S_j - e_r) / (M - 1)          exclusive centroid of row r = (j, i)
//   d[r][k] = e_r . c_k  (k != j),   d[r][j] = e_r . chat_r,   s = w d + b        (a plain dot product: e is not renormalised)
//   L = 1 / (N M) sum_r (logsumexp_k s[r][k] - s[r][j]),   g = (softmax(s) - onehot_j) / (N M)
//   dL/dw = sum g d,   dL/db = sum g
//   dL/de_r = (a) w sum_{k != j} g[r][k] c_k + w g[r][j] chat_r                                          the row's own similarities
//           + (b) (dc_j - c_j (c_j . dc_j)) / |S_j|,  dc_j = w sum_{r' of other speakers} g[r'][j] e_r'   through the inclusive centroid
//           + (c) sum_{i' != i} q_(j,i'),  q_r = w g[r][j] (e_r - chat_r (chat_r . e_r)) / (|u_r| (M - 1))   through the other rows' exclusive centroids
//
// Kernels — LDS and barriers only, no atomic and no wavefront intrinsic, every reduction a fixed-order tree or an ascending loop, so the
// SIMT emulator runs the same source and a loss and its gradients are the same bits on every run.  Sums and dot products are float64
// (a few thousand terms per launch: the rate of the float64 pipe is not what a step waits for) and round once; g, the loss triple, the
// similarities and demb are float32.
//   * ge2e_centroid_kernel: one workgroup per speaker: S_k, |S_k|, c_k.
//   * ge2e_row_kernel: one workgroup per row: u, |u|, chat; the N dot products with the centroid table staged through LDS in slabs of 16
//     speakers (16 threads share a dot product: thread (speaker s, part p) adds elements p, p + 16, ... in ascending order, then one thread
//     adds the 16 parts in ascending order; a slab row is E + 16 doubles — by the bank rule for 8-byte LDS reads that should put the two
//     speakers a 32-lane group reads on opposite halves of the 64 banks at E = 256: reasoning from the layout, NOT measured, no conflict
//     counter or timing was taken); the log-sum-exp with the maximum subtracted; g[r][.], the row's loss / w / b terms, q_r, optionally s.
//   * ge2e_fold_kernel: one workgroup: the row terms summed in float64 (a thread its consecutive rows in ascending order, then the 256
//     partial sums in ascending order) -> L, dL/dw, dL/db.
//   * ge2e_grad_kernel: one workgroup per speaker j, thread t = element t: dc_j once (a column walk over g, ascending rows), then for each of
//     its M utterances (a) + (b) + (c).  Every element of demb is written by exactly one thread of this launch.
// A zero S_k or u (embeddings that cancel) divides by zero as the definition does: NaN, in that speaker's rows.
// Cost: sized for a training batch (64 x 10: N M + M N + M M loop trips per thread of ge2e_grad_kernel, a few thousand).  The gradient kernel
// walks all N M rows and, per utterance, all N centroids serially in each thread, with only E of its 256 threads at work: at the admitted
// limits (N = 1024, M = 64) that is about 1.3e5 trips per thread in each of 1 024 workgroups, each trip a dependent float64 add.  No time has
// been measured anywhere near the limits; they bound the indices and the LDS arrays, they are not a statement about speed.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "compat.h"

namespace mtts {

constexpr int GE2E_THREADS = 256;
constexpr int GE2E_MAX_SPK = 1024;   // a row's N dot products in LDS: 8 KB
constexpr int GE2E_MAX_UTT = 64;
constexpr int GE2E_MAX_DIM = 256;    // the encoder's own limit (dvec_bad_shape); one element per thread
constexpr int GE2E_SLAB = 16;        // speakers of the centroid table staged in LDS at a time
constexpr int GE2E_PARTS = 16;       // threads that share one dot product (GE2E_SLAB * GE2E_PARTS == GE2E_THREADS)
constexpr int GE2E_SLAB_LD = GE2E_MAX_DIM + 16;

// The one predicate of the kernel-level entry and of the handle: null, or the refusal with its argument named.
inline const char* ge2e_bad_shape(int N, int M, int E, float w) {
    if (N < 2 || N > GE2E_MAX_SPK) return "n_spk must be in 2 .. 1024";
    if (M < 2 || M > GE2E_MAX_UTT) return "n_utt must be in 2 .. 64";
    if (E < 4 || E > GE2E_MAX_DIM || (E & 3)) return "E must be a multiple of 4 in 4 .. 256";
    if (w == 0.f || !std::isfinite(w)) return "w must be finite and not 0";
    return nullptr;
}

// where w and b are read from: device memory (the handle: no host round trip between steps) or the two values of the launch
struct Ge2eScal {
    const float* dev;   // [2] = w, b; null: the values below
    float w, b;
};
__device__ __forceinline__ double ge2e_w(const Ge2eScal& s) { return (double)(s.dev ? s.dev[0] : s.w); }
__device__ __forceinline__ double ge2e_b(const Ge2eScal& s) { return (double)(s.dev ? s.dev[1] : s.b); }

// layout of the scratch block: float64 tables, then g
struct Ge2eWs {
    double *S, *cen, *nS;   // [N][E], [N][E], [N]
    double *chat, *q;       // [N M][E] each
    double* terms;          // [N M][3]: row loss, row share of dL/dw, of dL/db
    float* g;               // [N M][N]
};
inline size_t ge2e_up256(size_t x) { return (x + 255) & ~(size_t)255; }
inline size_t ge2e_ws_bytes(long long rows, long long N, long long E) {
    const size_t d = sizeof(double);
    return 2 * ge2e_up256((size_t)(N * E) * d) + ge2e_up256((size_t)N * d) + 2 * ge2e_up256((size_t)(rows * E) * d) + ge2e_up256((size_t)rows * 3 * d) +
           ge2e_up256((size_t)(rows * N) * sizeof(float));
}
inline Ge2eWs ge2e_carve(void* ws, long long rows, long long N, long long E) {
    const size_t d = sizeof(double);
    char* p = (char*)ws;
    Ge2eWs k;
    k.S = (double*)p; p += ge2e_up256((size_t)(N * E) * d);
    k.cen = (double*)p; p += ge2e_up256((size_t)(N * E) * d);
    k.nS = (double*)p; p += ge2e_up256((size_t)N * d);
    k.chat = (double*)p; p += ge2e_up256((size_t)(rows * E) * d);
    k.q = (double*)p; p += ge2e_up256((size_t)(rows * E) * d);
    k.terms = (double*)p; p += ge2e_up256((size_t)rows * 3 * d);
    k.g = (float*)p;
    return k;
}

// sum / maximum of one value per thread, the same on every thread: a halving tree over red[GE2E_THREADS] (fixed order)
__device__ __forceinline__ double ge2e_tree_sum(double v, double* red) {
    const int tid = (int)threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = GE2E_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double t = red[0];
    __syncthreads();
    return t;
}
__device__ __forceinline__ double ge2e_tree_max(double v, double* red) {
    const int tid = (int)threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = GE2E_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid + s] > red[tid] ? red[tid + s] : red[tid];
        __syncthreads();
    }
    const double t = red[0];
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(GE2E_THREADS) void ge2e_centroid_kernel(const float* emb, int M, int E, Ge2eWs ws) {
    __shared__ double red[GE2E_THREADS];
    const int tid = (int)threadIdx.x, k = (int)blockIdx.x;
    double s = 0.0;
    if (tid < E)
        for (int i = 0; i < M; ++i) s += (double)emb[((size_t)k * M + i) * E + tid];
    const double nrm = sqrt(ge2e_tree_sum(s * s, red));
    if (tid < E) {
        ws.S[(size_t)k * E + tid] = s;
        ws.cen[(size_t)k * E + tid] = s / nrm;
    }
    if (tid == 0) ws.nS[k] = nrm;
}

__global__ __launch_bounds__(GE2E_THREADS) void ge2e_row_kernel(const float* emb, int N, int M, int E, Ge2eScal sc, Ge2eWs ws, float* sim) {
    __shared__ double es[GE2E_THREADS], ch[GE2E_THREADS], red[GE2E_THREADS], pr[GE2E_THREADS], dots[GE2E_MAX_SPK];
    __shared__ double cs[GE2E_SLAB][GE2E_SLAB_LD];
    const int tid = (int)threadIdx.x, r = (int)blockIdx.x, j = r / M;
    const double w = ge2e_w(sc), b = ge2e_b(sc);
    double e = 0.0, u = 0.0;
    if (tid < E) {
        e = (double)emb[(size_t)r * E + tid];
        u = (ws.S[(size_t)j * E + tid] - e) / (double)(M - 1);
    }
    const double nu = sqrt(ge2e_tree_sum(u * u, red));
    const double c_own = tid < E ? u / nu : 0.0;
    es[tid] = e;
    ch[tid] = c_own;
    if (tid < E) ws.chat[(size_t)r * E + tid] = c_own;
    const int spk = tid / GE2E_PARTS, part = tid % GE2E_PARTS;
    for (int k0 = 0; k0 < N; k0 += GE2E_SLAB) {
        __syncthreads();   // es / ch are written; the slab before this one is read
        for (int x = tid; x < GE2E_SLAB * E; x += GE2E_THREADS) {
            const int s = x / E, t = x - s * E, k = k0 + s;
            cs[s][t] = k >= N ? 0.0 : k == j ? ch[t] : ws.cen[(size_t)k * E + t];   // the row's own column: its exclusive centroid
        }
        __syncthreads();
        double p = 0.0;
        for (int t = part; t < E; t += GE2E_PARTS) p += es[t] * cs[spk][t];
        pr[tid] = p;
        __syncthreads();
        if (tid < GE2E_SLAB && k0 + tid < N) {
            double d = 0.0;
            for (int x = 0; x < GE2E_PARTS; ++x) d += pr[tid * GE2E_PARTS + x];
            dots[k0 + tid] = d;
        }
    }
    __syncthreads();
    double mx = -__builtin_huge_val();
    for (int k = tid; k < N; k += GE2E_THREADS) {
        const double s = w * dots[k] + b;
        mx = s > mx ? s : mx;
    }
    mx = ge2e_tree_max(mx, red);
    double se = 0.0;
    for (int k = tid; k < N; k += GE2E_THREADS) se += exp(w * dots[k] + b - mx);
    const double lse = mx + log(ge2e_tree_sum(se, red));
    const double inv = 1.0 / ((double)N * (double)M);
    double gw = 0.0, gb = 0.0;
    for (int k = tid; k < N; k += GE2E_THREADS) {
        const double s = w * dots[k] + b;
        const double g = (exp(s - lse) - (k == j ? 1.0 : 0.0)) * inv;
        ws.g[(size_t)r * N + k] = (float)g;
        if (sim) sim[(size_t)r * N + k] = (float)s;
        gw += g * dots[k];
        gb += g;
    }
    gw = ge2e_tree_sum(gw, red);
    gb = ge2e_tree_sum(gb, red);
    const double sj = w * dots[j] + b;
    if (tid == 0) {
        ws.terms[(size_t)r * 3] = lse - sj;
        ws.terms[(size_t)r * 3 + 1] = gw;
        ws.terms[(size_t)r * 3 + 2] = gb;
    }
    // what this row sends to the speaker's other utterances through its exclusive centroid (path c); g as the gradient kernel reads it
    const double gj = (double)(float)((exp(sj - lse) - 1.0) * inv);
    if (tid < E) ws.q[(size_t)r * E + tid] = w * gj * (e - c_own * dots[j]) / (nu * (double)(M - 1));
}

__global__ __launch_bounds__(GE2E_THREADS) void ge2e_fold_kernel(int rows, Ge2eWs ws, float* loss, float* grad_wb) {
    __shared__ double red[3][GE2E_THREADS];
    const int tid = (int)threadIdx.x, per = (rows + GE2E_THREADS - 1) / GE2E_THREADS;
    const int lo = tid * per, hi = lo + per < rows ? lo + per : rows;
    double a[3] = {0.0, 0.0, 0.0};
    for (int r = lo; r < hi; ++r)
        for (int x = 0; x < 3; ++x) a[x] += ws.terms[(size_t)r * 3 + x];
    for (int x = 0; x < 3; ++x) red[x][tid] = a[x];
    __syncthreads();
    if (tid == 0) {
        double t[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < GE2E_THREADS; ++k)
            for (int x = 0; x < 3; ++x) t[x] += red[x][k];
        loss[0] = (float)(t[0] / (double)rows);
        grad_wb[0] = (float)t[1];
        grad_wb[1] = (float)t[2];
    }
}

__global__ __launch_bounds__(GE2E_THREADS) void ge2e_grad_kernel(const float* emb, int N, int M, int E, Ge2eScal sc, Ge2eWs ws, float* demb) {
    __shared__ double red[GE2E_THREADS];
    const int tid = (int)threadIdx.x, j = (int)blockIdx.x, rows = N * M;
    const bool on = tid < E;
    const double w = ge2e_w(sc);
    double dc = 0.0;
    if (on)
        for (int r = 0; r < rows; ++r) {
            if (r / M == j) continue;
            dc += (double)ws.g[(size_t)r * N + j] * (double)emb[(size_t)r * E + tid];
        }
    dc *= w;
    const double c = on ? ws.cen[(size_t)j * E + tid] : 0.0;
    const double cdot = ge2e_tree_sum(c * dc, red);
    const double via_c = (dc - c * cdot) / ws.nS[j];
    if (!on) return;   // (after the last barrier)
    for (int i = 0; i < M; ++i) {
        const size_t r = (size_t)j * M + i;
        const float* g = ws.g + r * N;
        double a = 0.0;
        for (int k = 0; k < N; ++k) a += (double)g[k] * (k == j ? ws.chat[r * E + tid] : ws.cen[(size_t)k * E + tid]);
        double via_x = 0.0;
        for (int i2 = 0; i2 < M; ++i2)
            if (i2 != i) via_x += ws.q[((size_t)j * M + i2) * E + tid];
        demb[r * E + tid] = (float)(w * a + via_c + via_x);
    }
}

// loss [1], grad_wb [2] and demb [N M][E] on the device; sim [N M][N] or null.  The caller has checked ge2e_bad_shape.
inline void launch_ge2e_loss(int N, int M, int E, const float* emb, Ge2eScal sc, float* loss, float* grad_wb, float* demb, float* sim, const Ge2eWs& ws,
                             hipStream_t st) {
    MTTS_LAUNCH(ge2e_centroid_kernel, dim3((unsigned)N), dim3(GE2E_THREADS), st, emb, M, E, ws);
    MTTS_LAUNCH(ge2e_row_kernel, dim3((unsigned)(N * M)), dim3(GE2E_THREADS), st, emb, N, M, E, sc, ws, sim);
    MTTS_LAUNCH(ge2e_fold_kernel, dim3(1), dim3(GE2E_THREADS), st, N * M, ws, loss, grad_wb);
    MTTS_LAUNCH(ge2e_grad_kernel, dim3((unsigned)N), dim3(GE2E_THREADS), st, emb, N, M, E, sc, ws, demb);
}

// Trainer rule, the part between the backward pass and Adam: the gradients of w and b are multiplied by `scale` in place, then
// norm[0] = sqrt(sumsq[0] + dw^2 + db^2), the joint L2 norm of every gradient of the step (sumsq: the encoder's term).
__global__ void ge2e_joint_norm_kernel(const float* sumsq, float* grad_wb, float scale, float* norm) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const float dw = grad_wb[0] * scale, db = grad_wb[1] * scale;
        grad_wb[0] = dw;
        grad_wb[1] = db;
        norm[0] = (float)sqrt((double)sumsq[0] + (double)dw * (double)dw + (double)db * (double)db);
    }
}

}  // namespace mtts
