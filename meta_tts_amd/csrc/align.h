// Forced alignment by a flat-start monophone model: one diagonal Gaussian per phone class, Baum-Welch re-estimation in closed form, Viterbi
// to durations.  The first pass of every HMM forced aligner and no more; the definition is this project's
// own (include/mtts.h states it; tests/align_oracle.py restates it in float64 numpy in the same order).  Parity with MFA, Kaldi and HTK is
// UNPINNED, and alignment quality on real speech is not measured.
//
//   emission  b(t, s) = -1/2 sum_f [ (x[t][f] - mu[c][f])^2 (1 / var[c][f]) + log(2 pi var[c][f]) ], c = class of state s; float64, ascending f.
//   lattice   left to right, unit weights: into (t, s) come (t-1, s) stay, (t-1, s-1) advance, (t-1, s-2) skip if state s-1 is optional.
//             Start: state 0, or state 1 if state 0 is optional.  End: state S-1, or S-2 if state S-1 is optional.
//   forward   alpha(t, s) = b(t, s) + logsumexp(stay, advance, skip), logsumexp = m + log(sum exp(. - m)), m the largest term;
//             LL = logsumexp(alpha(T-1, S-1), alpha(T-1, S-2)); beta the mirror image; gamma = exp(alpha + beta - LL).
//   Viterbi   max in place of logsumexp, ties to stay, then advance, then skip; among end states ties to S-1.
//
// Kernels, all LDS + barriers, no wavefront intrinsic and no atomic, so the SIMT emulator runs the same source and an utterance's LL,
// gamma and durations are the same bits alone, in any batch, at any position and under any chunking:
//   * align_emission_kernel: class scores [rows][V] float64 for the packed frames of a chunk.  A workgroup takes 64 frames x 8 classes:
//     the frames are read coalesced into LDS (rows padded to an odd number of floats), the class tile's mu, 1 / var and log(2 pi var)
//     are made once per workgroup and held in LDS (57.6 KB in all); a thread owns one frame and two of the eight classes.
//   * align_sweep_kernel<MAX> — the hot path: a workgroup per utterance, lanes strided over the states, ONE barrier per frame, two
//     rotating float64 rows in LDS (the row written at t is the one read at t + 1), the states' classes and skip flags in LDS beside
//     them (40 KB).  The emission of a lane's first state for frame t + 1 is loaded before frame t's barrier.  One source for both
//     semirings: sum writes alpha to the ragged [sum T S] workspace, max writes a byte per cell of back-pointers ([t][s], so a wavefront's
//     stores are one contiguous run).
//   * align_backward_kernel: the mirror sweep from the last frame; the rows hold b + beta; alpha is overwritten with gamma.
//   * align_backtrack_kernel: a lane per utterance walks the back-pointers and counts the frames of each state.
//   * align_stats_kernel: per state, sum_t gamma, sum_t gamma x and sum_t gamma x^2 in ascending t — per utterance a gamma^T X product
//     with K = T.  A workgroup takes 8 states x all features and streams 32 frames at a time through LDS (x 16 KB, gamma 2 KB);
//     a thread owns one state and up to four features, nine float64 accumulators in registers.
//   * align_fold_kernel: a workgroup per class adds, utterance by utterance in call order, the sum over that utterance's states of the
//     class (ascending s, from zero) to the handle's running sums.  The order does not depend on how the corpus was cut.  It walks the
//     list of the class's states, which the host makes while it stages the chunk; no scan of all states per class.
//   * align_mstep_kernel: mu = sum gamma x / occ, var = max(sum gamma x^2 / occ - mu^2, var_floor g_f); a class below min_occ keeps its values.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "alignplan.h"
#include "devres.h"

namespace mtts {

constexpr int ALIGN_THREADS = 256;
constexpr int ALIGN_EM_ROWS = 64, ALIGN_EM_CLASSES = 8;
constexpr int ALIGN_ST_STATES = 8, ALIGN_ST_FRAMES = 32;

struct AlignUtt {
    int T, S;
    long long row;     // first frame of the utterance in the chunk's feature (and score) rows
    long long state;   // first state in the chunk's class / optional / duration / partial arrays
    long long cell;    // first cell of its T x S block in the alpha / gamma workspace and the back-pointer map
};

__device__ __forceinline__ double align_lse3(double a, double b, double c) {
    double m = a > b ? a : b;
    m = m > c ? m : c;
    if (m == -__builtin_huge_val()) return m;
    return m + log(exp(a - m) + exp(b - m) + exp(c - m));
}
// max with ties to the first: a (0), then b (1), then c (2)
__device__ __forceinline__ double align_max3(double a, double b, double c, unsigned char& from) {
    double best = a;
    from = 0;
    if (b > best) { best = b; from = 1; }
    if (c > best) { best = c; from = 2; }
    return best;
}

__global__ __launch_bounds__(ALIGN_THREADS) void align_emission_kernel(const float* x, long long n_rows, int F, int V, const double* mean, const double* var, double* score) {
    __shared__ float xs[ALIGN_EM_ROWS * (ALIGN_MAX_FEAT + 1)];
    __shared__ double mu[ALIGN_EM_CLASSES * ALIGN_MAX_FEAT], iv[ALIGN_EM_CLASSES * ALIGN_MAX_FEAT], lc[ALIGN_EM_CLASSES * ALIGN_MAX_FEAT];
    const int tid = (int)threadIdx.x, stride = F | 1;
    const long long row0 = (long long)blockIdx.x * ALIGN_EM_ROWS;
    const int c0 = (int)blockIdx.y * ALIGN_EM_CLASSES;
    const int rows = n_rows - row0 < ALIGN_EM_ROWS ? (int)(n_rows - row0) : ALIGN_EM_ROWS, nc = V - c0 < ALIGN_EM_CLASSES ? V - c0 : ALIGN_EM_CLASSES;
    const float* xg = x + row0 * F;
    for (int q = tid; q < rows * F; q += ALIGN_THREADS) xs[(q / F) * stride + q % F] = xg[q];
    for (int q = tid; q < nc * F; q += ALIGN_THREADS) {
        const double v = var[(size_t)c0 * F + q];
        mu[q] = mean[(size_t)c0 * F + q];
        iv[q] = 1.0 / v;
        lc[q] = log(6.283185307179586 * v);
    }
    __syncthreads();
    const int r = tid / 4;
    if (r >= rows) return;
    const float* xr = xs + r * stride;
    for (int c = tid % 4; c < nc; c += 4) {
        const double *m = mu + c * F, *i = iv + c * F, *l = lc + c * F;
        double acc = 0.0;
        for (int f = 0; f < F; ++f) {
            const double d = (double)xr[f] - m[f];
            acc += d * d * i[f] + l[f];
        }
        score[(size_t)(row0 + r) * V + c0 + c] = -0.5 * acc;
    }
}

// MAX = false: alpha -> `alpha`, LL -> end_value.  MAX = true: back-pointers -> `dir`, the Viterbi score -> end_value, its end state -> end_state.
template <bool MAX>
__global__ __launch_bounds__(ALIGN_THREADS) void align_sweep_kernel(const double* score, int V, const AlignUtt* utts, const int* cls, const unsigned char* opt, double* alpha,
                                                                    unsigned char* dir, double* end_value, int* end_state) {
    __shared__ double rows[2][ALIGN_MAX_STATES];
    __shared__ int meta[ALIGN_MAX_STATES];   // class of state s, + 65536 when state s - 1 may be skipped
    const AlignUtt u = utts[blockIdx.x];
    const int tid = (int)threadIdx.x, T = u.T, S = u.S;
    const int* c = cls + u.state;
    const unsigned char* o = opt + u.state;
    const double* b = score + (size_t)u.row * V;
    const double ninf = -__builtin_huge_val();
    double *prev = rows[0], *cur = rows[1];
    for (int s = tid; s < S; s += ALIGN_THREADS) {
        meta[s] = c[s] + (s > 1 && o[s - 1] ? 65536 : 0);
        const double v = s == 0 || (s == 1 && o[0]) ? b[c[s]] : ninf;
        prev[s] = v;
        if (MAX) dir[u.cell + s] = 0; else alpha[u.cell + s] = v;
    }
    const int c_first = tid < S ? c[tid] : 0;
    double b_first = tid < S && T > 1 ? b[(size_t)V + c_first] : 0.0;   // the emission of state `tid` for the frame about to be swept
    __syncthreads();
    for (int t = 1; t < T; ++t) {
        const double* bt = b + (size_t)t * V;
        const double b_next = tid < S && t + 1 < T ? bt[(size_t)V + c_first] : 0.0;
        const size_t at = (size_t)u.cell + (size_t)t * S;
        for (int s = tid; s < S; s += ALIGN_THREADS) {
            const int m = meta[s];
            const double stay = prev[s], adv = s > 0 ? prev[s - 1] : ninf, skip = m >= 65536 ? prev[s - 2] : ninf;
            const double e = s == tid ? b_first : bt[m & 65535];
            if (MAX) {
                unsigned char from;
                cur[s] = e + align_max3(stay, adv, skip, from);
                dir[at + s] = from;
            } else {
                const double a = e + align_lse3(stay, adv, skip);
                cur[s] = a;
                alpha[at + s] = a;
            }
        }
        b_first = b_next;
        __syncthreads();
        double* sw = prev;
        prev = cur;
        cur = sw;
    }
    if (tid == 0) {
        const double last = prev[S - 1], before = S > 1 && o[S - 1] ? prev[S - 2] : ninf;
        if (MAX) {
            end_value[blockIdx.x] = before > last ? before : last;
            end_state[blockIdx.x] = before > last ? S - 2 : S - 1;
        } else {
            end_value[blockIdx.x] = align_lse3(last, before, ninf);
        }
    }
}

// alpha in, gamma out (in place); the rows hold e(t, s) = b(t, s) + beta(t, s)
__global__ __launch_bounds__(ALIGN_THREADS) void align_backward_kernel(const double* score, int V, const AlignUtt* utts, const int* cls, const unsigned char* opt,
                                                                       const double* ll, double* alpha) {
    __shared__ double rows[2][ALIGN_MAX_STATES];
    __shared__ int meta[ALIGN_MAX_STATES];   // class of state s, + 65536 when state s + 1 may be skipped
    const AlignUtt u = utts[blockIdx.x];
    const int tid = (int)threadIdx.x, T = u.T, S = u.S;
    const int* c = cls + u.state;
    const unsigned char* o = opt + u.state;
    const double* b = score + (size_t)u.row * V;
    const double ninf = -__builtin_huge_val(), LL = ll[blockIdx.x];
    double *prev = rows[0], *cur = rows[1];
    const size_t last = (size_t)u.cell + (size_t)(T - 1) * S;
    for (int s = tid; s < S; s += ALIGN_THREADS) {
        meta[s] = c[s] + (s + 2 < S && o[s + 1] ? 65536 : 0);
        const double beta = s == S - 1 || (s == S - 2 && o[S - 1]) ? 0.0 : ninf;
        prev[s] = b[(size_t)(T - 1) * V + c[s]] + beta;
        alpha[last + s] = exp(alpha[last + s] + beta - LL);
    }
    const int c_first = tid < S ? c[tid] : 0;
    double b_first = tid < S && T > 1 ? b[(size_t)(T - 2) * V + c_first] : 0.0;
    __syncthreads();
    for (int t = T - 2; t >= 0; --t) {
        const double* bt = b + (size_t)t * V;
        const double b_next = tid < S && t > 0 ? b[(size_t)(t - 1) * V + c_first] : 0.0;
        const size_t at = (size_t)u.cell + (size_t)t * S;
        for (int s = tid; s < S; s += ALIGN_THREADS) {
            const int m = meta[s];
            const double beta = align_lse3(prev[s], s + 1 < S ? prev[s + 1] : ninf, m >= 65536 ? prev[s + 2] : ninf);
            cur[s] = (s == tid ? b_first : bt[m & 65535]) + beta;
            alpha[at + s] = exp(alpha[at + s] + beta - LL);
        }
        b_first = b_next;
        __syncthreads();
        double* sw = prev;
        prev = cur;
        cur = sw;
    }
}

__global__ __launch_bounds__(64) void align_backtrack_kernel(const AlignUtt* utts, int n_utts, const unsigned char* dir, const int* end_state, int* dur) {
    const int p = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (p >= n_utts) return;
    const AlignUtt u = utts[p];
    int* d = dur + u.state;
    for (int s = 0; s < u.S; ++s) d[s] = 0;
    int s = end_state[p];
    for (int t = u.T - 1; t > 0; --t) {
        d[s] += 1;
        s -= (int)dir[(size_t)u.cell + (size_t)t * u.S + s];
    }
    d[s] += 1;
}

// part [states][1 + 2 F]: occ, sum gamma x [F], sum gamma x^2 [F] of each state, ascending t
__global__ __launch_bounds__(ALIGN_THREADS) void align_stats_kernel(const float* x, int F, const AlignUtt* utts, const double* gamma, double* part) {
    __shared__ float xs[ALIGN_ST_FRAMES * ALIGN_MAX_FEAT];
    __shared__ double gs[ALIGN_ST_FRAMES * ALIGN_ST_STATES];
    const AlignUtt u = utts[blockIdx.y];
    const int s0 = (int)blockIdx.x * ALIGN_ST_STATES;
    if (s0 >= u.S) return;
    const int tid = (int)threadIdx.x, sl = tid / 32, fl = tid % 32, s = s0 + sl;
    double occ = 0.0, sx[4] = {0.0, 0.0, 0.0, 0.0}, sxx[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t0 = 0; t0 < u.T; t0 += ALIGN_ST_FRAMES) {
        const int nt = u.T - t0 < ALIGN_ST_FRAMES ? u.T - t0 : ALIGN_ST_FRAMES;
        const float* xg = x + (size_t)(u.row + t0) * F;
        for (int q = tid; q < nt * F; q += ALIGN_THREADS) xs[q] = xg[q];
        {
            const int tt = tid / ALIGN_ST_STATES, k = tid % ALIGN_ST_STATES;
            gs[tid] = tt < nt && s0 + k < u.S ? gamma[(size_t)u.cell + (size_t)(t0 + tt) * u.S + s0 + k] : 0.0;
        }
        __syncthreads();
        for (int tt = 0; tt < nt; ++tt) {
            const double g = gs[tt * ALIGN_ST_STATES + sl];
            occ += g;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int f = fl + 32 * k;
                if (f < F) {
                    const double v = (double)xs[tt * F + f];
                    sx[k] += g * v;
                    sxx[k] += g * (v * v);
                }
            }
        }
        __syncthreads();
    }
    if (s >= u.S) return;
    double* o = part + (size_t)(u.state + s) * (1 + 2 * F);
    if (fl == 0) o[0] = occ;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int f = fl + 32 * k;
        if (f < F) {
            o[1 + f] = sx[k];
            o[1 + F + f] = sxx[k];
        }
    }
}

// acc [V][W] += per utterance, in order, the sum over its states of class v (ascending s, from zero).  The states of class v are entries
// [list_start[v], list_start[v + 1]) of `list`, in chunk order (the host makes the lists while it stages the chunk); an entry is the
// state's index in the chunk, or -(index + 1) for the first state of the class in its utterance, where the utterance's sum starts.
__global__ __launch_bounds__(ALIGN_THREADS) void align_fold_kernel(const int* list_start, const int* list, const double* part, int W, double* acc) {
    const int v = (int)blockIdx.x, lo = list_start[v], hi = list_start[v + 1];
    if (lo == hi) return;
    for (int j = (int)threadIdx.x; j < W; j += ALIGN_THREADS) {
        double a = acc[(size_t)v * W + j], sum = 0.0;
        for (int k = lo; k < hi; ++k) {
            int s = list[k];
            if (s < 0) {
                if (k > lo) a += sum;
                sum = 0.0;
                s = -(s + 1);
            }
            sum += part[(size_t)s * W + j];
        }
        acc[(size_t)v * W + j] = a + sum;
    }
}

__global__ __launch_bounds__(ALIGN_THREADS) void align_mstep_kernel(const double* acc, int V, int F, const double* global_var, double var_floor, double min_occ, double* mean,
                                                                    double* var) {
    const int q = (int)blockIdx.x * ALIGN_THREADS + (int)threadIdx.x;
    if (q >= V * F) return;
    const int v = q / F, f = q % F, W = 1 + 2 * F;
    const double occ = acc[(size_t)v * W];
    if (!(occ >= min_occ)) return;
    const double m = acc[(size_t)v * W + 1 + f] / occ, floor = var_floor * global_var[f];
    const double s2 = acc[(size_t)v * W + 1 + F + f] / occ - m * m;
    mean[q] = m;
    var[q] = s2 > floor ? s2 : floor;
}

class Align {
public:
    DevHeap heap;
    hipStream_t stream = nullptr;
    std::string last_error;
    AlignLimits lim;
    bool have_model = false, in_em = false;
    double var_floor = 0.01, min_occ = 1e-3, total_ll = 0.0;
    double *mean = nullptr, *var = nullptr, *gvar = nullptr, *acc = nullptr;
    DevBuf<float> x;
    DevBuf<double> score, alpha, ll, part;
    DevBuf<unsigned char> dir, opt;
    DevBuf<int> cls, end_state, dur, fold_start, fold_list;
    DevBuf<AlignUtt> utts;
    std::vector<AlignUtt> h_utts;
    std::vector<int> h_fold_start, h_fold_list, h_fold_seen;
    bool launched_any = false;   // a call got as far as its first launch (a failure after that leaves partial statistics behind)

    int err(const std::string& s) { last_error = s; return -1; }
    int width() const { return 1 + 2 * lim.n_feat; }
    size_t model_count() const { return (size_t)lim.n_classes * lim.n_feat; }

    int init(const AlignLimits& l) {
        const std::string e = align_check_limits(l);
        if (!e.empty()) return err(e);
        lim = l;
        const size_t n = model_count() * sizeof(double);
        if (heap.alloc(mean, n) != hipSuccess || heap.alloc(var, n) != hipSuccess || heap.alloc(gvar, (size_t)l.n_feat * sizeof(double)) != hipSuccess ||
            heap.alloc(acc, (size_t)l.n_classes * width() * sizeof(double)) != hipSuccess)
            return err("mtts_align_create: out of device memory (model)");
        return 0;
    }

    int check_launch(const std::string& who) {
        const hipError_t e = hipGetLastError();
        return e == hipSuccess ? 0 : err(who + "kernel launch failed: " + hipGetErrorString(e));
    }

    int set_floor(double floor, double occ) {
        const std::string who = "mtts_align_set_floor: ";
        if (!std::isfinite(floor) || !(floor > 0.0)) return err(who + "var_floor must be finite and > 0");
        if (!std::isfinite(occ) || !(occ > 0.0)) return err(who + "min_occ must be finite and > 0");
        var_floor = floor;
        min_occ = occ;
        return 0;
    }

    int set_model(const double* m, const double* v, const double* g, const std::string& who = "mtts_align_set_model: ") {
        const std::string e = align_check_model(who, lim, m, v, g);
        if (!e.empty()) return err(e);
        have_model = false;
        in_em = false;
        DEV_CHECK(hipMemcpyAsync(mean, m, model_count() * sizeof(double), hipMemcpyHostToDevice, stream));
        DEV_CHECK(hipMemcpyAsync(var, v, model_count() * sizeof(double), hipMemcpyHostToDevice, stream));
        DEV_CHECK(hipMemcpyAsync(gvar, g, (size_t)lim.n_feat * sizeof(double), hipMemcpyHostToDevice, stream));
        DEV_CHECK(hipStreamSynchronize(stream));
        have_model = true;
        return 0;
    }

    int get_model(double* m, double* v, double* g) {
        const std::string who = "mtts_align_get_model: ";
        if (!have_model) return err(who + "no model loaded (mtts_align_set_model or mtts_align_flat_start)");
        if (!m || !v || !g) return err(who + "NULL mean, var or global_var");
        DEV_CHECK(hipMemcpyAsync(m, mean, model_count() * sizeof(double), hipMemcpyDeviceToHost, stream));
        DEV_CHECK(hipMemcpyAsync(v, var, model_count() * sizeof(double), hipMemcpyDeviceToHost, stream));
        DEV_CHECK(hipMemcpyAsync(g, gvar, (size_t)lim.n_feat * sizeof(double), hipMemcpyDeviceToHost, stream));
        DEV_CHECK(hipStreamSynchronize(stream));
        return 0;
    }

    // Every class = the mean and variance of all frames: float64 on the host, two passes, rows in call order (run once per fit; not a hot path).
    int flat_start(int n_utts, const int* n_frames, const float* xh) {
        const std::string who = "mtts_align_flat_start: ";
        long long rows = 0;
        const std::string e = align_check_frames(who, lim, n_utts, n_frames, xh, rows);
        if (!e.empty()) return err(e);
        const int F = lim.n_feat;
        std::vector<double> m((size_t)F, 0.0), g((size_t)F, 0.0);
        for (long long r = 0; r < rows; ++r)
            for (int f = 0; f < F; ++f) m[(size_t)f] += (double)xh[r * F + f];
        for (int f = 0; f < F; ++f) m[(size_t)f] /= (double)rows;
        for (long long r = 0; r < rows; ++r)
            for (int f = 0; f < F; ++f) {
                const double d = (double)xh[r * F + f] - m[(size_t)f];
                g[(size_t)f] += d * d;
            }
        for (int f = 0; f < F; ++f) {
            g[(size_t)f] /= (double)rows;
            if (!(g[(size_t)f] > 0.0)) return err(who + "feature " + std::to_string(f) + " is constant over all frames: its variance must be > 0");
        }
        std::vector<double> mm(model_count()), vv(model_count());
        for (size_t k = 0; k < model_count(); ++k) { mm[k] = m[k % (size_t)F]; vv[k] = g[k % (size_t)F]; }
        return set_model(mm.data(), vv.data(), g.data(), who);
    }

    // ---- a call's chunks -----------------------------------------------------------------------------------------------------------
    struct Need { bool sum, stats, viterbi; };

    int reserve(const std::vector<AlignChunk>& chunks, Need need) {
        AlignChunk top;   // every buffer is reserved for the largest chunk before anything runs
        for (const AlignChunk& c : chunks) {
            top.count = std::max(top.count, c.count);
            top.cells = std::max(top.cells, c.cells);
            top.rows = std::max(top.rows, c.rows);
            top.states = std::max(top.states, c.states);
        }
        if (grow(heap, x, (size_t)top.rows * lim.n_feat, stream, "feature rows", last_error) || grow(heap, score, (size_t)top.rows * lim.n_classes, stream, "class scores", last_error) ||
            grow(heap, utts, (size_t)top.count, stream, "utterance table", last_error) || grow(heap, cls, (size_t)top.states, stream, "state classes", last_error) ||
            grow(heap, opt, (size_t)top.states, stream, "optional flags", last_error) || grow(heap, ll, (size_t)top.count, stream, "end values", last_error) ||
            (need.sum && grow(heap, alpha, (size_t)top.cells, stream, "alpha / gamma workspace", last_error)) ||
            (need.stats && (grow(heap, part, (size_t)top.states * width(), stream, "per-state statistics", last_error) ||
                            grow(heap, fold_start, (size_t)lim.n_classes + 1, stream, "class list offsets", last_error) ||
                            grow(heap, fold_list, (size_t)top.states, stream, "class lists", last_error))) ||
            (need.viterbi && (grow(heap, dir, (size_t)top.cells, stream, "back-pointers", last_error) || grow(heap, end_state, (size_t)top.count, stream, "end states", last_error) ||
                              grow(heap, dur, (size_t)top.states, stream, "durations", last_error))))
            return -1;
        return 0;
    }

    // uploads chunk c (whose first frame / state in the caller's packed arrays are row0 / state0) and launches the emission kernel
    int stage(const AlignChunk& c, const int* n_frames, const int* n_states, const int* classes, const unsigned char* optional, const float* xh, long long row0, long long state0) {
        h_utts.resize((size_t)c.count);
        long long row = 0, state = 0, cell = 0;
        for (int q = 0; q < c.count; ++q) {
            const int T = n_frames[c.first + q], S = n_states[c.first + q];
            h_utts[(size_t)q] = AlignUtt{T, S, row, state, cell};
            row += T;
            state += S;
            cell += (long long)T * S;
        }
        DEV_CHECK(hipMemcpyAsync(x.p, xh + row0 * lim.n_feat, (size_t)c.rows * lim.n_feat * sizeof(float), hipMemcpyHostToDevice, stream));
        DEV_CHECK(hipMemcpyAsync(utts.p, h_utts.data(), (size_t)c.count * sizeof(AlignUtt), hipMemcpyHostToDevice, stream));
        DEV_CHECK(hipMemcpyAsync(cls.p, classes + state0, (size_t)c.states * sizeof(int), hipMemcpyHostToDevice, stream));
        DEV_CHECK(hipMemcpyAsync(opt.p, optional + state0, (size_t)c.states, hipMemcpyHostToDevice, stream));
        const dim3 grid((unsigned)((c.rows + ALIGN_EM_ROWS - 1) / ALIGN_EM_ROWS), (unsigned)((lim.n_classes + ALIGN_EM_CLASSES - 1) / ALIGN_EM_CLASSES));
        launched_any = true;
        MTTS_LAUNCH(align_emission_kernel, grid, dim3(ALIGN_THREADS), stream, (const float*)x.p, c.rows, lim.n_feat, lim.n_classes, (const double*)mean, (const double*)var, score.p);
        return 0;
    }

    // The fold's input: per class the chunk's states of that class, in chunk order (a counting sort, so the order within a class is the
    // order of the states), the first of each utterance marked by -(index + 1).
    int stage_fold(const AlignChunk& c, const int* classes, long long state0) {
        const int V = lim.n_classes;
        h_fold_start.assign((size_t)V + 1, 0);
        h_fold_list.resize((size_t)c.states);
        h_fold_seen.assign((size_t)V, -1);   // the last utterance in which the class was met
        for (long long k = 0; k < c.states; ++k) h_fold_start[(size_t)classes[state0 + k] + 1] += 1;
        for (int v = 0; v < V; ++v) h_fold_start[(size_t)v + 1] += h_fold_start[(size_t)v];
        std::vector<int> next(h_fold_start.begin(), h_fold_start.end() - 1);
        for (int q = 0; q < c.count; ++q) {
            const AlignUtt& u = h_utts[(size_t)q];
            for (int s = 0; s < u.S; ++s) {
                const int k = (int)u.state + s, v = classes[state0 + k];
                h_fold_list[(size_t)next[(size_t)v]++] = h_fold_seen[(size_t)v] == q ? k : -(k + 1);
                h_fold_seen[(size_t)v] = q;
            }
        }
        DEV_CHECK(hipMemcpyAsync(fold_start.p, h_fold_start.data(), ((size_t)V + 1) * sizeof(int), hipMemcpyHostToDevice, stream));
        DEV_CHECK(hipMemcpyAsync(fold_list.p, h_fold_list.data(), (size_t)c.states * sizeof(int), hipMemcpyHostToDevice, stream));
        return 0;
    }

    void launch_forward_backward(const AlignChunk& c) {
        const dim3 grid((unsigned)c.count), block(ALIGN_THREADS);
        MTTS_LAUNCH(align_sweep_kernel<false>, grid, block, stream, (const double*)score.p, lim.n_classes, (const AlignUtt*)utts.p, (const int*)cls.p, (const unsigned char*)opt.p,
                    alpha.p, (unsigned char*)nullptr, ll.p, (int*)nullptr);
        MTTS_LAUNCH(align_backward_kernel, grid, block, stream, (const double*)score.p, lim.n_classes, (const AlignUtt*)utts.p, (const int*)cls.p, (const unsigned char*)opt.p,
                    (const double*)ll.p, alpha.p);
    }

    // gamma_out == nullptr: an E step (statistics folded into acc); else posteriors only
    int forward_backward(const std::string& who, int n_utts, const int* n_frames, const int* n_states, const int* classes, const unsigned char* optional, const float* xh,
                         double* ll_out, double* gamma_out) {
        const std::string e = align_validate(who, lim, have_model, n_utts, n_frames, n_states, classes, optional, xh);
        if (!e.empty()) return err(e);
        if (!ll_out) return err(who + "NULL ll_out");
        const std::vector<AlignChunk> chunks = align_plan_chunks(lim, n_utts, n_frames, n_states);
        if (reserve(chunks, Need{true, gamma_out == nullptr, false})) return -1;
        long long row0 = 0, state0 = 0, cell0 = 0;
        for (const AlignChunk& c : chunks) {
            if (stage(c, n_frames, n_states, classes, optional, xh, row0, state0)) return -1;
            launch_forward_backward(c);
            if (gamma_out) {
                DEV_CHECK(hipMemcpyAsync(gamma_out + cell0, alpha.p, (size_t)c.cells * sizeof(double), hipMemcpyDeviceToHost, stream));
            } else {
                const dim3 grid((unsigned)((c.longest_states + ALIGN_ST_STATES - 1) / ALIGN_ST_STATES), (unsigned)c.count);
                MTTS_LAUNCH(align_stats_kernel, grid, dim3(ALIGN_THREADS), stream, (const float*)x.p, lim.n_feat, (const AlignUtt*)utts.p, (const double*)alpha.p, part.p);
                if (stage_fold(c, classes, state0)) return -1;
                MTTS_LAUNCH(align_fold_kernel, dim3((unsigned)lim.n_classes), dim3(ALIGN_THREADS), stream, (const int*)fold_start.p, (const int*)fold_list.p, (const double*)part.p,
                            width(), acc);
            }
            if (check_launch(who)) return -1;
            DEV_CHECK(hipMemcpyAsync(ll_out + c.first, ll.p, (size_t)c.count * sizeof(double), hipMemcpyDeviceToHost, stream));
            DEV_CHECK(hipStreamSynchronize(stream));   // (the staging vector and the device buffers are reused by the next chunk)
            row0 += c.rows;
            state0 += c.states;
            cell0 += c.cells;
        }
        return 0;
    }

    int em_begin() {
        const std::string who = "mtts_align_em_begin: ";
        if (!have_model) return err(who + "no model loaded (mtts_align_set_model or mtts_align_flat_start)");
        DEV_CHECK(hipMemsetAsync(acc, 0, (size_t)lim.n_classes * width() * sizeof(double), stream));
        total_ll = 0.0;
        in_em = true;
        return 0;
    }

    int em_accumulate(int n_utts, const int* n_frames, const int* n_states, const int* classes, const unsigned char* optional, const float* xh, double* ll_out) {
        const std::string who = "mtts_align_em_accumulate: ";
        if (!in_em) return err(who + "no iteration is open (mtts_align_em_begin)");
        launched_any = false;
        if (forward_backward(who, n_utts, n_frames, n_states, classes, optional, xh, ll_out, nullptr)) {
            // a refusal (nothing launched) leaves the iteration as it was; a failure after the first launch may have folded part of the
            // call into the sums: the iteration is closed, so that no em_finish makes a model from a partial corpus
            if (launched_any) {
                in_em = false;
                last_error += " (the iteration is closed: its statistics may hold part of this call; start again with mtts_align_em_begin)";
            }
            return -1;
        }
        for (int p = 0; p < n_utts; ++p) total_ll += ll_out[p];
        return 0;
    }

    int em_finish(double* total_out) {
        const std::string who = "mtts_align_em_finish: ";
        if (!in_em) return err(who + "no iteration is open (mtts_align_em_begin)");
        if (!total_out) return err(who + "NULL total_ll_out");
        const int n = lim.n_classes * lim.n_feat;
        MTTS_LAUNCH(align_mstep_kernel, dim3((unsigned)((n + ALIGN_THREADS - 1) / ALIGN_THREADS)), dim3(ALIGN_THREADS), stream, (const double*)acc, lim.n_classes, lim.n_feat,
                    (const double*)gvar, var_floor, min_occ, mean, var);
        if (check_launch(who)) return -1;
        DEV_CHECK(hipStreamSynchronize(stream));
        in_em = false;
        *total_out = total_ll;
        return 0;
    }

    int posteriors(int n_utts, const int* n_frames, const int* n_states, const int* classes, const unsigned char* optional, const float* xh, double* ll_out, double* gamma_out) {
        const std::string who = "mtts_align_posteriors: ";
        if (!gamma_out) return err(who + "NULL gamma_out");
        return forward_backward(who, n_utts, n_frames, n_states, classes, optional, xh, ll_out, gamma_out);
    }

    int align(int n_utts, const int* n_frames, const int* n_states, const int* classes, const unsigned char* optional, const float* xh, int* dur_out, double* score_out) {
        const std::string who = "mtts_align_align: ";
        const std::string e = align_validate(who, lim, have_model, n_utts, n_frames, n_states, classes, optional, xh);
        if (!e.empty()) return err(e);
        if (!dur_out || !score_out) return err(who + "NULL durations_out or score_out");
        const std::vector<AlignChunk> chunks = align_plan_chunks(lim, n_utts, n_frames, n_states);
        if (reserve(chunks, Need{false, false, true})) return -1;
        long long row0 = 0, state0 = 0;
        for (const AlignChunk& c : chunks) {
            if (stage(c, n_frames, n_states, classes, optional, xh, row0, state0)) return -1;
            MTTS_LAUNCH(align_sweep_kernel<true>, dim3((unsigned)c.count), dim3(ALIGN_THREADS), stream, (const double*)score.p, lim.n_classes, (const AlignUtt*)utts.p,
                        (const int*)cls.p, (const unsigned char*)opt.p, (double*)nullptr, dir.p, ll.p, end_state.p);
            MTTS_LAUNCH(align_backtrack_kernel, dim3((unsigned)((c.count + 63) / 64)), dim3(64), stream, (const AlignUtt*)utts.p, c.count, (const unsigned char*)dir.p,
                        (const int*)end_state.p, dur.p);
            if (check_launch(who)) return -1;
            DEV_CHECK(hipMemcpyAsync(dur_out + state0, dur.p, (size_t)c.states * sizeof(int), hipMemcpyDeviceToHost, stream));
            DEV_CHECK(hipMemcpyAsync(score_out + c.first, ll.p, (size_t)c.count * sizeof(double), hipMemcpyDeviceToHost, stream));
            DEV_CHECK(hipStreamSynchronize(stream));
            row0 += c.rows;
            state0 += c.states;
        }
        return 0;
    }
};

}  // namespace mtts
