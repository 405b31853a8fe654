// Exact t-SNE of d-vectors on the device: the numerical step of the reference's evaluation/visualize.py (VisualizeDvector.tsne,
// visualize.py:56-71: TSNE(n_components=2, perplexity=40, n_iter=300) over the concatenated d-vectors of five modes).
//
// The reference's call is sklearn's Barnes-Hut approximation on the CPU.  The job sizes are N = 3 040 (LibriTTS) and 8 640 (VCTK) points
// of dim 256; the exact algorithm is N^2 pair terms per iteration, which this device sweeps in well under a millisecond, so what runs
// here is the EXACT gradient (sklearn's method="exact": _joint_probabilities, _kl_divergence, _gradient_descent of
// sklearn/manifold/_t_sne.py and _binary_search_perplexity of _utils.pyx, restated in float64 numpy in tests/tsne_oracle.py).
//
// One buffer of n^2 float32 holds, one after the other, the squared distances, the conditional rows and the joint P (a workgroup of the
// perplexity search reads its row into LDS before it writes that row back, and no other workgroup reads it; the symmetrise pass gives
// every unordered pair to one thread).  Kernels, all LDS + barriers, no wavefront intrinsic and no atomic, so the SIMT emulator runs
// the same source and every result is bit-identical from call to call:
//   * tsne_sqdist_kernel: D[i][j] = sum_k (x_ik - x_jk)^2, the direct form (no cancellation), 16 x 16 outputs per workgroup with 64
//     dims of both row blocks in LDS.  Differences and the sum are fp64 in ascending k (a difference of two fp32 values is exact
//     there), rounded once to fp32 as sklearn's `distances.astype(np.float32)` does.  (a-b)^2 and (b-a)^2 are the same bits, so D is
//     symmetric bit for bit with an exact zero diagonal.
//   * tsne_perplexity_kernel: one workgroup per row, the row's distances in LDS.  sklearn's _binary_search_perplexity: beta from 1, at
//     most 100 steps, tolerance float(1e-5) on H - log(perplexity), double then bisect, a row sum of 0 replaced by float(1e-8), j = i
//     excluded.  exp, the sums and H in fp64; the sums in a fixed order (a thread's j = tid, tid + 256, ... ascending, 16 groups of 16
//     threads ascending, the 16 group sums ascending).  Emits the conditional row (fp32), the beta the row was evaluated at, and the
//     fp64 sum of the emitted fp32 values.
//   * tsne_symmetrise_kernel: P = max((C + C^T) / max(sum, eps), eps), eps = 2^-52, diagonal 0; sum = 2 x the row sums folded in row order.
//   * tsne_pair_kernel — the hot kernel, once per iteration: with num = 1 / (1 + |y_i - y_j|^2), per row i in one sweep
//     sum_j P_ij num (y_i - y_j), sum_j num^2 (y_i - y_j), the row's share of Z = sum num, and the row's smallest num.  Z is not needed
//     before the sweep.  A wavefront owns two rows and streams them coalesced along j (lane = j mod 64); a workgroup (8 rows) stages
//     Y in LDS 2048 points at a time.  fp32 throughout with IEEE division: a lane adds its terms in ascending j, then 4 groups of 16
//     lanes ascending, then the 4 group sums.  Bound by P's bytes, n^2 x 4 B per iteration.
//   * tsne_kl_kernel (on request; a logarithm per pair): row partials of sum_j P' log(max(P', eps) / max(num / Z, eps)), P' =
//     exaggeration x P, in fp64, one wavefront per row.
//   * tsne_grad_kernel: a thread per row.  Z = the row shares folded in fp64 in row order; grad = 4 (exaggeration x attractive -
//     repulsive / Z), formed in fp64 and rounded once to fp32.  sklearn floors Q = max(num / Z, eps) inside the gradient: the pair
//     pass cannot (Z is not known yet), so it records the row's smallest num, and a row with min num < eps Z — an embedding more than
//     about 1e6 wide; none in practice — recomputes its repulsive sum here, serially, with the floor applied pair by pair.  That
//     reads every row's Y, which is why the gradient is a launch of its own: all gradients exist before any Y moves.
//   * tsne_apply_kernel: sklearn's _gradient_descent rule in fp32 from that gradient: inc = update x grad < 0, gains += 0.2 on inc,
//     x 0.8 elsewhere, floored at min_gain, grad x gains, update = momentum x update - learning_rate x grad, Y += update; and the
//     row's |grad x gains|^2 in fp64 (the gradient norm sklearn tests is taken AFTER its in-place `grad *= gains`).
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "devres.h"

namespace mtts {

constexpr int TSNE_THREADS = 256;
constexpr int TSNE_MAX_POINTS = 12288;   // a row of distances in LDS: 48 KB; P at the cap: 604 MB
constexpr int TSNE_MAX_DIM = 65536;
constexpr int TSNE_ROWS = 8;             // rows per workgroup of the pair pass: two per wavefront
constexpr int TSNE_YCHUNK = 2048;        // points of Y staged in LDS at a time (16 KB)
constexpr int TSNE_ACC = 6;              // per row: attractive x, y; repulsive x, y; share of Z; smallest num
constexpr double TSNE_EPS = 2.220446049250313e-16;   // np.finfo(np.double).eps: sklearn's MACHINE_EPSILON

// sum of v(0 .. n-1) for every thread of the workgroup: thread t adds its ceil(n / 256) consecutive values in ascending order, then
// every thread adds the 256 partial sums in ascending order.  Two barriers; red: 256 doubles.
template <class F>
__device__ __forceinline__ double tsne_block_fold(int n, double* red, F v) {
    const int tid = (int)threadIdx.x, per = (n + TSNE_THREADS - 1) / TSNE_THREADS;
    const int lo = tid * per, hi = lo + per < n ? lo + per : n;
    double s = 0.0;
    for (int k = lo; k < hi; ++k) s += v(k);
    red[tid] = s;
    __syncthreads();
    double t = 0.0;
    for (int k = 0; k < TSNE_THREADS; ++k) t += red[k];
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(TSNE_THREADS) void tsne_sqdist_kernel(const float* X, int n, int dim, float* D) {
    __shared__ float xi[16][65], xj[16][65];
    const int tid = (int)threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int i0 = (int)blockIdx.y * 16, j0 = (int)blockIdx.x * 16;
    double acc = 0.0;
    for (int k0 = 0; k0 < dim; k0 += 64) {
        __syncthreads();
        for (int q = tid; q < 16 * 64; q += TSNE_THREADS) {
            const int r = q >> 6, c = q & 63;
            const bool in = k0 + c < dim;
            xi[r][c] = in && i0 + r < n ? X[(size_t)(i0 + r) * dim + k0 + c] : 0.f;
            xj[r][c] = in && j0 + r < n ? X[(size_t)(j0 + r) * dim + k0 + c] : 0.f;
        }
        __syncthreads();
        for (int k = 0; k < 64; ++k) {
            const double d = (double)xi[ty][k] - (double)xj[tx][k];
            acc += d * d;
        }
    }
    if (i0 + ty < n && j0 + tx < n) D[(size_t)(i0 + ty) * n + j0 + tx] = (float)acc;
}

// Row blockIdx.x of DP: squared distances in, the conditional probabilities out (in place).
__global__ __launch_bounds__(TSNE_THREADS) void tsne_perplexity_kernel(float* DP, int n, double log_perplexity, double* beta_out, double* rowsum) {
    __shared__ float ds[TSNE_MAX_POINTS];
    __shared__ double red[2 * TSNE_THREADS], red2[32];
    const int tid = (int)threadIdx.x, i = (int)blockIdx.x;
    float* row = DP + (size_t)i * n;
    for (int j = tid; j < n; j += TSNE_THREADS) ds[j] = row[j];
    __syncthreads();
    const double tol = (double)1e-5f, tiny = (double)1e-8f;   // (`cdef float` constants in _utils.pyx)
    double beta = 1.0, lo = -__builtin_huge_val(), hi = __builtin_huge_val(), beta_at = 1.0, sum_at = 1.0;
    for (int l = 0; l < 100; ++l) {
        double s = 0.0, sd = 0.0;
        for (int j = tid; j < n; j += TSNE_THREADS)
            if (j != i) {
                const double d = (double)ds[j], p = exp(-d * beta);
                s += p;
                sd += d * p;
            }
        red[tid] = s;
        red[TSNE_THREADS + tid] = sd;
        __syncthreads();
        if (tid < 32) {
            const double* src = red + (tid >> 4) * TSNE_THREADS + (tid & 15) * 16;
            double t = 0.0;
            for (int k = 0; k < 16; ++k) t += src[k];
            red2[tid] = t;
        }
        __syncthreads();
        double S = 0.0, SD = 0.0;
        for (int k = 0; k < 16; ++k) { S += red2[k]; SD += red2[16 + k]; }
        if (S == 0.0) S = tiny;
        const double diff = log(S) + beta * (SD / S) - log_perplexity;
        beta_at = beta;
        sum_at = S;
        if (fabs(diff) <= tol) break;   // (uniform: every thread holds the same sums)
        if (diff > 0.0) {
            lo = beta;
            beta = hi == __builtin_huge_val() ? beta * 2.0 : (beta + hi) / 2.0;
        } else {
            hi = beta;
            beta = lo == -__builtin_huge_val() ? beta / 2.0 : (beta + lo) / 2.0;
        }
    }
    double rs = 0.0;
    for (int j = tid; j < n; j += TSNE_THREADS) {
        const float c = j == i ? 0.f : (float)(exp(-(double)ds[j] * beta_at) / sum_at);
        row[j] = c;
        rs += (double)c;
    }
    red[tid] = rs;
    __syncthreads();
    if (tid < 16) {
        double t = 0.0;
        for (int k = 0; k < 16; ++k) t += red[tid * 16 + k];
        red2[tid] = t;
    }
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int k = 0; k < 16; ++k) t += red2[k];
        rowsum[i] = t;
        beta_out[i] = beta_at;
    }
}

// Workgroup i owns the pairs (i, j > i) and the diagonal element: no element is touched by two workgroups.
__global__ __launch_bounds__(TSNE_THREADS) void tsne_symmetrise_kernel(float* DP, int n, const double* rowsum) {
    __shared__ double red[TSNE_THREADS];
    const double total = 2.0 * tsne_block_fold(n, red, [&](int k) { return rowsum[k]; });
    const double denom = total > TSNE_EPS ? total : TSNE_EPS;
    const int i = (int)blockIdx.x;
    for (int j = i + (int)threadIdx.x; j < n; j += TSNE_THREADS) {
        if (j == i) { DP[(size_t)i * n + i] = 0.f; continue; }
        const double v = ((double)DP[(size_t)i * n + j] + (double)DP[(size_t)j * n + i]) / denom;
        const float p = (float)(v > TSNE_EPS ? v : TSNE_EPS);
        DP[(size_t)i * n + j] = p;
        DP[(size_t)j * n + i] = p;
    }
}

__device__ __forceinline__ void tsne_pair_term(float p, float dx, float dy, bool other, float* a) {
    const float num = 1.f / (1.f + (dx * dx + dy * dy));
    const float w = p * num, q = num * num;
    a[0] += w * dx;
    a[1] += w * dy;
    a[2] += q * dx;
    a[3] += q * dy;
    if (other) {
        a[4] += num;
        a[5] = num < a[5] ? num : a[5];
    }
}

__global__ __launch_bounds__(TSNE_THREADS) void tsne_pair_kernel(const float* P, const float* Y, int n, float* acc) {
    __shared__ float2 ys[TSNE_YCHUNK];   // one 8-byte LDS read per point
    __shared__ float red[4][2 * TSNE_ACC][64];
    __shared__ float red2[4][2 * TSNE_ACC][4];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i0 = (int)blockIdx.x * TSNE_ROWS + wave * 2;
    const int ia = i0 < n ? i0 : n - 1, ib = i0 + 1 < n ? i0 + 1 : n - 1;   // (rows past the end repeat the last one; nothing of theirs is written)
    const float yax = Y[2 * ia], yay = Y[2 * ia + 1], ybx = Y[2 * ib], yby = Y[2 * ib + 1];
    const float* pa = P + (size_t)ia * n;
    const float* pb = P + (size_t)ib * n;
    float a[2 * TSNE_ACC];
    for (int k = 0; k < 2 * TSNE_ACC; ++k) a[k] = k % TSNE_ACC == 5 ? 1.f : 0.f;
    for (int c0 = 0; c0 < n; c0 += TSNE_YCHUNK) {
        const int m = n - c0 < TSNE_YCHUNK ? n - c0 : TSNE_YCHUNK;
        __syncthreads();
        for (int t = tid; t < m; t += TSNE_THREADS) ys[t] = make_float2(Y[2 * (size_t)(c0 + t)], Y[2 * (size_t)(c0 + t) + 1]);
        __syncthreads();
        for (int jj = lane; jj < m; jj += 64) {
            const int j = c0 + jj;
            const float2 yj = ys[jj];
            const float yx = yj.x, yy = yj.y;
            const float p0 = pa[j], p1 = pb[j];
            tsne_pair_term(p0, yax - yx, yay - yy, j != ia, a);
            tsne_pair_term(p1, ybx - yx, yby - yy, j != ib, a + TSNE_ACC);
        }
    }
    for (int k = 0; k < 2 * TSNE_ACC; ++k) red[wave][k][lane] = a[k];
    __syncthreads();
    if (lane < 4 * 2 * TSNE_ACC) {
        const int k = lane >> 2, q = lane & 3;
        const bool is_min = k % TSNE_ACC == 5;
        float t = red[wave][k][16 * q];
        for (int r = 1; r < 16; ++r) {
            const float v = red[wave][k][16 * q + r];
            t = is_min ? (v < t ? v : t) : t + v;
        }
        red2[wave][k][q] = t;
    }
    __syncthreads();
    if (lane < 2 * TSNE_ACC) {
        const bool is_min = lane % TSNE_ACC == 5;
        float t = red2[wave][lane][0];
        for (int r = 1; r < 4; ++r) {
            const float v = red2[wave][lane][r];
            t = is_min ? (v < t ? v : t) : t + v;
        }
        const int row = i0 + lane / TSNE_ACC;
        if (row < n) acc[(size_t)row * TSNE_ACC + lane % TSNE_ACC] = t;
    }
}

__global__ __launch_bounds__(TSNE_THREADS) void tsne_kl_kernel(const float* P, const float* Y, int n, double exaggeration, const float* acc, double* klpart) {
    __shared__ double red[TSNE_THREADS], red2[16];
    const double Z = tsne_block_fold(n, red, [&](int k) { return (double)acc[(size_t)k * TSNE_ACC + 4]; });
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i = (int)blockIdx.x * 4 + wave, ic = i < n ? i : n - 1;
    const double yx = (double)Y[2 * ic], yy = (double)Y[2 * ic + 1];
    double s = 0.0;
    for (int j = lane; j < n; j += 64)
        if (j != ic) {
            const double p = (double)P[(size_t)ic * n + j] * exaggeration;
            const double dx = yx - (double)Y[2 * j], dy = yy - (double)Y[2 * j + 1];
            const double num = 1.0 / (1.0 + (dx * dx + dy * dy));
            const double qz = num / Z, q = qz > TSNE_EPS ? qz : TSNE_EPS;
            s += p * log((p > TSNE_EPS ? p : TSNE_EPS) / q);
        }
    red[tid] = s;
    __syncthreads();
    if (lane < 4) {
        double t = 0.0;
        for (int r = 0; r < 16; ++r) t += red[wave * 64 + lane * 16 + r];
        red2[wave * 4 + lane] = t;
    }
    __syncthreads();
    if (lane == 0 && i < n) klpart[i] = ((red2[wave * 4] + red2[wave * 4 + 1]) + red2[wave * 4 + 2]) + red2[wave * 4 + 3];
}

struct TsneStep {
    float momentum, learning_rate, min_gain;
};

// grad[i] = 4 (exaggeration x attractive_i - sum_j Q_ij num_ij (y_i - y_j)) for every row, from the sweep's sums.  A launch of its own in
// front of the step: a row on Q's floor reads every other row's Y here, so nothing may move Y until all gradients are formed.
__global__ __launch_bounds__(TSNE_THREADS) void tsne_grad_kernel(const float* Y, int n, double exaggeration, const float* acc, float* grad) {
    __shared__ double red[TSNE_THREADS];
    const double Z = tsne_block_fold(n, red, [&](int k) { return (double)acc[(size_t)k * TSNE_ACC + 4]; });
    const int i = (int)blockIdx.x * TSNE_THREADS + (int)threadIdx.x;
    if (i >= n) return;
    const float* a = acc + (size_t)i * TSNE_ACC;
    double qx = (double)a[2] / Z, qy = (double)a[3] / Z;
    // A pair of this row sits on Q's floor: the sum again, pair by pair.  One thread walks all n points, so a floored row holds its
    // workgroup for n dependent steps (about 8 640 at the largest job): acceptable only because it needs an embedding about 1e6 wide.
    if ((double)a[5] < TSNE_EPS * Z) {
        const float yx = Y[2 * i], yy = Y[2 * i + 1];
        qx = qy = 0.0;
        for (int j = 0; j < n; ++j) {
            if (j == i) continue;
            const float dx = yx - Y[2 * j], dy = yy - Y[2 * j + 1];
            const float num = 1.f / (1.f + (dx * dx + dy * dy));
            const double qz = (double)num / Z, q = (qz > TSNE_EPS ? qz : TSNE_EPS) * (double)num;
            qx += q * (double)dx;
            qy += q * (double)dy;
        }
    }
    grad[2 * i] = (float)(4.0 * (exaggeration * (double)a[0] - qx));
    grad[2 * i + 1] = (float)(4.0 * (exaggeration * (double)a[1] - qy));
}

// One descent step from `grad`, an element per thread pair (a thread per row): sklearn's gains / momentum rule in fp32.
__global__ __launch_bounds__(TSNE_THREADS) void tsne_apply_kernel(float* Y, float* U, float* G, int n, TsneStep s, const float* grad, double* gnpart) {
    const int i = (int)blockIdx.x * TSNE_THREADS + (int)threadIdx.x;
    if (i >= n) return;
    double gn = 0.0;
    for (int c = 0; c < 2; ++c) {
        const float g = grad[2 * i + c];
        float u = U[2 * i + c], gain = G[2 * i + c];
        gain = u * g < 0.f ? gain + 0.2f : gain * 0.8f;
        gain = gain < s.min_gain ? s.min_gain : gain;
        const float gg = g * gain;
        u = s.momentum * u - s.learning_rate * gg;
        U[2 * i + c] = u;
        G[2 * i + c] = gain;
        Y[2 * i + c] += u;
        gn += (double)gg * (double)gg;
    }
    gnpart[i] = gn;
}

// out[0] = part[0 .. n) folded in row order (one workgroup)
__global__ __launch_bounds__(TSNE_THREADS) void tsne_fold_kernel(const double* part, int n, double* out) {
    __shared__ double red[TSNE_THREADS];
    const double t = tsne_block_fold(n, red, [&](int k) { return part[k]; });
    if (threadIdx.x == 0) out[0] = t;
}

class Tsne {
public:
    DevHeap heap;
    hipStream_t stream = nullptr;
    std::string last_error;
    int max_points = 0, max_dim = 0, n = 0;
    bool have_state = false;
    float *P = nullptr, *X = nullptr, *Y = nullptr, *U = nullptr, *G = nullptr, *acc = nullptr, *grad = nullptr;
    double *beta = nullptr, *rowsum = nullptr, *klpart = nullptr, *gnpart = nullptr, *scal = nullptr;
    std::vector<float> h_tmp;

    int err(const std::string& s) { last_error = s; return -1; }

    int init(int max_points_, int max_dim_) {
        const char* who = "mtts_tsne_create: ";
        if (max_points_ < 2 || max_points_ > TSNE_MAX_POINTS)
            return err(std::string(who) + "max_points = " + std::to_string(max_points_) + " outside 2 .. " + std::to_string(TSNE_MAX_POINTS) +
                       " (the dense P is max_points^2 x 4 bytes and a row of distances must fit a workgroup's LDS)");
        if (max_dim_ < 1 || max_dim_ > TSNE_MAX_DIM) return err(std::string(who) + "max_dim = " + std::to_string(max_dim_) + " outside 1 .. " + std::to_string(TSNE_MAX_DIM));
        max_points = max_points_;
        max_dim = max_dim_;
        const size_t np = (size_t)max_points;
        const bool ok = heap.alloc(P, np * np * sizeof(float)) == hipSuccess && heap.alloc(X, np * (size_t)max_dim * sizeof(float)) == hipSuccess &&
                        heap.alloc(Y, np * 2 * sizeof(float)) == hipSuccess && heap.alloc(U, np * 2 * sizeof(float)) == hipSuccess &&
                        heap.alloc(G, np * 2 * sizeof(float)) == hipSuccess && heap.alloc(grad, np * 2 * sizeof(float)) == hipSuccess &&
                        heap.alloc(acc, np * TSNE_ACC * sizeof(float)) == hipSuccess && heap.alloc(beta, np * sizeof(double)) == hipSuccess &&
                        heap.alloc(rowsum, np * sizeof(double)) == hipSuccess && heap.alloc(klpart, np * sizeof(double)) == hipSuccess &&
                        heap.alloc(gnpart, np * sizeof(double)) == hipSuccess && heap.alloc(scal, 2 * sizeof(double)) == hipSuccess;
        if (!ok) {
            heap.release_all();
            return err(std::string(who) + "out of device memory (P is " + std::to_string(np * np * sizeof(float) >> 20) + " MB at max_points = " + std::to_string(max_points) + ")");
        }
        return 0;
    }

    int check_launch(const char* who) {
        const hipError_t e = hipGetLastError();
        return e == hipSuccess ? 0 : err(std::string(who) + "kernel launch failed: " + hipGetErrorString(e));
    }
    static bool all_finite(const float* p, size_t count) {
        for (size_t k = 0; k < count; ++k)
            if (!std::isfinite(p[k])) return false;
        return true;
    }
    int check_points(const std::string& who, int n_) {
        if (n_ < 2) return err(who + "n = " + std::to_string(n_) + ": at least 2 points are needed");
        if (n_ > max_points) return err(who + "n = " + std::to_string(n_) + " exceeds the handle's max_points = " + std::to_string(max_points));
        return 0;
    }

    int affinities(const float* X_host, int n_, int dim, double perplexity, float* P_out, double* beta_out) {
        const std::string who = "mtts_tsne_affinities: ";
        if (!X_host) return err(who + "NULL X");
        if (check_points(who, n_)) return -1;
        if (dim < 1 || dim > max_dim) return err(who + "dim = " + std::to_string(dim) + " outside 1 .. max_dim = " + std::to_string(max_dim));
        if (!(perplexity > 0.0) || !std::isfinite(perplexity)) return err(who + "perplexity must be positive and finite");
        if (!(perplexity < (double)n_)) return err(who + "perplexity (" + std::to_string(perplexity) + ") must be less than n (" + std::to_string(n_) + ")");
        if (!all_finite(X_host, (size_t)n_ * dim)) return err(who + "X holds a non-finite value");
        n = 0;
        have_state = false;
        DEV_CHECK(hipMemcpyAsync(X, X_host, (size_t)n_ * dim * sizeof(float), hipMemcpyHostToDevice, stream));
        const unsigned tiles = (unsigned)((n_ + 15) / 16);
        MTTS_LAUNCH(tsne_sqdist_kernel, dim3(tiles, tiles), dim3(TSNE_THREADS), stream, (const float*)X, n_, dim, P);
        MTTS_LAUNCH(tsne_perplexity_kernel, dim3((unsigned)n_), dim3(TSNE_THREADS), stream, P, n_, std::log(perplexity), beta, rowsum);
        MTTS_LAUNCH(tsne_symmetrise_kernel, dim3((unsigned)n_), dim3(TSNE_THREADS), stream, P, n_, (const double*)rowsum);
        if (check_launch(who.c_str())) return -1;
        if (P_out) DEV_CHECK(hipMemcpyAsync(P_out, P, (size_t)n_ * n_ * sizeof(float), hipMemcpyDeviceToHost, stream));
        if (beta_out) DEV_CHECK(hipMemcpyAsync(beta_out, beta, (size_t)n_ * sizeof(double), hipMemcpyDeviceToHost, stream));
        DEV_CHECK(hipStreamSynchronize(stream));
        n = n_;
        return 0;
    }

    int set_affinities(const float* P_host, int n_) {
        const std::string who = "mtts_tsne_set_affinities: ";
        if (!P_host) return err(who + "NULL P");
        if (check_points(who, n_)) return -1;
        const size_t count = (size_t)n_ * n_;
        for (size_t k = 0; k < count; ++k)
            if (!std::isfinite(P_host[k]) || P_host[k] < 0.f) return err(who + "P holds a non-finite or negative value");
        n = 0;
        have_state = false;
        DEV_CHECK(hipMemcpyAsync(P, P_host, count * sizeof(float), hipMemcpyHostToDevice, stream));
        DEV_CHECK(hipStreamSynchronize(stream));
        n = n_;
        return 0;
    }

    int set_state(const float* Y_host, const float* U_host, const float* G_host) {
        const std::string who = "mtts_tsne_set_state: ";
        if (n < 2) return err(who + "no affinities yet (mtts_tsne_affinities / mtts_tsne_set_affinities)");
        if (!Y_host) return err(who + "NULL Y");
        const size_t count = (size_t)n * 2;
        if (!all_finite(Y_host, count) || (U_host && !all_finite(U_host, count)) || (G_host && !all_finite(G_host, count)))
            return err(who + "Y, update or gains hold a non-finite value");
        have_state = false;
        h_tmp.assign(count, 1.f);
        DEV_CHECK(hipMemcpyAsync(Y, Y_host, count * sizeof(float), hipMemcpyHostToDevice, stream));
        if (U_host) DEV_CHECK(hipMemcpyAsync(U, U_host, count * sizeof(float), hipMemcpyHostToDevice, stream));
        else DEV_CHECK(hipMemsetAsync(U, 0, count * sizeof(float), stream));
        DEV_CHECK(hipMemcpyAsync(G, G_host ? G_host : h_tmp.data(), count * sizeof(float), hipMemcpyHostToDevice, stream));
        DEV_CHECK(hipStreamSynchronize(stream));
        have_state = true;
        return 0;
    }

    int get_state(float* Y_host, float* U_host, float* G_host) {
        const std::string who = "mtts_tsne_get_state: ";
        if (!have_state) return err(who + "no state yet (mtts_tsne_set_state)");
        const size_t bytes = (size_t)n * 2 * sizeof(float);
        if (Y_host) DEV_CHECK(hipMemcpyAsync(Y_host, Y, bytes, hipMemcpyDeviceToHost, stream));
        if (U_host) DEV_CHECK(hipMemcpyAsync(U_host, U, bytes, hipMemcpyDeviceToHost, stream));
        if (G_host) DEV_CHECK(hipMemcpyAsync(G_host, G, bytes, hipMemcpyDeviceToHost, stream));
        DEV_CHECK(hipStreamSynchronize(stream));
        return 0;
    }

    void launch_pair() {
        MTTS_LAUNCH(tsne_pair_kernel, dim3((unsigned)((n + TSNE_ROWS - 1) / TSNE_ROWS)), dim3(TSNE_THREADS), stream, (const float*)P, (const float*)Y, n, acc);
    }
    void launch_kl(double exaggeration) {
        MTTS_LAUNCH(tsne_kl_kernel, dim3((unsigned)((n + 3) / 4)), dim3(TSNE_THREADS), stream, (const float*)P, (const float*)Y, n, exaggeration, (const float*)acc, klpart);
        MTTS_LAUNCH(tsne_fold_kernel, dim3(1), dim3(TSNE_THREADS), stream, (const double*)klpart, n, scal);
    }
    void launch_grad(double exaggeration) {
        MTTS_LAUNCH(tsne_grad_kernel, dim3((unsigned)((n + TSNE_THREADS - 1) / TSNE_THREADS)), dim3(TSNE_THREADS), stream, (const float*)Y, n, exaggeration, (const float*)acc, grad);
    }
    void launch_apply(const TsneStep& s) {
        MTTS_LAUNCH(tsne_apply_kernel, dim3((unsigned)((n + TSNE_THREADS - 1) / TSNE_THREADS)), dim3(TSNE_THREADS), stream, Y, U, G, n, s, (const float*)grad, gnpart);
    }

    int gradient(double exaggeration, float* grad_out, double* kl_out) {
        const std::string who = "mtts_tsne_gradient: ";
        if (!have_state) return err(who + "no state yet (mtts_tsne_set_state)");
        if (!grad_out) return err(who + "NULL grad_out");
        if (!(exaggeration > 0.0) || !std::isfinite(exaggeration)) return err(who + "exaggeration must be positive and finite");
        launch_pair();
        launch_grad(exaggeration);
        if (kl_out) launch_kl(exaggeration);
        if (check_launch(who.c_str())) return -1;
        DEV_CHECK(hipMemcpyAsync(grad_out, grad, (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToHost, stream));
        if (kl_out) DEV_CHECK(hipMemcpyAsync(kl_out, scal, sizeof(double), hipMemcpyDeviceToHost, stream));
        DEV_CHECK(hipStreamSynchronize(stream));
        return 0;
    }

    int run(int n_iter, double exaggeration, double momentum, double learning_rate, double min_gain, double* kl_out, double* grad_norm_out) {
        const std::string who = "mtts_tsne_run: ";
        if (!have_state) return err(who + "no state yet (mtts_tsne_set_state)");
        if (n_iter < 1) return err(who + "n_iter = " + std::to_string(n_iter) + ": at least one iteration");
        if (!(exaggeration > 0.0) || !std::isfinite(exaggeration)) return err(who + "exaggeration must be positive and finite");
        if (!(momentum >= 0.0) || !std::isfinite(momentum)) return err(who + "momentum must be non-negative and finite");
        if (!(learning_rate > 0.0) || !std::isfinite(learning_rate)) return err(who + "learning_rate must be positive and finite");
        if (!(min_gain >= 0.0) || !std::isfinite(min_gain)) return err(who + "min_gain must be non-negative and finite");
        const TsneStep s{(float)momentum, (float)learning_rate, (float)min_gain};
        for (int it = 0; it < n_iter; ++it) {
            launch_pair();
            if (kl_out && it == n_iter - 1) launch_kl(exaggeration);   // at the state the last step starts from, as _gradient_descent's `error`
            launch_grad(exaggeration);
            launch_apply(s);
        }
        if (grad_norm_out) MTTS_LAUNCH(tsne_fold_kernel, dim3(1), dim3(TSNE_THREADS), stream, (const double*)gnpart, n, scal + 1);
        if (check_launch(who.c_str())) return -1;
        double h[2] = {0.0, 0.0};
        if (kl_out) DEV_CHECK(hipMemcpyAsync(&h[0], scal, sizeof(double), hipMemcpyDeviceToHost, stream));
        if (grad_norm_out) DEV_CHECK(hipMemcpyAsync(&h[1], scal + 1, sizeof(double), hipMemcpyDeviceToHost, stream));
        DEV_CHECK(hipStreamSynchronize(stream));
        if (kl_out) *kl_out = h[0];
        if (grad_norm_out) *grad_norm_out = std::sqrt(h[1]);
        return 0;
    }
};

}  // namespace mtts
