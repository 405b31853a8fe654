// Mel-cepstral distortion along a dynamic-time-warping path, with log-F0 error and voiced/unvoiced disagreement on the same path: the
// objective figure for "does the synthesis say what the recording says" (DESIGN.md section 1 row f12).  The reference has no such step;
// the definition is this project's own (include/mtts.h states it; tests/mcd_oracle.py restates it in float64 numpy in the same
// summation order).  Parity with SPTK / WORLD mel-cepstra is UNPINNED.
//
//   cepstra   c_k = sum_n B[k][n] m[n], k = 1 .. K, over a natural-log mel frame m; B = rows 1 .. K of the orthonormal DCT-II, designed
//             on the host in float64; the sum in float64 in ascending n.
//   distance  d(i, j) = sqrt(sum_k (a_ik - b_jk)^2), float64, ascending k.
//   DTW       D(0, 0) = d(0, 0); D(i, j) = d(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)), ties to the first in that order; no band, no
//             slope constraint.  The path runs back from (Ta-1, Tb-1) to (0, 0); L = its length.
//   MCD       (10 sqrt(2) / ln 10) D(Ta-1, Tb-1) / L  [dB]
//   F0        along the path, summed in the order of the walk BACK (from the end to the start): steps with both frames voiced (f0 > 0),
//             the RMSE of 1200 log2(fa / fb) over them [cents], steps with exactly one side voiced.
//
// Kernels, all LDS + barriers, no wavefront intrinsic and no atomic, so the SIMT emulator runs the same source and a pair's result is
// the same bits alone, in any batch, at any position and under any chunking (nothing of a pair's arithmetic depends on its neighbours):
//   * mcd_cepstra_kernel: the packed log-mel rows of a call -> [rows][K] float64.  The basis goes into LDS once per workgroup (rows
//     padded to an odd number of doubles: 13 rows read at once fall into different banks); a thread per output (row, k), 8 outputs per
//     thread, so neighbouring threads share a mel row and differ in the basis row.
//   * dtw_sweep_kernel — the hot path: one workgroup per pair sweeps the anti-diagonals s = i + j, whose cells are independent; lanes
//     stride over the diagonal.  The last two diagonals and the one being written are float64 in LDS, indexed by i, and rotate: the
//     diagonal written at s is the one read as s - 2 two steps before, so ONE barrier per diagonal orders everything.  d(i, j) is
//     computed in the sweep from the cepstra (consecutive lanes read consecutive rows of both sides: served by L1 / L2); no Ta x Tb
//     cost matrix exists.  The only Ta x Tb object is the direction map, one byte per cell, stored DIAGONAL-MAJOR (diagonal s starts
//     at dtw_diag_offset(s), cell i of it at + i - ilo(s)) so that a wavefront's 64 byte stores are one contiguous run.  The LDS
//     capacity is a template parameter (512 / 1024 / 2048 rows: 12 / 24 / 48 KiB, 13 / 6 / 3 workgroups per CU by LDS), chosen per
//     chunk from its longest A side; the arithmetic is the same in all three.
//   * dtw_backtrack_kernel: one lane per pair walks the direction map back, counts L, takes the F0 figures, and writes the path from
//     the END of the pair's slot backwards (step k of the walk at slot Ta + Tb - 1 - k), so that the last L entries are the path from
//     (0, 0) forward; the host moves them to the front.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "devres.h"
#include "dtwplan.h"

namespace mtts {

constexpr int DTW_THREADS = 256;
constexpr int DTW_CEP_PER_THREAD = 8;
constexpr int DTW_OUT = 6;   // D, L, MCD, n_voiced_both, cents RMSE, n_vuv_mismatch

struct DtwPair {
    int ta, tb;
    long long row_a, row_b;   // first row of each side in the chunk's cepstra (and F0) buffer
    long long cell;           // first byte of the pair's direction map
    long long step;           // first (i, j) slot of the pair's path
};

// cells on the diagonals before s (a Ta x Tb grid: diagonal s holds i = max(0, s - Tb + 1) .. min(Ta - 1, s))
__host__ __device__ __forceinline__ long long dtw_diag_offset(int s, int ta, int tb) {
    const long long m = ta < tb ? ta : tb, M = ta < tb ? tb : ta, S = s;
    if (S <= m) return S * (S + 1) / 2;
    if (S <= M) return m * (m + 1) / 2 + (S - m) * m;
    const long long n = S - M;
    return m * (m + 1) / 2 + (M - m) * m + n * ((long long)ta + tb - 1) - n * (M + S - 1) / 2;
}

__global__ __launch_bounds__(DTW_THREADS) void mcd_cepstra_kernel(const float* mel, long long n_rows, int n_mel, int n_coef, const double* basis, double* cep) {
    __shared__ double bs[DTW_MAX_COEF * (DTW_MAX_MEL + 1)];
    const int tid = (int)threadIdx.x, stride = n_mel | 1;
    for (int q = tid; q < n_coef * n_mel; q += DTW_THREADS) bs[(q / n_mel) * stride + q % n_mel] = basis[q];
    __syncthreads();
    const long long total = n_rows * n_coef;
    for (int r = 0; r < DTW_CEP_PER_THREAD; ++r) {
        const long long idx = ((long long)blockIdx.x * DTW_CEP_PER_THREAD + r) * DTW_THREADS + tid;
        if (idx >= total) return;
        const float* m = mel + idx / n_coef * n_mel;
        const double* b = bs + (int)(idx % n_coef) * stride;
        double s = 0.0;
        for (int n = 0; n < n_mel; ++n) s += b[n] * (double)m[n];
        cep[idx] = s;
    }
}

template <int CAP>
__global__ __launch_bounds__(DTW_THREADS) void dtw_sweep_kernel(const double* cep, int n_coef, const DtwPair* pairs, unsigned char* dir, double* d_end) {
    __shared__ double diag[3][CAP];
    const DtwPair pr = pairs[blockIdx.x];
    const int tid = (int)threadIdx.x, ta = pr.ta, tb = pr.tb;
    const double* A = cep + pr.row_a * n_coef;
    const double* B = cep + pr.row_b * n_coef;
    unsigned char* map = dir + pr.cell;
    double *cur = diag[0], *p1 = diag[1], *p2 = diag[2];   // diagonals s, s - 1, s - 2
    const double inf = __builtin_huge_val();
    long long off = 0;
    for (int s = 0; s < ta + tb - 1; ++s) {
        const int ilo = s - tb + 1 > 0 ? s - tb + 1 : 0, ihi = s < ta - 1 ? s : ta - 1;
        for (int i = ilo + tid; i <= ihi; i += DTW_THREADS) {
            const int j = s - i;
            const double* a = A + (size_t)i * n_coef;
            const double* b = B + (size_t)j * n_coef;
            double q = 0.0;
            for (int k = 0; k < n_coef; ++k) {
                const double t = a[k] - b[k];
                q += t * t;
            }
            // (i - 1, j - 1) is cell i - 1 of diagonal s - 2; (i - 1, j) cell i - 1 and (i, j - 1) cell i of diagonal s - 1
            double best = i > 0 && j > 0 ? p2[i - 1] : (s == 0 ? 0.0 : inf);
            unsigned char from = 0;
            const double up = i > 0 ? p1[i - 1] : inf, left = j > 0 ? p1[i] : inf;
            if (up < best) { best = up; from = 1; }
            if (left < best) { best = left; from = 2; }
            cur[i] = sqrt(q) + best;
            map[off + (i - ilo)] = from;
        }
        off += ihi - ilo + 1;
        __syncthreads();
        double* t = p2;
        p2 = p1;
        p1 = cur;
        cur = t;
    }
    if (tid == 0) d_end[blockIdx.x] = p1[ta - 1];
}

// f0 == nullptr: no F0 figures (NaN in their columns); path == nullptr: no path
__global__ __launch_bounds__(64) void dtw_backtrack_kernel(const DtwPair* pairs, int n_pairs, const unsigned char* dir, const double* d_end, const double* f0, double mcd_scale,
                                                           int* path, double* out) {
    const int p = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (p >= n_pairs) return;
    const DtwPair pr = pairs[p];
    const unsigned char* map = dir + pr.cell;
    const double nan = __builtin_nan("");
    int i = pr.ta - 1, j = pr.tb - 1, L = 0, both = 0, one = 0;
    double ss = 0.0;
    for (;;) {
        ++L;
        if (path) {
            int* slot = path + 2 * (pr.step + (pr.ta + pr.tb - 1 - L));
            slot[0] = i;
            slot[1] = j;
        }
        if (f0) {
            const double fa = f0[pr.row_a + i], fb = f0[pr.row_b + j];
            if (fa > 0.0 && fb > 0.0) {
                const double c = 1200.0 * log2(fa / fb);
                ss += c * c;
                ++both;
            } else if (fa > 0.0 || fb > 0.0) {
                ++one;
            }
        }
        if (i == 0 && j == 0) break;
        const int s = i + j, ilo = s - pr.tb + 1 > 0 ? s - pr.tb + 1 : 0;
        const unsigned char from = map[dtw_diag_offset(s, pr.ta, pr.tb) + (i - ilo)];
        if (from != 2) --i;
        if (from != 1) --j;
    }
    double* o = out + (size_t)p * DTW_OUT;
    const double D = d_end[p];
    o[0] = D;
    o[1] = (double)L;
    o[2] = mcd_scale * D / (double)L;
    o[3] = f0 ? (double)both : nan;
    o[4] = f0 && both > 0 ? sqrt(ss / (double)both) : nan;
    o[5] = f0 ? (double)one : nan;
}

class Dtw {
public:
    DevHeap heap;
    hipStream_t stream = nullptr;
    std::string last_error;
    DtwLimits lim;
    bool have_basis = false;
    double* basis = nullptr;
    DevBuf<float> mel;
    DevBuf<double> cep, f0, d_end, out;
    DevBuf<unsigned char> dir;
    DevBuf<DtwPair> pairs;
    DevBuf<int> path;
    std::vector<DtwPair> h_pairs;
    std::vector<int> h_path;

    int err(const std::string& s) { last_error = s; return -1; }

    int init(const DtwLimits& l) {
        const std::string e = dtw_check_limits(l);
        if (!e.empty()) return err(e);
        lim = l;
        if (heap.alloc(basis, (size_t)l.n_coef * l.n_mel * sizeof(double)) != hipSuccess) return err("mtts_dtw_create: out of device memory (basis)");
        return 0;
    }

    int check_launch(const char* who) {
        const hipError_t e = hipGetLastError();
        return e == hipSuccess ? 0 : err(std::string(who) + "kernel launch failed: " + hipGetErrorString(e));
    }

    int load_basis(const double* B) {
        const std::string who = "mtts_dtw_load_basis: ";
        if (!B) return err(who + "NULL basis");
        const size_t count = (size_t)lim.n_coef * lim.n_mel;
        for (size_t k = 0; k < count; ++k)
            if (!std::isfinite(B[k])) return err(who + "the basis holds a non-finite value");
        have_basis = false;
        DEV_CHECK(hipMemcpyAsync(basis, B, count * sizeof(double), hipMemcpyHostToDevice, stream));
        DEV_CHECK(hipStreamSynchronize(stream));
        have_basis = true;
        return 0;
    }

    void launch_cepstra(long long rows) {
        const long long per = (long long)DTW_THREADS * DTW_CEP_PER_THREAD, blocks = (rows * lim.n_coef + per - 1) / per;
        MTTS_LAUNCH(mcd_cepstra_kernel, dim3((unsigned)blocks), dim3(DTW_THREADS), stream, (const float*)mel.p, rows, lim.n_mel, lim.n_coef, (const double*)basis, cep.p);
    }

    int cepstra(int n_utts, const int* n_frames, const float* log_mel, double* cep_out) {
        const std::string who = "mtts_dtw_cepstra: ";
        if (!have_basis) return err(who + "no basis loaded (mtts_dtw_load_basis)");
        if (n_utts < 1 || !n_frames || !log_mel || !cep_out) return err(who + "bad arguments (n_utts < 1 or NULL pointer)");
        // both sides of a chunk's worth of pairs at most: rows <= 2 max_pairs max_frames <= 2^32, far inside the launch grid
        if (n_utts > 2 * (long long)lim.max_pairs) return err(who + "n_utts = " + std::to_string(n_utts) + " exceeds 2 x the handle's max_pairs = " + std::to_string(lim.max_pairs));
        long long rows = 0;
        for (int u = 0; u < n_utts; ++u) {
            if (n_frames[u] < 1) return err(who + "utterance " + std::to_string(u) + ": n_frames = " + std::to_string(n_frames[u]) + ": at least 1 frame is needed");
            if (n_frames[u] > lim.max_frames)
                return err(who + "utterance " + std::to_string(u) + ": n_frames = " + std::to_string(n_frames[u]) + " exceeds the handle's max_frames = " + std::to_string(lim.max_frames));
            rows += n_frames[u];
        }
        for (long long k = 0; k < rows * lim.n_mel; ++k)
            if (!std::isfinite(log_mel[k])) return err(who + "log_mel holds a non-finite value (row " + std::to_string(k / lim.n_mel) + ")");
        if (grow(heap, mel, (size_t)rows * lim.n_mel, stream, "log-mel rows", last_error) || grow(heap, cep, (size_t)rows * lim.n_coef, stream, "cepstra", last_error)) return -1;
        DEV_CHECK(hipMemcpyAsync(mel.p, log_mel, (size_t)rows * lim.n_mel * sizeof(float), hipMemcpyHostToDevice, stream));
        launch_cepstra(rows);
        if (check_launch(who.c_str())) return -1;
        DEV_CHECK(hipMemcpyAsync(cep_out, cep.p, (size_t)rows * lim.n_coef * sizeof(double), hipMemcpyDeviceToHost, stream));
        DEV_CHECK(hipStreamSynchronize(stream));
        return 0;
    }

    void launch_sweep(int count, int longest_a) {
        const dim3 grid((unsigned)count), block(DTW_THREADS);
        if (longest_a <= 512) MTTS_LAUNCH(dtw_sweep_kernel<512>, grid, block, stream, (const double*)cep.p, lim.n_coef, (const DtwPair*)pairs.p, dir.p, d_end.p);
        else if (longest_a <= 1024) MTTS_LAUNCH(dtw_sweep_kernel<1024>, grid, block, stream, (const double*)cep.p, lim.n_coef, (const DtwPair*)pairs.p, dir.p, d_end.p);
        else MTTS_LAUNCH(dtw_sweep_kernel<DTW_MAX_FRAMES>, grid, block, stream, (const double*)cep.p, lim.n_coef, (const DtwPair*)pairs.p, dir.p, d_end.p);
    }

    int mcd_batch(int n_pairs, const int* frames_a, const float* mel_a, const int* frames_b, const float* mel_b, const int* f0_frames_a, const double* f0_a,
                  const int* f0_frames_b, const double* f0_b, double* out_host, int* path_len, int* path_host) {
        const std::string who = "mtts_dtw_mcd_batch: ";
        const std::string e = dtw_validate(lim, have_basis, n_pairs, frames_a, mel_a, frames_b, mel_b, f0_frames_a, f0_a, f0_frames_b, f0_b, out_host);
        if (!e.empty()) return err(e);
        const std::vector<DtwChunk> chunks = dtw_plan_chunks(lim, n_pairs, frames_a, frames_b);
        DtwChunk top;   // every buffer is reserved for the largest chunk before anything runs
        for (const DtwChunk& c : chunks) {
            top.count = std::max(top.count, c.count);
            top.cells = std::max(top.cells, c.cells);
            top.rows_a = std::max(top.rows_a, c.rows_a + c.rows_b);
            top.steps = std::max(top.steps, c.steps);
        }
        const size_t rows = (size_t)top.rows_a;
        if (grow(heap, mel, rows * lim.n_mel, stream, "log-mel rows", last_error) || grow(heap, cep, rows * lim.n_coef, stream, "cepstra", last_error) ||
            grow(heap, dir, (size_t)top.cells, stream, "direction map", last_error) || grow(heap, pairs, (size_t)top.count, stream, "pair table", last_error) ||
            grow(heap, d_end, (size_t)top.count, stream, "end costs", last_error) || grow(heap, out, (size_t)top.count * DTW_OUT, stream, "results", last_error) ||
            (f0_a && grow(heap, f0, rows, stream, "F0 tracks", last_error)) || (path_host && grow(heap, path, (size_t)top.steps * 2, stream, "paths", last_error)))
            return -1;
        const double mcd_scale = 10.0 * std::sqrt(2.0) / std::log(10.0);
        long long row_a0 = 0, row_b0 = 0, step0 = 0;   // where the chunk starts in the caller's packed arrays
        for (const DtwChunk& c : chunks) {
            h_pairs.resize((size_t)c.count);
            long long ra = 0, rb = c.rows_a, cell = 0, step = 0;
            int longest_a = 0;
            for (int q = 0; q < c.count; ++q) {
                const int ta = frames_a[c.first + q], tb = frames_b[c.first + q];
                h_pairs[(size_t)q] = DtwPair{ta, tb, ra, rb, cell, step};
                ra += ta;
                rb += tb;
                cell += (long long)ta * tb;
                step += ta + tb - 1;
                longest_a = std::max(longest_a, ta);
            }
            DEV_CHECK(hipMemcpyAsync(mel.p, mel_a + row_a0 * lim.n_mel, (size_t)c.rows_a * lim.n_mel * sizeof(float), hipMemcpyHostToDevice, stream));
            DEV_CHECK(hipMemcpyAsync(mel.p + c.rows_a * lim.n_mel, mel_b + row_b0 * lim.n_mel, (size_t)c.rows_b * lim.n_mel * sizeof(float), hipMemcpyHostToDevice, stream));
            DEV_CHECK(hipMemcpyAsync(pairs.p, h_pairs.data(), (size_t)c.count * sizeof(DtwPair), hipMemcpyHostToDevice, stream));
            if (f0_a) {
                DEV_CHECK(hipMemcpyAsync(f0.p, f0_a + row_a0, (size_t)c.rows_a * sizeof(double), hipMemcpyHostToDevice, stream));
                DEV_CHECK(hipMemcpyAsync(f0.p + c.rows_a, f0_b + row_b0, (size_t)c.rows_b * sizeof(double), hipMemcpyHostToDevice, stream));
            }
            launch_cepstra(c.rows_a + c.rows_b);
            launch_sweep(c.count, longest_a);
            MTTS_LAUNCH(dtw_backtrack_kernel, dim3((unsigned)((c.count + 63) / 64)), dim3(64), stream, (const DtwPair*)pairs.p, c.count, (const unsigned char*)dir.p,
                        (const double*)d_end.p, (const double*)(f0_a ? f0.p : nullptr), mcd_scale, path_host ? path.p : nullptr, out.p);
            if (check_launch(who.c_str())) return -1;
            DEV_CHECK(hipMemcpyAsync(out_host + (size_t)c.first * DTW_OUT, out.p, (size_t)c.count * DTW_OUT * sizeof(double), hipMemcpyDeviceToHost, stream));
            if (path_host) {
                h_path.resize((size_t)c.steps * 2);
                DEV_CHECK(hipMemcpyAsync(h_path.data(), path.p, (size_t)c.steps * 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
            }
            DEV_CHECK(hipStreamSynchronize(stream));   // (the staging vectors and the device buffers are reused by the next chunk)
            for (int q = 0; q < c.count; ++q) {
                const DtwPair& pr = h_pairs[(size_t)q];
                const int L = (int)out_host[(size_t)(c.first + q) * DTW_OUT + 1], cap = pr.ta + pr.tb - 1;
                if (path_len) path_len[c.first + q] = L;
                if (path_host) {   // the walk filled the slot from its end: the last L entries, moved to the front
                    int* dst = path_host + 2 * (step0 + pr.step);
                    const int* src = h_path.data() + 2 * (pr.step + cap - L);
                    for (int k = 0; k < 2 * L; ++k) dst[k] = src[k];
                    for (int k = 2 * L; k < 2 * cap; ++k) dst[k] = -1;
                }
            }
            row_a0 += c.rows_a;
            row_b0 += c.rows_b;
            step0 += c.steps;
        }
        return 0;
    }
};

}  // namespace mtts
