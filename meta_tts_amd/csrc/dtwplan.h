// The host half of mtts_dtw_mcd_batch (dtw.h): the limits a handle is created with, the validation of a call, and the cut of its pairs
// into chunks.  Plain C++ with no device or runtime call in it, so that a stand-alone program can run it under the host sanitizers
// (tools/dtw_plan_check.cpp).
#pragma once
#include <cmath>
#include <string>
#include <vector>

namespace mtts {

constexpr int DTW_MAX_FRAMES = 2048;               // three float64 diagonals in LDS: 48 KiB
constexpr int DTW_MAX_COEF = 34;
constexpr int DTW_MAX_MEL = 128;                   // the basis in LDS: 34 x 129 doubles = 35 KB
constexpr long long DTW_MAX_CELLS = 1ll << 33;     // the direction map is one byte per cell
constexpr int DTW_MAX_PAIRS = 1 << 20;

struct DtwLimits {
    int n_mel = 0, n_coef = 0, max_frames = 0;
    long long max_cells = 0;
    int max_pairs = 0;
};

// pairs [first, first + count) of a call; rows = mel frames of each side, cells = sum Ta Tb, steps = sum (Ta + Tb - 1)
struct DtwChunk {
    int first = 0, count = 0;
    long long cells = 0, rows_a = 0, rows_b = 0, steps = 0;
};

// "" or the reason mtts_dtw_create refuses
inline std::string dtw_check_limits(const DtwLimits& l) {
    const std::string who = "mtts_dtw_create: ";
    if (l.n_mel < 2 || l.n_mel > DTW_MAX_MEL) return who + "n_mel = " + std::to_string(l.n_mel) + " outside 2 .. " + std::to_string(DTW_MAX_MEL);
    if (l.n_coef < 1 || l.n_coef > DTW_MAX_COEF) return who + "n_coef = " + std::to_string(l.n_coef) + " outside 1 .. " + std::to_string(DTW_MAX_COEF);
    if (l.n_coef >= l.n_mel) return who + "n_coef = " + std::to_string(l.n_coef) + " must be less than n_mel = " + std::to_string(l.n_mel) + " (c0 is dropped)";
    if (l.max_frames < 1 || l.max_frames > DTW_MAX_FRAMES)
        return who + "max_frames = " + std::to_string(l.max_frames) + " outside 1 .. " + std::to_string(DTW_MAX_FRAMES) + " (three float64 diagonals must fit a workgroup's LDS)";
    if (l.max_cells < 1 || l.max_cells > DTW_MAX_CELLS) return who + "max_cells = " + std::to_string(l.max_cells) + " outside 1 .. " + std::to_string(DTW_MAX_CELLS);
    if (l.max_pairs < 1 || l.max_pairs > DTW_MAX_PAIRS) return who + "max_pairs = " + std::to_string(l.max_pairs) + " outside 1 .. " + std::to_string(DTW_MAX_PAIRS);
    return "";
}

// "" or the reason one side's frame counts are refused; adds the side's rows to `rows`
inline std::string dtw_check_frames(const std::string& who, const DtwLimits& l, int n, const int* frames, const char* side, long long& rows) {
    for (int p = 0; p < n; ++p) {
        const std::string at = who + "pair " + std::to_string(p) + ": frames_" + side + " = " + std::to_string(frames[p]);
        if (frames[p] < 1) return at + ": at least 1 frame is needed";
        if (frames[p] > l.max_frames) return at + " exceeds the handle's max_frames = " + std::to_string(l.max_frames);
        rows += frames[p];
    }
    return "";
}

// "" or the reason a call of mtts_dtw_mcd_batch is refused.  Everything is checked here, before any launch.
inline std::string dtw_validate(const DtwLimits& l, bool have_basis, int n_pairs, const int* frames_a, const float* mel_a, const int* frames_b, const float* mel_b,
                                const int* f0_frames_a, const double* f0_a, const int* f0_frames_b, const double* f0_b, const double* out) {
    const std::string who = "mtts_dtw_mcd_batch: ";
    if (!have_basis) return who + "no basis loaded (mtts_dtw_load_basis)";
    if (n_pairs < 1) return who + "n_pairs = " + std::to_string(n_pairs) + ": at least 1 pair is needed";
    if (!frames_a || !mel_a || !frames_b || !mel_b || !out) return who + "NULL frames_a, mel_a, frames_b, mel_b or out";
    if ((f0_a == nullptr) != (f0_b == nullptr)) return who + (f0_a ? "f0_a given without f0_b" : "f0_b given without f0_a") + " (both F0 tracks or neither)";
    if (f0_a && (!f0_frames_a || !f0_frames_b)) return who + "F0 tracks given without f0_frames_a / f0_frames_b";
    long long rows_a = 0, rows_b = 0;
    std::string e = dtw_check_frames(who, l, n_pairs, frames_a, "a", rows_a);
    if (e.empty()) e = dtw_check_frames(who, l, n_pairs, frames_b, "b", rows_b);
    if (!e.empty()) return e;
    for (int p = 0; p < n_pairs; ++p) {
        const long long cells = (long long)frames_a[p] * frames_b[p];
        if (cells > l.max_cells)
            return who + "pair " + std::to_string(p) + ": " + std::to_string(frames_a[p]) + " x " + std::to_string(frames_b[p]) + " = " + std::to_string(cells) +
                   " cells exceed the handle's max_cells = " + std::to_string(l.max_cells);
        if (f0_a && f0_frames_a[p] != frames_a[p])
            return who + "pair " + std::to_string(p) + ": f0_frames_a = " + std::to_string(f0_frames_a[p]) + " but frames_a = " + std::to_string(frames_a[p]) + " (an F0 track has one value per mel frame)";
        if (f0_a && f0_frames_b[p] != frames_b[p])
            return who + "pair " + std::to_string(p) + ": f0_frames_b = " + std::to_string(f0_frames_b[p]) + " but frames_b = " + std::to_string(frames_b[p]) + " (an F0 track has one value per mel frame)";
    }
    for (int side = 0; side < 2; ++side) {
        const float* m = side ? mel_b : mel_a;
        const long long count = (side ? rows_b : rows_a) * l.n_mel;
        for (long long k = 0; k < count; ++k)
            if (!std::isfinite(m[k])) return who + "mel_" + (side ? "b" : "a") + " holds a non-finite value (row " + std::to_string(k / l.n_mel) + ")";
        const double* f = side ? f0_b : f0_a;
        for (long long k = 0; f && k < (side ? rows_b : rows_a); ++k)
            if (!std::isfinite(f[k]) || f[k] < 0.0) return who + "f0_" + (side ? "b" : "a") + " holds a negative or non-finite value (frame " + std::to_string(k) + "; 0 = unvoiced)";
    }
    return "";
}

// The pairs of a validated call, in order, cut into chunks of at most max_cells cells and max_pairs pairs: a chunk takes pairs while
// they fit, so no pair is ever split and every chunk holds at least one.
inline std::vector<DtwChunk> dtw_plan_chunks(const DtwLimits& l, int n_pairs, const int* frames_a, const int* frames_b) {
    std::vector<DtwChunk> chunks;
    DtwChunk c;
    for (int p = 0; p < n_pairs; ++p) {
        const long long cells = (long long)frames_a[p] * frames_b[p];
        if (c.count > 0 && (c.cells + cells > l.max_cells || c.count >= l.max_pairs)) {
            chunks.push_back(c);
            c = DtwChunk();
            c.first = p;
        }
        c.count += 1;
        c.cells += cells;
        c.rows_a += frames_a[p];
        c.rows_b += frames_b[p];
        c.steps += frames_a[p] + frames_b[p] - 1;
    }
    if (c.count > 0) chunks.push_back(c);
    return chunks;
}

}  // namespace mtts
