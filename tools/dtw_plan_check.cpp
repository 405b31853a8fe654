// Stand-alone check of the host half of mtts_dtw_mcd_batch (meta_tts_amd/csrc/dtwplan.h: limits, validation, chunk planner), meant to be
// built with the host sanitizers and run on the CPU; it touches no device:
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Imeta_tts_amd/csrc tools/dtw_plan_check.cpp -o dtw_plan_check && ./dtw_plan_check
// Exit status 0 and "ok" when every expectation holds; a sanitizer report or a failed expectation ends it with another status.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

#include "dtwplan.h"

using namespace mtts;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)
static bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

static DtwLimits limits(int max_frames, long long max_cells, int max_pairs) {
    DtwLimits l;
    l.n_mel = 8; l.n_coef = 7; l.max_frames = max_frames; l.max_cells = max_cells; l.max_pairs = max_pairs;
    return l;
}

// every chunk within both limits, the chunks a partition of the pairs in order, the sums right, and greedy: the next pair would not have fitted
static void check_plan(const DtwLimits& l, const std::vector<int>& ta, const std::vector<int>& tb) {
    const int n = (int)ta.size();
    const std::vector<DtwChunk> chunks = dtw_plan_chunks(l, n, ta.data(), tb.data());
    int next = 0;
    for (size_t c = 0; c < chunks.size(); ++c) {
        const DtwChunk& k = chunks[c];
        EXPECT(k.first == next && k.count >= 1 && k.count <= l.max_pairs && k.cells <= l.max_cells);
        long long cells = 0, ra = 0, rb = 0, steps = 0;
        for (int p = k.first; p < k.first + k.count; ++p) { cells += (long long)ta[p] * tb[p]; ra += ta[p]; rb += tb[p]; steps += ta[p] + tb[p] - 1; }
        EXPECT(cells == k.cells && ra == k.rows_a && rb == k.rows_b && steps == k.steps);
        next = k.first + k.count;
        if (next < n) EXPECT(k.count == l.max_pairs || k.cells + (long long)ta[next] * tb[next] > l.max_cells);
    }
    EXPECT(next == n);
}

int main() {
    // limits
    EXPECT(dtw_check_limits(limits(320, 1000, 4)).empty());
    EXPECT(has(dtw_check_limits(limits(2049, 1000, 4)), "max_frames = 2049 outside 1 .. 2048"));
    EXPECT(has(dtw_check_limits(limits(320, 0, 4)), "max_cells = 0 outside"));
    EXPECT(has(dtw_check_limits(limits(320, DTW_MAX_CELLS + 1, 4)), "max_cells"));
    EXPECT(has(dtw_check_limits(limits(320, 1000, 0)), "max_pairs = 0 outside"));
    { DtwLimits l = limits(320, 1000, 4); l.n_coef = 8; EXPECT(has(dtw_check_limits(l), "must be less than n_mel")); }
    { DtwLimits l = limits(320, 1000, 4); l.n_coef = 35; l.n_mel = 80; EXPECT(has(dtw_check_limits(l), "n_coef = 35 outside")); }

    // validation: buffers of exactly the size the arguments describe, so that a read past them is a sanitizer report
    const DtwLimits l = limits(320, 1000, 4);
    {
        const std::vector<int> ta{7, 3}, tb{9, 2};
        std::vector<float> ma(10 * 8, -5.f), mb(11 * 8, -4.f);
        std::vector<double> fa(10, 100.0), fb(11, 0.0), out(12);
        auto run = [&](bool basis, const std::vector<int>& a, const std::vector<int>& b, const int* fta, const double* pfa, const int* ftb, const double* pfb) {
            return dtw_validate(l, basis, (int)a.size(), a.data(), ma.data(), b.data(), mb.data(), fta, pfa, ftb, pfb, out.data());
        };
        EXPECT(run(true, ta, tb, nullptr, nullptr, nullptr, nullptr).empty());
        EXPECT(run(true, ta, tb, ta.data(), fa.data(), tb.data(), fb.data()).empty());
        EXPECT(has(run(false, ta, tb, nullptr, nullptr, nullptr, nullptr), "no basis loaded"));
        EXPECT(has(run(true, {7, 0}, tb, nullptr, nullptr, nullptr, nullptr), "pair 1: frames_a = 0: at least 1 frame"));
        EXPECT(has(run(true, ta, {9, -3}, nullptr, nullptr, nullptr, nullptr), "pair 1: frames_b = -3: at least 1 frame"));
        EXPECT(has(run(true, {321, 3}, tb, nullptr, nullptr, nullptr, nullptr), "pair 0: frames_a = 321 exceeds the handle's max_frames = 320"));
        EXPECT(has(run(true, ta, tb, ta.data(), fa.data(), nullptr, nullptr), "f0_a given without f0_b"));
        EXPECT(has(run(true, ta, tb, nullptr, nullptr, tb.data(), fb.data()), "f0_b given without f0_a"));
        EXPECT(has(run(true, ta, tb, nullptr, fa.data(), nullptr, fb.data()), "without f0_frames_a / f0_frames_b"));
        const std::vector<int> fta{7, 2}, ftb{8, 2};
        EXPECT(has(run(true, ta, tb, fta.data(), fa.data(), tb.data(), fb.data()), "pair 1: f0_frames_a = 2 but frames_a = 3"));
        EXPECT(has(run(true, ta, tb, ta.data(), fa.data(), ftb.data(), fb.data()), "pair 0: f0_frames_b = 8 but frames_b = 9"));
        fa[9] = -1.0;
        EXPECT(has(run(true, ta, tb, ta.data(), fa.data(), tb.data(), fb.data()), "f0_a holds a negative or non-finite value (frame 9"));
        fa[9] = 100.0;
        mb[11 * 8 - 1] = std::numeric_limits<float>::infinity();
        EXPECT(has(run(true, ta, tb, nullptr, nullptr, nullptr, nullptr), "mel_b holds a non-finite value (row 10)"));
        mb[11 * 8 - 1] = -4.f;
        EXPECT(has(dtw_validate(l, true, 0, ta.data(), ma.data(), tb.data(), mb.data(), nullptr, nullptr, nullptr, nullptr, out.data()), "n_pairs = 0"));
        EXPECT(has(dtw_validate(l, true, 2, ta.data(), ma.data(), tb.data(), mb.data(), nullptr, nullptr, nullptr, nullptr, nullptr), "NULL"));
    }
    {   // Ta Tb > max_cells, with a product that would overflow 32 bits on a larger handle
        const std::vector<int> ta{32}, tb{32};
        std::vector<float> m(32 * 8, 0.f);
        std::vector<double> out(6);
        EXPECT(has(dtw_validate(l, true, 1, ta.data(), m.data(), tb.data(), m.data(), nullptr, nullptr, nullptr, nullptr, out.data()), "32 x 32 = 1024 cells exceed the handle's max_cells = 1000"));
    }

    // the planner: hand-made cases, then random ones against the invariants
    {
        const std::vector<int> ta{10, 10, 30, 10, 10}, tb{10, 10, 30, 10, 10};   // cells 100, 100, 900, 100, 100
        const std::vector<DtwChunk> c = dtw_plan_chunks(l, 5, ta.data(), tb.data());
        EXPECT(c.size() == 3 && c[0].count == 2 && c[1].first == 2 && c[1].count == 2 && c[1].cells == 1000 && c[2].first == 4 && c[2].count == 1);
        const std::vector<DtwChunk> by_pairs = dtw_plan_chunks(limits(320, 1 << 20, 2), 5, ta.data(), tb.data());
        EXPECT(by_pairs.size() == 3 && by_pairs[0].count == 2 && by_pairs[1].count == 2 && by_pairs[2].count == 1);
        const std::vector<DtwChunk> one = dtw_plan_chunks(limits(320, 1 << 20, 64), 5, ta.data(), tb.data());
        EXPECT(one.size() == 1 && one[0].count == 5 && one[0].cells == 1300 && one[0].steps == 19 * 4 + 59);
        EXPECT(dtw_plan_chunks(l, 0, ta.data(), tb.data()).empty());
    }
    std::mt19937 rng(12345);
    for (int round = 0; round < 400; ++round) {
        const DtwLimits lr = limits(2048, 2048ll * 2048 + (long long)(rng() % 5000000), 1 + (int)(rng() % 9));   // (every single pair fits)
        const int n = 1 + (int)(rng() % 40);
        std::vector<int> ta((size_t)n), tb((size_t)n);
        for (int p = 0; p < n; ++p) { ta[(size_t)p] = 1 + (int)(rng() % 2048); tb[(size_t)p] = 1 + (int)(rng() % 2048); }
        check_plan(lr, ta, tb);
    }
    {   // the largest legal call shape: sums stay in 64 bits
        const DtwLimits big = limits(2048, DTW_MAX_CELLS, DTW_MAX_PAIRS);
        const std::vector<int> ta(4096, 2048), tb(4096, 2048);
        check_plan(big, ta, tb);
        const std::vector<DtwChunk> c = dtw_plan_chunks(big, 4096, ta.data(), tb.data());
        EXPECT(c.size() == 2 && c[0].cells == DTW_MAX_CELLS);
    }
    if (failures) { std::fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    std::puts("ok");
    return 0;
}
