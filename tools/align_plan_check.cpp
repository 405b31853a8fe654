// Stand-alone check of the host half of the mtts_align entries (meta_tts_amd/csrc/alignplan.h: limits, model and call validation, chunk
// planner), meant to be built with the host sanitizers and run on the CPU; it touches no device:
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Imeta_tts_amd/csrc tools/align_plan_check.cpp -o align_plan_check && ./align_plan_check
// Exit status 0 and "ok" when every expectation holds; a sanitizer report or a failed expectation ends it with another status.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

#include "alignplan.h"

using namespace mtts;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)
static bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

static AlignLimits limits(int max_frames, int max_states, long long max_cells, int max_utts) {
    AlignLimits l;
    l.n_feat = 4; l.n_classes = 5; l.max_frames = max_frames; l.max_states = max_states; l.max_cells = max_cells; l.max_utts = max_utts;
    return l;
}

// every chunk within both limits, the chunks a partition of the utterances in order, the sums right, and greedy: the next one would not have fitted
static void check_plan(const AlignLimits& l, const std::vector<int>& T, const std::vector<int>& S) {
    const int n = (int)T.size();
    const std::vector<AlignChunk> chunks = align_plan_chunks(l, n, T.data(), S.data());
    int next = 0;
    for (const AlignChunk& k : chunks) {
        EXPECT(k.first == next && k.count >= 1 && k.count <= l.max_utts && k.cells <= l.max_cells);
        long long cells = 0, rows = 0, states = 0;
        int longest = 0;
        for (int u = k.first; u < k.first + k.count; ++u) { cells += (long long)T[u] * S[u]; rows += T[u]; states += S[u]; longest = S[u] > longest ? S[u] : longest; }
        EXPECT(cells == k.cells && rows == k.rows && states == k.states && longest == k.longest_states);
        next = k.first + k.count;
        if (next < n) EXPECT(k.count == l.max_utts || k.cells + (long long)T[next] * S[next] > l.max_cells);
    }
    EXPECT(next == n);
}

int main() {
    // limits
    EXPECT(align_check_limits(limits(320, 64, 1000, 4)).empty());
    EXPECT(has(align_check_limits(limits(0, 64, 1000, 4)), "max_frames = 0 outside 1 .. "));
    EXPECT(has(align_check_limits(limits(320, 2049, 1000, 4)), "max_states = 2049 outside 1 .. 2048"));
    EXPECT(has(align_check_limits(limits(320, 64, 0, 4)), "max_cells = 0 outside"));
    EXPECT(has(align_check_limits(limits(320, 64, ALIGN_MAX_CELLS + 1, 4)), "max_cells"));
    EXPECT(has(align_check_limits(limits(320, 64, 1000, 65536)), "max_utts = 65536 outside 1 .. 65535"));
    { AlignLimits l = limits(320, 64, 1000, 4); l.n_feat = 129; EXPECT(has(align_check_limits(l), "n_feat = 129 outside 1 .. 128")); }
    { AlignLimits l = limits(320, 64, 1000, 4); l.n_classes = 0; EXPECT(has(align_check_limits(l), "n_classes = 0 outside 1 .. 512")); }

    const AlignLimits l = limits(40, 8, 200, 4);
    // the model: buffers of exactly the size the limits describe, so that a read past them is a sanitizer report
    {
        std::vector<double> mean(5 * 4, 0.5), var(5 * 4, 2.0), g(4, 1.0);
        const std::string who = "set_model: ";
        EXPECT(align_check_model(who, l, mean.data(), var.data(), g.data()).empty());
        EXPECT(has(align_check_model(who, l, nullptr, var.data(), g.data()), "NULL mean, var or global_var"));
        var[4 * 4 + 3] = 0.0;
        EXPECT(has(align_check_model(who, l, mean.data(), var.data(), g.data()), "var holds a value that is not finite and > 0 (class 4, feature 3)"));
        var[4 * 4 + 3] = std::numeric_limits<double>::quiet_NaN();
        EXPECT(has(align_check_model(who, l, mean.data(), var.data(), g.data()), "var holds a value"));
        var[4 * 4 + 3] = 2.0;
        mean[0] = std::numeric_limits<double>::infinity();
        EXPECT(has(align_check_model(who, l, mean.data(), var.data(), g.data()), "mean holds a non-finite value (class 0, feature 0)"));
        mean[0] = 0.5;
        g[3] = -1.0;
        EXPECT(has(align_check_model(who, l, mean.data(), var.data(), g.data()), "global_var holds a value that is not finite and > 0 (feature 3)"));
    }
    // a call: two utterances, T = 10 and 6, S = 3 and 2
    {
        const std::string who = "call: ";
        const std::vector<int> T{10, 6}, S{3, 2};
        std::vector<int> cls{0, 1, 2, 4, 0};
        std::vector<unsigned char> opt{0, 1, 0, 0, 1};
        std::vector<float> x(16 * 4, -1.f);
        auto run = [&](bool model, const std::vector<int>& t, const std::vector<int>& s) {
            return align_validate(who, l, model, (int)t.size(), t.data(), s.data(), cls.data(), opt.data(), x.data());
        };
        EXPECT(run(true, T, S).empty());
        EXPECT(has(run(false, T, S), "no model loaded"));
        EXPECT(has(align_validate(who, l, true, 0, T.data(), S.data(), cls.data(), opt.data(), x.data()), "n_utts = 0"));
        EXPECT(has(align_validate(who, l, true, 2, T.data(), S.data(), nullptr, opt.data(), x.data()), "NULL n_frames, n_states, classes, optional or x"));
        EXPECT(has(align_validate(who, l, true, 2, T.data(), S.data(), cls.data(), opt.data(), nullptr), "NULL"));
        EXPECT(has(run(true, {10, 0}, S), "utterance 1: n_frames = 0: at least 1 frame"));
        EXPECT(has(run(true, {41, 6}, S), "utterance 0: n_frames = 41 exceeds the handle's max_frames = 40"));
        EXPECT(has(run(true, T, {3, 0}), "utterance 1: n_states = 0: at least 1 state"));
        EXPECT(has(run(true, {1, 6}, S), "utterance 0: 2 mandatory states exceed n_frames = 1"));
        cls[3] = 5;
        EXPECT(has(run(true, T, S), "utterance 1: state 0: class 5 outside 0 .. n_classes - 1 = 4"));
        cls[3] = -1;
        EXPECT(has(run(true, T, S), "utterance 1: state 0: class -1 outside"));
        cls[3] = 4;
        opt[2] = 1;   // states 1 and 2 of utterance 0
        EXPECT(has(run(true, T, S), "utterance 0: states 1 and 2 are adjacent optional states"));
        opt[2] = 0;
        opt[3] = 1;   // the last state of utterance 0 is not next to the first of utterance 1: states 0 and 1 of utterance 1 are
        EXPECT(has(run(true, T, S), "utterance 1: states 0 and 1 are adjacent optional states"));
        opt[3] = 0;
        x[16 * 4 - 1] = std::numeric_limits<float>::quiet_NaN();
        EXPECT(has(run(true, T, S), "x holds a non-finite value (row 15)"));
        x[16 * 4 - 1] = -1.f;
        long long rows = 0;
        EXPECT(align_check_frames(who, l, 2, T.data(), x.data(), rows).empty() && rows == 16);
        rows = 0;
        EXPECT(has(align_check_frames(who, l, 2, nullptr, x.data(), rows), "NULL n_frames or x"));
    }
    {   // S > max_states and T S > max_cells, on buffers of their own size
        const std::string who = "call: ";
        const std::vector<int> T{30}, S9{9}, S7{7};
        std::vector<int> cls(9, 0);
        std::vector<unsigned char> opt(9, 0);
        std::vector<float> x(30 * 4, 0.f);
        EXPECT(has(align_validate(who, l, true, 1, T.data(), S9.data(), cls.data(), opt.data(), x.data()), "utterance 0: n_states = 9 exceeds the handle's max_states = 8"));
        EXPECT(has(align_validate(who, l, true, 1, T.data(), S7.data(), cls.data(), opt.data(), x.data()), "30 x 7 = 210 cells exceed the handle's max_cells = 200"));
    }

    // the planner: hand-made cases, then random ones against the invariants
    {
        const std::vector<int> T{10, 10, 30, 10, 10}, S{5, 5, 6, 2, 4};   // cells 50, 50, 180, 20, 40
        const std::vector<AlignChunk> c = align_plan_chunks(l, 5, T.data(), S.data());
        EXPECT(c.size() == 3 && c[0].count == 2 && c[1].first == 2 && c[1].count == 2 && c[1].cells == 200 && c[1].longest_states == 6 && c[2].first == 4 && c[2].count == 1);
        const std::vector<AlignChunk> by_utts = align_plan_chunks(limits(40, 8, 1 << 20, 2), 5, T.data(), S.data());
        EXPECT(by_utts.size() == 3 && by_utts[0].count == 2 && by_utts[1].count == 2 && by_utts[2].count == 1);
        const std::vector<AlignChunk> one = align_plan_chunks(limits(40, 8, 1 << 20, 64), 5, T.data(), S.data());
        EXPECT(one.size() == 1 && one[0].count == 5 && one[0].cells == 340 && one[0].rows == 70 && one[0].states == 22);
        EXPECT(align_plan_chunks(l, 0, T.data(), S.data()).empty());
    }
    std::mt19937 rng(12345);
    for (int round = 0; round < 400; ++round) {
        const AlignLimits lr = limits(4096, 2048, 4096ll * 2048 + (long long)(rng() % 5000000), 1 + (int)(rng() % 9));   // (every single utterance fits)
        const int n = 1 + (int)(rng() % 40);
        std::vector<int> T((size_t)n), S((size_t)n);
        for (int u = 0; u < n; ++u) { T[(size_t)u] = 1 + (int)(rng() % 4096); S[(size_t)u] = 1 + (int)(rng() % 2048); }
        check_plan(lr, T, S);
    }
    {   // the largest legal call shape: sums stay in 64 bits
        const AlignLimits big = limits(ALIGN_MAX_FRAMES, ALIGN_MAX_STATES, ALIGN_MAX_CELLS, ALIGN_MAX_UTTS);
        const std::vector<int> T(64, 1 << 18), S(64, 2048);   // 2^29 cells each
        check_plan(big, T, S);
        const std::vector<AlignChunk> c = align_plan_chunks(big, 64, T.data(), S.data());
        EXPECT(c.size() == 32 && c[0].cells == ALIGN_MAX_CELLS && c[0].count == 2);
    }
    if (failures) { std::fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    std::puts("ok");
    return 0;
}
