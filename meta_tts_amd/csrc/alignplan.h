// The host half of the mtts_align entries (align.h): the limits a handle is created with, the validation of a model and of a call, and the
// cut of a call's utterances into chunks.  Plain C++ with no device or runtime call in it, so that a stand-alone program can run it
// under the host sanitizers (tools/align_plan_check.cpp).
#pragma once
#include <cmath>
#include <string>
#include <vector>

namespace mtts {

constexpr int ALIGN_MAX_FEAT = 128;
constexpr int ALIGN_MAX_CLASSES = 512;
constexpr int ALIGN_MAX_STATES = 2048;               // two float64 rows of the sweep in LDS: 32 KiB
constexpr int ALIGN_MAX_FRAMES = 1 << 20;
constexpr long long ALIGN_MAX_CELLS = 1ll << 30;     // the alpha / gamma workspace is one float64 per cell
constexpr int ALIGN_MAX_UTTS = 65535;                // the statistics kernel has an utterance per grid row

struct AlignLimits {
    int n_feat = 0, n_classes = 0, max_frames = 0, max_states = 0;
    long long max_cells = 0;
    int max_utts = 0;
};

// utterances [first, first + count) of a call; rows = sum T, states = sum S, cells = sum T S
struct AlignChunk {
    int first = 0, count = 0;
    long long cells = 0, rows = 0, states = 0;
    int longest_states = 0;
};

// "" or the reason mtts_align_create refuses
inline std::string align_check_limits(const AlignLimits& l) {
    const std::string who = "mtts_align_create: ";
    auto outside = [&](const char* name, long long v, long long hi) { return who + name + " = " + std::to_string(v) + " outside 1 .. " + std::to_string(hi); };
    if (l.n_feat < 1 || l.n_feat > ALIGN_MAX_FEAT) return outside("n_feat", l.n_feat, ALIGN_MAX_FEAT);
    if (l.n_classes < 1 || l.n_classes > ALIGN_MAX_CLASSES) return outside("n_classes", l.n_classes, ALIGN_MAX_CLASSES);
    if (l.max_frames < 1 || l.max_frames > ALIGN_MAX_FRAMES) return outside("max_frames", l.max_frames, ALIGN_MAX_FRAMES);
    if (l.max_states < 1 || l.max_states > ALIGN_MAX_STATES) return outside("max_states", l.max_states, ALIGN_MAX_STATES) + " (two float64 rows must fit a workgroup's LDS)";
    if (l.max_cells < 1 || l.max_cells > ALIGN_MAX_CELLS) return outside("max_cells", l.max_cells, ALIGN_MAX_CELLS);
    if (l.max_utts < 1 || l.max_utts > ALIGN_MAX_UTTS) return outside("max_utts", l.max_utts, ALIGN_MAX_UTTS);
    return "";
}

// "" or the reason a model is refused: mean [V][F] finite, var [V][F] finite and > 0, global_var [F] finite and > 0
inline std::string align_check_model(const std::string& who, const AlignLimits& l, const double* mean, const double* var, const double* global_var) {
    if (!mean || !var || !global_var) return who + "NULL mean, var or global_var";
    for (long long k = 0; k < (long long)l.n_classes * l.n_feat; ++k) {
        const std::string at = "class " + std::to_string(k / l.n_feat) + ", feature " + std::to_string(k % l.n_feat);
        if (!std::isfinite(mean[k])) return who + "mean holds a non-finite value (" + at + ")";
        if (!std::isfinite(var[k]) || !(var[k] > 0.0)) return who + "var holds a value that is not finite and > 0 (" + at + ")";
    }
    for (int f = 0; f < l.n_feat; ++f)
        if (!std::isfinite(global_var[f]) || !(global_var[f] > 0.0)) return who + "global_var holds a value that is not finite and > 0 (feature " + std::to_string(f) + ")";
    return "";
}

// "" or the reason the frame counts and features of a call are refused (flat_start checks only these); adds the rows to `rows`
inline std::string align_check_frames(const std::string& who, const AlignLimits& l, int n_utts, const int* n_frames, const float* x, long long& rows) {
    if (n_utts < 1) return who + "n_utts = " + std::to_string(n_utts) + ": at least 1 utterance is needed";
    if (!n_frames || !x) return who + "NULL n_frames or x";
    for (int u = 0; u < n_utts; ++u) {
        const std::string at = who + "utterance " + std::to_string(u) + ": n_frames = " + std::to_string(n_frames[u]);
        if (n_frames[u] < 1) return at + ": at least 1 frame is needed";
        if (n_frames[u] > l.max_frames) return at + " exceeds the handle's max_frames = " + std::to_string(l.max_frames);
        rows += n_frames[u];
    }
    for (long long k = 0; k < rows * l.n_feat; ++k)
        if (!std::isfinite(x[k])) return who + "x holds a non-finite value (row " + std::to_string(k / l.n_feat) + ")";
    return "";
}

// "" or the reason a call of em_accumulate / posteriors / align is refused.  Everything is checked here, before any launch.
inline std::string align_validate(const std::string& who, const AlignLimits& l, bool have_model, int n_utts, const int* n_frames, const int* n_states, const int* classes,
                                  const unsigned char* optional, const float* x) {
    if (!have_model) return who + "no model loaded (mtts_align_set_model or mtts_align_flat_start)";
    if (n_utts < 1) return who + "n_utts = " + std::to_string(n_utts) + ": at least 1 utterance is needed";
    if (!n_frames || !n_states || !classes || !optional || !x) return who + "NULL n_frames, n_states, classes, optional or x";
    long long s0 = 0;
    for (int u = 0; u < n_utts; ++u) {
        const std::string at = who + "utterance " + std::to_string(u) + ": ";
        const int T = n_frames[u], S = n_states[u];
        if (T < 1) return at + "n_frames = " + std::to_string(T) + ": at least 1 frame is needed";
        if (T > l.max_frames) return at + "n_frames = " + std::to_string(T) + " exceeds the handle's max_frames = " + std::to_string(l.max_frames);
        if (S < 1) return at + "n_states = " + std::to_string(S) + ": at least 1 state is needed";
        if (S > l.max_states) return at + "n_states = " + std::to_string(S) + " exceeds the handle's max_states = " + std::to_string(l.max_states);
        if ((long long)T * S > l.max_cells)
            return at + std::to_string(T) + " x " + std::to_string(S) + " = " + std::to_string((long long)T * S) + " cells exceed the handle's max_cells = " + std::to_string(l.max_cells);
        int mandatory = 0;
        for (int s = 0; s < S; ++s) {
            const int c = classes[s0 + s];
            if (c < 0 || c >= l.n_classes) return at + "state " + std::to_string(s) + ": class " + std::to_string(c) + " outside 0 .. n_classes - 1 = " + std::to_string(l.n_classes - 1);
            if (optional[s0 + s] && s > 0 && optional[s0 + s - 1]) return at + "states " + std::to_string(s - 1) + " and " + std::to_string(s) + " are adjacent optional states";
            mandatory += optional[s0 + s] ? 0 : 1;
        }
        if (mandatory > T) return at + std::to_string(mandatory) + " mandatory states exceed n_frames = " + std::to_string(T);
        s0 += S;
    }
    long long rows = 0;
    return align_check_frames(who, l, n_utts, n_frames, x, rows);
}

// The utterances of a validated call, in order, cut into chunks of at most max_cells cells and max_utts utterances: a chunk takes
// utterances while they fit, so none is ever split and every chunk holds at least one.
inline std::vector<AlignChunk> align_plan_chunks(const AlignLimits& l, int n_utts, const int* n_frames, const int* n_states) {
    std::vector<AlignChunk> chunks;
    AlignChunk c;
    for (int u = 0; u < n_utts; ++u) {
        const long long cells = (long long)n_frames[u] * n_states[u];
        if (c.count > 0 && (c.cells + cells > l.max_cells || c.count >= l.max_utts)) {
            chunks.push_back(c);
            c = AlignChunk();
            c.first = u;
        }
        c.count += 1;
        c.cells += cells;
        c.rows += n_frames[u];
        c.states += n_states[u];
        c.longest_states = n_states[u] > c.longest_states ? n_states[u] : c.longest_states;
    }
    if (c.count > 0) chunks.push_back(c);
    return chunks;
}

}  // namespace mtts
