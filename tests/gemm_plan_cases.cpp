// The launch plans of the fp32 / bf16 GEMM launcher (meta_tts_amd/csrc/gemm_launch.h) at the launch shapes that decide something, one
// line per plan — tests/test_gemm_plan.py compares them with tests/golden/gemm_plan*.txt.  Host compiler, -DMTTS_EMU, no device, no
// Python: the planner is pure, operand pointers are null (or the address of `mark` where a pointer's presence is what decides) and
// nothing is launched — MTTS_LAUNCH is replaced by a stand-in that notes which kernel symbol it was handed.
//
//   <case>: <kernel symbol> grid (x, y, z) | S <split> place <0 / 1 / 2> start <slot> | ... per problem, launch order
//   <case>: kind <GemmKind of the last launch of a flush>
//   <case>: refused: <message>
//
// -DGEMM_PLAN_RECORD_PARENT: the same cases through a launcher WITHOUT a planner (the gemm.h this one replaced: gemm_launch /
// gemm_batch_begin / gemm_batch_end), read off the stand-in's arguments.  That is how the fixture was recorded, see the test.
#include <cxxabi.h>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <typeinfo>
#include <vector>

#include "compat.h"
#undef MTTS_LAUNCH
namespace mtts {
template <auto K, class... A> void plan_record(dim3 grid, const A&... a);
}
#define MTTS_LAUNCH(kernel, grid, block, stream, ...) plan_record<(kernel)>((grid), __VA_ARGS__)
#include "gemm.h"
#include "gemm_bf16.h"

namespace mtts {

struct Launched { std::string kernel; dim3 grid; std::vector<GemmArgs> one; std::vector<GemmMulti> multi; };   // (the arguments: one of the two, by value)
static std::vector<Launched> g_launched;
static void keep_args(Launched& l, const GemmArgs& g) { l.one.push_back(g); }
static void keep_args(Launched& l, const GemmMulti& mp) { l.multi.push_back(mp); }
template <class... A> static void keep_args(Launched&, const A&...) {}
template <auto K> struct KernelTag {};
template <auto K> static std::string kernel_symbol() {
    int status = 0;
    char* d = abi::__cxa_demangle(typeid(KernelTag<K>).name(), nullptr, nullptr, &status);   // "mtts::KernelTag<&void mtts::gemm_f32_kernel<0, 64, 64, 32, true, 2, 2, 0, 4, false>(mtts::GemmArgs)>"
    std::string name = d ? d : typeid(KernelTag<K>).name();
    free(d);
    const size_t a = name.find("<&"), b = name.rfind('(');
    if (a != std::string::npos && b != std::string::npos && b > a) name = name.substr(a + 2, b - a - 2);
    for (const char* drop : {"(", "void ", "mtts::"})
        for (size_t p; (p = name.find(drop)) != std::string::npos;) name.erase(p, std::string(drop).size());
    return name;
}
template <auto K, class... A> void plan_record(dim3 grid, const A&... a) {
    Launched l;
    l.kernel = kernel_symbol<K>();
    l.grid = grid;
    keep_args(l, a...);
    g_launched.push_back(l);
}

static const char* g_case = "";
static void print_head(const std::string& kernel, dim3 grid) { printf("%s: %s grid (%u, %u, %u)", g_case, kernel.c_str(), grid.x, grid.y, grid.z); }
static void print_kind(int kind) { printf("%s: kind %d\n", g_case, kind); }   // (GemmCtx::last_kind: of the last launch of a flush)
static void print_prob(int S, int place, int start) { printf(" | S %d place %d start %d", S, place, start); }
static void print_refusal(const char* why) { printf("%s: refused: %s\n", g_case, why); }

struct Problem { int form; GemmArgs g; int max_M, max_N, groups; int tile = 0; long long total_M = 0; };

#if defined(GEMM_PLAN_RECORD_PARENT)
static void print_launched(const GemmCtx& cx, const Launched& l) {
    print_head(l.kernel, l.grid);
    for (const GemmArgs& g : l.one) print_prob(g.splitk, cx.last_place, 0);
    for (const GemmMulti& mp : l.multi)
        for (int j = 0; j < mp.n; ++j) print_prob(mp.g[j].splitk, mp.xcd_group[j] == -2 ? 1 : (mp.xcd_group[j] == -3 ? 2 : 0), mp.start[j]);
    printf("\n");
}
static void run(const char* name, GemmCtx& cx, bool batch, const std::vector<Problem>& probs) {
    g_case = name;
    g_launched.clear();
    if (batch) gemm_batch_begin(cx);
    for (const Problem& p : probs) {
        const size_t before = g_launched.size();
        gemm_launch(cx, p.form, p.g, p.max_M, p.max_N, p.groups, nullptr, p.tile, 0.0, p.total_M);
        for (size_t i = before; i < g_launched.size(); ++i) {
            const Launched& l = g_launched[i];
            print_launched(cx, l);
        }
        if (g_launched.size() > before) print_kind(cx.last_kind);
        if (cx.error) { print_refusal(cx.error); cx.error = nullptr; }
    }
    if (batch) {
        const size_t before = g_launched.size();
        gemm_batch_end(cx, nullptr);
        for (size_t i = before; i < g_launched.size(); ++i) {
            const Launched& l = g_launched[i];
            print_launched(cx, l);
        }
        if (g_launched.size() > before) print_kind(cx.last_kind);
        if (cx.error) { print_refusal(cx.error); cx.error = nullptr; }
    }
}
#else
static void print_plans(const GemmCtx& cx, std::vector<GemmPending>& q, const GemmRequest& req) {
    int kind = -1;
    gemm_plan_queue(cx, q, req, [&](GemmLaunchPlan& pl) {
        if (pl.error) return print_refusal(pl.error);
        g_launched.clear();
        gemm_kernel_launch(pl.id, pl.mp, pl.grid, nullptr);   // (the stand-in: names the symbol the identity stands for)
        if (g_launched.empty()) return;   // (an identity that names no kernel launches nothing)
        print_head(g_launched[0].kernel, pl.grid);
        for (int i = 0; i < pl.mp.n; ++i) print_prob(pl.prob[i].splitk, pl.prob[i].place, pl.mp.start[i]);
        printf("\n");
        kind = pl.rec.kernel;
    });
    if (kind >= 0) print_kind(kind);
    q.clear();
}
static void print_single(const GemmCtx& cx, const GemmPending& p, int tile) {
    GemmLaunchPlan pl = gemm_plan_single(cx, p, tile);
    if (pl.error) return print_refusal(pl.error);
    g_launched.clear();
    gemm_kernel_launch(pl.id, pl.mp, pl.grid, nullptr);
    if (g_launched.empty()) return;
    print_head(g_launched[0].kernel, pl.grid);
    print_prob(pl.prob[0].splitk, pl.prob[0].place, 0);
    printf("\n");
    print_kind(pl.rec.kernel);
}
// gemm_launch's routing, with "print the plan" in the place of "issue it"
static void run(const char* name, GemmCtx& cx, bool batch, const std::vector<Problem>& probs) {
    g_case = name;
    std::vector<GemmPending> q;
    for (const Problem& p : probs) {
        GemmPending pd;
        if (!gemm_make_pending(cx, pd, p.form, p.g, p.max_M, p.max_N, p.groups, 0.0, p.total_M, 0.0, -1)) {
            if (cx.error) { print_refusal(cx.error); cx.error = nullptr; }
            continue;
        }
        if (p.tile == 0) {
            q.push_back(pd);
            if (!batch || (int)q.size() == kGemmMultiMax) print_plans(cx, q, GemmRequest{});
        } else if (pd.g.A2 && !batch) {
            q.push_back(pd);
            print_plans(cx, q, gemm_family_request(p.tile));
        } else print_single(cx, pd, p.tile);
    }
    if (!q.empty()) print_plans(cx, q, GemmRequest{});
}
#endif

// ---- the problems: FastSpeech2's own (d = 256, FFT conv k = 9 over 1024 filters, PostNet k = 5 over 512 with an 80-channel output) ----
static float mark;                       // a pointer whose presence decides (A2 / B2, bf16 planes, dimptr, LnFuse::y, colsum)
static int mark_i;
static int host_dims[8];
static GemmArgs nt(int M, int N, int K) { GemmArgs g; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldb = K; g.ldc = N; return g; }
static Problem P(int form, const GemmArgs& g, int max_M, int max_N, int groups = 1, int tile = 0, long long total_M = 0) { return Problem{form, g, max_M, max_N, groups, tile, total_M}; }
static Problem linear(int rows, int N, int K, int tile = 0) { return P(GEMM_NT, nt(rows, N, K), rows, N, 1, tile); }
static Problem conv_fwd(int rows, int cin, int cout, int k) { GemmArgs g = nt(rows, cout, k * cin); g.lda = cin; return P(GEMM_NT, g, rows, cout); }
static Problem conv_dgrad(int rows, int cin, int cout, int k) {
    GemmArgs g = nt(rows, cin, k * cout);
    g.lda = cout; g.ldb = k * cin; g.taps = k; g.tap_k = cout; g.tap_bstride = cin;
    return P(GEMM_NN, g, rows, cin);
}
static Problem conv_wgrad(int rows, int cin, int cout, int k) { GemmArgs g = nt(cout, k * cin, rows); g.lda = cout; g.ldb = cin; g.ldc = k * cin; return P(GEMM_TN, g, cout, k * cin, 1, 0, cout); }
static Problem dual(Problem p) { p.g.A2 = &mark; p.g.B2 = &mark; return p; }
static Problem tiled(Problem p, int tile) { p.tile = tile; return p; }
// `groups` tasks of ragged row counts (host_dims known): M-ragged (forward, dgrad: sel 0) or K-ragged (wgrad: sel 2)
static Problem tasks(Problem p, int groups, int sel, bool with_host_dims = true) {
    long long total = 0;
    int mx = 0;
    for (int z = 0; z < groups; ++z) { host_dims[z] = 1500 + 137 * ((z * 5) % 8); total += host_dims[z]; mx = std::max(mx, host_dims[z]); }
    p.g.dimptr = &mark_i; p.g.dim_sel = sel; p.g.host_dims = with_host_dims ? host_dims : nullptr;
    p.groups = groups;
    if (sel == 0) { p.max_M = mx; p.g.M = mx; p.total_M = total; }
    else { p.g.K = mx; p.total_M = (long long)p.max_M * groups; }
    return p;
}
static Problem planes(Problem p, bool only) { p.g.Ah = (const bf16_t*)&mark; p.g.Bh = (const bf16_t*)&mark; p.g.plane_only = only; return p; }
static Problem ln(Problem p) { p.g.ln.y = &mark; return p; }

static void cases() {
    static int ctrs[4];
    GemmCtx plain, ws, bf, bfws;   // no workspace (the kernel entries) / a bound workspace (a handle); fp32 / bf16 mode
    ws.wsp.ws = bfws.wsp.ws = &mark; ws.wsp.ctr = bfws.wsp.ctr = ctrs;
    bf.bf16 = bfws.bf16 = true;
    const int R1 = 1984, R8 = 17047;   // rows of a single-task rank's batch / of the 8-task meta-batch
    // stand-alone or multi: the 768-workgroup line
    run("alone/under", ws, false, {linear(R1, 256, 256)});
    run("alone/at-768", ws, false, {linear(64 * 192, 256, 256)});
    run("alone/over", ws, false, {linear(64 * 192 + 1, 256, 256)});
    // split-K of the long chains of an under-filled batch
    run("splitk/k9-dgrad-chain", ws, false, {conv_dgrad(R1, 256, 1024, 9)});
    run("splitk/k9-pair", ws, true, {conv_wgrad(R1, 256, 1024, 9), conv_dgrad(R1, 256, 1024, 9)});
    run("splitk/cap-8", ws, false, {linear(64, 64, 16384)});
    run("splitk/cap-nch16", ws, false, {linear(64, 64, 530)});
    run("splitk/cap-nch16-dual", ws, false, {dual(linear(64, 64, 530))});
    // (1600 tile slots over ragged groups that hold 100 tiles' rows: S = 4 would need 6400 of the workspace's 4096 slabs; the second problem's fit)
    run("splitk/workspace-budget", ws, true, {P(GEMM_NT, nt(64 * 200, 64, 16384), 64 * 200, 64, 8, 0, 64 * 100), linear(64, 64, 16000)});
    { GemmCtx c = ws; c.no_splitk = true; run("splitk/no_splitk", c, false, {conv_dgrad(R1, 256, 1024, 9)}); }
    run("splitk/no-workspace", plain, false, {conv_dgrad(R1, 256, 1024, 9)});
    // placement: task-per-XCD schedule (8 groups; 4 / 2 under MTTS_XCD_SCHED_MIN_GROUPS), panel order, XCD-grouped order
    for (int groups : {8, 4, 2}) {
        const std::string n = std::to_string(groups);
        run(("place/tasks" + n + "-fwd").c_str(), ws, false, {tasks(conv_fwd(0, 256, 1024, 9), groups, 0)});
        run(("place/tasks" + n + "-pair").c_str(), ws, true, {tasks(conv_wgrad(0, 256, 1024, 9), groups, 2), tasks(conv_dgrad(0, 256, 1024, 9), groups, 0)});
        run(("place/tasks" + n + "-no-host-dims").c_str(), ws, false, {tasks(conv_fwd(0, 256, 1024, 9), groups, 0, false)});
    }
    run("place/panel-B-larger", ws, false, {conv_fwd(600, 256, 1024, 9)});
    run("place/panel-B-smaller", ws, false, {linear(600, 256, 256)});
    run("place/panel-B-larger-tile64", ws, false, {tiled(conv_fwd(600, 256, 1024, 9), 64)});
    run("place/panel-pair", ws, true, {conv_fwd(600, 256, 1024, 9), linear(600, 256, 256)});
    // BK: 32 for long K-contiguous panels, 16 otherwise
    run("bk/NT-K1024", ws, false, {linear(R8, 1024, 1024)});
    { Problem p = linear(R8, 1024, 1024); p.form = GEMM_NN; run("bk/NN-K1024", ws, false, {p}); }
    { Problem p = linear(R8, 1024, 1024); p.form = GEMM_TN; run("bk/TN-K1024", ws, false, {p}); }
    { Problem p = linear(R8, 1024, 1024); p.g.table = (const GemmGroupDesc*)&mark; run("bk/table-K1024", ws, false, {p}); }
    run("bk/NT-K1023", ws, false, {linear(R8, 1024, 1023)});
    run("bk/tap80-alone", ws, false, {conv_dgrad(R8 * 4, 512, 80, 5)});
    run("bk/tap80-multi", ws, true, {conv_dgrad(R8, 512, 80, 5), conv_wgrad(R8, 512, 80, 5)});
    run("bk/tap72-alone", ws, false, {conv_dgrad(R8 * 4, 512, 72, 5)});   // (no channel count of the model: a tap that is no multiple of 16 keeps the generic K-loop)
    run("bk/tap72-multi", ws, true, {conv_dgrad(R8, 512, 72, 5), conv_wgrad(R8, 512, 72, 5)});
    run("bk/tap1024-multi", ws, true, {conv_dgrad(R8, 256, 1024, 9), conv_wgrad(R8, 256, 1024, 9)});
    run("bk/shortK-multi", ws, true, {linear(R8, 256, 256), linear(R8, 768, 256)});
    { GemmCtx c = ws; c.prefer_bk16 = true; run("bk/prefer_bk16", c, true, {conv_dgrad(R8, 256, 1024, 9), conv_wgrad(R8, 256, 1024, 9)}); }
    run("bk/tile-codes", ws, false, {linear(R1, 256, 256, 64), linear(R1, 256, 256, 128), linear(R1, 256, 256, 1064), linear(R1, 256, 256, 2064),
                                     linear(R1, 256, 256, 3064), linear(R1, 256, 256, 3128), linear(R1, 256, 256, 2128), linear(R1, 256, 256, 4064)});
    // a batch goes out when it holds kGemmMultiMax problems
    run("multi/six", ws, true, {linear(R1, 256, 256), linear(R1, 256, 512), linear(R1, 256, 768), linear(R1, 512, 256), linear(R1, 768, 256), linear(R1, 1024, 256)});
    run("multi/seven", ws, true, {linear(R1, 256, 256), linear(R1, 256, 512), linear(R1, 256, 768), linear(R1, 512, 256), linear(R1, 768, 256), linear(R1, 1024, 256), linear(R8, 80, 256)});
    // dual-source problems exist in the multi-problem kernels only
    run("dual/alone", ws, false, {dual(linear(R8, 1024, 256))});
    run("dual/alone-longK", ws, false, {dual(linear(R8, 1024, 1024))});
    for (int tile : {64, 1064, 2064, 3064, 4064, 128}) run(("dual/tile-" + std::to_string(tile)).c_str(), ws, false, {tiled(dual(linear(R1, 256, 256)), tile)});
    run("dual/tile-128-bf16", bfws, false, {tiled(dual(linear(R1, 256, 256)), 128)});
    run("dual/tile-in-open-batch", ws, true, {linear(R1, 256, 256), tiled(dual(linear(R1, 256, 256)), 64)});
    run("dual/pair", ws, true, {dual(conv_dgrad(R1, 256, 1024, 9)), conv_wgrad(R1, 256, 1024, 9)});
    // bf16 mode: the 128x128 tile from 512 workgroups of it
    run("bf16/alone-512", bfws, false, {linear(128 * 128, 512, 256)});
    run("bf16/alone-508", bfws, false, {linear(128 * 127, 512, 256)});
    run("bf16/pair-512", bfws, true, {linear(128 * 64, 512, 256), linear(128 * 64, 512, 512)});
    run("bf16/pair-510", bfws, true, {linear(128 * 64, 512, 256), linear(128 * 63 + 64, 512, 512)});
    run("bf16/pair-dual", bfws, true, {dual(linear(128 * 64, 512, 256)), linear(128 * 64, 512, 512)});
    run("bf16/planes-alone", bfws, false, {planes(conv_fwd(R8, 256, 1024, 9), false), planes(linear(R8, 1024, 256), false), planes(linear(R1, 256, 256), true)});
    run("bf16/planes-pair", bfws, true, {planes(conv_fwd(R1, 256, 1024, 9), true), conv_wgrad(R1, 256, 1024, 9)});
    run("bf16/planes-with-fp32-only", bfws, true, {planes(conv_fwd(R1, 256, 1024, 9), true), dual(conv_dgrad(R1, 512, 80, 5)), conv_wgrad(R1, 512, 80, 5)});
    run("bf16/tap80-keeps-fp32", bfws, true, {conv_dgrad(R8, 512, 80, 5), conv_wgrad(R8, 512, 80, 5)});
    run("bf16/plane-only-outside-bf16-mode", ws, false, {planes(linear(R1, 256, 256), true)});
    run("bf16/planes-dropped-outside-bf16-mode", ws, false, {planes(linear(R1, 256, 256), false)});
    // row-complete LayerNorm epilogue
    run("ln/alone-small", ws, false, {ln(linear(R1, 256, 1024))});
    run("ln/alone-large", ws, false, {ln(linear(R8 * 4, 256, 1024))});
    run("ln/alone-large-shortK", ws, false, {ln(linear(R8 * 4, 256, 256))});
    run("ln/N-512", ws, false, {ln(linear(R1, 512, 1024))});
    run("ln/no-counters", plain, false, {ln(linear(R1, 256, 1024))});
    run("ln/tile-128", ws, false, {tiled(ln(linear(R1, 256, 1024)), 128)});
    run("ln/bf16-mode", bfws, false, {ln(linear(R1, 256, 1024))});
}

}  // namespace mtts

int main() {
    mtts::cases();
    return 0;
}
