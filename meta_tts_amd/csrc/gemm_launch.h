// Host half of gemm.h (included at its end): PLAN — pure host code that turns the queued problems and the context's read-only settings
// into a GemmLaunchPlan (kernel identity, grid, per-problem split / placement / start slot, profiler record; no HIP call, no write to the
// context) — and ISSUE, which binds the workspace pointers into a plan's arguments, brackets and makes the launch and keeps the books.
// tests/test_gemm_plan.py pins the plans of the workload's deciding shapes on a CPU.
#pragma once
#include "gemm.h"

namespace mtts {

constexpr int kGemmXcdSwizzle = 1;     // XCD-grouped tile order of the plain grids (xcd_group_remap)
constexpr int kGemmDefaultBk = 16;     // K-slice of the register-staged kernels (32 for long K-contiguous panels, see gemm_plan_single)
constexpr bool kGemmDefaultPipe = true;  // software-pipelined K-loop
inline int gemm_kloop_variant() { return knobs().kloop; }   // K-loop variant of the pipelined 64x64 kernels (gemm_f32_kloop: KL): same k order in every accumulator chain, bit-identical
// The KL >= 1 loops step their operand pointers by loop-invariant distances, which needs conv taps that are whole multiples of the K-slice
// (every channel count of the model is a multiple of 16; anything else keeps the generic KL = 0 loop)
inline int gemm_kloop_for(const GemmArgs& g, int bk) {
    const bool ok = (g.taps <= 1 || g.tap_k % bk == 0) && (g.a_tap_k >= 0x40000000 || g.a_tap_k % bk == 0);
    return ok ? gemm_kloop_variant() : 0;
}

// Split-K workspace (partial tiles + tile counters): used by one GemmCtx, allocated once from its owner's heap by the owner's create.
struct GemmWorkspace { float* ws = nullptr; int* ctr = nullptr; };
constexpr long long kSplitWsFloats = 16ll << 20;  // 64 MB of partial tiles
constexpr int kSplitCtrs = 1 << 16;
constexpr int kLnCtrs = 4096;                     // the last kLnCtrs counters: arrival counters of row-complete LayerNorm epilogues (LnFuse)

// Launch batching: between gemm_batch_begin() and gemm_batch_end() every eligible gemm_launch (automatic tile choice) is queued
// instead of launched; gemm_batch_end() issues the queue as ONE launch (gemm_f32_multi_kernel / gemm_glds_multi_kernel).
// The caller guarantees the queued problems are mutually independent and that nothing launched before gemm_batch_end()
// reads their outputs (engine: the wgrad / dgrad pair of a layer, dQ / dK / dV of an attention block).
struct GemmPending { int form; GemmArgs g; int max_M, max_N, groups; double flops, rows, bytes; int tag = -1; };   // tag: the caller's index of the problem (GemmCtx::note)
struct GemmBatch { bool open = false; std::vector<GemmPending> q; };
// What a caller asks of a launch beyond the problems themselves.  tile: the tile code of a stand-alone launch (0: automatic).  family: the
// kernel family forced on a multi-problem launch — 16 / 32 (BK of the register-staged kernel) or 4064 (LDS-DMA) —, family_tile its block
// tile in bf16 mode (explicit tile codes of dual-source problems, mtts_gemm_f32_grouped).
struct GemmRequest { int tile = 0, family = 0, family_tile = 0; };
inline GemmRequest gemm_family_request(int tile_code) {
    const int code = tile_code % 10000;
    return GemmRequest{0, code == 4064 ? 4064 : (code / 2000 ? 32 : 16), code % 1000 == 128 ? 128 : 64};
}

// Every piece of MUTABLE launcher state — the launch-batching queue, the per-launch profiler, the split-K workspace —
// lives in a context owned by one handle (Engine / Vocoder / ...), so two handles on two host threads share nothing
// (include/mtts.h conventions).  The workspace is allocated by the owner's create, never lazily; a context without one (the
// handle-less kernel entry points) never splits K.  One context = one stream (the split-K slabs / counters of consecutive
// launches are reused in stream order).
struct GemmCtx {
    GemmBatch batch;
    GemmProfiler prof;
    GemmWorkspace wsp;
    int last_kind = GK_OTHER;  // kernel kind of the last launch (profiler)
    long long plane_problems = 0;   // problems launched on the plane-staged K-loop (bf16 mode; a test / diagnostic counter)
    bool bf16 = false;         // numerics mode of the owner: bf16 operand family (gemm_bf16.h) for every problem it can take
    const char* error = nullptr;   // sticky: a launch the launcher refused (the C ABI entry points turn it into an error return)
    bool prefer_bk16 = false;   // multi-problem launches of this context take the BK = 16 kernels (20 KB of LDS per workgroup instead of 37) whatever their K
    int wave_prio = 0;      // GemmArgs::wave_prio of every launch of this context (the engine sets it on the critical stream's context while side streams carry work)
    bool no_glds = false;   // never pick the LDS-DMA kernels (48 KB of LDS per workgroup: a side-stream launch would leave no LDS for the main stream's)
    bool no_splitk = false;   // never split K (the split factor follows the batch's size: an owner whose results must not depend on what else is in the batch sets it)
    // What the launcher decided for the problems queued under a tag (gemm_enqueue: mtts_gemm_f32_grouped): the split factor and the
    // placement (0 plain / XCD-grouped order, 1 task-per-XCD schedule, 2 panel order).  Host bookkeeping only.
    int note_splitk[kGemmMultiMax] = {0}, note_place[kGemmMultiMax] = {0};
    int last_place = 0;   // placement of the last stand-alone launch
    void note(int tag, int S, int place) { if (tag >= 0 && tag < kGemmMultiMax) { note_splitk[tag] = S; note_place[tag] = place; } }
    DevHeap* heap = nullptr;   // the owner's: the workspace and the profiler's events come from it and go back with it
    int alloc_workspace(DevHeap& h) {
        heap = &h;
        if (wsp.ws) return 0;
        if (h.alloc(wsp.ws, kSplitWsFloats * sizeof(float)) != hipSuccess || h.alloc_zeroed(wsp.ctr, (kSplitCtrs + 16) * sizeof(int)) != hipSuccess) {
            h.give_back(wsp.ws);
            h.give_back(wsp.ctr);
            return -1;
        }
        return 0;
    }
};

// ---- kernel identity: which kernel symbol a plan names ---------------------------------------------------------------------------
// LDS-DMA family (gemm_glds.h, device builds only).  Round 5: with the interleaved K-loop (KL = 4) the register-staged kernels beat it in the
// latency regime it was built for (profiles/r05_kloop_ab.md), so the automatic choice takes it only under MTTS_GLDS=1 (knobs.h) — GemmCtx::no_glds
// (engine.h: set_regime) can then still veto it per pass; tile code 4064 selects the family explicitly (kernel tests, micro-benchmarks).
enum GemmFamily { GF_F32 = 0, GF_GLDS = 1, GF_BF16 = 2 };   // register-staged fp32 (gemm.h), LDS-DMA (gemm_glds.h), bf16 operands (gemm_bf16.h)
struct GemmKernelId {
    int family = GF_F32;
    bool multi = false;   // a multi-problem kernel (GemmMulti) / a stand-alone one (GemmArgs)
    int form = GEMM_NT;   // stand-alone: the GemmForm; bf16 family: GEMM_NT_H = the plane-staged K-loop (multi: gemm_bf16_multi_planes_kernel)
    int tile = 64, bk = kGemmDefaultBk;
    bool pipe = kGemmDefaultPipe;   // register-staged stand-alone kernels
    int kl = 0;           // K-loop variant of the pipelined 64x64 register-staged kernels
    bool dual = false;    // multi: the kernel also runs second sources (GemmArgs::A2)
    bool lnf = false;     // row-complete LayerNorm epilogue (LnFuse)
    int pf = 1;           // bf16 family: slices in flight
    int ablate = 0;       // MTTS_GEMM_ABLATION builds: diagnostic stage ablation (gemm_f32_kloop)
};
// the GemmKind (one per real kernel symbol) of an identity; GK_OTHER: nothing the profiler's table names
inline int gemm_kind_of(const GemmKernelId& k) {
    const bool t64 = k.tile == 64, t128 = k.tile == 128;
    switch (k.family) {
    case GF_GLDS: return k.multi ? (k.dual ? GK_GLDS_MULTI_DUAL : GK_GLDS_MULTI) : GK_GLDS + k.form;
    case GF_BF16:
        if (k.multi) return t128 ? (k.dual ? GK_BF16_MULTI128_DUAL : GK_BF16_MULTI128) : k.form == GEMM_NT_H ? GK_BF16_MULTI64_PLANES : (k.dual ? GK_BF16_MULTI64_DUAL : GK_BF16_MULTI64);
        if (k.form == GEMM_NT_H) return t128 ? GK_BF16_128_H : (k.bk == 64 ? GK_BF16_64_H64 : GK_BF16_64_H32);
        return t128 ? GK_BF16_128 + k.form : (t64 ? GK_BF16_64 + k.form : GK_OTHER);
    default:
        if (k.multi) return k.bk == 32 ? (k.dual ? GK_MULTI32_DUAL : GK_MULTI32) : (k.dual ? GK_MULTI16_DUAL : GK_MULTI16);
        if (t128) return GK_F32_128 + k.form;
        return t64 && k.pipe ? (k.bk == 32 ? GK_F32_64_BK32 : GK_F32_64_BK16) + k.form : GK_OTHER;
    }
}
#if defined(MTTS_EMU)
constexpr bool kGemmHasGlds = false;
#else
constexpr bool kGemmHasGlds = true;
inline void gemm_glds_launch(const GemmKernelId& k, const GemmArgs& g, dim3 grid, hipStream_t stream);
inline void gemm_glds_multi_launch(const GemmKernelId& k, const GemmMulti& mp, dim3 grid, hipStream_t stream);
#endif
inline int gemm_glds_mode() { return knobs().glds; }
inline bool gemm_glds_ok(const GemmArgs& g) { return !(g.taps > 1 && g.tap_k % 32 != 0); }
// bf16 operand family (gemm_bf16.h)
inline bool gemm_bf16_ok(const GemmArgs& g);
inline bool gemm_bf16_planes_ok(int form, const GemmArgs& g);
inline GemmKernelId gemm_bf16_id(int form, const GemmArgs& g, int T, int pf_req);   // stand-alone; pf_req: tile code / 1000 (MTTS_BF16_PF_SWEEP builds)
inline GemmKernelId gemm_bf16_multi_id(const GemmMulti& mp, int T, bool dual);
inline void gemm_bf16_launch(const GemmKernelId& k, const GemmArgs& g, dim3 grid, hipStream_t stream);
inline void gemm_bf16_multi_launch(const GemmKernelId& k, const GemmMulti& mp, dim3 grid, hipStream_t stream);

// Register-staged fp32 kernels: every instantiation the library carries, once.  An identity outside the table launches nothing.
constexpr int gemm_f32_key(int tile, int bk, bool pipe, int kl, bool lnf) { return (((tile * 64 + bk) * 2 + pipe) * 8 + kl) * 2 + lnf; }
template <int F>
inline void gemm_f32_launch(const GemmKernelId& k, const GemmArgs& g, dim3 grid, hipStream_t stream) {
    const dim3 block(256);
    switch (gemm_f32_key(k.tile, k.bk, k.pipe, k.kl, k.lnf)) {
    case gemm_f32_key(64, 32, true, 4, false): MTTS_LAUNCH((gemm_f32_kernel<F, 64, 64, 32, true, 2, 2, 0, 4>), grid, block, stream, g); break;
    case gemm_f32_key(64, 32, true, 1, false): MTTS_LAUNCH((gemm_f32_kernel<F, 64, 64, 32, true, 2, 2, 0, 1>), grid, block, stream, g); break;
    case gemm_f32_key(64, 32, true, 0, false): MTTS_LAUNCH((gemm_f32_kernel<F, 64, 64, 32, true, 2, 2, 0, 0>), grid, block, stream, g); break;
    case gemm_f32_key(64, 16, true, 4, false): MTTS_LAUNCH((gemm_f32_kernel<F, 64, 64, 16, true, 2, 2, 0, 4>), grid, block, stream, g); break;
    case gemm_f32_key(64, 16, true, 0, false): MTTS_LAUNCH((gemm_f32_kernel<F, 64, 64, 16, true, 2, 2, 0, 0>), grid, block, stream, g); break;
    case gemm_f32_key(64, 32, false, 0, false): MTTS_LAUNCH((gemm_f32_kernel<F, 64, 64, 32, false>), grid, block, stream, g); break;
    case gemm_f32_key(64, 16, false, 0, false): MTTS_LAUNCH((gemm_f32_kernel<F, 64, 64, 16, false>), grid, block, stream, g); break;
    case gemm_f32_key(128, 32, true, 0, false): MTTS_LAUNCH((gemm_f32_kernel<F, 128, 128, 32, true>), grid, block, stream, g); break;
    case gemm_f32_key(128, 32, false, 0, false): MTTS_LAUNCH((gemm_f32_kernel<F, 128, 128, 32, false>), grid, block, stream, g); break;
    case gemm_f32_key(128, 16, true, 0, false): MTTS_LAUNCH((gemm_f32_kernel<F, 128, 128, 16, true>), grid, block, stream, g); break;
    case gemm_f32_key(128, 16, false, 0, false): MTTS_LAUNCH((gemm_f32_kernel<F, 128, 128, 16, false>), grid, block, stream, g); break;
    // row-complete LayerNorm epilogue (LnFuse): NT only
    case gemm_f32_key(64, 32, true, 4, true): if constexpr (F == GEMM_NT) MTTS_LAUNCH((gemm_f32_kernel<GEMM_NT, 64, 64, 32, true, 2, 2, 0, 4, true>), grid, block, stream, g); break;
    case gemm_f32_key(64, 16, true, 4, true): if constexpr (F == GEMM_NT) MTTS_LAUNCH((gemm_f32_kernel<GEMM_NT, 64, 64, 16, true, 2, 2, 0, 4, true>), grid, block, stream, g); break;
    }
}
inline void gemm_f32_multi_launch(const GemmKernelId& k, const GemmMulti& mp, dim3 grid, hipStream_t stream) {
    const dim3 block(256);
    switch (gemm_f32_key(64, k.bk, k.dual, k.kl, k.lnf)) {   // (the `pipe` position carries `dual`)
    case gemm_f32_key(64, 32, false, 4, false): MTTS_LAUNCH((gemm_f32_multi_kernel<64, 64, 32, 4>), grid, block, stream, mp); break;
    case gemm_f32_key(64, 32, false, 1, false): MTTS_LAUNCH((gemm_f32_multi_kernel<64, 64, 32, 1>), grid, block, stream, mp); break;
    case gemm_f32_key(64, 32, false, 0, false): MTTS_LAUNCH((gemm_f32_multi_kernel<64, 64, 32, 0>), grid, block, stream, mp); break;
    case gemm_f32_key(64, 32, false, 4, true): MTTS_LAUNCH((gemm_f32_multi_kernel<64, 64, 32, 4, true>), grid, block, stream, mp); break;
    case gemm_f32_key(64, 16, false, 4, false): MTTS_LAUNCH((gemm_f32_multi_kernel<64, 64, 16, 4>), grid, block, stream, mp); break;
    case gemm_f32_key(64, 16, false, 0, false): MTTS_LAUNCH((gemm_f32_multi_kernel<64, 64, 16, 0>), grid, block, stream, mp); break;
    case gemm_f32_key(64, 16, false, 4, true): MTTS_LAUNCH((gemm_f32_multi_kernel<64, 64, 16, 4, true>), grid, block, stream, mp); break;
    case gemm_f32_key(64, 32, true, 4, false): MTTS_LAUNCH((gemm_f32_multi_dual_kernel<64, 64, 32, 4>), grid, block, stream, mp); break;
    case gemm_f32_key(64, 32, true, 1, false): MTTS_LAUNCH((gemm_f32_multi_dual_kernel<64, 64, 32, 1>), grid, block, stream, mp); break;
    case gemm_f32_key(64, 32, true, 0, false): MTTS_LAUNCH((gemm_f32_multi_dual_kernel<64, 64, 32, 0>), grid, block, stream, mp); break;
    case gemm_f32_key(64, 16, true, 4, false): MTTS_LAUNCH((gemm_f32_multi_dual_kernel<64, 64, 16, 4>), grid, block, stream, mp); break;
    case gemm_f32_key(64, 16, true, 0, false): MTTS_LAUNCH((gemm_f32_multi_dual_kernel<64, 64, 16, 0>), grid, block, stream, mp); break;
    }
}
// kernel identity -> launch.  mp: the arguments of a multi-problem kernel; a stand-alone kernel takes mp.g[0].
inline void gemm_kernel_launch(const GemmKernelId& k, const GemmMulti& mp, dim3 grid, hipStream_t stream) {
    const GemmArgs& g = mp.g[0];
    if (k.family == GF_BF16) return k.multi ? gemm_bf16_multi_launch(k, mp, grid, stream) : gemm_bf16_launch(k, g, grid, stream);
#if !defined(MTTS_EMU)
    if (k.family == GF_GLDS) return k.multi ? gemm_glds_multi_launch(k, mp, grid, stream) : gemm_glds_launch(k, g, grid, stream);
#endif
    if (k.multi) return gemm_f32_multi_launch(k, mp, grid, stream);
#if defined(MTTS_GEMM_ABLATION)
#define MTTS_ABL(A) if (k.ablate == A && k.form == GEMM_NT) { MTTS_LAUNCH((gemm_f32_kernel<GEMM_NT, 64, 64, 16, true, 2, 2, A>), grid, dim3(256), stream, g); return; }
    MTTS_ABL(1) MTTS_ABL(2) MTTS_ABL(3) MTTS_ABL(4) MTTS_ABL(7) MTTS_ABL(8) MTTS_ABL(15) MTTS_ABL(6) MTTS_ABL(14)
#undef MTTS_ABL
#endif
    if (k.form == GEMM_NT) gemm_f32_launch<GEMM_NT>(k, g, grid, stream);
    else if (k.form == GEMM_NN) gemm_f32_launch<GEMM_NN>(k, g, grid, stream);
    else if (k.form == GEMM_TN) gemm_f32_launch<GEMM_TN>(k, g, grid, stream);
}

// ---- plan -----------------------------------------------------------------------------------------------------------------------
// n-tiles of a problem's grid: the tiles of C plus the column-sum tile (GemmArgs::colsum)
inline int gemm_tiles_n(const GemmArgs& g, int max_N, int t) { return (max_N + t - 1) / t + (g.colsum ? 1 : 0); }
// workgroups of a problem at tile t, over the rows its groups really have (rows = their sum): the launcher's measure of a launch's size
inline double gemm_wgs(const GemmArgs& g, double rows, int max_N, int t) { return std::ceil(rows / t) * gemm_tiles_n(g, max_N, t); }
inline double gemm_wgs(const GemmPending& p, int t) { return gemm_wgs(p.g, p.rows, p.max_N, t); }
// Launches up to this many 64x64 workgroups are the latency regime: few workgroups per CU.  Split-K, the panel order and (MTTS_GLDS=1) the
// LDS-DMA kernels apply there — larger launches take the plain register-staged kernels (5 vs 3 workgroups per CU resident: +3 % on the
// full 8-task step) — and a single queued problem stays a multi-problem launch there (gemm_goes_alone).
constexpr double kGemmLatencyWgs = 768.0;
// block tile of a bf16 launch: 128x128 once the launch still fills the chip twice over with it (the MFMA rate is 16x the fp32 kernels':
// a 64x64 tile moves 1 byte per 16 flop through the L2 -> LDS path), 64x64 for under-filled launches
inline int gemm_bf16_tile(double wgs128) { return wgs128 >= 512.0 ? 128 : 64; }

// LnFuse (requested by the caller through g.ln.y): can this launch carry it — the engine asks first.
inline bool gemm_ln_fusable(const GemmCtx& cx, int form, const GemmArgs& g, int max_M, int groups) {
    return form == GEMM_NT && !cx.bf16 && cx.wsp.ctr != nullptr && gemm_kloop_variant() == 4 && g.N <= 256 && g.N % 4 == 0 && !g.table && !g.c_rowmap && !g.A2 &&
           !(g.flags & GEMM_ACCUM) && !g.colsum && (long long)groups * ((max_M + 63) / 64) <= kLnCtrs;
}
// ... and its counter slice: ln_off = first of its counters among the launch's (-1: no epilogue), `used` = counters handed out so far.
// false: the request cannot be honoured.
inline bool gemm_ln_plan(const GemmCtx& cx, const GemmPending& p, GemmArgs& g, int tile, int& used, int& ln_off) {
    ln_off = -1;
    if (!g.ln.y) return true;
    const int tiles_m = (p.max_M + 63) / 64;
    if (tile != 64 || !gemm_ln_fusable(cx, p.form, g, p.max_M, p.groups) || used + p.groups * tiles_m > kLnCtrs) return false;
    ln_off = used;
    g.tiles_pg = tiles_m;   // (counter stride between groups; the problem is never split, so the split-K meaning of the field is free)
    g.splitk = 1;
    used += p.groups * tiles_m;
    return true;
}

// Task-per-XCD schedule (XcdSched) of a problem: 8 (opt-in 4 / 2) groups whose sizes the caller knows on the host, whole tiles.  MTTS_XCD_SCHED=0: off.
inline bool gemm_xcd_sched_for(GemmArgs& g, int max_M, int max_N, int groups, int S, int tile) {
    g.xs.on = 0;
    if (!knobs().xcd_sched || (groups != 8 && groups != 4 && groups != 2) || groups < knobs().xcd_sched_min_groups || !g.host_dims || !g.dimptr || g.table || S != 1) return false;
    int dims[8] = {0};
    for (int z = 0; z < groups; ++z) dims[z] = g.host_dims[z] * g.dim_mult;
    const int tn = gemm_tiles_n(g, max_N, tile);
    if (g.dim_sel == 0) xcd_sched_build(g.xs, dims, 1, tn, 0, tile, groups);
    else xcd_sched_build(g.xs, dims, 2, 1, ((max_M + tile - 1) / tile) * tn, 64, groups);
    if (g.xs.maxlen <= 0) g.xs.on = 0;
    if (knobs().xcd_sched_debug && g.xs.on) fprintf(stderr, "xcd_sched cls %d tn %d maxlen %d pool %d\n", g.xs.on, g.xs.tn, g.xs.maxlen, g.xs.P[8]);
    return g.xs.on != 0;
}
inline long gemm_xcd_sched_slots(const XcdSched& s) { return 8L * s.maxlen * (s.on == 1 ? s.tn : 1); }
// Panel order (xcd_panel_locate) for a problem: TASK mode, fewer than 8 groups (the task-per-XCD schedule covers 8), an under-filled
// launch, and a B operand (N x K: the weight image of a forward / input-gradient problem) that is the bigger of the two — otherwise the
// m-tile-major grouping, which keeps an m-tile's A panel in one L2, is already the right one.  Measured (profiles/r04_ab_log.md): the
// k = 9 input gradient of a single-task rank 212 -> 194 us, its step 35.17 -> 34.73 ms.  MTTS_PANEL_ORDER=0: off (A/B runs).
inline bool gemm_panel_order_for(const GemmPending& p) {
    const GemmArgs& g = p.g;
    if (!knobs().panel_order || g.table || p.groups >= 8 || p.groups < 1) return false;
    if (gemm_wgs(p, 64) > kGemmLatencyWgs) return false;   // chip-filling launches: measured slightly worse (C2: +1 %)
    const double K = (double)gemm_keff(g);
    const double a_bytes = p.form == GEMM_TN ? p.rows * p.max_M : p.rows / p.groups * (g.lda > 0 ? g.lda : K);   // unique bytes behind the A operand (per group)
    const double b_bytes = p.form == GEMM_TN ? p.rows * p.max_N : (double)p.max_N * K;
    return b_bytes > a_bytes;
}
// Placement of a problem's tiles at split S and tile T: 1 task-per-XCD schedule (built into g.xs), else 2 panel order, else 0 (XCD-grouped order)
inline int gemm_place(const GemmPending& p, GemmArgs& g, int S, int T) {
    if (gemm_xcd_sched_for(g, p.max_M, p.max_N, p.groups, S, T)) return 1;
    return gemm_panel_order_for(p) ? 2 : 0;
}

struct GemmLaunchPlan {
    const char* error = nullptr;   // a refusal: nothing below counts
    GemmKernelId id;
    dim3 grid;
    GemmMulti mp;                  // the kernel's arguments (stand-alone: mp.g[0]) — start slots, XCD schedules, panel fields — but for the pointers `prob` stands for
    struct Prob {
        int splitk = 1, place = 0, tag = -1;
        long long ws_off = 0, ctr_off = 0;   // splitk > 1: its slabs and tile counters inside the context's workspace
        int ln_off = -1;                     // >= 0: its LnFuse arrival counters inside the workspace's last kLnCtrs
    } prob[kGemmMultiMax];
    GemmProfiler::Rec rec{};       // rec.kernel = the GemmKind; events and site tag are the issue step's
};
inline GemmLaunchPlan gemm_refusal(const char* why) { GemmLaunchPlan pl; pl.error = why; return pl; }

// One problem on a stand-alone kernel.  code = 0: automatic — a 64x64 grid (bf16 mode: 128x128 for chip-filling launches).  An explicit
// tile code picks one kernel: 64 / 128 (+1000 software pipeline, +2000 BK = 32), 4064 LDS-DMA (kernel tests, micro-benchmarks).
// Stand-alone launches never split K: the long chains of under-filled batches are cut in gemm_plan_multi.
inline GemmLaunchPlan gemm_plan_single(const GemmCtx& cx, const GemmPending& p, int code) {
    if (p.g.A2) return gemm_refusal("dual-source GEMM handed to a stand-alone kernel (explicit tile code inside an open batch)");   // (they exist in the multi-problem kernels only)
    GemmLaunchPlan pl;
    pl.mp.n = 1; pl.mp.form[0] = p.form; pl.mp.groups[0] = p.groups;
    GemmArgs& g = pl.mp.g[0];
    g = p.g;
    g.swizzle = kGemmXcdSwizzle;
    g.wave_prio = cx.wave_prio;
    const bool bf16 = cx.bf16 && gemm_bf16_ok(g);
    int tile = code != 0 ? code : (bf16 ? gemm_bf16_tile(gemm_wgs(p, 128)) : 64);
    bool glds = false;
    if (tile == 4064) { glds = kGemmHasGlds && !bf16 && gemm_glds_ok(g); tile = 64; }
    else if (code == 0 && !bf16) glds = kGemmHasGlds && gemm_glds_mode() && gemm_glds_ok(g) && gemm_wgs(p, 64) <= kGemmLatencyWgs && !cx.no_glds && !g.ln.y;
    bool pipe = kGemmDefaultPipe;
    int bk = kGemmDefaultBk;
    const int ablate = tile / 10000;
    tile %= 10000;
    if (tile >= 1000) { pipe = (tile / 1000) & 1; bk = (tile / 2000) ? 32 : 16; tile %= 1000; }
    if (code == 0 && !g.table && gemm_keff(g) >= 1024 && (p.form == GEMM_NT || p.form == GEMM_TN)) bk = 32;  // long K-contiguous panels: full 128-B lines per row
    if (g.taps > 1 && g.tap_k % 32 != 0) bk = 16;  // a K-slice must not straddle two conv taps
    int ln_used = 0;
    if (!gemm_ln_plan(cx, p, g, bf16 ? 0 : tile, ln_used, pl.prob[0].ln_off)) return gemm_refusal("row-complete LayerNorm epilogue requested for a launch that cannot carry it");
    GemmKernelId& k = pl.id;
    if (bf16) k = gemm_bf16_id(p.form, g, tile, (code % 10000) / 1000);   // (bf16 tile codes: T + 1000 * slices in flight, 0 = default)
    else if (glds) { k.family = GF_GLDS; k.form = p.form; }
    else {
        k.form = p.form; k.tile = tile; k.bk = bk; k.pipe = pipe; k.ablate = ablate;
        if (pipe && tile == 64) {
            k.lnf = p.form == GEMM_NT && pl.prob[0].ln_off >= 0;
            k.kl = k.lnf ? 4 : gemm_kloop_for(g, bk);
            if (bk == 16 && k.kl != 4) k.kl = 0;   // (BK = 16 exists with the KL = 0 and 4 loops)
        }
    }
    const int tiles_m = (p.max_M + tile - 1) / tile, tiles_n = gemm_tiles_n(g, p.max_N, tile);
    pl.grid = dim3((unsigned)(tiles_m * tiles_n), 1, (unsigned)p.groups);
    const int place = pl.prob[0].place = gemm_place(p, g, 1, tile);
    if (place == 1) pl.grid = dim3((unsigned)gemm_xcd_sched_slots(g.xs), 1, 1);   // 1-D, task-per-XCD order
    else if (place == 2) {
        g.swizzle = 2; g.po_tiles_m = tiles_m;
        pl.grid = dim3((unsigned)xcd_panel_slots(tiles_m, tiles_n, 1), 1, (unsigned)p.groups);
    }
    pl.prob[0].tag = p.tag;
    GemmProfiler::Rec& rec = pl.rec;
    rec.kernel = gemm_kind_of(k); rec.flops = p.flops; rec.form = p.form; rec.tile = bf16 ? 16000 + tile : (glds ? 4064 : tile);
    rec.N = p.max_N; rec.K = gemm_keff(g); rec.groups = p.groups; rec.rows = p.rows; rec.bytes = p.bytes;
    return pl;
}

// Problems q[0 .. n) — sorted, longest K-loop first — as ONE launch of a multi-problem kernel, laid out problem-major over a 1-D grid.
inline GemmLaunchPlan gemm_plan_multi(const GemmCtx& cx, const GemmPending* q, int n, const GemmRequest& req) {
    GemmLaunchPlan pl;
    GemmMulti& mp = pl.mp;
    GemmProfiler::Rec& rec = pl.rec;
    mp.n = n;
    // split-K for the long chains of an under-filled batch: a tile whose K-loop is longer than two thirds (swept: 1 / 1.25 .. 1 / 1.5)
    // of the whole batch's per-CU work would finish last on its own (single-task ranks: the k=9 dgrad tile, 576 slices, beside a
    // batch that is worth ~590 slices per CU), so it is cut into S workgroups (rendezvous in splitk_combine)
    double work = 0.0, wgs64 = 0.0, wgs128 = 0.0;
    bool any_dual = false;   // dual-source problems (GemmArgs::A2) need the kernels that run second sources
    bool bf16 = cx.bf16;     // bf16 numerics mode: the whole launch takes the bf16 operand family when every problem qualifies; block tile T
    for (int i = 0; i < n; ++i) {
        const GemmPending& p = q[i];
        work += gemm_wgs(p, 64) * std::max(1, (gemm_keff(p.g) + 15) / 16);
        wgs64 += gemm_wgs(p, 64);
        wgs128 += gemm_wgs(p, 128);
        any_dual = any_dual || p.g.A2 != nullptr;
        bf16 = bf16 && gemm_bf16_ok(p.g);
    }
    const double per_cu = work / 256.0;
    const bool small_batch = wgs64 <= kGemmLatencyWgs;
    const int T = !bf16 ? 64 : (req.family_tile ? req.family_tile : gemm_bf16_tile(wgs128));
    long long ws_off = 0, ctr_off = 0;
    int ln_used = 0, maxK = 0;
    bool bk32 = true;
    rec.splitk = 1;   // (the largest split factor among the launch's problems)
    for (int i = 0; i < n; ++i) {
        const GemmPending& p = q[i];
        GemmArgs& g = mp.g[i];
        GemmLaunchPlan::Prob& pp = pl.prob[i];
        mp.form[i] = p.form; mp.groups[i] = p.groups; g = p.g;
        g.swizzle = 0; g.splitk = 1; g.wave_prio = cx.wave_prio;
        const int tiles_m = (p.max_M + T - 1) / T, tiles_n = gemm_tiles_n(g, p.max_N, T), tiles = tiles_m * tiles_n;
        int S = 1;
        const int nch = (gemm_keff(g) + 15) / 16;
        constexpr double ratio = 1.5;
        if (knobs().batch_splitk && !cx.no_splitk && small_batch && T == 64 && !g.table && !g.colsum && !g.ln.y && nch > per_cu / ratio) {
            S = (int)std::min<double>(std::min<double>(std::ceil(nch / std::max(per_cu / ratio, 1.0)), nch / 16), 8);
            const long long slots = (long long)tiles * p.groups;
            if (S < 2 || ws_off + slots * S * 4096 > kSplitWsFloats || ctr_off + slots > kSplitCtrs - kLnCtrs || !cx.wsp.ws) S = 1;
            else {
                g.splitk = S; g.tiles_pg = tiles;
                pp.ws_off = ws_off; pp.ctr_off = ctr_off;
                rec.splitk = std::max(rec.splitk, S);
                ws_off += slots * S * 4096; ctr_off += slots;
            }
        }
        if (!gemm_ln_plan(cx, p, g, bf16 ? 0 : T, ln_used, pp.ln_off)) return gemm_refusal("row-complete LayerNorm epilogue requested for a launch that cannot carry it");
        pp.splitk = S; pp.tag = p.tag;
        pp.place = gemm_place(p, g, S, T);
        mp.tiles_pg[i] = tiles * S;
        long slots = (long)tiles * S * p.groups;
        if (pp.place == 1) { mp.xcd_group[i] = -2; slots = gemm_xcd_sched_slots(g.xs); }
        else if (pp.place == 2) {
            mp.xcd_group[i] = -3;
            mp.po_tm[i] = (short)tiles_m; mp.po_tn[i] = (short)tiles_n; mp.po_s[i] = (short)S;
            slots = (long)xcd_panel_slots(tiles_m, tiles_n, S) * p.groups;
        } else mp.xcd_group[i] = kGemmXcdSwizzle ? std::min(tiles_n * S, 64) : 0;
        mp.start[i + 1] = mp.start[i] + (int)((slots + 7) & ~7L);   // (every problem starts on a multiple of 8: workgroup slot % 8 = XCD)
        if (g.taps > 1 && g.tap_k % 32 != 0) bk32 = false;
        maxK = std::max(maxK, gemm_keff(g));
        rec.flops += p.flops; rec.rows += p.rows; rec.bytes += p.bytes;
    }
    pl.grid = dim3((unsigned)mp.start[n], 1, 1);
    // BK = 32 stages K-contiguous operands in full 128-byte lines (half the load instructions, TA transactions and barriers
    // per flop); needs every tapped problem's tap length to be a multiple of 32 and pays off only for long K.  Default since round 3
    // (profiles/r03_sk_queue.md: the multi-problem launches with K >= 1024 run at 0.676 instead of 0.646 of the fp32 matrix peak, the
    // whole step is unchanged, a single-task rank gains 1.7 %).
    bool glds = gemm_glds_mode() && small_batch && !cx.no_glds && ln_used == 0;
    if (req.family) { glds = req.family == 4064; bk32 = bk32 && req.family == 32; if (bk32) maxK = std::max(maxK, 1024); }
    for (int i = 0; i < n; ++i) glds = glds && gemm_glds_ok(mp.g[i]);
    GemmKernelId& k = pl.id;
    if (bf16) { k = gemm_bf16_multi_id(mp, T, any_dual); glds = false; }
    else if (glds && kGemmHasGlds) { k.family = GF_GLDS; k.multi = true; k.dual = any_dual; }
    else {
        k.multi = true; k.dual = any_dual; k.lnf = ln_used > 0 && !any_dual;
        k.bk = bk32 && maxK >= 1024 && !cx.prefer_bk16 ? 32 : 16;
        k.kl = gemm_kloop_variant();
        for (int i = 0; i < n; ++i) k.kl = std::min(k.kl, gemm_kloop_for(mp.g[i], k.bk));
        if (k.lnf) k.kl = 4;
        else if (k.bk == 16 && k.kl != 4) k.kl = 0;   // (BK = 16 exists with the KL = 0 and 4 loops)
    }
    rec.kernel = gemm_kind_of(k); rec.form = 3; rec.tile = bf16 ? 16000 + T : (glds ? 4064 : 64);
    rec.N = n; rec.K = maxK; rec.groups = mp.start[n];   // multi: N = problems, K = longest K, groups = workgroups
    return pl;
}

// A single queued problem takes a stand-alone kernel — unless it is dual-source (those exist in the multi-problem kernels only) or the
// launch is in the latency regime, where it stays a multi-problem launch so that the long-chain split-K rule applies (the k=9 dgrad of a
// single-task rank is 124 tiles x 288 slices: alone it would run at one tile per CU).  MTTS_SINGLE_MULTI=0: always alone.
inline bool gemm_goes_alone(const GemmPending* q, int n) { return n == 1 && !q[0].g.A2 && (!knobs().single_multi || gemm_wgs(q[0], 64) > kGemmLatencyWgs); }
inline GemmLaunchPlan gemm_plan_part(const GemmCtx& cx, const GemmPending* q, int n, const GemmRequest& req) {
    return gemm_goes_alone(q, n) ? gemm_plan_single(cx, q[0], 0) : gemm_plan_multi(cx, q, n, req);
}
// The plans of a whole queue, handed to each(plan) in launch order: one — or two, when the batch mixes plane-only problems (bf16 mode:
// the input-gradient conv over the weight's transposed shadow has no fp32 B operand) with problems the bf16 kernels cannot take (a
// dual-source tangent product whose tap length is not a multiple of 32: the Hessian-vector pass through the PostNet's output layer).
// Then the plane-only problems go out on the bf16 family and the rest on the fp32 family; the problems of a batch are independent, so
// the cut changes nothing but the launch count.  Sorts q by effective K (stable), plane-only problems first when it cuts.
template <class Each>
inline void gemm_plan_queue(const GemmCtx& cx, std::vector<GemmPending>& q, const GemmRequest& req, Each&& each) {
    std::stable_sort(q.begin(), q.end(), [](const GemmPending& x, const GemmPending& y) { return gemm_keff(x.g) > gemm_keff(y.g); });
    const int n = (int)q.size();
    int planes = 0;
    bool bf16 = cx.bf16, planes_ok = cx.bf16;
    for (const GemmPending& p : q) {
        bf16 = bf16 && gemm_bf16_ok(p.g);
        if (p.g.plane_only) { ++planes; planes_ok = planes_ok && gemm_bf16_ok(p.g); }
    }
    if (gemm_goes_alone(q.data(), n) || bf16 || planes == 0) { GemmLaunchPlan pl = gemm_plan_part(cx, q.data(), n, req); each(pl); return; }
    if (!planes_ok || planes == n) { GemmLaunchPlan pl = gemm_refusal("plane-only GEMM problem queued outside the bf16 plane path"); each(pl); return; }
    std::stable_partition(q.begin(), q.end(), [](const GemmPending& p) { return p.g.plane_only; });
    const int cut[3] = {0, planes, n};
    const GemmRequest reqs[2] = {GemmRequest{0, 0, req.family_tile}, req};
    for (int h = 0; h < 2; ++h) { GemmLaunchPlan pl = gemm_plan_part(cx, q.data() + cut[h], cut[h + 1] - cut[h], reqs[h]); each(pl); }
}

// ---- issue ----------------------------------------------------------------------------------------------------------------------
inline void gemm_issue(GemmCtx& cx, GemmLaunchPlan& pl, hipStream_t stream) {
    if (pl.error) { cx.error = pl.error; return; }
    for (int i = 0; i < pl.mp.n; ++i) {
        GemmArgs& g = pl.mp.g[i];
        const GemmLaunchPlan::Prob& pp = pl.prob[i];
        if (pp.splitk > 1) { g.ws = cx.wsp.ws + pp.ws_off; g.tile_ctr = cx.wsp.ctr + pp.ctr_off; }
        g.ln.ctr = pp.ln_off >= 0 ? cx.wsp.ctr + (kSplitCtrs - kLnCtrs) + pp.ln_off : nullptr;
        if (pl.id.family == GF_BF16 && g.Ah) ++cx.plane_problems;
        cx.note(pp.tag, pp.splitk, pp.place);
    }
    GemmProfiler& prof = cx.prof;
    if (prof.enabled) { pl.rec.e0 = prof.get(*cx.heap); pl.rec.e1 = prof.get(*cx.heap); hipEventRecord(pl.rec.e0, stream); }
    gemm_kernel_launch(pl.id, pl.mp, pl.grid, stream);
    cx.last_kind = pl.rec.kernel;
    if (!pl.id.multi) cx.last_place = pl.prob[0].place;
    if (prof.enabled) {
        hipEventRecord(pl.rec.e1, stream);
        pl.rec.tag = prof.tag;
        prof.recs.push_back(pl.rec);
    }
}

// ---- the launcher's front door ----------------------------------------------------------------------------------------------------
inline void gemm_batch_begin(GemmCtx& cx) { cx.batch.open = true; }
// issues the queue (req: a kernel family forced on its multi-problem launch) and closes the batch
inline void gemm_batch_end(GemmCtx& cx, hipStream_t stream, const GemmRequest& req = GemmRequest{}) {
    GemmBatch& b = cx.batch;
    b.open = false;
    if (b.q.empty()) return;
    gemm_plan_queue(cx, b.q, req, [&](GemmLaunchPlan& pl) { gemm_issue(cx, pl, stream); });
    b.q.clear();
}
// A problem as the queue and the planner take it; false: nothing to do, or refused (cx.error).  max_M / max_N bound the tile grid over all
// groups.  total_M = sum of the groups' row counts (0: max_M * groups).  alg_flops / alg_bytes: algorithmic (unpadded) work, profiler only.
// The bf16 planes are kept only where the plane-staged K-loop will run (bf16 mode, an NT problem it can take), the twin of C in bf16 mode only.
inline bool gemm_make_pending(GemmCtx& cx, GemmPending& p, int form, const GemmArgs& g_in, int max_M, int max_N, int groups, double alg_flops, long long total_M, double alg_bytes, int tag) {
    if (max_M <= 0 || max_N <= 0 || groups <= 0) return false;
    p = GemmPending{form, g_in, max_M, max_N, groups, alg_flops, total_M > 0 ? (double)total_M : (double)max_M * groups, alg_bytes, tag};
    GemmArgs& g = p.g;
    if (!(cx.bf16 && gemm_bf16_ok(g) && gemm_bf16_planes_ok(form, g))) {
        if (g.plane_only) { cx.error = "plane-only GEMM problem outside the bf16 plane path"; return false; }
        g.Ah = g.Bh = nullptr;
    }
    if (!cx.bf16) g.Ch = nullptr;
    return true;
}
// queues a problem for the next gemm_batch_end, which reports what it decided for it under `tag` (GemmCtx::note); never launches
inline void gemm_enqueue(GemmCtx& cx, int form, const GemmArgs& g, int max_M, int max_N, int groups, int tag) {
    GemmPending p;
    if (gemm_make_pending(cx, p, form, g, max_M, max_N, groups, 0.0, 0, 0.0, tag)) cx.batch.q.push_back(p);
}
// Host launcher.  tile = 0: automatic — the problem goes through the launch queue: with the open batch's other problems (the batch goes
// out when it holds kGemmMultiMax), or alone.  An explicit tile code launches at once on the stand-alone kernel it names
// (gemm_plan_single); for a dual-source problem it names the family of a multi-problem launch of that one problem.
inline void gemm_launch(GemmCtx& cx, int form, const GemmArgs& g, int max_M, int max_N, int groups, hipStream_t stream,
                        int tile = 0, double alg_flops = 0.0, long long total_M = 0, double alg_bytes = 0.0) {
    GemmPending p;
    if (!gemm_make_pending(cx, p, form, g, max_M, max_N, groups, alg_flops, total_M, alg_bytes, -1)) return;
    GemmBatch& b = cx.batch;
    if (tile == 0) {
        const bool open = b.open;
        b.q.push_back(p);
        if (!open || (int)b.q.size() == kGemmMultiMax) { gemm_batch_end(cx, stream); b.open = open; }
    } else if (p.g.A2 && !b.open) {
        b.q.push_back(p);
        gemm_batch_end(cx, stream, gemm_family_request(tile));
    } else {
        GemmLaunchPlan pl = gemm_plan_single(cx, p, tile);
        gemm_issue(cx, pl, stream);
    }
}

}  // namespace mtts
