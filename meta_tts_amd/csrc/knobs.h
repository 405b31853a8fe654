// Every MTTS_* environment switch of the library: one field per switch, read once per process.  Unset: the member initialiser.  Set: atoi of the
// value (on / off switches are tested "!= 0").  The default is the shipped arm; the other arm is the simple reference a test compares it with, or a
// measurement tool's.  DESIGN.md section 9 lists the same names; tests/test_knob_table.py keeps that table, this file and the environments of
// the tests / tools in step.  NOT here: MTTS_GEMM_DUMP (gemm.h: GemmProfiler::report), which bench.py sets and clears inside a running process.
#pragma once
#include <cstdlib>

namespace mtts {

struct Knobs {
    int kloop = 4;                  // gemm.h: K-loop variant of the pipelined 64x64 kernels, 0 / 1 / 4 (anything else: 4); bit-identical (tools/kloop_forms.py, profiles/r05_kloop_ab.md)
    int glds = 0;                   // 1: launches of <= 768 workgroups take the LDS-DMA family again, the round 3-4 rule (tools/so_tolerance_bisect.py; tile code 4064 needs no switch)
    int xcd_sched = 1;              // 0: no task-per-XCD schedule (tests/test_xcd_schedule.py)
    int xcd_sched_min_groups = 8;   // 2 / 4: the schedule also for the 2- / 4-group launches of a multi-rank job's ranks (same test)
    int xcd_sched_debug = 0;        // present: one stderr line per scheduled problem — the test's proof that the schedule is in use
    int panel_order = 1;            // 0: m-tile-major XCD order for under-filled launches too (tests/test_deferred_paths.py)
    int single_multi = 1;           // 0: a single queued problem always leaves the batch for the stand-alone launcher (same test)
    int batch_splitk = 1;           // 0: never cut K in the batch regime (tools/so_tolerance_bisect.py; fp32 roundoff)
    int defer_wgrad = 1;            // engine.h: 0: weight gradients on the main stream, first and second order (tests/test_deferred_paths.py, tests/test_gpu_timed_config.py)
    int side_pred_all = 1;          // 0: side-stream predictors only in the deferred regime (tests/test_deferred_paths.py)
    int pred_side = 1;              // 0: teacher-forced predictors' forward on the main stream (same tests as defer_wgrad)
    int pred_early = 1;             // 0: the predictors' backward at its textual place (same)
    int pred_batch = 1;             // 0: embeddings and predictors in reference order (tests/test_deferred_paths.py)
    int enc_ahead = 1;              // 0: no encoder run-ahead (same tests as defer_wgrad)
    int enc_ahead_all = 1;          // 0: run-ahead only in the deferred regime (tests/test_deferred_paths.py)
    int enc_ahead_query = 1;        // 0: the query pass's encoder does not run ahead (same test)
    int upd_overlap = 1;            // 0: the inner SGD step as one launch after the backward (same test, bit for bit)
    int ln_fold_side = 1;           // 0: beyond the deferred regime the LayerNorm gamma / beta folds stay in the critical chain (same test)
    int side_bk16 = 1;              // 0: the weight-gradient stream's batches on the BK = 32 kernels again (tests/test_gpu_timed_config.py)
    int main_prio = 1;              // 0 / 2: the critical stream's wavefronts never / in every regime at raised priority (tests/test_deferred_paths.py)
    int fused_attn = 1;             // 0: attention forward as GEMM + softmax + GEMM, also in mtts_sdpa_fwd (tests/test_deferred_paths.py)
    int attn_sort = 1;              // 0: attention groups in batch order (same test, bit for bit)
    int ln_fuse = 0;                // 1: LayerNorm as the producing GEMM's row-complete epilogue: bit-identical, measured slower (same test; profiles/r05_ab_log.md)
    int so_keep_act = 1;            // engine_so.inc, each a reference arm of tests/test_deferred_paths.py: 0: the reverse sweep replays every inner step's forward
    int so_keep_grad = 1;           // 0: the tangent backward recomputes the primal input gradients
    int so_defer_post = 1;          // 0: the PostNet layers' hv(W) products inside the tangent launches
    int so_fuse_drop = 1;           // 0: the tangent blocks' dropout as launches of its own
    int so_ln_part = 1;             // 0: hv(gamma) / hv(beta) by a two-launch reduction in front of the tangent backward (fp32 roundoff)
    int so_pred_side = 1;           // 0: the hv reductions of the predictors' projections on the critical stream
    int so_table_side = 1;          // 0: the embedding tables' hv on the critical stream
    int ablate_ln = 0;              // read only under -DMTTS_ABLATE: 1 = TIMING ONLY, wrong results, every LayerNorm launch dropped (profiles/r05_ab_log.md)
    int attn_diag_mask = 0;         // read only under -DMTTS_ATTN_DIAG: AttnFwdArgs::diag of mtts_sdpa_fwd (tools/attn_phases.sh)
};

inline Knobs read_knobs() {
    Knobs k;
    const struct { const char* name; int* v; } table[] = {
        {"MTTS_KLOOP", &k.kloop}, {"MTTS_GLDS", &k.glds}, {"MTTS_XCD_SCHED", &k.xcd_sched}, {"MTTS_XCD_SCHED_MIN_GROUPS", &k.xcd_sched_min_groups},
        {"MTTS_PANEL_ORDER", &k.panel_order}, {"MTTS_SINGLE_MULTI", &k.single_multi}, {"MTTS_BATCH_SPLITK", &k.batch_splitk},
        {"MTTS_DEFER_WGRAD", &k.defer_wgrad}, {"MTTS_SIDE_PRED_ALL", &k.side_pred_all}, {"MTTS_PRED_SIDE", &k.pred_side}, {"MTTS_PRED_EARLY", &k.pred_early},
        {"MTTS_PRED_BATCH", &k.pred_batch}, {"MTTS_ENC_AHEAD", &k.enc_ahead}, {"MTTS_ENC_AHEAD_ALL", &k.enc_ahead_all}, {"MTTS_ENC_AHEAD_QUERY", &k.enc_ahead_query},
        {"MTTS_UPD_OVERLAP", &k.upd_overlap}, {"MTTS_LN_FOLD_SIDE", &k.ln_fold_side}, {"MTTS_SIDE_BK16", &k.side_bk16}, {"MTTS_MAIN_PRIO", &k.main_prio},
        {"MTTS_FUSED_ATTN", &k.fused_attn}, {"MTTS_ATTN_SORT", &k.attn_sort}, {"MTTS_LN_FUSE", &k.ln_fuse}, {"MTTS_SO_KEEP_ACT", &k.so_keep_act},
        {"MTTS_SO_KEEP_GRAD", &k.so_keep_grad}, {"MTTS_SO_DEFER_POST", &k.so_defer_post}, {"MTTS_SO_FUSE_DROP", &k.so_fuse_drop}, {"MTTS_SO_LN_PART", &k.so_ln_part},
        {"MTTS_SO_PRED_SIDE", &k.so_pred_side}, {"MTTS_SO_TABLE_SIDE", &k.so_table_side},
#if defined(MTTS_ABLATE)
        {"MTTS_ABLATE_LN", &k.ablate_ln},
#endif
#if defined(MTTS_ATTN_DIAG)
        {"MTTS_ATTN_DIAG_MASK", &k.attn_diag_mask},
#endif
    };
    for (const auto& t : table)
        if (const char* e = getenv(t.name)) *t.v = atoi(e);
    if (k.kloop != 0 && k.kloop != 1 && k.kloop != 4) k.kloop = 4;
    k.glds = k.glds != 0;
    k.xcd_sched_debug = getenv("MTTS_XCD_SCHED_DEBUG") != nullptr;
    return k;
}
inline const Knobs& knobs() {
    static const Knobs k = read_knobs();
    return k;
}

}  // namespace mtts
