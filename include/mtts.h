/* libmtts — C ABI of the MI355X-native Meta-TTS hot path (FastSpeech2 forward/backward inside the
 * MAML inner/outer loop).  Plain C, raw pointers and sizes only; no torch / C++ types cross this
 * boundary.  The reference (SungFeng-Huang/Meta-TTS) is pure Python with no FFI layer, so every
 * entry point below names the Python interface it sits beneath (file:line under /root/reference);
 * INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions: every function returns 0 on success, non-zero on error (mtts_last_error() gives the
 * message); nothing throws across the ABI.  A handle owns all device memory it needs (allocated in
 * mtts_create for the stated capacities; no allocation afterwards — with ONE exception: second-order MAML,
 * mtts_meta_grad(second_order = 1) / mtts_hvp_support, allocates its tangent arena, its per-step activation and gradient
 * sets and its deferred-gradient buffers on FIRST use, so first-order / baseline / inference users do not pay for them;
 * mtts_reserve_second_order(h, steps) makes that allocation explicit and up-front).  All work is enqueued on the
 * handle's HIP stream (mtts_set_stream) and is asynchronous w.r.t. the host unless a function
 * copies results to a host pointer, in which case it synchronises that stream.  For small plans the
 * handle additionally uses two private non-blocking streams (parameter gradients, encoder run-ahead);
 * they are forked from and joined back into the handle's stream with events inside the same call, so
 * ordering against the caller's stream is exactly as if everything ran on it.  A handle must not
 * be used from two host threads at once, but DIFFERENT handles share no mutable state (launch queue,
 * profiler, split-K workspace and numerics mode are per handle) and may be driven from different host
 * threads concurrently.  "host" pointers are host memory, "dev" pointers device.
 */
#ifndef MTTS_H
#define MTTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mtts_handle mtts_handle;

/* Sizes of config/model/base.yaml:1-30 plus what the reference reads from disk:
 * vocab = len(text.symbols)+1 (transformer/Models.py:40), n_speaker = len(speakers.json)
 * (lightning/model/speaker_encoder.py:49-50), pitch/energy min/max = stats.json
 * (lightning/model/modules.py:41-46), PostNet sizes (transformer/Layers.py:72-78). */
typedef struct mtts_model_cfg {
    int d_model, enc_layers, dec_layers, enc_heads, dec_heads, d_ff, k1, k2;
    int vp_filter, vp_kernel, n_bins, max_seq_len, n_mel, vocab, n_speaker;
    int postnet_dim, postnet_kernel, postnet_layers;
    float pitch_min, pitch_max, energy_min, energy_max;
    /* adapt.modules of config/algorithm/<name>.yaml as a bit mask over
     * {0 encoder, 1 variance_adaptor, 2 decoder, 3 mel_linear, 4 postnet, 5 speaker_emb}
     * (lightning/systems/base_adaptor.py:31-35) */
    int adapt_mask;
    /* transformer.{encoder,decoder}_dropout, variance_predictor.dropout (config/model/base.yaml:10-11,16); the PostNet's
     * 0.5 is hard-coded in the reference (transformer/Layers.py:133-134).  Only used after mtts_set_dropout(h, 1, seed). */
    float enc_dropout, dec_dropout, vp_dropout;
    /* preprocess_config["preprocessing"]["pitch" | "energy"]["feature"] == "frame_level" (lightning/model/modules.py:28-33,139-148,
     * loss.py:54-63): that feature's targets are [B][T_max] (one value per mel frame) and its predictor / embedding / loss run on
     * the frame rectangle after the length regulator.  0 = phoneme_level (config/preprocess/LibriTTS.yaml).  First- and second-order. */
    int pitch_frame_level, energy_frame_level;
} mtts_model_cfg;

/* One padded batch: elements [2:] of the reference 12-tuple (lightning/collate.py:47-60), host memory,
 * int64 where the reference uses LongTensor. */
typedef struct mtts_batch {
    int B, S_max, T_max;
    const int64_t* speakers;  /* [B]                 batch[2]  */
    const int64_t* texts;     /* [B][S_max]          batch[3]  */
    const int64_t* src_lens;  /* [B]                 batch[4]  */
    const float* mels;        /* [B][T_max][n_mel]   batch[6]  */
    const int64_t* mel_lens;  /* [B]                 batch[7]  */
    const float* pitches;     /* [B][S_max]          batch[9]   ([B][T_max] when pitch is frame-level)  */
    const float* energies;    /* [B][S_max]          batch[10]  ([B][T_max] when energy is frame-level) */
    const int64_t* durations; /* [B][S_max]          batch[11] */
    /* NULL, or [B][d_model] speaker embeddings used INSTEAD of the table lookup — `speaker_emb: dvec`, where batch[2] is
     * (ref_mels, ref_slices) and the embedding is the d-vector encoder's output (speaker_encoder.py:71-76; mtts_dvector_embed).
     * `speakers` is ignored then; no speaker-table gradient (the embeddings are inputs: no tangent in second-order passes either). */
    const float* spk_emb;
} mtts_batch;

/* ---- lifecycle (System.__init__, lightning/systems/system.py:30-48) ---------------------------- */
int mtts_create(const mtts_model_cfg* cfg, int device, int max_tasks, int max_B, int max_S, int max_T,
                mtts_handle** out);
void mtts_destroy(mtts_handle* h);
const char* mtts_last_error(mtts_handle* h); /* h may be NULL: error of the last failed mtts_create */
int mtts_set_stream(mtts_handle* h, void* hip_stream);
/* ---- gradient accumulation (main.py:62 `accumulate_grad_batches=grad_acc_step`): with accumulate != 0 the next mtts_meta_grad /
 * mtts_plain_grad calls ADD their (already grad_scale-d) result to the outer-gradient buffer instead of overwriting it; the caller
 * passes grad_scale / grad_acc_step, all-reduces and steps the optimizer once per grad_acc_step batches (systems.Trainer). */
int mtts_set_grad_accumulation(mtts_handle* h, int accumulate);

/* Numerics mode of the handle's contractions (every Linear / Conv1d / attention product, forward and backward; csrc/gemm_bf16.h).
 * 0 (default): fp32 operands on the fp32-input MFMA — the reference's own arithmetic (main.py:110-112 passes no `precision=`), the
 *    mode every parity gate (mel L1 <= 1e-4) is stated in.
 * 1: bf16 operands (rounded to nearest even once, on the way into LDS), exact products, fp32 accumulation — BASELINE.json configs[1]
 *    ("multi-task baseline bf16 on 1xMI355X"; what `Trainer(precision="bf16")` / torch.autocast(bfloat16) would make of the Linear /
 *    Conv1d / bmm ops).  Parameters, optimizer state, LayerNorm / BatchNorm / softmax / losses and every tensor in HBM stay fp32.
 *    The few problems whose conv taps do not cover whole 32-element K-slices (the PostNet's 80-channel output layer in its
 *    input-gradient form) keep the fp32 kernels — unless planes serve them, see below.  The long NT problems (the FFT blocks' and the
 *    PostNet's convolutions, forward and input gradient) read their operands from bf16 PLANES: a twin of the activation slab and a
 *    shadow of the weight (refreshed from the fp32 master once per pass; the input gradient as an NT problem over the transposed
 *    shadow) — the same rounded values, half the bytes through L2.  Allocated the first time the mode is selected (about half the
 *    activation arena + 2 bytes per shadowed weight element, twice).
 * 2: mode 1 without the planes (every operand is read as fp32 and rounded on its way into LDS): the A/B and test arm of mode 1 — the
 *    forward results are bit-identical to mode 1's.
 * May be switched between calls; applies to the handle's three streams. */
int mtts_set_numerics(mtts_handle* h, int mode);
int mtts_get_numerics(mtts_handle* h);

/* Train-mode dropout (nn.Dropout / F.dropout sites of SubLayers.py:54,90, modules.py:223,235, Layers.py:133-134).
 * Off by default — the parity configuration (SURVEY.md Appendix B.5 patches dropout to identity).  When on, masks are a
 * counter-based function of (seed, pass, site, element) regenerated in backward and in the second-order replay. */
int mtts_set_dropout(mtts_handle* h, int enable, unsigned seed);
int mtts_synchronize(mtts_handle* h);

/* ---- parameters: reference state_dict names without the "model." prefix,
 * torch layouts on the host side ((out,in) Linear, (Cout,Cin,k) Conv1d) -------------------------- */
int mtts_param_count(mtts_handle* h);
int mtts_param_info(mtts_handle* h, int index, const char** name, int* ndim, int shape[4], int64_t* flat_offset,
                    int* adapted);
int64_t mtts_param_total(mtts_handle* h);  /* floats in the flat parameter / gradient space */
int64_t mtts_adapt_start(mtts_handle* h);  /* first float of the adapted (fast-weight) slice */
int mtts_load_param(mtts_handle* h, const char* name, const float* host, int64_t numel);
/* which: 0 parameter, 1 outer gradient, 2 per-task gradient, 3 fast weight of `task`, 4 Adam m, 5 Adam v,
 * 6 Hessian-vector product of `task` (after mtts_hvp_support / a second-order mtts_meta_grad) */
int mtts_export_param(mtts_handle* h, const char* name, int which, int task, float* host, int64_t numel);
/* checkpoint resume: which = 0 parameter, 4 Adam exp_avg, 5 Adam exp_avg_sq; and the Adam step count
 * (PL ckpt["optimizer_states"], main.py:63 resume_from_checkpoint) */
int mtts_import_state(mtts_handle* h, const char* name, int which, const float* host, int64_t numel);
int mtts_set_optimizer_step(mtts_handle* h, int64_t step);
/* BatchNorm1d buffers of PostNet layer `layer` (running_mean, running_var, num_batches_tracked) */
int mtts_set_bn_buffers(mtts_handle* h, int layer, const float* mean_host, const float* var_host, int64_t tracked);
int mtts_get_bn_buffers(mtts_handle* h, int layer, float* mean_host, float* var_host, int64_t* tracked);

/* variance_adaptor.pitch_bins / energy_bins (frozen nn.Parameters, modules.py:57-71; n = n_bins - 1 boundaries each).  mtts_create
 * builds them from the cfg's stats.json min/max; a checkpoint trained on another corpus carries its own (system.py corpus-mismatch
 * branch), which the host layer installs here.  Either pointer may be NULL. */
int mtts_set_bins(mtts_handle* h, const float* pitch_bins_host, const float* energy_bins_host, int n);
int mtts_get_bins(mtts_handle* h, float* pitch_bins_host, float* energy_bins_host, int n);

/* ---- batches: slot 0 = support (or a plain batch), slot 1 = query.  `spk_from`/`average_spk`
 * reproduce forward_learner(..., sup_batch[2], *qry_batch[3:], average_spk_emb=True)
 * (lightning/systems/base_adaptor.py:64-70,122) --------------------------------------------------- */
int mtts_set_batches(mtts_handle* h, int slot, int n_tasks, const mtts_batch* batches, const mtts_batch* spk_from,
                     int average_spk);

/* ---- FastSpeech2.forward, teacher-forced (lightning/model/fastspeech2.py:40-112) and
 * FastSpeech2Loss.forward (lightning/model/loss.py:19-92) ---------------------------------------- */
int mtts_forward(mtts_handle* h, int slot, int use_fast_weights, int train_mode);
/* Same forward with the reference's p/e/d_control arguments.  A batch set without mels/durations runs
 * free-running (modules.py:132-137): durations = clamp(round(exp(logd)-1)*d_control, 0) on device, ONE
 * device->host copy per task sizes the frame spaces (the reference syncs once per phoneme), then the
 * decoder / PostNet run on the predicted length.  train_mode != 0 reproduces the reference's
 * post-adaptation synthesis (clone left in .train(): batch-stat BatchNorm, truncation at max_seq_len). */
int mtts_synthesize(mtts_handle* h, int slot, int use_fast_weights, int train_mode, float p_control, float e_control,
                    float d_control);
/* d_rounded [B][S_max] (duration_rounded of the 10-tuple), mel_lens [B], T_cap = width of mel / mel_post rows */
int mtts_get_durations(mtts_handle* h, int slot, int task, float* d_rounded, int64_t* mel_lens, int* t_cap);
/* copy the outputs of task `task` to host: mel, mel_post [B][T_cap][n_mel] (T_cap = min(T_max, max_seq_len));
 * p, e, logd [B][S_max] (p / e are [B][T_cap] for a frame-level feature).  Any pointer may be NULL. */
/* device view of the last forward's mel (postnet = 0) or mel_post (1) of one task: utterance b, frame t, channel c at
 * mel_dev[b * utt_stride + t * n_mel + c], t < t_cap.  Valid until the next set_batches / forward on that slot. */
int mtts_get_mel_device(mtts_handle* h, int slot, int task, int postnet, const float** mel_dev, int* t_cap, int64_t* utt_stride);
int mtts_get_outputs(mtts_handle* h, int slot, int task, float* mel, float* mel_post, float* p, float* e, float* logd);
int mtts_loss(mtts_handle* h, int slot, float* losses_host /* [n_tasks][6]: total, mel, postnet, pitch, energy, duration */);
/* gradient of scale * total loss w.r.t. every parameter of the touched modules -> per-task gradient */
int mtts_backward(mtts_handle* h, int slot, int use_fast_weights, float scale, int need_encoder);

/* ---- MAML: BaseAdaptorSystem.adapt + meta_learn (lightning/systems/base_adaptor.py:98-124),
 * learn2learn MAML.clone/adapt (lightning/systems/utils.py:17-77).  second_order = 1 is the reference's training
 * mode (`first_order = not train`, base_adaptor.py:107): the query gradient is propagated back through the inner
 * SGD steps by a Hessian-vector-product recursion (forward-over-reverse, csrc/engine_so.inc).  Produces the outer gradient
 * sum_t grad_scale * dL_query,t/dtheta in the handle's outer-gradient buffer.  Host loss pointers may
 * be NULL (then nothing synchronises). ------------------------------------------------------------ */
int mtts_meta_grad(mtts_handle* h, int steps, float inner_lr, float grad_scale, int second_order,
                   float* qry_losses_host /* [n_tasks][6] */, float* sup_losses_host /* [steps][n_tasks][6] */);
/* Pre-allocates everything a second-order mtts_meta_grad of `steps` inner steps would allocate on first use (the tangent arena, one
 * activation set and one gradient set per step — ~0.95 GB per full-size task and step —, the per-layer tangent-gradient buffers of the
 * deferred Hessian-vector weight gradients): after it, second-order calls allocate nothing.  Sets that do not fit are skipped (the
 * engine then recomputes: same results up to rounding, slower); returns 0 unless the mandatory tangent arena itself cannot be allocated. */
int mtts_reserve_second_order(mtts_handle* h, int steps);
/* Hessian-vector product of the support loss (slot 0) at the current fast weights in the direction currently held
 * in the per-task gradient buffer (e.g. after mtts_backward): the building block of the second-order sweep,
 * exposed for parity tests against torch.autograd (export with which = 6). */
int mtts_hvp_support(mtts_handle* h);
/* ---- iMAML (lightning/systems/imaml.py:22-150, lightning/systems/utils.py:120-189; `hypergrad` is an empty submodule of the
 * reference: its conjugate gradient is restated, parity unpinned there).  mtts_set_inner_prox(reg) adds the proximal term
 * 0.5 * reg * |theta_a - w|^2 (imaml.py:41-46,69) to the inner loss of every subsequent mtts_adapt / mtts_meta_grad step (0 = off).
 * Hypergradient of the query loss after mtts_adapt:  begin (query pass at the adapted weights; b = dL_q/dw, v = 0) ->
 * K x cg_step (one conjugate-gradient iteration on a * (H_support + reg * I), a = inner_lr; the Hessian-vector product runs on the
 * batch currently in slot 0, so a fresh support mini-batch may be set before each call: `imaml.stochastic`, imaml.py:88-91) ->
 * finish: outer gradient buffer := sum over local tasks of grad_scale * clip_t(a * reg * v_t) on the adapted parameters, 0 elsewhere
 * (imaml.py:125-131 clips every task's hypergradient to max_norm BEFORE the mean over ranks; max_norm <= 0: no clipping);
 * task_norms_host [n_tasks] (optional) receives the unclipped norms. */
int mtts_set_inner_prox(mtts_handle* h, float reg_param);
int mtts_imaml_begin(mtts_handle* h, float* qry_losses_host /* [n_tasks][6] */);
int mtts_imaml_cg_step(mtts_handle* h, float inner_lr, float reg_param, float tol);
int mtts_imaml_finish(mtts_handle* h, float inner_lr, float reg_param, float grad_scale, float max_norm, float* task_norms_host);
/* BaseAdaptorSystem.adapt alone (few-shot test loop, base_adaptor.py:155-189): `steps` first-order inner steps
 * on slot 0; reset != 0 starts from a fresh clone of theta, else continues on the current fast weights. */
int mtts_adapt(mtts_handle* h, int steps, float inner_lr, int reset, float* sup_losses_host /* [steps][n_tasks][6] */);
/* The inner SGD step (learn2learn maml_update through systems/utils.py:39-47: p <- p - lr * g per adapted parameter) runs module by module on
 * a stream of the handle behind the backward that produces the gradients, instead of as one pass between that backward and the next
 * forward (MTTS_UPD_OVERLAP=0, iMAML's proximal step and architectures without the module table keep the single pass; results are
 * bit-identical).  Returns the launches the LAST inner step's update took: > 1 module by module, 0 the single pass. */
int mtts_inner_update_launches(mtts_handle* h);
/* BaselineSystem.training_step (lightning/systems/baseline.py:25-36): plain gradient of slot's batches */
int mtts_plain_grad(mtts_handle* h, int slot, float grad_scale, float* losses_host);
/* device pointer of the outer gradient (mtts_param_total floats) — the buffer the host all-reduces
 * over RCCL between ranks (PL strategy="ddp", main.py:32) */
float* mtts_outer_grad_ptr(mtts_handle* h);
/* The exchange step over RCCL / xGMI without leaving the library (PL strategy="ddp", main.py:30-38: DDP's gradient all-reduce): one
 * communicator per handle = per rank.  Rank 0 calls mtts_comm_unique_id (128 bytes = NCCL_UNIQUE_ID_BYTES) and hands the id to the
 * other ranks over any out-of-band channel; every rank then calls mtts_comm_init (collective).  mtts_allreduce_outer enqueues
 * ncclAllReduce(SUM, fp32, in place) of the whole outer-gradient buffer on the handle's stream: ordered after the meta-gradient
 * kernels and before the following mtts_outer_update, no host synchronisation.  Each rank scales its contribution by
 * 1 / total_tasks through grad_scale, so the sum is the mean the reference takes.  librccl.so is resolved with dlopen on first use. */
int mtts_comm_available(mtts_handle* h);   /* 0 when librccl can be loaded in this process (every rank probes before rank 0 makes the id) */
int mtts_comm_unique_id(mtts_handle* h, void* id128);
int mtts_comm_init(mtts_handle* h, const void* id128, int rank, int world_size);
int mtts_allreduce_outer(mtts_handle* h);
/* Overlapped, bucketed exchange (DDP's bucketed gradient all-reduce overlapping the backward, main.py:30-38): call BEFORE the gradient call
 * that fills the outer gradient (mtts_meta_grad first or second order, mtts_plain_grad; with gradient accumulation: the window's LAST
 * call).  That call then cuts the flat buffer at module boundaries in backward-completion order (PostNet, decoder L-1 + mel_linear ...
 * decoder 0, variance adaptor, speaker table, encoder L-1 ... encoder 0 + word embedding) and issues one ncclAllReduce per bucket on a
 * communication stream of the handle the moment the backward has completed the module — behind events of the main and the
 * weight-gradient side stream — while the main stream continues; the exchange tail goes out first.  The following mtts_allreduce_outer
 * only makes the handle's stream wait for those collectives (its time is the EXPOSED part of the exchange).  One-shot: disarmed by
 * the gradient call.  Returns 0 when armed, 1 when the overlapped path is not available (no communicator, an
 * architecture whose modules are not contiguous runs of the flat buffer) — mtts_allreduce_outer then reduces the whole buffer as before.
 * Results equal the one-shot exchange's (the same floats, the same collective, in pieces).  mtts_allreduce_launches: collectives the
 * last overlapped exchange issued (buckets + tail). */
int mtts_arm_allreduce_overlap(mtts_handle* h);
/* Take the arming back (a caller whose gradient call will not happen after all: an exception between arming and the call, an aborted
 * accumulation window).  The gradient calls also disarm on EVERY exit path, failures included, so a stale flag can never make a later,
 * unrelated gradient call of this rank issue collectives its peers do not.  mtts_comm_init makes the ranks agree on the bucket table
 * (a SUM of (n, n^2) over the ranks): if any rank has no table, the overlap is off on all of them — mtts_allreduce_bucket_agreement: 1 agreed,
 * 0 disagreed (overlap off everywhere), -1 no communicator. */
int mtts_disarm_allreduce_overlap(mtts_handle* h);
int mtts_allreduce_bucket_agreement(mtts_handle* h);
int mtts_allreduce_launches(mtts_handle* h);
/* What DDP moves between ranks BESIDES the gradient rides behind the flat outer gradient in the same buffer and the same collective:
 * [n_total .. n_total+6) the six losses of the last mtts_meta_grad / mtts_plain_grad call, summed over this rank's tasks and scaled by its
 * grad_scale — the SUM over ranks is the mean `self.log_dict(..., sync_dist=True)` reports (meta.py:78-79, baseline.py:35); behind them the
 * PostNet BatchNorm running_mean | running_var of every layer, weighted so that the SUM is rank 0's buffers (mode 0, default: DDP's
 * broadcast_buffers, main.py:32) or the mean over ranks (mode 1).  mtts_allreduce_outer packs, reduces mtts_outer_sync_floats() floats and
 * installs the reduced buffers itself; a caller that runs the collective on its own (torch.distributed on mtts_outer_grad_ptr) brackets
 * it with mtts_sync_pack(h, w) (w = this rank's BatchNorm weight: 1 / 0 for mode 0, 1 / world for mode 1) and mtts_sync_unpack.
 * mtts_get_synced_losses: the six reduced loss scalars (after the collective; with one rank, after mtts_sync_pack). */
int64_t mtts_outer_sync_floats(mtts_handle* h);
int mtts_sync_pack(mtts_handle* h, float bn_weight);
int mtts_sync_unpack(mtts_handle* h);
int mtts_get_synced_losses(mtts_handle* h, float* out6_host);
int mtts_set_bn_sync(mtts_handle* h, int mode);
/* clip_grad_norm_(max_norm) (main.py:61) + Adam (lightning/optimizer.py:9-15) with the learning rate of
 * lightning/scheduler.py:11-23 supplied by the caller.  grad_dev NULL = the internal outer gradient. */
int mtts_outer_update(mtts_handle* h, const float* grad_dev, float lr, float beta1, float beta2, float eps,
                      float weight_decay, float max_norm, float* grad_norm_host);
int mtts_reset_optimizer(mtts_handle* h);
/* Hooks for a module trained in front of the engine (the speaker encoder): the gradient of the last backward pass w.r.t. the
 * per-utterance speaker vectors of `task` (out [B][d_model], host); a device scalar added to the squared gradient norm inside
 * mtts_outer_update (NULL: none); the device address of the norm mtts_outer_update computes. */
int mtts_get_speaker_grad(mtts_handle* h, int task, int B, float* out);
int mtts_set_extra_grad_sumsq(mtts_handle* h, const float* sumsq_dev);
const float* mtts_grad_norm_dev(mtts_handle* h);

/* ---- measurement: per-launch HIP-event timing of this handle's GEMM launches on its stream.
 * report: out[kind][4] = {launches, total ms, total algorithmic flops, total algorithmic bytes (every operand and the output
 * moved once, fp32)}; `kinds` = mtts_profile_kinds() rows, one per real kernel symbol — mtts_profile_kernel_name(kind) is the name
 * a rocprofv3 kernel trace prints for it (csrc/gemm.h: GemmKind).  (bench.py roofline leg) */
int mtts_profile_gemm(mtts_handle* h, int enable);
int mtts_profile_kinds(void);
const char* mtts_profile_kernel_name(int kind);
int mtts_profile_report(mtts_handle* h, double* out, int kinds);

/* ---- kernel-level entry points (parity tests; dev pointers; stream may be NULL) ----------------
 * form 0: C[M,N] = alpha*A[M,K]*B[N,K]^T + bias   1: C = A[M,K]*B[K,N]   2: C[M,N] = A[K,M]^T*B[K,N]
 * flags bit0 ReLU, bit1 accumulate;
 * tile 0 (auto: the launch queue — a plain 64x64 grid, the LDS-DMA kernels for under-filled launches) / 64 / 128 (+1000 software-pipelined
 * variant, +2000 BK = 32) / 4064 LDS-DMA kernel.  These handle-less entries never split K (no hidden workspace). */
int mtts_gemm_f32(int form, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                  const float* bias, float alpha, int flags, int tile, void* hip_stream);
/* Dual-source product in one accumulator chain: C = alpha * (op(A, B) + op(A2, B2)) + bias, same form / sizes / leading dimensions for
 * both pairs — the shape of every tangent product of second-order MAML, t(X W) = tX W + X tW (csrc/gemm.h: GemmArgs::A2;
 * reference: the double backward that `higher` records for lightning/systems/base_adaptor.py:107). */
int mtts_gemm_f32_dual(int form, int M, int N, int K, const float* A, int lda, const float* B, int ldb, const float* A2, const float* B2,
                       float* C, int ldc, const float* bias, float alpha, int flags, int tile, void* hip_stream);
/* The grouped launcher at kernel level (csrc/gemm.h: gemm_launch / gemm_batch_end as the engine drives them): n = 1 .. 6 problems of any
 * mix of forms in ONE launch.  A descriptor carries the GemmArgs fields of the same names:
 *   groups (blockIdx.z), max_M / max_N bound the tile grid over all groups; TASK mode: group z adds z * a_gs / b_gs / c_gs / bias_gs / ...
 *   (elements) to the bases, and dimptr[z * dim_stride] * dim_mult (DEVICE ints) replaces M (dim_sel 0) or K (dim_sel 2); host_dims = the
 *   same values on the HOST (enables the task-per-XCD schedule of 8-group launches); TABLE mode: `table` = DEVICE array of `groups`
 *   group records, offsets in elements, ld* 0 = inherit; a group with M <= 0 or K <= 0 is skipped — nothing of it is written;
 *   epilogue: v = alpha * acc + bias[n]; flags bit1: v += C; bit0: ReLU; bit2: v < 0 -> act_slope * v; relu_ref (leading dimension
 *   ld_relu): v kept only where relu_ref[m][n] > 0; rowmask[m] == 0: v = 0; c_rowmap[m]: output row (< 0: row dropped; the accumulate
 *   read is at the remapped row);  taps > 1 (form 1): the conv input-gradient tap walk of mtts_conv1d_f32 mode 1;  a_tap_rows != 0 (forms 0 / 1):
 *   k = tap * a_tap_k + kin reads A row m + tap * a_tap_rows (a_tap_k % 32 == 0);  colsum (form 2): colsum[z * colsum_gs + m] = sum over the
 *   group's K rows r of A[r][m] * colsum_w[z * colsum_w_gs + 4 r] (colsum_w is [rows][4], only column 0 counts); A2 / B2: dual source.
 * family 0 (auto) / 4064 (force the LDS-DMA kernels: device build only; -1 where they cannot take a problem, and -1 after the launch if any
 * other kernel ran — a forced family never falls back silently).
 * splitk_ws / splitk_ctr: both NULL (K is never split) or the CALLER's device workspace of mtts_gemm_splitk_ws_bytes() /
 * mtts_gemm_splitk_ctr_bytes() bytes, counters zeroed once (a launch leaves them zero); nothing is allocated inside.
 * report (host, [n][2], may be NULL): per problem the split factor S and the placement (0 plain, 1 task-per-XCD schedule, 2 panel order).
 * Returns -1 without launching for: n outside 1..6, a family other than 0 / 4064, one of splitk_ws / splitk_ctr without the other, NULL
 * operands, one of A2 / B2 without the other, a form outside 0..2, groups / max_M / max_N < 1, flag bits beyond 0..2, colsum on a form
 * other than 2, with a table or without colsum_w, a_tap_rows != 0 with a_tap_k % 32 != 0 or on form 2, table together with dimptr,
 * host_dims without dimptr, dimptr with dim_stride < 1, dim_mult < 1 or dim_sel other than 0 / 2, relu_ref with ld_relu < 1, taps > 1 on
 * a form other than 1 or with tap_k < 1 (family 4064: with tap_k % 32 != 0). */
typedef struct mtts_gemm_group {
    long long a_off, b_off, c_off;
    int M, N, K;
    int lda, ldb, ldc;
} mtts_gemm_group;
typedef struct mtts_gemm_desc {
    const float* A; const float* B; float* C; const float* A2; const float* B2;
    long long a_gs, b_gs, c_gs, a2_gs, b2_gs;
    const int* dimptr; const int* host_dims; const mtts_gemm_group* table;
    const float* bias; long long bias_gs;
    const unsigned char* rowmask; long long rowmask_gs;
    const float* relu_ref; long long relu_ref_gs;
    const int* c_rowmap; long long c_rowmap_gs;
    float* colsum; long long colsum_gs;
    const float* colsum_w; long long colsum_w_gs;
    int form, groups, max_M, max_N;
    int M, N, K, lda, ldb, ldc;
    int dim_stride, dim_sel, dim_mult;
    int ld_relu, flags;
    float alpha, act_slope;
    int taps, tap_k, tap_bstride, a_tap_k, a_tap_rows;
} mtts_gemm_desc;
int64_t mtts_gemm_splitk_ws_bytes(void);
int64_t mtts_gemm_splitk_ctr_bytes(void);
int mtts_gemm_f32_grouped(const mtts_gemm_desc* probs, int n, int family, float* splitk_ws, int* splitk_ctr, int* report, void* hip_stream);
/* The bf16 operand family on one problem (csrc/gemm_bf16.h): C = alpha * (op(A, B) [+ op(A2, B2)]) + bias with fp32 A / B in memory,
 * rounded to bf16 on the way into LDS, v_mfma_f32_32x32x16_bf16, fp32 accumulation.  A2 / B2 both NULL or both set.  tile 0 (auto) / 64 / 128
 * (+ 1000 * K-slices kept in flight per workgroup: micro-benchmarks). */
int mtts_gemm_bf16(int form, int M, int N, int K, const float* A, int lda, const float* B, int ldb, const float* A2, const float* B2,
                   float* C, int ldc, const float* bias, float alpha, int flags, int tile, void* hip_stream);
/* bf16 operand planes at kernel level (numerics mode 1's long NT problems): mtts_to_bf16 rounds n (a multiple of 8) floats to bf16
 * (round to nearest even) — the plane of an activation slab; mtts_gemm_bf16_planes computes C[M][N] = alpha * Ah[M][K] . Bh[N][K]^T
 * (+ bias, flags as mtts_gemm_f32) from the two planes and, when Ch is set, writes C's own bf16 twin beside it.  K, lda, ldb in whole
 * groups of 8.  mtts_plane_problems: how many GEMM problems of this handle have run on the plane-staged K-loop so far. */
int mtts_to_bf16(const float* src, unsigned short* dst, long long n, void* stream);
int mtts_gemm_bf16_planes(int M, int N, int K, const unsigned short* Ah, int lda, const unsigned short* Bh, int ldb, float* C, unsigned short* Ch,
                          int ldc, const float* bias, float alpha, int flags, int tile, void* stream);
long long mtts_plane_problems(mtts_handle* h);
/* Host-only self check of the task-per-XCD workgroup schedule of 8- / 4- / 2-group launches (csrc/gemm.h: XcdSched): builds the schedule
 * for the `groups` group sizes `dims` (cls 1: M-ragged, units = m-tiles of 64 rows with tn tiles each; cls 2: K-ragged, units_per_group
 * tiles per group whose cost is dims[z]) and walks every workgroup slot.  Returns the number of slots when every (group, tile) is visited
 * exactly once, -1 otherwise; *max_load_permille (optional) = heaviest XCD's work in 1/1000 of a perfect eighth. */
int mtts_xcd_schedule_check(const int* dims, int groups, int cls, int tn, int units_per_group, int* max_load_permille);
/* Conv1d over one zero-guarded sequence, channels-last: x [L][Cin] with >= k/2 zero rows before and
 * after, w [Cout][k][Cin].  mode 0: y = conv(x) + bias; 1: dx = dgrad(dy); 2: dw = wgrad(dy, x) */
int mtts_conv1d_f32(int mode, int L, int Cin, int Cout, int k, const float* x_or_dy, const float* w_or_x, float* out,
                    const float* bias, int tile, void* hip_stream);

/* ---- kernel-level entry points of the HBM-bound (non-GEMM) kernels, so each can be parity-tested alone (dev pointers; rows are
 * dense [rows][C] fp32 matrices, C % 4 == 0, C <= 1024; `ws` = caller-allocated device scratch of mtts_kernel_ws_bytes(rows, n_mat)
 * bytes; nothing is allocated inside; asynchronous on `stream` apart from a <= 64-byte descriptor upload) -------------------
 * layernorm: transformer/SubLayers.py:55,91 + modules.py:222-235 (eps 1e-5): z = a + res (res may be NULL; z may be NULL),
 *   y = LN(z) * gamma + beta on rows with mask != 0 (mask NULL: all), 0 elsewhere; stats[row] = (mean, rstd).  bwd: dz, dgamma, dbeta.
 * softmax / sdpa: transformer/Modules.py:14-25 for n_mat independent (sequence, head) pairs of length L; S, P are
 *   [n_mat][L][ldS], ldS = (L + 3) & ~3; q, k, v, o are [n_mat][L][dk].  softmax_bwd turns dP into dS = alpha * P o (dP - rowsum(dP o P)) in place.
 * batchnorm: PostNet BatchNorm1d in training mode over the rows with inrect != 0 (transformer/Layers.py:129-137), optional tanh;
 *   stats [3C] = mean | rstd | unbiased var.  bwd takes n_in = number of such rows.
 * table_grad: nn.Embedding backward, dtable [V][C] fully written, rows summed in ascending order, skip_row (padding_idx) stays 0. */
int64_t mtts_kernel_ws_bytes(int rows, int n_mat);
int mtts_layernorm_fwd(int rows, int C, const float* a, const float* res, const float* gamma, const float* beta, const unsigned char* mask,
                       float* z, float* y, float* stats, void* ws, void* hip_stream);
int mtts_layernorm_bwd(int rows, int C, const float* dy, const float* z, const float* stats, const float* gamma, const unsigned char* mask,
                       float* dz, float* dgamma, float* dbeta, void* ws, void* hip_stream);
int mtts_softmax_fwd(int n_mat, int L, float* S, void* ws, void* hip_stream);
int mtts_softmax_bwd(int n_mat, int L, const float* P, float* dP, float alpha, void* ws, void* hip_stream);
int mtts_sdpa_fwd(int n_mat, int L, int dk, const float* q, const float* k, const float* v, float* P, float* o, void* ws, void* hip_stream);
/* attention in the packed layout the engine runs: n_seq sequences of lens[i] rows starting at row row0[i] (host arrays) of
 *   qkv / gqkv [rows][3 * heads * dk] (column blocks Q | K | V, one head = dk columns) and O / dO [rows][heads * dk]; group
 *   n = seq * heads + head keeps its P / dS matrix [L][ldS], ldS = (L + 3) & ~3, at the running sum of L * ldS.  fwd: P = softmax(Q K^T /
 *   sqrt(dk)), O = P V; path 0 = the engine's route (the fused kernel where it serves the launch, else GEMM + softmax + GEMM), 1 = the
 *   three launches.  bwd: dS = P o (dP - rowsum(dP o P)) / sqrt(dk) with dP = dO V^T, gqkv = dS K | dS^T Q | P^T dO.  Rows outside the
 *   sequences are neither read into a result nor written; P and dS may hold anything on entry (their pad columns are written, zero).
 *   ws = mtts_attn_packed_ws_bytes(n_seq, heads) bytes of device scratch.  -1: null pointer, dk % 4, n_seq / heads / a length < 1, a
 *   negative row0, ws_bytes too small, path not 0 / 1. */
int64_t mtts_attn_packed_ws_bytes(int n_seq, int heads);
int mtts_attn_packed_fwd(int n_seq, int heads, int dk, const int* lens, const int* row0, int path, const float* qkv, float* P, float* O,
                         void* ws, int64_t ws_bytes, void* hip_stream);
int mtts_attn_packed_bwd(int n_seq, int heads, int dk, const int* lens, const int* row0, const float* qkv, const float* P, const float* dO,
                         float* dS, float* gqkv, void* ws, int64_t ws_bytes, void* hip_stream);
int mtts_batchnorm_fwd(int rows, int C, const float* x, const unsigned char* inrect, const float* gamma, const float* beta, int do_tanh,
                       float* stats, float* y, void* ws, void* hip_stream);
int mtts_batchnorm_bwd(int rows, int n_in, int C, const float* dy, const float* y, const float* x, const float* stats, const unsigned char* inrect,
                       const float* gamma, int do_tanh, float* dx, float* dgamma, float* dbeta, void* ws, void* hip_stream);
int mtts_table_grad(int rows, int C, int V, const float* dx, const int* idx, int skip_row, float* dtable, void* ws, void* hip_stream);
/* length_regulate (replaces LengthRegulator.LR / expand, lightning/model/modules.py:167-190, and its autograd transpose):
 *   fwd: out[r][:] = x[src[r]][:] (+ spk[:]) (+ pos[row_t[r]][:]) for r < n_frames, zeros where src[r] < 0; spk [C], pos [*][C] and row_t
 *   may be NULL (plain gather; pos needs row_t).  bwd: dx[p][:] (+)= sum of dout over frame rows [first[p], first[p] + count[p]).
 * layernorm_jvp / softmax_jvp: the forward-mode (tangent) twins the second-order path is built from (csrc/tangent.h), on the z / stats
 *   written by mtts_layernorm_fwd resp. the probabilities written by mtts_softmax_fwd; tgamma / tbeta / tres / mask may be NULL. */
int mtts_length_regulate_fwd(int n_frames, int C, const float* x, const int* src, const float* spk, const float* pos, const int* row_t, float* out,
                             void* ws, void* hip_stream);
int mtts_length_regulate_bwd(int n_phonemes, int C, const float* dout, const int* first, const int* count, float* dx, int accumulate, void* ws,
                             void* hip_stream);
int mtts_layernorm_jvp(int rows, int C, const float* ta, const float* tres, const float* z, const float* stats, const float* gamma, const float* tgamma,
                       const float* tbeta, const unsigned char* mask, float* ty, void* ws, void* hip_stream);
int mtts_softmax_jvp(int n_mat, int L, const float* P, float* tS, void* ws, void* hip_stream);
/* The rest of the second-order row kernels (csrc/tangent.h; ColArgs modes 5 and 6 of csrc/rowops.h), one entry per kernel.  "t" prefixes
 * the tangent of a forward value, "tg" the tangent of a gradient, "h" a tangent parameter gradient (= Hessian-vector product row).
 * layernorm_jvp_full: layernorm_jvp that also keeps tz_out [rows][C] = ta + tres and tstats_out [rows][2] (either may be NULL).
 * layernorm_jvp_bwd: primal dz and tangent tgz of the LayerNorm backward, hgamma / hbeta [C]; relu_on_z multiplies both by [z > 0];
 *   two_launch 0: hgamma / hbeta from the kernel's own 8-row partials, 1: from a column reduction of its own (another summation order).
 * softmax_jvp_bwd: in place, dP -> dS = alpha P (dP - c), tgP -> tg_S; pad columns [L, ldS) are zeroed.
 * batchnorm_jvp: tsum [2C] = [sum tx xhat | sum tx] over the inrect rows and ta = tangent of y; y / stats from mtts_batchnorm_fwd.
 * batchnorm_jvp_bwd: dx, tdx, hgamma, hbeta; dgamma / dbeta from mtts_batchnorm_bwd, tsum / ta from mtts_batchnorm_jvp.
 * rowdot_jvp: tout [rows] = valid ? tx . w + x . tw + tb : 0 (tb: one float);  rowdot_jvp_bwd: dx = dout w, tdx = tgout w + dout tw.
 * tgamma / tbeta / tw / tb / mask may be NULL. */
int mtts_layernorm_jvp_full(int rows, int C, const float* ta, const float* tres, const float* z, const float* stats, const float* gamma,
                            const float* tgamma, const float* tbeta, const unsigned char* mask, float* ty, float* tz_out, float* tstats_out, void* ws,
                            void* hip_stream);
int mtts_layernorm_jvp_bwd(int rows, int C, const float* dy, const float* tgy, const float* z, const float* stats, const float* tz, const float* tstats,
                           const float* gamma, const float* tgamma, const unsigned char* mask, int relu_on_z, int two_launch, float* dz, float* tgz,
                           float* hgamma, float* hbeta, void* ws, void* hip_stream);
int mtts_softmax_jvp_bwd(int n_mat, int L, const float* P, const float* tP, float* dP, float* tgP, float alpha, void* ws, void* hip_stream);
int mtts_batchnorm_jvp(int rows, int n_in, int C, const float* x, const float* tx, const float* stats, const float* gamma, const float* tgamma,
                       const float* tbeta, const float* y, const unsigned char* inrect, int do_tanh, float* tsum, float* ta, void* ws, void* hip_stream);
int mtts_batchnorm_jvp_bwd(int rows, int n_in, int C, const float* dy, const float* tgy, const float* y, const float* ta, const float* x, const float* tx,
                           const float* stats, const float* tsum, const float* gamma, const float* tgamma, const float* dgamma, const float* dbeta,
                           const unsigned char* inrect, int do_tanh, float* dx, float* tdx, float* hgamma, float* hbeta, void* ws, void* hip_stream);
int mtts_rowdot_jvp(int rows, int C, const float* x, const float* tx, const float* w, const float* tw, const float* tb, const unsigned char* valid,
                    float* tout, void* ws, void* hip_stream);
int mtts_rowdot_jvp_bwd(int rows, int C, const float* dout, const float* tgout, const float* w, const float* tw, float* dx, float* tdx, void* ws,
                        void* hip_stream);
/* Multi-task entries of the loss, optimizer and variance-adaptor row kernels (csrc/rowops.h), each through the launcher the engine uses.
 * `tasks` in 1 .. 8; rows / B / Mr / Mp / nF / nP are HOST int arrays [tasks] (per-task counts, >= 0, the largest >= 1); `ts` is a HOST
 * int64 array of task strides in elements (>= 0), one per array in the order given below ("row": the per-row masks and index lists of the
 * entry); task t of an array starts at t * stride.  `ws` = mtts_kernel_ws_bytes(largest count, 0) bytes.  Rows at or past a task's count are
 * not touched.  C % 4 == 0, 4 <= C <= 1024; -1 (nothing launched) on a bad argument.
 *   embed_pos            out = valid ? emb[tok] + pos[row_t] : 0 (pos shared)                                    ts: emb, row, out
 *   speaker_vec          spk[b] = table[ids[b]], or (average) the mean of table[ids[0 .. n)], n = ids[n_ids_max]    ts: table, ids, spk
 *   speaker_table_grad   its transpose, dtable [n_speaker][C] fully written                                      ts: dspk, ids, dtable
 *   add_rowvec           out = inrect ? x + vec[row_b] : 0                                                       ts: x, vec, row, out
 *   bucket_embed_add     out = inrect ? x + table[bucketize(val * control, bins[nb])] : 0; idx_out = bucket | -1 ts: x, val, table, row, out
 *   rowdot / rowdot_bwd  out = valid ? dot(x, w) + b : 0 (w, b share "par") / dx = dout * w                  ts: x, par, row, out / dout, par, dx
 *   segsum               out[b] (+)= sum of X rows [start[b], start[b] + len[b])                                 ts: X, seg, out
 *   duration_round       d = max(round(exp(logd) - 1) * d_control, 0)  (modules.py:132-136)                      ts: pred
 *   fill_padded          X rows with valid == 0 := inrect ? bias : 0, in place                                   ts: X, bias, row
 *   gather               out = rowmap >= 0 ? src[rowmap] : 0                                                     ts: src, row, out
 *   length_regulate_rect out = x[f_src[r2f]] where both indices are >= 0, else 0                                 ts: x, f, row, out
 *   loss / loss_grad     loss.py:19-92.  ptr[15] (HOST array of device pointers): mel, mel_post, mel_tgt [Mr][n_mel], rvalid [Mr] (bytes), pp, ep,
 *                        logd, p_tgt, e_tgt [Mp], dur [Mp] (ints), pvalid [Mp] (bytes), pp_r, ep_r, p_tgt_r, e_tgt_r [Mr] (NULL unless that level is
 *                        frame); nF / nP = the valid rows among Mr / Mp (the divisors).  losses [tasks][6] = total, mel, postnet mel, pitch, energy,
 *                        duration; the gradients are scale * d(total)/d(prediction).                ts: mel, rrow, prow, pred, pred_r
 * The flat optimizer kernels take n4 = float4 per task array and the grid cap (n_partials in 1 .. 4096 / max_blocks >= 1):
 *   sumsq_norm  out_norm[0] = sqrt(sum g^2 (+ extra[0])), partial [n_partials] caller scratch;  adam_clip  clip_grad_norm_(max_norm; <= 0: none) on the
 *   device norm + Adam step `step` on w, m, v in place;  sgd_update  w[t] -= lr g[t];  sum_tasks  out (+)= scale * sum_t g[t];  broadcast  dst[t] = src. */
int mtts_rows_embed_pos(int tasks, const int* rows, int C, const float* emb, const float* pos, const int* tok, const int* row_t, const unsigned char* valid,
                        float* out, const int64_t* ts, void* ws, void* hip_stream);
int mtts_rows_speaker_vec(int tasks, const int* B, int C, const float* table, const int* ids, int n_ids_max, int average, float* spk, const int64_t* ts,
                          void* ws, void* hip_stream);
int mtts_rows_speaker_table_grad(int tasks, const int* B, int C, int n_speaker, const float* dspk, const int* ids, int n_ids_max, int average, float* dtable,
                                 const int64_t* ts, void* ws, void* hip_stream);
int mtts_rows_add_rowvec(int tasks, const int* rows, int C, const float* x, const float* vec, const int* row_b, const unsigned char* inrect, float* out,
                         const int64_t* ts, void* ws, void* hip_stream);
int mtts_rows_bucket_embed_add(int tasks, const int* rows, int C, const float* x, const float* val, float control, const float* bins, int nb,
                               const float* table, const unsigned char* inrect, int* idx_out, float* out, const int64_t* ts, void* ws, void* hip_stream);
int mtts_rows_rowdot(int tasks, const int* rows, int C, const float* x, const float* w, const float* b, const unsigned char* valid, float* out,
                     const int64_t* ts, void* ws, void* hip_stream);
int mtts_rows_rowdot_bwd(int tasks, const int* rows, int C, const float* dout, const float* w, float* dx, const int64_t* ts, void* ws, void* hip_stream);
int mtts_rows_segsum(int tasks, const int* B, int C, const float* X, const int* start, const int* len, float* out, int accumulate, const int64_t* ts,
                     void* ws, void* hip_stream);
int mtts_rows_duration_round(int tasks, const int* rows, const float* logd, float d_control, float* d_rounded, const int64_t* ts, void* ws, void* hip_stream);
int mtts_rows_fill_padded(int tasks, const int* rows, int C, float* X, const float* bias, const unsigned char* inrect, const unsigned char* valid,
                          const int64_t* ts, void* ws, void* hip_stream);
int mtts_rows_gather(int tasks, const int* rows, int C, const float* src, const int* rowmap, float* out, const int64_t* ts, void* ws, void* hip_stream);
int mtts_rows_length_regulate_rect(int tasks, const int* rows, int C, const float* x, const int* f_src, const int* r2f, float* out, const int64_t* ts,
                                   void* ws, void* hip_stream);
int mtts_rows_loss(int tasks, const int* Mr, const int* Mp, const int* nF, const int* nP, int n_mel, int pitch_frame, int energy_frame,
                   const void* const* ptr, const int64_t* ts, float* losses, void* ws, void* hip_stream);
int mtts_rows_loss_grad(int tasks, const int* Mr, const int* Mp, const int* nF, const int* nP, int n_mel, int pitch_frame, int energy_frame,
                        const void* const* ptr, const int64_t* ts, float scale, float* dmel, float* dpost, float* dpp, float* dep, float* dlogd, float* dpp_r,
                        float* dep_r, void* ws, void* hip_stream);
int mtts_sumsq_norm(const float* g, int64_t n4, int n_partials, const float* extra, float* partial, float* out_norm, void* hip_stream);
int mtts_adam_clip(float* w, const float* g, float* m, float* v, int64_t n4, const float* norm, float max_norm, float lr, float b1, float b2, float eps,
                   int step, float weight_decay, int max_blocks, void* hip_stream);
int mtts_sgd_update(int tasks, float* w, int64_t w_ts, const float* g, int64_t g_ts, int64_t n4, float lr, int max_blocks, void* hip_stream);
int mtts_sum_tasks(int tasks, const float* g, int64_t g_ts, float scale, float* out, int64_t n4, int accumulate, int max_blocks, void* hip_stream);
int mtts_broadcast(int tasks, const float* src, float* dst, int64_t dst_ts, int64_t n4, int max_blocks, void* hip_stream);
/* The d-vector speaker encoder's kernels (mtts_dvector_* below), one at a time: raw device pointers, no scratch, asynchronous on the
 * stream, -1 (nothing launched) on a null required pointer or a shape mtts_dvector_create refuses: H a multiple of 64 in 64 .. 1024, E a
 * multiple of 4 in 4 .. 256, N, T, B >= 1.  Gate order i, f, g, o.
 * lstm_recurrent: xp [N][T][4H] (input projection, biases included), whhT [H][4H] (weight_hh TRANSPOSED) -> hlast [N][H], hseq [N][T][H]
 * or NULL, and gates [N][T][4H] (after their non-linearities) / cseq [N][T][H] / hprev [N][T][H]: all three (training) or all NULL.
 * lstm_bptt: dh_ext [N][T][H] or NULL, dh_last [N][H] or NULL, whh [4H][H] -> dgates [N][T][4H] (gradient of the gate pre-activations).
 * dvec_head: part = raw / ||raw||, raw = relu(hlast wT + bias) (wT [H][E]; eraw [N][E] = raw or NULL); dvec_head_bwd: w [E][H].
 * dvec_utterance: out[b] = normalize(mean(part[off[b] .. off[b+1]))) with off [B + 1] device ints; dvec_utterance_bwd: dout -> dpart. */
int mtts_lstm_recurrent(int N, int T, int H, const float* xp, const float* whhT, float* hseq, float* hlast, float* gates, float* cseq, float* hprev,
                        void* hip_stream);
int mtts_lstm_bptt(int N, int T, int H, const float* gates, const float* cseq, const float* dh_ext, const float* dh_last, const float* whh,
                   float* dgates, void* hip_stream);
int mtts_dvec_head(int N, int H, int E, const float* hlast, const float* wT, const float* bias, float* part, float* eraw, void* hip_stream);
int mtts_dvec_head_bwd(int N, int H, int E, const float* eraw, const float* dpart, const float* w, float* dz, float* dh_last, void* hip_stream);
int mtts_dvec_utterance(int B, int E, const float* part, const int* off, float* out, void* hip_stream);
int mtts_dvec_utterance_bwd(int B, int E, const float* part, const int* off, const float* dout, float* dpart, void* hip_stream);

/* ---- MelGAN generator: mel -> waveform --------------------------------------------
 * Replaces `LightningMelGAN.inverse / infer`, lightning/utils.py:8-30 (vocoder.mel2wav of torch.hub
 * "descriptinc/melgan-neurips"; the generator is an un-vendored dependency: architecture of that hub entry, weights
 * supplied by the caller).  Tensors (weight-norm already folded, see meta_tts_amd/vocoder.py):
 *   conv_in.w [C0][7][n_mel], conv_in.b [C0];  up{s}.w [r][C_out][2*C_in] (phase-major polyphase image of the
 *   ConvTranspose1d), up{s}.b;  res{s}.{j}.w1 [C][3][C], .b1, .w2 [C][C], .b2, .ws [C][C], .bs;  conv_out.w [7][C_last],
 *   conv_out.b [1];  C0 = ngf << n_ratios.
 * infer: mel [B][T_max][n_mel] (host), mel_lens[b] frames valid, every value multiplied by mel_scale (the reference
 * passes mel / ln 10) -> wav [B][T_max * hop] floats in (-1, 1), the first mel_lens[b] * hop samples of a row written.
 * infer_device: same with device pointers (no copies, no synchronisation; runs on the vocoder's stream); mel_utt_stride =
 * floats between consecutive utterances of mel_dev (0: T_max * n_mel) so that the engine's own mel buffer can be fed as it
 * is (mtts_get_mel_device). */
typedef struct mtts_vocoder mtts_vocoder;
int mtts_vocoder_create(int n_mel, int ngf, int n_res, const int* ratios, int n_ratios, int device, int max_B, int max_T,
                        mtts_vocoder** out);
void mtts_vocoder_destroy(mtts_vocoder* h);
const char* mtts_vocoder_last_error(mtts_vocoder* h);
int mtts_vocoder_set_stream(mtts_vocoder* h, void* hip_stream);
int mtts_vocoder_hop(mtts_vocoder* h);
int mtts_vocoder_param_count(mtts_vocoder* h);
int mtts_vocoder_param_info(mtts_vocoder* h, int index, char* name, int name_cap, int64_t* numel);
int mtts_vocoder_load(mtts_vocoder* h, const char* name, const float* data, int64_t numel);
int mtts_vocoder_infer(mtts_vocoder* h, const float* mel, int B, int T_max, const int* mel_lens, float mel_scale, float* wav);
int mtts_vocoder_infer_device(mtts_vocoder* h, const float* mel_dev, int64_t mel_utt_stride, int B, int T_max, const int* mel_lens,
                              float mel_scale, float* wav_dev);

/* ---- HiFi-GAN generator: mel -> waveform, the second neural vocoder ------------------------
 * Stands behind the `name == "HiFi-GAN"` branch of utils/model.py:32-50 (vocoder(mels).squeeze(1)).  The generator is NOT part of the
 * reference tree (neither its code nor generator_universal.pth.tar): parity with published weights is UNPINNED; what is pinned is this
 * definition (the published Generator with ResBlock type "1"), restated in torch by tests/hifigan_oracle.py:
 *     x = conv_pre(mel)                                  Conv1d(n_mel -> C0, k 7, zero pad 3)
 *     for i in 0..n_up-1:
 *         x = leaky_relu(x, 0.1);  x = ups[i](x)         ConvTranspose1d(C_i -> C_i/2, k = 2 r_i, stride r_i, pad r_i/2)
 *         x = (1/n_k) * sum_j resblocks[i*n_k + j](x)    (the "MRF" mean over the n_k kernel sizes)
 *     x = leaky_relu(x, 0.01);  x = conv_post(x)         Conv1d(C_last -> 1, k 7, zero pad 3);  tanh
 *     ResBlock1(k, (d_0..d_{m-1})): for each d:  t = leaky_relu(x, 0.1);  t = conv(k, dilation d, zero pad d(k-1)/2)(t)
 *                                                t = leaky_relu(t, 0.1);  t = conv(k, dilation 1, zero pad (k-1)/2)(t);  x = t + x
 * Zero padding is applied at each utterance's own ends: an utterance of a ragged batch is computed as if it were alone.
 * create: rates [n_rates] (each even and >= 2; the transposed kernel is 2 * rate, the published V1 / V2 / V3 relation), res_kernels
 * [n_res_kernels <= 4] odd and <= 11, res_dilations [n_res_kernels][n_dil <= 4] in 1..5, resblock_type 1 (2 is refused), n_mel a
 * multiple of 16, initial_channels a multiple of 16 << n_rates; anything else is refused with a message that names the argument.
 * direct_max_channels: 0, 32 or 64 — stages whose channel count is 32 or 64 and <= this value take the direct convolution kernel
 * (csrc/hifigan.h) instead of the grouped GEMM; 0: GEMM route everywhere.  Both routes compute the same definition.
 * Tensors (weight-norm already folded, see meta_tts_amd/hifigan.py):
 *   conv_pre.w [C0][7][n_mel], conv_pre.b [C0];  ups.{i}.w [r][C_out][2*C_in] (phase-major polyphase image: x[q-1] | x[q]), ups.{i}.b;
 *   resblocks.{i*n_k+j}.convs1.{m}.w and .convs2.{m}.w [C][k][C], .b [C];  conv_post.w [7][C_last], conv_post.b [1].
 * infer / infer_device: the pointer, stride, stream and asynchrony contract of the MelGAN entries above; mel_lens[b] in 4..T_max. */
typedef struct mtts_hifigan mtts_hifigan;
int mtts_hifigan_create(int n_mel, int initial_channels, const int* rates, int n_rates, const int* res_kernels, int n_res_kernels,
                        const int* res_dilations, int n_dil, int resblock_type, int direct_max_channels, int device, int max_B, int max_T,
                        mtts_hifigan** out);
void mtts_hifigan_destroy(mtts_hifigan* h);
const char* mtts_hifigan_last_error(mtts_hifigan* h);
int mtts_hifigan_set_stream(mtts_hifigan* h, void* hip_stream);
int mtts_hifigan_hop(mtts_hifigan* h);
int mtts_hifigan_param_count(mtts_hifigan* h);
int mtts_hifigan_param_info(mtts_hifigan* h, int index, char* name, int name_cap, int64_t* numel);
int mtts_hifigan_load(mtts_hifigan* h, const char* name, const float* data, int64_t numel);
int mtts_hifigan_infer(mtts_hifigan* h, const float* mel, int B, int T_max, const int* mel_lens, float mel_scale, float* wav);
int mtts_hifigan_infer_device(mtts_hifigan* h, const float* mel_dev, int64_t mel_utt_stride, int B, int T_max, const int* mel_lens,
                              float mel_scale, float* wav_dev);
/* Numerics of the generator.  Mode 0 (fp32) is the default and is what create built, bit for bit.  Mode 1, "bf16 operands", is the
 * definition above with these changes, restated in torch by tests/hifigan_bf16_oracle.py:
 *   - rounded convolutions: conv_pre, the polyphase images of every ups[i] and every residual convolution multiply operands rounded to
 *     bf16 (round to nearest even); products are exact, accumulation is fp32;
 *   - what gets rounded: the activation operand is the value the fp32 route feeds the convolution — mel * mel_scale for conv_pre, the
 *     LeakyReLU image of x elsewhere — each element rounded once; the weight operand is the folded fp32 weight, rounded once (when the
 *     operand is staged, or when the direct kernel's image is packed at load / set_numerics);
 *   - what stays fp32: bias, LeakyReLU, residual add, the MRF mean, every tensor in HBM, and conv_post + tanh;
 *   - zero padding stays at each utterance's own ends, and no split-K is used: an utterance is the same bits alone or in any ragged batch.
 * set_numerics(mode, direct_max_channels): mode 0 takes direct_max_channels 0 / 32 / 64, mode 1 takes 0 / 32 / 64 / 128 (stages of 32,
 * 64 or 128 channels and <= the value run hg_conv_direct_bf16_kernel, the rest the bf16 GEMM family); anything else is refused before
 * any launch with a message naming the argument.  Tensors loaded after the call are re-packed.  get_numerics: the mode in force.
 * conv_bf16 (kernel-level, for tests): ONE convolution of mode 1 on HOST arrays, without the network around it:
 *   v = bias + conv(k odd <= 11, dilation d in 1..5, zero pad d (k-1)/2)(bf16(leaky_relu(x, in_slope))) with bf16(w)
 *   epilogue 0: out = leaky_relu(v, 0.1);  1: out = v + res;  2: mrf = (mrf_init ? 0 : mrf) + inv_nk * (v + res)
 * x, res, out, mrf [B][T_max][C] with C in {32, 64, 128}, B <= max_B, w [C][k][C], lens[b] in 1..T_max; rows >= lens[b] of out / mrf
 * are left untouched.  route 0: the direct kernel; route 1: the GEMM route (pad pass, bf16 GEMM family, accumulate epilogue). */
int mtts_hifigan_set_numerics(mtts_hifigan* h, int mode, int direct_max_channels);
int mtts_hifigan_get_numerics(mtts_hifigan* h);
int mtts_hifigan_conv_bf16(mtts_hifigan* h, int route, int C, int k, int d, int B, int T_max, const int* lens, const float* x, const float* w,
                           const float* bias, float in_slope, int epilogue, const float* res, float* mrf, float inv_nk, int mrf_init, float* out);

/* ---- d-vector speaker encoder, forward only (`speaker_emb: dvec`) -------------------------
 * Replaces `SpeakerEncoder.forward` for emb_type "dvec" (lightning/model/speaker_encoder.py:54-60,71-76): the frozen
 * resemblyzer `VoiceEncoder` (un-vendored; architecture restated by the reference's own GE2E class, :11-31: LSTM(n_mels -> hidden,
 * `layers` layers, batch_first) + Linear(hidden -> emb) + ReLU), applied to the partial utterances of the batch
 * (`spk_ref_mel_slices`, lightning/collate.py:29-43): partial embedding = L2-normalised ReLU(Linear(final hidden state of the last
 * layer)); utterance embedding = F.normalize(mean of its partials).  The trained variants ("encoder", "scratch_encoder") are the
 * mtts_dvector_enable_training / embed_train / backward / adam_step entries further down.
 * Tensors (torch names and layouts): lstm.weight_ih_l{k} [4*hidden][in], lstm.weight_hh_l{k} [4*hidden][hidden],
 * lstm.bias_ih_l{k}, lstm.bias_hh_l{k} [4*hidden] (gate order i, f, g, o), linear.weight [emb][hidden], linear.bias [emb].
 * embed: mels [n_partials][frames][n_mels] (host), utt_offsets [n_utts + 1] (partials of utterance b = [off[b], off[b+1]),
 * off[0] = 0, off[n_utts] = n_partials) -> out [n_utts][emb] (host; feed it to mtts_batch.spk_emb); partial_out
 * [n_partials][emb] or NULL.  Synchronous. */
typedef struct mtts_dvector mtts_dvector;
int mtts_dvector_create(int n_mels, int hidden, int layers, int emb, int max_partials, int frames, int max_utts, int device, mtts_dvector** out);
void mtts_dvector_destroy(mtts_dvector* h);
/* HIP stream of this handle's launches (default: the null stream).  A trained encoder exchanges device scalars with the engine (its
 * gradient's sum of squares -> mtts_set_extra_grad_sumsq, the joint norm <- mtts_grad_norm_dev): put both handles on ONE stream. */
int mtts_dvector_set_stream(mtts_dvector* h, void* hip_stream);
const char* mtts_dvector_last_error(mtts_dvector* h);
int mtts_dvector_load(mtts_dvector* h, const char* name, const float* data, int64_t numel);
int mtts_dvector_embed(mtts_dvector* h, const float* mels, int n_partials, const int* utt_offsets, int n_utts, float* out, float* partial_out);
/* Trained speaker encoders (`speaker_emb: encoder` / `scratch_encoder`, config/algorithm/{encoder,scratch_encoder}.yaml: baseline
 * systems whose optimizer also owns the LSTM; speaker_encoder.py:54-55,59-60).  enable_training allocates the saved-state, gradient
 * and Adam buffers.  embed_train = embed that keeps the gate activations / cell states for the backward sweep; backward takes
 * dout [n_utts][emb] (host) = dLoss/d(embedding) — mtts_get_speaker_grad of the engine — and fills the parameter gradients by
 * back-propagation through time (hand-derived; autograd of nn.LSTM in the reference).  grad_sumsq returns a DEVICE scalar, the sum
 * of squares of those gradients, to be handed to mtts_set_extra_grad_sumsq so that mtts_outer_update clips by the joint norm of all
 * parameters (main.py:61); adam_step then applies the same clip coefficient (norm_dev = mtts_grad_norm_dev(engine), NULL: no clip)
 * and the Adam rule of optimizer.py:9-15.  export / import: which = 0 parameter, 1 gradient, 2 Adam m, 3 Adam v. */
int mtts_dvector_enable_training(mtts_dvector* h);
int mtts_dvector_embed_train(mtts_dvector* h, const float* mels, int n_partials, const int* utt_offsets, int n_utts, float* out);
int mtts_dvector_backward(mtts_dvector* h, const float* dout);
const float* mtts_dvector_grad_sumsq(mtts_dvector* h);
int mtts_dvector_adam_step(mtts_dvector* h, const float* norm_dev, float max_norm, float lr, float b1, float b2, float eps, float weight_decay);
int mtts_dvector_set_optimizer_step(mtts_dvector* h, int step);
int mtts_dvector_export(mtts_dvector* h, const char* name, int which, float* out, int64_t numel);
int mtts_dvector_import(mtts_dvector* h, const char* name, int which, const float* data, int64_t numel);

/* ---- GE2E training of the d-vector encoder ------------------------------------------------
 * The objective the reference's from-scratch encoder class is named after (`GE2E`, speaker_encoder.py:11-31).  No GE2E loss code exists
 * in the reference tree: what follows is the softmax variant of Wan et al. 2018 ("Generalized end-to-end loss for speaker
 * verification") as the Real-Time-Voice-Cloning trainer states it, written down from memory.  Parity with any published GE2E code is
 * UNPINNED; what is pinned is THIS definition, restated in float64 torch with autograd by tests/ge2e_oracle.py.
 *
 * Definition.  Embeddings e[j][i], speaker j of N >= 2, utterance i of M >= 2, dimension E, rows speaker-major (row = j * M + i).  They
 * arrive L2-normalised from the encoder; the loss does not rely on that.  S_k = sum_i e[k][i].
 *   1. inclusive centroid  c_k = S_k / |S_k|  (the normalised mean)
 *   2. exclusive centroid  chat_ji = u / |u|,  u = (S_j - e[j][i]) / (M - 1)
 *   3. similarities        s[ji][k] = w * (e[j][i] . c_k) + b  for k != j,   s[ji][j] = w * (e[j][i] . chat_ji) + b
 *                          (a plain dot product: e is not renormalised to a cosine)
 *   4. loss                L = 1 / (N M) * sum_ji ( logsumexp_k s[ji][k] - s[ji][j] )
 *   5. gradients           dL/de does NOT detach the centroids; with g = (softmax - onehot) / (N M):
 *                          dL/dw = sum g[ji][k] * (e . centroid)[ji][k],   dL/db = sum g[ji][k]
 *   6. trainer rule        w0 = 10, b0 = -5; the gradients of w and b are multiplied by 0.01; then the joint L2 norm of ALL gradients
 *                          (LSTM, linear, w, b) is clipped to 3 (coefficient min(1, 3 / (norm + 1e-6))); then Adam with lr 1e-4, betas
 *                          (0.9, 0.999), eps 1e-8, no weight decay, bias-corrected as the adam_step entry above.  All are arguments.
 * Limits, refused before any launch with the argument named: 2 <= N <= 1024, 2 <= M <= 64, E a multiple of 4 in 4 .. 256, w finite
 * and not 0.  The limits bound indices and on-chip arrays; the kernels are sized for training batches (64 x 10), and no time has been
 * measured near the limits, where the gradient kernel's serial walks (about 1.3e5 loop trips per thread at 1024 x 64) dominate.
 * Embeddings of a speaker that cancel (S_k = 0 or u = 0) give NaN, as the definition does.  No atomics: a loss and its
 * gradients are the same bits on every run.
 *
 * ge2e_loss: the loss kernels alone on raw DEVICE pointers, asynchronous on hip_stream.  emb [n_spk * n_utt][E] -> loss3 [3] = L, dL/dw,
 * dL/db; demb [n_spk * n_utt][E]; sim [n_spk * n_utt][n_spk] = s, or NULL; ws: scratch of at least ge2e_ws_bytes bytes (0: shape refused).
 * The refusal is read through the d-vector last_error entry with a NULL handle.
 *
 * Handle entries (enable_training first).  w and b live on the device with their own gradient and Adam state; they are NOT tensors of
 * the encoder: load / export / import and the state-dict names are what they were.
 *   ge2e_enable: allocates the loss scratch for any n_spk * n_utt <= max_utts and sets (w, b) = (w0, b0), their Adam state to 0.
 *   ge2e_forward_backward: mels [n_spk * n_utt][frames][n_mels] speaker-major, one partial utterance per utterance, on the host or
 *     (mels_on_device = 1) already on the device, read in place; training forward, loss, dL/de straight into the backward sweep.
 *     Everything is enqueued on the handle's stream; the call waits only when loss_host [1] or sim_host [n_spk * n_utt][n_spk] is given.
 *     n_spk * n_utt <= max_utts and <= max_partials.
 *   ge2e_step: rule 6 on the device, no host round trip: scale, joint norm, clip + Adam on the encoder and on (w, b); the optimizer
 *     step count is the one set_optimizer_step sets.
 *   ge2e_get / ge2e_set: which = 0 value, 1 gradient, 2 Adam m, 3 Adam v of (w, b); wb2_host [2]. */
int mtts_ge2e_loss(int n_spk, int n_utt, int E, const float* emb, float w, float b, float* loss3, float* demb, float* sim, void* ws, size_t ws_bytes,
                   void* hip_stream);
size_t mtts_ge2e_ws_bytes(int n_spk, int n_utt, int E);
int mtts_dvector_ge2e_enable(mtts_dvector* h, float w0, float b0);
int mtts_dvector_ge2e_forward_backward(mtts_dvector* h, const float* mels, int mels_on_device, int n_spk, int n_utt, float* loss_host, float* sim_host);
int mtts_dvector_ge2e_step(mtts_dvector* h, float lr, float b1, float b2, float eps, float max_norm, float scalar_grad_scale);
int mtts_dvector_ge2e_get(mtts_dvector* h, int which, float* wb2_host);
int mtts_dvector_ge2e_set(mtts_dvector* h, int which, const float* wb2_host);

/* ---- waveform -> log-mel spectrogram + frame energy (front-end STFT / mel extraction) ------
 * Replaces `TacotronSTFT.mel_spectrogram` behind `Audio.tools.get_mel_from_wav` (audio/stft.py:128-178, audio/tools.py:8-15):
 * clip to [-1, 1], reflect-pad filter_length / 2, windowed DFT of every hop-spaced frame (STFT.transform, stft.py:52-77), magnitude,
 * mel = log(max(mel_basis @ magnitude, 1e-5)), energy = ||magnitude||_2 per frame.
 * load: forward_basis [2 * (filter_length / 2 + 1)][filter_length] = the reference's `STFT.forward_basis` buffer (real rows then
 * imaginary rows, window folded in, stft.py:27-46); mel_basis [n_mel][filter_length / 2 + 1] = `TacotronSTFT.mel_basis`
 * (librosa.filters.mel, stft.py:143-147).  Either may be NULL to keep what was loaded before.
 * mel_spectrogram: wav [n_samples] (host) -> mel [T][n_mel] (host; the reference returns the transpose, (n_mel, T)), energy [T],
 * T = n_samples / hop_length + 1; returns T, or < 0 on error.  Synchronous. */
typedef struct mtts_stft mtts_stft;
int mtts_stft_create(int filter_length, int hop_length, int n_mel, int max_samples, int device, mtts_stft** out);
void mtts_stft_destroy(mtts_stft* h);
int mtts_stft_set_stream(mtts_stft* h, void* hip_stream);
const char* mtts_stft_last_error(mtts_stft* h);
int mtts_stft_load(mtts_stft* h, const float* forward_basis, const float* mel_basis);
int mtts_stft_mel_spectrogram(mtts_stft* h, const float* wav, int n_samples, float* mel, float* energy);

/* ---- spectrogram -> waveform: the inverse half of the same handle (Griffin-Lim) -----------------
 * Frames are frame-major ([frame][bin], F = filter_length / 2 + 1 bins), the transpose of the reference's (B, F, T) tensors.
 * load_inverse: inverse_basis [2F][filter_length] = the reference's `STFT.inverse_basis` buffer (np.linalg.pinv(scale *
 * fourier_basis).T in float32, scale = filter_length / hop_length, times the window, stft.py:33-45); window_sq [filter_length] = the
 * squared centre-padded window that `window_sumsquare` adds up (audio_processing.py:7-63).  Both required.
 * transform: STFT.transform (stft.py:52-77) of one waveform: reflect padding by filter_length / 2 WITHOUT clipping, magnitude
 * sqrt(re^2 + im^2) and phase atan2(im, re), each [T][F], T = n_samples / hop_length + 1.  Returns T, < 0 on error
 * (n_samples <= filter_length / 2: the reference's F.pad raises).
 * inverse: STFT.inverse (stft.py:79-119) of n_utts spectrograms of n_frames[u] frames each: magnitude, phase [sum T][F];
 * overlap-add, division by the window envelope where it exceeds float32 tiny, x filter_length / hop_length, trim filter_length / 2
 * at both ends.  out: the waveforms packed one after another, hop_length * (T_u - 1) samples each.
 * griffin_lim: audio_processing.py:66-80 with the starting phases `angles` [sum T][F] drawn by the caller (the reference draws
 * np.angle(np.exp(2j pi U[0, 1)))), then n_iters x (transform, inverse with the new phase and the fixed magnitude).
 * n_iters = 0 is `inverse`.
 * inv_mel: the computation of tools.py:18-37 (inv_mel_spec) up to the waveform: log_mel [sum Tm][n_mel] (the mel basis of
 * mtts_stft_load must be loaded), magnitude = 1000 * exp(mel)^T @ mel_basis with the LAST frame of every utterance dropped, then
 * griffin_lim with angles [sum (Tm - 1)][F].  out: hop_length * (Tm_u - 2) samples per utterance.
 * inverse / griffin_lim / inv_mel return the total number of output samples, < 0 on error.  With n_iters > 0 every T must satisfy
 * hop_length * (T - 1) > filter_length / 2 (the next transform's reflect padding; T >= 1 otherwise), n_iters >= 0; errors are reported
 * before any launch.  The workspace grows on demand beyond what max_samples reserved.  All utterances of a call share every launch.
 * Synchronous. */
int mtts_stft_load_inverse(mtts_stft* h, const float* inverse_basis, const float* window_sq);
int mtts_stft_transform(mtts_stft* h, const float* wav, int n_samples, float* magnitude, float* phase);
int64_t mtts_stft_inverse(mtts_stft* h, int n_utts, const int* n_frames, const float* magnitude, const float* phase, float* out);
int64_t mtts_stft_griffin_lim(mtts_stft* h, int n_utts, const int* n_frames, const float* magnitude, const float* angles, int n_iters, float* out);
int64_t mtts_stft_inv_mel(mtts_stft* h, int n_utts, const int* n_mel_frames, const float* log_mel, const float* angles, int n_iters, float* out);

/* ---- waveform batches -> the values of the preprocessed feature tree (the reference's preprocessor/preprocessor.py) -------------
 * The device steps of `Preprocessor.process_utterance` (:188-306) and `build_from_path` (:60-185) on the same handle.  All
 * utterances of a call share every launch; host pointers go in and out; every function returns 0, or < 0 with the reason in
 * mtts_stft_last_error, and every error below is reported before any launch.  dtype: 0 = float32, 1 = float64.  Synchronous.
 * mel_batch: get_mel_from_wav (:227-229) of n_utts waveforms packed one after another in `wavs` (n_samples[u] each), each result
 * truncated to keep_frames[u] frames (sum(duration); < 0 or keep_frames == NULL: all): T_u = min(n_samples[u] / hop_length + 1,
 * keep_frames[u]); mel [sum T][n_mel] log-mel (frame-major, the layout the tree stores), energy [sum T].  Errors: n_samples[u] <=
 * filter_length / 2, keep_frames[u] == 0.  An utterance's rows are bit-identical whatever else is in the call.
 * phoneme_average: :231-261 for n_utts utterances: values packed [sum n_frames], durations packed [sum n_phones], out packed
 * [sum n_phones] of the same dtype.  interpolate != 0 (pitch): interp1d over the zero (unvoiced) frames first, linear between the
 * nearest voiced frames, the first / last voiced value outside them.  Then the reference's in-place loop values[i] =
 * mean(values[pos : pos + d]) (0 where d == 0), pos = durations before i, first n_phones entries — including its aliasing when
 * some pos < i (more zero durations than frames so far), where a later mean reads entries the loop has already overwritten.
 * float64 is summed in float64, float32 in float32.  Errors: n_phones > n_frames (S > T), negative durations, interpolate with
 * fewer than two voiced frames (the reference drops utterances with at most one).
 * outlier_stats: remove_outlier (:348-356) for n_utts value sets packed in `values` (n_values[u] each, at most 4096): the 25th /
 * 75th percentile by numpy's linear rule, keep[i] = (p25 - 1.5 IQR < v < p75 + 1.5 IQR) as packed bytes, and partials [n_utts][3] =
 * (count, mean, sum of squared deviations) of the kept values in float64, the sums `StandardScaler.partial_fit` forms.
 * merge_stats: partial_fit's update (:106-109; sklearn's incremental mean / variance) of state = (count, mean, M2) — zeros to
 * start — with n_partials partials in the order given; deterministic.  mean = state[1], the population std = sqrt(state[2] / state[0]).
 * normalize: :358-369 over n packed values: out [n] float64 = (values - mean) / std, minmax = (min, max) of out.  Error: std == 0. */
int mtts_stft_mel_batch(mtts_stft* h, int n_utts, const int* n_samples, const int* keep_frames, const float* wavs, float* mel, float* energy);
int mtts_stft_phoneme_average(mtts_stft* h, int n_utts, const int* n_frames, const int* n_phones, const int* durations, const void* values, int dtype,
                              int interpolate, void* out);
int mtts_stft_outlier_stats(mtts_stft* h, int n_utts, const int* n_values, const void* values, int dtype, unsigned char* keep, double* partials);
int mtts_stft_merge_stats(mtts_stft* h, double* state, int n_partials, const double* partials);
int mtts_stft_normalize(mtts_stft* h, int64_t n, const void* values, int dtype, double mean, double std, double* out, double* minmax);

/* ---- speaker-similarity evaluation: wavs -> d-vectors, similarity, centroids -----------------------------
 * Replaces the device-worthy part of the reference's `evaluation/` package (wavs_to_dvector.py: `encoder.embed_utterance(
 * preprocess_wav(path))` one wav at a time on the CPU; pair_similarity.py:68-88, centroid_similarity.py:47-118: cosine similarity;
 * wavs_to_dvector.py:176-183: centroids) and `spk_ref_mel_slices` of preprocessor/preprocessor.py:263-299.  resemblyzer is un-vendored:
 * its front-end is restated from the published recipe.  Of its `preprocess_wav`, resampling and -30 dBFS normalisation are the next
 * section's and silence trimming the one after (both opt-in; the detector there is this project's own: parity with webrtcvad is
 * UNPINNED).  In THESE entries waveforms are 16 kHz float32 as they are.
 * power_mel_batch: resemblyzer's `wav_to_mel_spectrogram` of n_utts waveforms packed in `wavs` as they are: mel [sum T][n_mel], T_u =
 * n_samples[u] / hop_length + 1, = mel_basis @ (re^2 + im^2) of the centred, reflect-padded frames (power; no clip, no log, no clamp).
 * An utterance's rows are bit-identical whatever else is in the call.  Errors (before any launch): n_samples[u] <= filter_length / 2.
 * embed_device: mtts_dvector_embed over a partial stack mels_dev [n_partials][frames][n_mels] that is ALREADY on the device (read in
 * place); utt_offsets, out, partial_out are host arrays as in embed.  The input projections name a fixed GEMM kernel: the d-vector of an
 * utterance is bit-identical alone, in any batch and under any chunking.  Synchronous.
 * embed_wavs: n_utts waveforms packed one after another in `wavs` (n_samples[u] each) -> out [n_utts][emb].  `stft` is an mtts_stft
 * handle created at filter_length 400, hop_length 160, n_mel 40 and loaded with forward_basis(400, 400, "hann") and the mel filter bank
 * of (16000, 400, 40).  Per utterance: the partial rule (windows of partial_frames mel frames every frame_step frames over
 * ceil((n + 1) / hop) frames, the last dropped when (n - its first sample) / (partial_frames * hop) < min_coverage and it is not the
 * only one; resemblyzer: partial_frames 160, frame_step round(16000 / 1.3 / 160) = 77, min_coverage 0.75), zero-extension of the
 * waveform to the last window's end, mel = mel_basis @ (re^2 + im^2) of the centred, reflect-padded frames (power, no log, no clamp),
 * the windows gathered on the device into the encoder's partial stack, then embed_device.  n_partials_out [n_utts] = windows per
 * utterance; slices_out (or NULL) = those stacks [sum n_partials][partial_frames][n_mel] — the `spk_ref_mel_slices` payload.
 * h == NULL: front-end only (slices_out required, out ignored).  All utterances of a chunk share every launch; a chunk is as many
 * consecutive utterances as fit the encoder's max_partials / max_utts; results do not depend on the chunking (bit-identical).  With the
 * two handles on different streams the stages are ordered by events.  Refused before any launch, with the reason in BOTH handles'
 * last_error: NULL pointers, n_samples[u] <= filter_length / 2, one utterance with more partials than max_partials, handles on
 * different devices, a partial shape the encoder was not created for, bases not loaded.  Synchronous.
 * cosine_indexed: sim[i] = <a, b> / (max(||a||, eps) max(||b||, eps)), a = a[index_a[i]], b = b[index_b[i]] (torch's
 * nn.CosineSimilarity(dim=1, eps)); a [n_a][dim], b [n_b][dim], n pairs; host arrays.  The reference's np.repeat expansions become
 * index arrays.  centroids: out[s] = m / ||m||_2, m = mean of vectors[offsets[s] .. offsets[s + 1]) (ragged lists, offsets [n_speakers
 * + 1] from 0; dim <= 1024).  Both accumulate in float64 in a fixed order (deterministic, no atomics) and round once. */
int mtts_stft_power_mel_batch(mtts_stft* h, int n_utts, const int* n_samples, const float* wavs, float* mel);
int mtts_dvector_embed_device(mtts_dvector* h, const float* mels_dev, int n_partials, const int* utt_offsets, int n_utts, float* out, float* partial_out);
int mtts_dvector_embed_wavs(mtts_dvector* h, mtts_stft* stft, int n_utts, const int* n_samples, const float* wavs, int partial_frames, int frame_step,
                            double min_coverage, float* out, int* n_partials_out, float* slices_out);
int mtts_dvector_cosine_indexed(mtts_dvector* h, const float* a, int n_a, const float* b, int n_b, int dim, int n, const int* index_a, const int* index_b,
                                double eps, float* sim);
int mtts_dvector_centroids(mtts_dvector* h, const float* vectors, const int* offsets, int n_speakers, int dim, float* out);

/* ---- rate conversion and volume normalisation of waveform batches ----------------------------------------
 * The stage in front of the packed waveform buffer of an mtts_stft handle: what `librosa.load(path, sampling_rate)` does in the
 * reference's corpus loaders (preprocessor/libritts.py:37, vctk.py:35, preprocessor.py:205) and the first two steps of resemblyzer's
 * `preprocess_wav` (evaluation/wavs_to_dvector.py:206-296, preprocessor.py:265).  Opt-in: a handle without a resampler behaves as before.
 * Neither library is vendored; parity with them is UNPINNED.  What is computed, exactly: with up / down = target_sr / orig_sr reduced,
 *   y[n] = sum_m h[n * down - m * up] x[m]   over |n * down - m * up| <= H, 0 <= m < n_in,   n_out = ceil(n_in * up / down),
 * for a filter h[-H .. H] on the grid of the up-sampled rate (designed by the caller in float64: meta_tts_amd/audio/resample.py builds
 * the Kaiser-windowed sinc, sum(h) = up, and equals scipy.signal.resample_poly with that window).  Silence trimming: the section after next.
 * load_resampler: the filter as a polyphase bank, float32 [taps][up], rounded once from float64:
 *   bank[t][p] = h[((p * down) mod up) + (t - lead) * up]   (0 where that index falls outside -H .. H),
 * so that y[n] = sum_t bank[t][n mod up] * x[floor(n * down / up) + lead - t], added in tap order in float32 (FMA).  With K =
 * floor(H / up): lead = K + 1, taps = 2 K + 2 covers every phase.  Column p = n mod up is the fastest index: consecutive outputs read
 * consecutive addresses.  Replaces a bank loaded before.  Errors: up, down, taps < 1, lead outside 0 .. taps - 1, a bank above 2^22
 * entries, a ratio so steep that the input span of 256 outputs (255 * down / up + taps + 1 samples) exceeds the 4096 a workgroup stages.
 * resample_batch: n_utts waveforms packed one after another in `wavs` (n_in[u] source-rate samples each; host) -> out, the resampled
 * waveforms packed one after another (ceil(n_in[u] * up / down) each; host).  target_dbfs: NaN = no normalisation; else resemblyzer's
 * normalize_volume(y, target_dbfs, increase_only) per utterance on the RESAMPLED signal: dBFS = 10 log10(mean(y^2)), change =
 * target_dbfs - dBFS; left as it is when change < 0 and increase_only != 0 (and when y is all zeros), else y *= 10^(change / 20), the
 * float64 product rounded once.  gains (or NULL): float64 [n_utts], the gain applied (1 where left as it is).  mean(y^2) is a float64
 * sum in a fixed order (one partial per 256-thread workgroup, then in workgroup order): no atomics.  An utterance's output and gain
 * are bit-identical alone, in any batch, at any position.  Errors, before any launch: no resampler loaded, n_utts < 1 or > 65535, NULL
 * pointers, n_in[u] < 1, a resampled length beyond the handle's max_samples.  Synchronous.
 * embed_wavs_resampled: mtts_dvector_embed_wavs with n_samples[u] counted at the SOURCE rate: every chunk's waveforms are uploaded at
 * the source rate, resampled (and normalised, target_dbfs / increase_only as above) on the device straight into the packed waveform
 * buffer, zero-extended there, and go through the same chain (pad, STFT, power mel, gather, encoder); the front-end-rate signal never
 * visits the host.  The partial rule applies to the resampled length; results are bit-identical to embed_wavs on resample_batch's
 * output.  Errors: those of both entries, under this entry's name. */
int mtts_stft_load_resampler(mtts_stft* h, int up, int down, int taps, int lead, const float* bank);
int mtts_stft_resample_batch(mtts_stft* h, int n_utts, const int* n_in, const float* wavs, double target_dbfs, int increase_only, float* out, double* gains);
int mtts_dvector_embed_wavs_resampled(mtts_dvector* h, mtts_stft* stft, int n_utts, const int* n_samples, const float* wavs, int partial_frames, int frame_step,
                                      double min_coverage, double target_dbfs, int increase_only, float* out, int* n_partials_out, float* slices_out);

/* ---- fundamental frequency of waveform batches --------------------------------------------------------------
 * The pitch feature of the preprocessing stage, on the packed waveform buffer of an mtts_stft handle.  The reference calls pyworld's
 * DIO + StoneMask (preprocessor/preprocessor.py:214-220); pyworld is not vendored and NOT restated: parity with it is UNPINNED.  What is
 * computed is YIN (de Cheveigne & Kawahara 2002) on DIO's frame grid.  Opt-in: a handle without a pitch configuration behaves as before.
 * load_pitch: tau_max = ceil(sampling_rate / f0_floor), tau_min = floor(sampling_rate / f0_ceil), W = the smallest multiple of 64 that
 * is >= 1.5 tau_max (512 at 22 050 Hz and 71 Hz), L = W + tau_max; the hop is the handle's hop_length.  Replaces a configuration loaded
 * before.  Errors: f0_ceil <= f0_floor, tau_min < 2, fewer than two lags in [tau_min, tau_max), non-finite or non-positive arguments
 * (silence_rms may be 0), a frame span W + tau_max beyond what a workgroup stages in LDS (about 4700 samples).
 * f0_batch: n_utts waveforms packed one after another in `wavs` (float32, n_samples[u] each; host) -> f0 (float64) and aperiodicity
 * (float32, or NULL), packed one after another, T_u = n_samples[u] / hop_length + 1 values per utterance (mel_batch's and DIO's frame
 * count).  Frame t reads s = x[t hop - L / 2 .. + L), zeros outside its utterance (never a neighbouring utterance's samples):
 *   d(tau)  = sum_{j < W} (s[j] - s[j + tau])^2 for tau = 0 .. tau_max, float32 FMAs in ascending j;
 *   d'(0) = 1, d'(tau) = d(tau) tau / sum_{k = 1 .. tau} d(k) in float32 (1 where the running sum is 0);
 *   f0 = 0 if mean(s[0 : W]^2) < silence_rms^2, or if no tau in [tau_min, tau_max) has d'(tau) < threshold; else tau = the smallest
 *   such lag, moved forward while d'(tau + 1) < d'(tau) (within the range), and f0 = sampling_rate / (tau + off), off = 0.5 (y0 - y2) /
 *   (y0 - 2 y1 + y2) over y = d'(tau - 1 .. tau + 1) in float64 (0 when the denominator is 0, and at tau = tau_min or tau_max - 1).
 *   aperiodicity = the chosen d'(tau), 1 for an unvoiced frame.
 * A frame's values depend on its utterance's samples and the configuration only: bit-identical alone, in any batch, at any position.
 * Returns the total number of frames, < 0 on error.  Errors, before any launch: no configuration loaded, n_utts < 1 or > 65535, NULL
 * n_samples / wavs / f0, n_samples[u] < 1 or beyond the handle's max_samples.  Synchronous. */
int mtts_stft_load_pitch(mtts_stft* h, int sampling_rate, double f0_floor, double f0_ceil, double threshold, double silence_rms);
int64_t mtts_stft_f0_batch(mtts_stft* h, int n_utts, const int* n_samples, const float* wavs, double* f0, float* aperiodicity);

/* ---- silence trimming of waveform batches: the last step of `preprocess_wav` -----------------------------------
 * resemblyzer's `trim_long_silences` asks webrtcvad for a voiced / unvoiced decision per 30 ms window and post-processes the flags.
 * webrtcvad's GMM decision is third party and NOT restated: parity with it is UNPINNED.  Everything around that decision is restated
 * exactly, and a caller who owns webrtcvad injects its decisions through flags_in.  Opt-in: a handle without a VAD configuration
 * behaves as before and allocates nothing for this stage.
 * load_vad: resemblyzer's values are sampling_rate 16000, window_ms 30, ma_width 8, max_silence 6.  floor_db, noise_quantile and
 * margin_db (the Python layer: -50, 0.1, 10) are this project's choice and have not been tuned against webrtcvad.  Replaces a
 * configuration loaded before.  Errors: sampling_rate or window_ms < 1, window_ms * sampling_rate not a multiple of 1000, ma_width or
 * max_silence outside 1 .. 64, noise_quantile outside [0, 1], non-finite thresholds.
 * Per utterance of n samples:
 *   1. windows: W = window_ms * sampling_rate / 1000 (480), n_w = floor(n / W); the last n mod W samples are dropped.
 *   2. e[w] = mean of x^2 over window w: every product float32 x float32 held exactly in float64, the sum in float64 in a fixed order
 *      (a lane's samples w W + lane, + 64, ... ascending, then a fixed tree over the 64 lanes); no atomics.
 *   3. noise = the k-th smallest e[w] of this utterance, k = floor(noise_quantile * (n_w - 1)): an order statistic, no interpolation.
 *   4. raw[w] = (e[w] >= max(10^(floor_db / 10), noise * 10^(margin_db / 10))).  With flags_in (one byte per window, packed over the
 *      utterances, nonzero = voiced) steps 2 to 4 are skipped and raw = flags_in.
 *   5. moving average of width ma_width over raw, zero padded by (ma_width - 1) / 2 on the left and ma_width / 2 on the right, rounded
 *      half to even to bool: smooth[w] = (2 * count > ma_width).  At width 8: at least 5 of raw[w - 3 .. w + 4]; 4 of 8 round to 0.
 *   6. binary dilation by a centred structure of max_silence + 1 ones: mask[w] = any of smooth[w - max_silence / 2 .. w + (max_silence
 *      + 1) / 2] (w - 3 .. w + 3 at max_silence 6).
 *   7. out = the samples of the kept windows in order, n_out = W * (kept windows).  When the mask keeps no window (n < W, digital
 *      silence) the utterance passes through AS IT IS, all n samples with the tail, and n_voiced_out = 0 reports it (resemblyzer would
 *      hand an empty array to the next stage).
 * An utterance's result depends on its samples and the configuration only: bit-identical alone, in any batch, at any position.
 * trim_batch: n_utts waveforms packed one after another in `wavs` (n_samples[u] each; host) -> out, the trimmed ones packed one after
 * another (room for sum n_samples), n_out [n_utts]; optional: n_voiced_out [n_utts] kept windows, mask_out [sum n_w] bytes, energy_out
 * [sum n_w] float64 (not written when flags_in is given).  Returns the total number of output samples, < 0 on error.
 * embed_wavs_preprocessed: all of `preprocess_wav` chained in front of mtts_dvector_embed_wavs: every chunk's waveforms are resampled
 * when a resampler is loaded (n_samples[u] then counts SOURCE-rate samples) and normalised (target_dbfs, increase_only as in
 * resample_batch; NaN: not; without a resampler target_dbfs must be NaN), trimmed, and compacted into the packed waveform buffer over
 * zeros; then the pad / STFT / power mel / gather / encoder chain.  The front-end-rate signal never visits the host.  The partial rule
 * applies to the TRIMMED length: n_partials_out and slices_out count the trimmed utterances' partials, n_trimmed_out [n_utts] (or NULL)
 * the trimmed lengths.  Chunks are planned from the untrimmed lengths (trimming only shortens, so every capacity check holds before
 * any launch); the host reads a chunk's trimmed lengths back once.  Results are bit-identical under any chunking, and to embed_wavs on
 * trim_batch's output of resample_batch's output.  The VAD window must be longer than filter_length / 2.
 * Errors of both entries, before any launch (the chained entry: in both handles' last_error, with those of embed_wavs_resampled): no
 * VAD configuration loaded, NULL pointers, n_utts < 1 or > 65535, n_samples[u] < 1 or (at the detector's rate) beyond max_samples, more
 * than 4096 windows in one utterance.  Synchronous, on the handle's stream. */
int mtts_stft_load_vad(mtts_stft* h, int sampling_rate, int window_ms, int ma_width, int max_silence, double floor_db, double noise_quantile,
                       double margin_db);
int64_t mtts_stft_trim_batch(mtts_stft* h, int n_utts, const int* n_samples, const float* wavs, const unsigned char* flags_in, float* out, int* n_out,
                             int* n_voiced_out, unsigned char* mask_out, double* energy_out);
int mtts_dvector_embed_wavs_preprocessed(mtts_dvector* h, mtts_stft* stft, int n_utts, const int* n_samples, const float* wavs, int partial_frames,
                                         int frame_step, double min_coverage, double target_dbfs, int increase_only, float* out, int* n_partials_out,
                                         float* slices_out, int* n_trimmed_out);

/* ---- waveform sources of the d-vector chain (csrc/wavsource.h) -----------------------------------------------------
 * embed_wavs_source: the three entries above behind one signature, with the place the n_utts waveforms live as an argument.
 *   MTTS_WAV_HOST_F32    data = host float32, packed one after another: exactly the three entries above (same code path, same launches).
 *   MTTS_WAV_HOST_PCM16  data = host int16, packed one after another.  Every chunk's raw samples are uploaded at 2 bytes per sample and
 *                        widened on the device, x = v / 32768 — exact in float32, so the results equal those of the float32 source
 *                        holding int16 / 32768 bit for bit.
 *   MTTS_WAV_DEVICE_F32  data = device float32, utterance u at data + u * row_stride (floats), n_samples[u] <= row_stride; what lies
 *                        beyond n_samples[u] in a row is never read.  producer_stream: the HIP stream whose work fills `data`; the
 *                        front-end's stream waits for an event recorded on it when the call starts (no host synchronisation), and the
 *                        rows may be reused once the call has returned.  quantize_scale s > 0: every sample goes through a 16-bit
 *                        file's round trip first, q = trunc(x * s) clamped to [-32768, 32767], x' = q / 32768 (s = max_wav_value, 32768
 *                        in the reference configs; |x * s| >= 32768 is outside the contract, the clamp only keeps the result defined);
 *                        0: the floats as they are.  row_stride, producer_stream and quantize_scale are ignored (and quantize_scale
 *                        must be 0) for the host kinds.
 * stages: bit 0 = resample (+ normalise to target_dbfs unless NaN) as embed_wavs_resampled does, bit 1 = trim as embed_wavs_preprocessed
 * does (through the resampler when one is loaded); 0 = the plain chain, where target_dbfs and increase_only are ignored.  n_samples,
 * the partial rule and the outputs are those of the entry with the same stages; n_trimmed_out is written with bit 1 only.
 * Errors, before any launch and in both handles' last_error, besides those of the entry with the same stages: NULL source or data,
 * unknown kind or stages, row_stride smaller than a length, negative quantize_scale, quantize_scale on a host source. */
enum { MTTS_WAV_HOST_F32 = 0, MTTS_WAV_HOST_PCM16 = 1, MTTS_WAV_DEVICE_F32 = 2 };
typedef struct mtts_wav_source {
    int kind;
    const void* data;
    int64_t row_stride;
    void* producer_stream;
    float quantize_scale;
} mtts_wav_source;
int mtts_dvector_embed_wavs_source(mtts_dvector* h, mtts_stft* stft, const mtts_wav_source* src, int stages, int n_utts, const int* n_samples,
                                   int partial_frames, int frame_step, double min_coverage, double target_dbfs, int increase_only, float* out,
                                   int* n_partials_out, float* slices_out, int* n_trimmed_out);

/* ---- exact t-SNE of d-vectors: the numerical step of evaluation/visualize.py ------------------------------------
 * The reference calls sklearn's TSNE(n_components=2, perplexity=40, n_iter=300), Barnes-Hut on the CPU.  This handle runs sklearn's
 * method="exact" definition (sklearn 1.7: _binary_search_perplexity, _joint_probabilities, _kl_divergence, _gradient_descent) on the
 * device: n^2 pair terms per iteration.  Two components only, squared Euclidean distances only.  All array arguments are host memory.
 * create: room for max_points points of max_dim features.  The dense joint P is max_points^2 x 4 bytes of device memory (298 MB at
 * 8 640 points); max_points is capped at 12 288 (604 MB; a row of distances must also fit a workgroup's LDS) and refused beyond,
 * as is max_points < 2 or max_dim outside 1 .. 65 536.  Every other entry refuses, with a message in last_error and before any launch:
 * a NULL handle or required pointer, n < 2, n > max_points, non-finite input.
 * affinities: X [n][dim] float32 -> the joint P on the handle; optional P_out [n][n] float32, beta_out [n] float64.
 *   D[i][j] = sum_k (x_ik - x_jk)^2 in float64 (ascending k), rounded once to float32 as sklearn rounds its distances: symmetric bit for
 *   bit, exact zero diagonal.  Per row the binary search of _binary_search_perplexity (beta from 1, at most 100 steps, tolerance
 *   float(1e-5) on H - log(perplexity), double then bisect, a row sum of 0 replaced by float(1e-8), j = i excluded), float64 in a fixed
 *   order; the conditional row is stored as float32 and beta_out is the beta it was evaluated at.  P = max((C + C^T) / max(sum, eps),
 *   eps), eps = 2^-52, diagonal 0, stored as float32, symmetric bit for bit.  Also refused: dim outside 1 .. max_dim, perplexity not
 *   in (0, n).  Forgets the descent state.
 * set_affinities: the caller's own P [n][n] float32 (finite, non-negative; taken as it is: not normalised, not symmetrised).
 *   Forgets the descent state.
 * set_state / get_state: Y, update, gains, each [n][2] float32.  set: update NULL = zeros, gains NULL = ones.  get: NULL = not wanted.
 * gradient: at the current state, without stepping: grad_out [n][2] = 4 sum_j (exaggeration P_ij - Q_ij) num_ij (y_i - y_j), num_ij =
 *   1 / (1 + |y_i - y_j|^2), Q_ij = max(num_ij / Z, eps), Z = sum_{i != j} num_ij; kl_out (or NULL) = sum_{i != j} P' log(max(P', eps)
 *   / Q), P' = exaggeration P: sklearn's _kl_divergence on the P it is handed (it is handed exaggeration P during its first phase).
 *   The pair sums are float32 in a fixed order (lane = j mod 64 ascending, 4 groups of 16 lanes, the 4 group sums), Z is folded in
 *   float64 in row order, KL is float64 throughout.  Q's floor inside the gradient: the sweep records each row's smallest num, and a
 *   row with min num < eps Z recomputes its repulsive sum with the floor applied pair by pair.
 * run: n_iter iterations of _gradient_descent's rule with no host synchronisation between them (one at the end): inc = update grad
 *   < 0; gains += 0.2 on inc, x 0.8 elsewhere, floored at min_gain; grad x= gains; update = momentum update - learning_rate grad;
 *   Y += update, in float32.  kl_out (or NULL): the KL of the state the LAST iteration started from (sklearn's `error`);
 *   grad_norm_out (or NULL): the 2-norm of the last iteration's grad x gains (what sklearn compares with min_grad_norm).  Also
 *   refused: n_iter < 1, exaggeration or learning_rate not positive, momentum or min_gain negative.
 * Every result is bit-identical from call to call (no atomics); run(a + b) equals run(a) then run(b). */
typedef struct mtts_tsne mtts_tsne;
int mtts_tsne_create(int max_points, int max_dim, int device, mtts_tsne** out);
void mtts_tsne_destroy(mtts_tsne* h);
const char* mtts_tsne_last_error(mtts_tsne* h);
int mtts_tsne_set_stream(mtts_tsne* h, void* hip_stream);
int mtts_tsne_affinities(mtts_tsne* h, const float* X, int n, int dim, double perplexity, float* P_out, double* beta_out);
int mtts_tsne_set_affinities(mtts_tsne* h, const float* P, int n);
int mtts_tsne_set_state(mtts_tsne* h, const float* Y, const float* update, const float* gains);
int mtts_tsne_get_state(mtts_tsne* h, float* Y, float* update, float* gains);
int mtts_tsne_gradient(mtts_tsne* h, double exaggeration, float* grad_out, double* kl_out);
int mtts_tsne_run(mtts_tsne* h, int n_iter, double exaggeration, double momentum, double learning_rate, double min_gain, double* kl_out,
                  double* grad_norm_out);

/* ---- mel-cepstral distortion along a DTW path, with F0 figures on the same path (csrc/dtw.h) ---------------------
 * Scores whether two utterances of different length SAY the same thing: a synthesis (on predicted durations) against its recording.  The
 * reference has no such step; this is the project's own definition, and parity with SPTK / WORLD mel-cepstra is UNPINNED.
 *   cepstra   for a natural-log mel frame m[0 .. n_mel) (what TacotronSTFT produces): c_k = sum_n B[k][n] m[n], k = 1 .. K.  B = rows 1 .. K
 *             of the orthonormal DCT-II (scipy.fft.dct(type=2, norm="ortho"); c_0 dropped), designed on the host in float64 and loaded
 *             as float64 [K][n_mel].  The sum is float64 in ascending n.  1 <= K <= 34, K < n_mel <= 128.
 *   distance  d(i, j) = sqrt(sum_k (a_ik - b_jk)^2), float64 in ascending k.
 *   DTW       D(0, 0) = d(0, 0); D(i, j) = d(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)), unit weights, ties to the first in that order,
 *             no band and no slope constraint.  The path runs back from (Ta-1, Tb-1) to (0, 0); L = its number of cells.
 *   MCD       (10 sqrt(2) / ln 10) D(Ta-1, Tb-1) / L, in dB.
 *   F0        both tracks or neither; float64, one value per mel frame, 0 = unvoiced (as mtts_stft_f0_batch returns them).  Along the
 *             path, summed in the order of the walk back (from (Ta-1, Tb-1) to (0, 0)): the number of cells with both frames voiced, the
 *             RMSE of 1200 log2(fa / fb) over those cells in cents (NaN when there is none), the number of cells with exactly one side voiced.
 * create: n_coef = K; max_frames <= 2048 bounds either side of a pair (three float64 diagonals of the sweep live in a workgroup's LDS);
 *   max_cells <= 2^33 bounds sum Ta Tb of one chunk — the direction map, one byte per cell in a workspace the handle owns and grows on
 *   demand, is the only Ta x Tb object; max_pairs <= 2^20 bounds the pairs of one chunk.
 * cepstra: n_utts <= 2 max_pairs utterances of 1 <= n_frames[u] <= max_frames frames (refused by name otherwise, before any launch), log_mel
 *   packed [sum T][n_mel] host float32 -> cep_out [sum T][K] host float64.
 * mcd_batch: pair p aligns frames_a[p] rows of mel_a with frames_b[p] rows of mel_b (both packed [sum T][n_mel] host float32, pairs one
 *   after another).  f0_a / f0_b (packed [sum T] host float64) may both be NULL; when given, f0_frames_a / f0_frames_b hold each track's
 *   own length and must equal frames_a / frames_b.  out [n_pairs][6] float64: D(Ta-1, Tb-1), L, MCD, n_voiced_both, cents RMSE,
 *   n_vuv_mismatch; columns 3 .. 5 are NaN without F0.  path_len [n_pairs] (or NULL) = L.  path (or NULL): pair p owns the (Ta + Tb - 1)
 *   (i, j) int pairs that follow those of the pairs before it; its first L hold the path from (0, 0) forward, the rest -1.
 *   The call is a plan: validate; cut the pairs, in order, into chunks of sum Ta Tb <= max_cells and at most max_pairs pairs; reserve
 *   every buffer for the largest chunk; run chunk by chunk.  A pair's out row and path are bit-identical alone, in any batch, at any
 *   position and under any chunking.  Synchronous.
 * Refused with < 0, the reason (naming the pair and the limit) in last_error, before any launch, the handle staying usable: no basis
 *   loaded; a frame count < 1 or > max_frames; Ta Tb > max_cells; an F0 track on one side only; an F0 length that differs from the frame
 *   count; non-finite mel values; negative or non-finite F0; NULL required pointers. */
typedef struct mtts_dtw mtts_dtw;
int mtts_dtw_create(int n_mel, int n_coef, int max_frames, int64_t max_cells, int max_pairs, int device, mtts_dtw** out);
void mtts_dtw_destroy(mtts_dtw* h);
const char* mtts_dtw_last_error(mtts_dtw* h);
int mtts_dtw_set_stream(mtts_dtw* h, void* hip_stream);
int mtts_dtw_load_basis(mtts_dtw* h, const double* basis);
int mtts_dtw_cepstra(mtts_dtw* h, int n_utts, const int* n_frames, const float* log_mel, double* cep_out);
int mtts_dtw_mcd_batch(mtts_dtw* h, int n_pairs, const int* frames_a, const float* mel_a, const int* frames_b, const float* mel_b, const int* f0_frames_a,
                       const double* f0_a, const int* f0_frames_b, const double* f0_b, double* out, int* path_len, int* path);

/* ---- forced alignment: flat-start monophone EM, Viterbi to durations (csrc/align.h) -----------------------------
 * Phoneme durations from features and phone sequences, so that a corpus without third-party TextGrids gets past preprocessing.  The
 * classical first pass of an HMM forced aligner and no more: one diagonal Gaussian per phone class, Baum-Welch re-estimation in closed
 * form, Viterbi to durations; no network, no optimiser.  The definition is this project's own, restated in float64 numpy by
 * tests/align_oracle.py.  Parity with MFA, Kaldi and HTK is UNPINNED, and alignment quality on real speech is not measured.
 *   features  x[t][f] float32, t < T, f < F = n_feat, 1 <= F <= 128; any packed [sum T][F] rows (the Python layer feeds natural-log mels).
 *   model     V = n_classes phone classes, 1 <= V <= 512, each a float64 mean mu[v][f] and variance var[v][f] > 0; beside them the
 *             flat-start variance g[f] > 0 of every feature (global_var), which scales the variance floor.
 *   utterance S states, 1 <= S <= max_states <= 2048; state s has a class c[s] and a flag opt[s] (1: the state may be skipped, e.g. a
 *             silence between words).  Two adjacent optional states are refused, and so are more mandatory states than frames.
 *   emission  b(t, s) = -1/2 sum_f [ (x[t][f] - mu[c][f])^2 (1 / var[c][f]) + log(2 pi var[c][f]) ], c = c[s]; float64, the reciprocal rounded
 *             once, the bracket added in ascending f.
 *   lattice   left to right, every allowed transition of weight 1 (no transition probabilities): into (t, s) come (t-1, s) stay,
 *             (t-1, s-1) advance and, only if opt[s-1], (t-1, s-2) skip.  A path starts at t = 0 in state 0, or in state 1 if opt[0]; it
 *             ends at t = T-1 in state S-1, or in state S-2 if opt[S-1].
 *   forward   alpha(t, s) = b(t, s) + logsumexp(stay, advance, skip) in that order; logsumexp = m + log(sum exp(. - m)), m the largest
 *             term (a missing predecessor is -inf; all -inf gives -inf).  LL = logsumexp(alpha(T-1, S-1), alpha(T-1, S-2)).  beta is the
 *             mirror image (beta(T-1, end) = 0; successors stay, advance, skip, each with its emission at t+1 added first);
 *             gamma(t, s) = exp((alpha + beta) - LL).
 *   Viterbi   the same recursion with max; ties go to stay, then advance, then skip; among the end states ties go to S-1.  dur[s] = the
 *             frames the path spends in state s (0 for a skipped optional state); sum dur = T.
 *   flat start  every class gets the mean and variance (two passes, float64, rows in call order) of all frames of the call; g = that variance.
 *   EM        em_begin; any number of em_accumulate(batch); em_finish.  accumulate adds per class occ = sum gamma, sum gamma x and
 *             sum gamma x^2 over the batch's states of that class: per state in ascending t, then one utterance's per-class sum (its
 *             states in ascending s, from zero) after another's, in call order.  finish sets mu = sum gamma x / occ and
 *             var = max(sum gamma x^2 / occ - mu^2, var_floor g[f]) (var_floor 0.01 by default); a class with occ < min_occ (default 1e-3)
 *             keeps its parameters; it returns sum LL of the iteration's utterances, added in call order.
 * create: max_frames <= 2^20, max_states <= 2048 (two float64 rows of the sweep live in a workgroup's LDS), max_cells <= 2^30 bounds
 *   sum T S of one chunk (the alpha / gamma workspace, float64 per cell, and the back-pointers, a byte per cell, which the handle owns
 *   and grows on demand), max_utts <= 65535 the utterances of one chunk.
 * Batches: n_frames [n_utts], n_states [n_utts], classes [sum S] int32, optional [sum S] bytes, x [sum T][F] host float32, utterances one
 *   after another.  A call is a plan: validate; cut the utterances, in order, into chunks of sum T S <= max_cells and at most max_utts;
 *   reserve every buffer for the largest chunk; run chunk by chunk.  Synchronous.
 *   em_accumulate: ll_out [n_utts]; a refusal leaves the open iteration as it was, a runtime failure after the call's first launch closes it
 *   (its sums may hold part of the call; start again with em_begin).  em_finish: total_ll_out [1].  posteriors: ll_out [n_utts], gamma_out packed [sum T S], utterance u's
 *   block row-major [T][S].  align: durations_out [sum S] int32, score_out [n_utts] = the Viterbi path's log-likelihood.
 *   set_model / get_model: mean and var [V][F], global_var [F], host float64.
 * No atomics and no wavefront intrinsics; every reduction is an ascending loop.  An utterance's LL, gamma and durations are bit-identical
 *   alone, in any batch, at any position and under any chunking; the model after em_finish is bit-identical for any max_cells and for
 *   any cut of the corpus into em_accumulate calls.
 * Refused with < 0, the reason (naming the utterance and the limit) in last_error, before any launch, the handle staying usable: T < 1 or
 *   > max_frames; S < 1 or > max_states; T S > max_cells; more mandatory states than frames; adjacent optional states; a class id outside
 *   0 .. V-1; non-finite features; var <= 0 or non-finite model values; em_accumulate or em_finish without em_begin; no model loaded; NULL
 *   required pointers; a feature that is constant over all frames of flat_start. */
typedef struct mtts_align mtts_align;
int mtts_align_create(int n_feat, int n_classes, int max_frames, int max_states, int64_t max_cells, int max_utts, int device, mtts_align** out);
void mtts_align_destroy(mtts_align* h);
const char* mtts_align_last_error(mtts_align* h);
int mtts_align_set_stream(mtts_align* h, void* hip_stream);
int mtts_align_set_model(mtts_align* h, const double* mean, const double* var, const double* global_var);
int mtts_align_get_model(mtts_align* h, double* mean, double* var, double* global_var);
int mtts_align_set_floor(mtts_align* h, double var_floor, double min_occ);
int mtts_align_flat_start(mtts_align* h, int n_utts, const int* n_frames, const float* x);
int mtts_align_em_begin(mtts_align* h);
int mtts_align_em_accumulate(mtts_align* h, int n_utts, const int* n_frames, const int* n_states, const int* classes, const unsigned char* optional, const float* x,
                             double* ll_out);
int mtts_align_em_finish(mtts_align* h, double* total_ll_out);
int mtts_align_posteriors(mtts_align* h, int n_utts, const int* n_frames, const int* n_states, const int* classes, const unsigned char* optional, const float* x,
                          double* ll_out, double* gamma_out);
int mtts_align_align(mtts_align* h, int n_utts, const int* n_frames, const int* n_states, const int* classes, const unsigned char* optional, const float* x,
                     int* durations_out, double* score_out);

/* ---- MOSNet: magnitude spectrograms / waveforms -> naturalness scores -------------------------------
 * Stands behind evaluation/compute_mos.py (NeuralMOS.compute_mosnet, speechmetrics' MOSNet on one wav at a time).  Neither speechmetrics,
 * its TensorFlow model nor cnn_blstm.h5 is part of the reference tree: parity with the published weights is UNPINNED, and so are the
 * analysis window (a symmetric Hamming window, which lives in the forward basis the caller loads) and the recurrent activation (sigmoid,
 * tf.keras 2's default); what is pinned is this definition — the published CNN-BLSTM MOSNet (Lo et al. 2019) in inference mode —
 * restated in torch by tests/mosnet_oracle.py:
 *   input     per utterance a magnitude spectrogram [T][n_freq]: |STFT| at 16 kHz, n_fft = 2 (n_freq - 1) = 512, hop 256, window length
 *             n_fft, centred with reflection padding; T = n / 256 + 1.
 *   conv      four blocks of C = 16, 32, 64, 128: Conv2d(C_prev -> C), Conv2d(C -> C), Conv2d(C -> C), 3x3 kernels (time x frequency),
 *             bias + ReLU each, C_prev of the first = 1; the third of a block has stride (1, 3).  Padding is TensorFlow's "same": in time one
 *             zero row before and after the utterance's OWN first and last frame (a ragged batch equals its utterances scored alone); in
 *             frequency one zero column each side at stride 1, and at stride 3, F_in -> F_out = ceil(F_in / 3), total = max((F_out - 1) 3 +
 *             3 - F_in, 0), left = total / 2 (floor), right = total - left.  n_freq = 257: widths 257 -> 86 -> 29 -> 10 -> 4, left 0, 0, 0, 1.
 *   features  [F4 * 128] per frame, frequency-major then channel (Keras' Reshape((-1, 4 * 128)) of a channels-last tensor).
 *   BLSTM     128 units per direction, gate order i, f, g, o, sigmoid recurrent activation, tanh elsewhere, zero initial state; the
 *             backward direction starts at the utterance's own last frame; outputs concatenated [forward | backward] = 256.
 *   head      Dense(256 -> 128) + ReLU, Dense(128 -> 1) = the frame score; the utterance score is the mean of its own T frame scores.
 * create: n_freq is a parameter (tests use narrow spectra; the channel counts stay the published four and the BLSTM input is 128 F4);
 *   max_frames_per_call bounds sum T of one call (the activations are [sum T][n_freq][16] floats, twice), max_utts <= 65535 its utterances.
 * Tensors (device images, packed by meta_tts_amd/mosnet.py from torch-layout weights):
 *   conv.0.w [9][16] (tap = 3 dt + df), conv.{l}.w [9][cin / 8][cout][8] (input channel 8 q + e at [tap][q][n][e]), conv.{l}.b [cout];
 *   blstm.w_ih [2][512][128 F4] and blstm.b [2][512] (forward, then backward), blstm.w_hh [2][32][512][4] (hidden unit 4 k + e of gate
 *   column g at [dir][k][g][e]);  dense.w [128][256], dense.b [128];  frame_score.w [128], frame_score.b [1].
 * score: mag [sum T][n_freq] host float32, utterances one after another -> utt_scores [n_utts], frame_scores [sum T] (or NULL).
 * score_wavs: waveforms (host float32, one after another, n_samples[u] each) through `front` — pack, upload, reflect pad, forward STFT,
 *   magnitude — and, with resampled != 0, behind the resampler loaded on `front` (n_samples then counts source-rate samples; no volume
 *   normalisation); the network reads the front-end's magnitudes where they lie, neither the 16 kHz signal nor the magnitudes visit the
 *   host.  n_frames_out [n_utts] = each utterance's T.  `front` must have filter_length 2 (n_freq - 1) and a forward basis loaded; the
 *   whole chain runs on front's stream.
 * An utterance's scores are bit-identical alone, in any batch and at any position.  Both entries are synchronous.  Refused with < 0,
 *   the reason in last_error, before any launch, the handle staying usable: NULL required pointers; a tensor that has not been loaded;
 *   n_utts < 1, > max_utts or > 65535; T < 1; sum T > max_frames_per_call (cutting a list into calls is the caller's job); non-finite
 *   magnitudes (score only); a front of another filter length or without a basis; no resampler loaded although resampled; a waveform
 *   too short for the reflection padding or longer than front's max_samples.  load refuses an unknown name and a wrong numel. */
typedef struct mtts_mosnet mtts_mosnet;
int mtts_mosnet_create(int n_freq, int max_frames_per_call, int max_utts, int device, mtts_mosnet** out);
void mtts_mosnet_destroy(mtts_mosnet* h);
const char* mtts_mosnet_last_error(mtts_mosnet* h);
int mtts_mosnet_set_stream(mtts_mosnet* h, void* hip_stream);
int mtts_mosnet_param_count(mtts_mosnet* h);
int mtts_mosnet_param_info(mtts_mosnet* h, int index, char* name, int name_cap, int64_t* numel);
int mtts_mosnet_load(mtts_mosnet* h, const char* name, const float* data, int64_t numel);
int mtts_mosnet_score(mtts_mosnet* h, int n_utts, const int* n_frames, const float* mag, float* utt_scores, float* frame_scores);
int mtts_mosnet_score_wavs(mtts_mosnet* h, mtts_stft* front, int n_utts, const int* n_samples, const float* wavs, int resampled, float* utt_scores,
                           int* n_frames_out, float* frame_scores);

#ifdef __cplusplus
}
#endif
#endif /* MTTS_H */
