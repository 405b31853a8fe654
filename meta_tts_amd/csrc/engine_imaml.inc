// iMAML (included inside class Engine): proximal inner loop + conjugate-gradient hypergradient.
//
// Reference: lightning/systems/imaml.py:41-46 (bias_reg_f), :50-73 (regularised adapt), :76-139 (meta_learn: CG, per-task clip,
// reduce, optimizer step) and lightning/systems/utils.py:120-189 (CG over `hypergrad`, an empty submodule in the reference tree:
// the recurrence below is the published conjugate-gradient of that package restated — parity unpinned at that dependency).
//
// With the fixed-point map of one regularised SGD step  Phi(w, theta) = w - a * grad_w [ L_s(w) + (lambda/2) |theta_a - w|^2 ]:
//     (I - dPhi/dw)^T v = a (H_s(w) + lambda I) v = grad_w L_q(w)         K CG iterations from v = 0  (utils.py:160-176)
//     d/d theta_a = (dPhi/d theta)^T v + dL_q/d theta = a * lambda * v    (the outer loss does not see theta_a directly)
// Only the adapted parameters receive a hypergradient (utils.py:147-150 builds `hparams` from the learner's names).  Every
// Hessian-vector product is the forward-over-reverse product of engine_so.inc on the batch CURRENTLY in slot 0, so the host
// layer can feed a fresh support mini-batch per application (`imaml.stochastic: true`, imaml.py:88-91).  All CG scalars stay
// on the device (one set per task: the tasks of a meta-batch are independent systems solved in the same launches).
float *im_x = nullptr, *im_r = nullptr, *im_scal = nullptr, *im_partial = nullptr;
bool im_ready = false;
float inner_prox = 0.f;  // lambda of the proximal term in the inner loop (0 = plain MAML)
static constexpr int kImBlocks = 256;
enum { IM_RS = 0, IM_PAP, IM_ALPHA, IM_BETA, IM_RSNEW, IM_ACTIVE, IM_NORM, IM_COEF, IM_STRIDE = 8 };

int enable_imaml() {
    if (im_ready) return 0;
    if (enable_second_order(1)) return -1;
    if (n_adapt <= 0) { set_error("iMAML needs at least one adapted module"); return -1; }
    DEV_CHECK(mem.alloc(im_x, (size_t)n_adapt * cap_tasks * sizeof(float)));
    DEV_CHECK(mem.alloc(im_r, (size_t)n_adapt * cap_tasks * sizeof(float)));
    DEV_CHECK(mem.alloc(im_scal, (size_t)cap_tasks * IM_STRIDE * sizeof(float)));
    DEV_CHECK(mem.alloc(im_partial, (size_t)cap_tasks * kImBlocks * sizeof(float)));
    im_ready = true;
    return 0;
}

// out[task][slot] = sum_i a_i * (ca * b_i + cb * a_i)   (deterministic two-stage reduction)
void im_dot(const float* a, long long a_ts, const float* b, long long b_ts, float ca, float cb, int slot, int nt) {
    MTTS_LAUNCH(dot_partial_kernel, dim3(kImBlocks, 1, nt), dim3(256), stream, a, a_ts, b, b_ts, ca, cb, n_adapt / 4, im_partial, (int)kImBlocks);
    MTTS_LAUNCH(dot_final_kernel, dim3(nt), dim3(64), stream, (const float*)im_partial, (int)kImBlocks, im_scal, (int)IM_STRIDE, slot);
}

// query pass at the adapted weights: b = grad_w L_q; x = 0, r = p = b
int imaml_begin(float* losses_out) {
    Plan& sp = plans[0];
    Plan& qp = plans[1];
    if (sp.tasks != qp.tasks || sp.tasks < 1) { set_error("support/query plans not set"); return -1; }
    if (enable_imaml()) return -1;
    const int nt = qp.tasks;
    Pass pq{&qp, true, true};
    if (forward(pq)) return -1;
    if (loss(pq, losses_out ? losses_out : losses)) return -1;
    if (backward(pq, 1.f, encoder_adapted())) return -1;   // a non-adapted encoder's query gradient is not part of the hypergradient (see header)
    // b = p lives in the per-task gradient buffer (grad + adapt_start): it is what the HVP reads as direction
    DEV_CHECK(hipMemsetAsync(im_x, 0, (size_t)n_adapt * cap_tasks * sizeof(float), stream));
    launch_copy_tasks(TS{grad + adapt_start, n_total}, TS{im_r, n_adapt}, n_adapt / 4, nt, stream, 4096);
    im_dot(im_r, n_adapt, im_r, n_adapt, 1.f, 0.f, IM_RS, nt);
    launch_cg_scalar(im_scal, nt, 0, 0.f, stream);
    return 0;
}

// one CG iteration; A p = a (H p + lambda p) with H = Hessian of the support loss of the batch now in slot 0
int imaml_cg_step(float inner_lr, float reg, float tol) {
    Plan& sp = plans[0];
    if (!im_ready || sp.tasks < 1) { set_error("imaml_begin has not run"); return -1; }
    const int nt = sp.tasks;
    if (hvp_support()) return -1;                // hv = H p   (p = adapted slice of the gradient buffer)
    float* p = grad + adapt_start;
    const float* Hp = hv + adapt_start;
    // pAp = sum p * a (Hp + lambda p)
    im_dot(p, n_total, Hp, n_total, inner_lr, inner_lr * reg, IM_PAP, nt);
    launch_cg_scalar(im_scal, nt, 1, tol, stream);   // alpha = rs / pAp
    MTTS_LAUNCH(cg_update_r_kernel, dim3(blocks_for(n_adapt / 4), 1, nt), dim3(256), stream, im_r, n_adapt, (const float*)p, Hp, n_total,
                inner_lr, inner_lr * reg, (const float*)im_scal, (int)IM_STRIDE, n_adapt / 4);
    im_dot(im_r, n_adapt, im_r, n_adapt, 1.f, 0.f, IM_RSNEW, nt);
    launch_cg_scalar(im_scal, nt, 2, tol, stream);   // converged? else beta = rs_new / rs, rs = rs_new
    MTTS_LAUNCH(cg_update_xp_kernel, dim3(blocks_for(n_adapt / 4), 1, nt), dim3(256), stream, im_x, n_adapt, p, n_total, (const float*)im_r,
                (const float*)im_scal, (int)IM_STRIDE, n_adapt / 4);
    return 0;
}

// outer[adapted] = sum_t grad_scale * clip_t(a * lambda * x_t), outer[elsewhere] = 0; clip_t = min(1, max_norm / (|g_t| + 1e-6))
// (imaml.py:125-131 clips each task's hypergradient BEFORE the reduction over ranks; max_norm <= 0: no clipping)
int imaml_finish(float inner_lr, float reg, float grad_scale, float max_norm, float* norms_out_host) {
    Plan& sp = plans[0];
    if (!im_ready || sp.tasks < 1) { set_error("imaml_begin has not run"); return -1; }
    const int nt = sp.tasks;
    im_dot(im_x, n_adapt, im_x, n_adapt, 1.f, 0.f, IM_NORM, nt);
    MTTS_LAUNCH(cg_clip_kernel, dim3(1), dim3(64), stream, im_scal, nt, inner_lr * reg, max_norm, grad_scale);
    DEV_CHECK(hipMemsetAsync(outer, 0, (size_t)n_total * sizeof(float), stream));
    MTTS_LAUNCH(sum_tasks_coef_kernel, dim3(blocks_for(n_adapt / 4)), dim3(256), stream, (const float*)im_x, n_adapt, nt, (const float*)im_scal,
                (int)IM_STRIDE, (int)IM_COEF, outer + adapt_start, n_adapt / 4);
    if (norms_out_host) {
        std::vector<float> sc((size_t)nt * IM_STRIDE);
        DEV_CHECK(hipStreamSynchronize(stream));
        DEV_CHECK(hipMemcpy(sc.data(), im_scal, sc.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int t = 0; t < nt; ++t) norms_out_host[t] = sc[(size_t)t * IM_STRIDE + IM_NORM];
    }
    return 0;
}
