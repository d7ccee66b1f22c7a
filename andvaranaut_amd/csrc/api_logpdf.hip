// mi_gp_logpdf (include/mi_gp.h): the joint log predictive density of trial points given the resident factorisation, and its
// gradients w.r.t. the trial inputs and outputs.  The value is phase 1 of mi_gp_append (conditional_block(), api_gp.hip) without
// the commit; the gradient adds three kernels of grad_predict.hip.  A file of its own: the host-only schedule-trace program
// (tests/sched_trace) links api_gp.hip against stand-ins of the launchers that file uses.
#include "gp_handle.h"

// ---------------------------------------------------------------- joint log predictive density of trial points
// doubles of mi_gp_logpdf's work block: mi_gp_append's (4 * 128 * ldw + 65600), then S^-1 (16384) and gamma (128)
constexpr long LOGPDF_TAIL = 65600 + MINV_ELEMS + 128;
extern "C" long mi_gp_logpdf_work(long ldw) { return (ldw < 128 || (ldw & 1)) ? -1 : 4 * 128 * ldw + LOGPDF_TAIL; }

// log p(y2 | y1, X1, X2, theta) = LML(n + k) - LML(n) and its gradients w.r.t. the trial inputs and outputs, from the resident
// factor: conditional_block() (mi_gp_append's phase 1) gives L22 and beta2, hence the value; nothing is committed.  Gradients are
// the last k rows of the joint system's data gradient (oracle lml_grad_data), in block form with U = L^-T resident:
//   gamma = L22^-T beta2 (= the joint alpha's trial block),  P = L21 U11^T,  Q = S^-1 P,
//   C = gamma (alpha1 - P^T gamma)^T + Q   (k x n: alpha_J alpha_J^T - K_J^-1, trial rows x training columns)
//   D = gamma gamma^T - S^-1               (k x k: trial rows x trial columns)
//   dy = -gamma,  dx_im = sum_j C_ij dk(x*_i, x_j)/dx*_im + sum_j D_ij dk(x*_i, x*_j)/dx*_im.
// Work block behind mi_gp_append's layout: P overwrites K21, Q and then C overwrite L21 (neither is needed by then).
extern "C" int mi_gp_logpdf(mi_gp_handle* h, const double* Xnew_dev, const double* ynew_dev, const double* diag_new_dev, int k,
                            double* work_dev, long ldw, double* logp_out, double* dx_dev, double* dy_dev) {
  if (!h) { set_global_error("mi_gp_logpdf: null handle"); return -1; }
  if (int r = refuse_plain_model(h, "mi_gp_logpdf")) return r;
  const bool grad = dx_dev || dy_dev;
  char why[160] = "";
  if (!Xnew_dev || !ynew_dev || !work_dev || !logp_out) snprintf(why, sizeof(why), "null point, value, work or result buffer");
  else if (k < 1 || k > 128) snprintf(why, sizeof(why), "1 <= k <= 128 (got %d)", k);
  else if (!h->factored) snprintf(why, sizeof(why), "call mi_gp_factor first");
  else if (!diag_new_dev != !h->diag_dev) snprintf(why, sizeof(why), "diag_new_dev must be given exactly when a diagonal is set (mi_gp_set_diag)");
  else if (ldw < h->np || (ldw & 1)) snprintf(why, sizeof(why), "ldw must be even and >= padded n = %d", h->np);
  else if (grad && (!h->buf.Z_dev || !h->buf.W_dev)) snprintf(why, sizeof(why), "gradients need Z_dev and W_dev in mi_gp_set_data");
  else if (grad && (size_t)(h->cfg.nkern + 1) * h->cfg.d * sizeof(double) > PREDICT_GRAD_MAX_LDS)
    snprintf(why, sizeof(why), "gradients: (nkern + 1) * d must fit %d bytes of LDS (d <= %d here)", (int)PREDICT_GRAD_MAX_LDS,
             (int)(PREDICT_GRAD_MAX_LDS / sizeof(double)) / (h->cfg.nkern + 1));
  if (why[0]) { snprintf(h->err, sizeof(h->err), "mi_gp_logpdf: %s", why); return -1; }
  HCK(hipSetDevice(h->device), "hipSetDevice");
  const hipStream_t st = h->stream;
  const bool prof = h->prof_level >= 1;
  // (U first: the conditional block then takes the one-GEMM route, and a block that is not positive definite still leaves a
  // handle that mi_gp_predict_grad would have left)
  if (grad)
    if (int r = make_u_resident(h)) return r;
  if (prof) HCK(hipEventRecord(h->ev[0], st), "event");
  double stats[3];
  if (int r = conditional_block(h, Xnew_dev, ynew_dev, diag_new_dev, k, work_dev, ldw, stats)) return r;
  if (prof) HCK(hipEventRecord(h->ev[1], st), "event");
  const int info = (int)stats[2];
  if (info != INFO_OK) {
    *logp_out = -INFINITY;
    snprintf(h->err, sizeof(h->err), "mi_gp_logpdf: the trial block is not positive definite (pivot %d)", info);
    return info;
  }
  *logp_out = -0.5 * stats[1] - stats[0] - 0.5 * (double)k * LOG_2PI;
  if (grad) {
    const int n = h->n, np = h->np, ntc = h->ntc;
    const long ld = h->buf.lda, R = 128L * ldw;
    double *Cw = work_dev, *P = work_dev + R, *S = work_dev + 4 * R;
    double *Linv22 = S + 3 * MINV_ELEMS, *Sinv = work_dev + 4 * R + 65600, *gamma = Sinv + MINV_ELEMS;
    const Eval E = one_eval(h);
    HCK(launch_tile_inverse_rows(S, 128, 0, Linv22, 0, 0, 1, 1, st), "L22 inverse");
    HCK(launch_logpdf_sinv(Linv22, S + MINV_ELEMS, Sinv, gamma, st), "S inverse");
    // P = L21 U11^T (U11 upper: k >= column tile) and Q = S^-1 P: the two products of mi_gp_append's commit
    HCK(gemm_call(h, E, 0, 0, {work_dev, ldw}, {h->buf.Z_dev, ld}, {P, ldw}, 1, ntc, np, 0, 1, 1.0, 0.0, 1), "L21 U11^T");
    HCK(gemm_call(h, E, 0, 1, {Sinv, 128}, {P, ldw}, {Cw, ldw}, 1, ntc, 128, 0, 0, 1.0, 0.0, 1), "S^-1 P");
    HCK(launch_logpdf_weights(Cw, P, ldw, h->one.alpha_dev, gamma, n, k, dy_dev, st), "weights");
    if (prof) HCK(hipEventRecord(h->ev[2], st), "event");
    if (dx_dev)
      HCK(launch_logpdf_grad(h->spec, h->one.theta_dev, h->buf.X_dev, n, Xnew_dev, k, Cw, ldw, gamma, Sinv, dx_dev, st), "logpdf_grad");
    if (prof) HCK(hipEventRecord(h->ev[3], st), "event");
    HCK(hipStreamSynchronize(st), "stream sync");
  }
  if (prof) {
    if (!grad) HCK(hipEventSynchronize(h->ev[1]), "event sync");  // (recorded behind the conditional block's synchronisation)
    float ms = 0.f;
    h->t_logpdf_ms[1] = h->t_logpdf_ms[2] = 0.0;
    (void)hipEventElapsedTime(&ms, h->ev[0], h->ev[1]); h->t_logpdf_ms[0] = ms;
    if (grad) {
      (void)hipEventElapsedTime(&ms, h->ev[1], h->ev[2]); h->t_logpdf_ms[1] = ms;
      (void)hipEventElapsedTime(&ms, h->ev[2], h->ev[3]); h->t_logpdf_ms[2] = ms;
    }
  }
  return 0;
}
