// The leave-one-out objective of mi_gp_lml_grad (option 48 = 1, include/mi_gp.h): L_LOO = sum_i log p(y_i | y_-i), Rasmussen &
// Williams section 5.4.2, and its exact gradient w.r.t. theta in reverse mode.  A consumer of resident state like mi_gp_kfold:
// the ordinary evaluation has left P = K^-1 in the lower triangle of W_dev and alpha = P y; with p_i = P_ii
//   L_LOO = sum_i [ 1/2 log p_i - 1/2 alpha_i^2 / p_i - 1/2 log 2 pi ]            (mi_gp_kfold's singleton densities, summed)
//   dL_LOO/dP_ii = 1/2 (1 + alpha_i^2 / p_i) / p_i = 1/2 s_i^2,   dL_LOO/dalpha_i = -alpha_i / p_i = -e_i
// and with dP = -P dK P, dalpha = -P dK alpha
//   dL_LOO/dtheta_k = 1/2 sum_ij [ (alpha_i w_j + w_i alpha_j) - M_ij ] dK_ij/dtheta_k,   w = P e,  M = (P diag s)(P diag s)^T.
// That is the LML gradient's contraction 1/2 sum (alpha_i alpha_j - Kinv_ij) dK_ij with the matrix G' = M - (alpha w^T + w alpha^T)
// in the place of K^-1 and a zero vector in the place of alpha: launch_grad_contract as it is.  Cost: ONE lower-trapezoid GEMM
// with k = np (np^3 flops, about what the evaluation in front of it costs) whatever ntheta is, where the forward form (R & W
// eq. 5.13) costs one N^3 product per hyper-parameter.  B = P diag(s) goes to Z_dev as a full matrix, G' to the lower triangle of
// K_dev: both are scratch between evaluations (the factor and U = L^-T are not resident after mi_gp_lml_grad).
#include "gp_handle.h"

int loo_objective(mi_gp_handle* h, double* value, double* grad) {
  const int n = h->n, np = h->np;
  const long ld = h->buf.lda;
  HCK(hipSetDevice(h->device), "hipSetDevice");
  if (!h->loo_vec_dev || h->loo_cap < h->cap) HCK(size_loo_vectors(h, h->cap), "leave-one-out vectors");
  const long vl = (h->loo_cap + 127) / 128 * 128;
  double *e = h->loo_vec_dev, *s = e + vl, *q = s + vl, *w = q + vl, *logp = w + 2 * vl, *scal = logp + vl;
  const double* zero = w + vl;  // (zeroed by size_loo_vectors, never written)
  const hipStream_t st = h->stream;
  const Eval E = one_eval(h);
  const double *P = h->buf.W_dev, *alpha = h->one.alpha_dev;
  double *B = h->buf.Z_dev, *G = h->buf.K_dev;
  h->have_u = false;  // (Z_dev is this call's scratch)
  HCK(launch_loo_weights(P, ld, alpha, n, e, s, q, logp, scal, st), "loo_weights");
  HCK(launch_loo_scale_mirror(P, ld, s, n, np, B, ld, st), "loo_scale_mirror");
  HCK(launch_loo_gemv(B, ld, q, n, w, st), "loo_gemv");
  HCK(launch_loo_rank2_init(alpha, w, n, np, G, ld, st), "loo_rank2_init");
  // G' += B B^T over the lower tiles (the padding rows and columns of B are zero: so is the padding of G')
  HCK(gemm_call(h, E, 0, 0, {B, ld}, {B, ld}, {G, ld}, h->ntc, h->ntc, np, 1, 0, 1.0, 1.0, 1), "loo syrk");
  HCK(launch_grad_contract(h->spec, h->one.theta_dev, h->buf.X_dev, n, G, ld, zero, h->one.part_dev, h->one.grad_host, st),
      "grad_contract");
  double sc[2] = {0.0, 0.0};
  HCK(hipMemcpyAsync(sc, scal, sizeof(sc), hipMemcpyDeviceToHost, st), "scalar download");
  // The triangular inverse of the next gradient evaluation rewrites the diagonal and upper tiles of Z_dev and never the tiles
  // below them, which hold zeros (include/mi_gp.h): B is taken out again, all of it
  HCK(hipMemset2DAsync(B, sizeof(double) * ld, 0, sizeof(double) * np, np, st), "Z_dev restore");
  HCK(hipStreamSynchronize(st), "stream sync");
  const int bad = (int)sc[1];
  if (bad != 0) {
    *value = -INFINITY;
    for (int i = 0; i < h->ntheta; ++i) grad[i] = 0.0;
    return bad;
  }
  *value = sc[0];
  for (int i = 0; i < h->ntheta; ++i) grad[i] = h->one.grad_host[i];
  return 0;
}
