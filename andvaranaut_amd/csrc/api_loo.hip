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
//
// Option 49 = b > 1: the k-fold objective over the contiguous folds I_f = [f b, min((f + 1) b, n)), the sum of mi_gp_kfold's
// logp over them.  With C = chol(P_II), M = C^-1, t = M alpha_I, tau = |t|^2 (mi_gp_kfold's quantities) and Sigma_I = M^T M
//   L_CV = sum_f [ -1/2 tau_f + sum_i log C_ii - |I_f|/2 log 2 pi ]
//   dL_CV/dP_II = 1/2 (e e^T + Sigma_I) = 1/2 R R^T,   dL_CV/dalpha_I = -e_I,   e_I = M^T t,   R = M^T + e t^T / (1 + sqrt(1 + tau))
// (R is M^T times the symmetric square root of I + t t^T: no second factorisation).  diag(s) becomes blockdiag(R_f),
// B[:, I_f] = P[:, I_f] R_f, q_I = t / sqrt(1 + tau) so that R q = e and w = B q = P e -- and from B on the tail is the one above,
// launch for launch.  b = 1 takes the leave-one-out path itself; b >= n is the log marginal likelihood by another route.
#include "gp_handle.h"

// The handle's scratch of option 49's fold pass for up to cap points: a work block as mi_gp_kfold lays it out (fold_layout(), for
// cv_pass(cap) folds per pass: no result depends on it), behind it what the objective adds -- R [padded cap][128] and the
// per-fold logp [padded cap].  Every element is written before it is read.
constexpr int CV_PASS_MAX = 128;
static int cv_pass(int cap) { return cap / 2 + 1 < CV_PASS_MAX ? cap / 2 + 1 : CV_PASS_MAX; }  // (folds of two points or more)
static long cv_padded(int cap) { return (cap + 127) / 128 * 128; }
static double* cv_R(const CapBlock& cv) { return cv.p + fold_work_len(cv_pass(cv.cap), cv_padded(cv.cap)); }

// The fold pass of option 49: mi_gp_kfold's gather and batched leaf over passes of the handle's scratch, then per fold t, e_I,
// q_I, R_f and the logp (cv_fold_kernel); the folds' sum and the first bad index in one launch behind the last pass.  idx / ptr:
// the caller's host lists, staged from here (they live until the caller synchronises the stream).
static int cv_fold_pass(mi_gp_handle* h, int b, std::vector<int>& idx, std::vector<int>& ptr, double* e, double* q, double* scal) {
  const int n = h->n;
  const hipStream_t st = h->stream;
  const long vl = cv_padded(h->cap);
  if (int r = ensure_block(h, BLK_CV, fold_work_len(cv_pass(h->cap), vl) + vl * 128 + vl, "k-fold scratch")) return r;
  const CapBlock& cv = h->blocks[BLK_CV];
  const int nfolds = (n + b - 1) / b;
  const FoldWork w = fold_layout(cv.p, cv_pass(cv.cap), n, nfolds);
  double *R = cv_R(cv), *flogp = R + cv_padded(cv.cap) * 128;
  idx.resize(n);
  ptr.resize(nfolds + 1);
  for (int i = 0; i < n; ++i) idx[i] = i;
  for (int f = 0; f <= nfolds; ++f) ptr[f] = f * b < n ? f * b : n;
  const int r = fold_pass(h, w, nfolds, ptr.data(), idx.data(), [&](int f0, int nf) {
    return launch_cv_fold(w.blocks, w.minv, w.vecs, w.ptr, w.info, f0, nf, flogp, e, q, R, st);
  });
  if (r != 0) return r;
  HCK(launch_cv_reduce(flogp, w.ptr, w.info, nfolds, scal, st), "cv_reduce");
  return 0;
}

int loo_objective(mi_gp_handle* h, double* value, double* grad) {
  const int n = h->n, np = h->np;
  const long ld = h->buf.lda;
  HCK(hipSetDevice(h->device), "hipSetDevice");
  // The vectors e, s, q, w, the zero vector and the per-point logp (vl apart), then 8 scalars, all zero: the zero vector among them
  // is never written again.  They are cleared ON THE HANDLE'S STREAM, in front of the tail's kernels: hipMemset of device memory
  // returns before the fill has run, and the handle's streams are non-blocking, so a fill on the null stream can land behind the
  // first tail's kernels and wipe what they wrote (e, s, q and the scalars: a first evaluation with L_LOO = 0 and a zero
  // gradient, and a MAP fit that ends elsewhere).
  const CapBlock& loo = h->blocks[BLK_LOO];
  const size_t len = (size_t)6 * ((h->cap + 127) / 128 * 128) + 8;
  bool fresh = false;
  if (int r = ensure_block(h, BLK_LOO, len, "leave-one-out vectors", &fresh)) return r;
  if (fresh) HCK(hipMemsetAsync(loo.p, 0, sizeof(double) * len, h->stream), "leave-one-out vectors");
  const long vl = (loo.cap + 127) / 128 * 128;
  double *e = loo.p, *s = e + vl, *q = s + vl, *w = q + vl, *logp = w + 2 * vl, *scal = logp + vl;
  const double* zero = w + vl;  // (zeroed with the block, never written)
  const hipStream_t st = h->stream;
  const Eval E = one_eval(h);
  const double *P = h->buf.W_dev, *alpha = h->one.alpha_dev;
  double *B = h->buf.Z_dev, *G = h->buf.K_dev;
  h->have_u = false;  // (Z_dev is this call's scratch)
  std::vector<int> fold_idx, fold_ptr;  // (the staged lists of option 49: alive until the stream is synchronised)
  if (h->cv_block > 1) {
    const int r = cv_fold_pass(h, h->cv_block, fold_idx, fold_ptr, e, q, scal);
    if (r != 0) return r;
    HCK(launch_cv_mirror_multiply(P, ld, cv_R(h->blocks[BLK_CV]), h->cv_block, n, np, B, ld, st), "cv_mirror_multiply");
  } else {
    HCK(launch_loo_weights(P, ld, alpha, n, e, s, q, logp, scal, st), "loo_weights");
    HCK(launch_loo_scale_mirror(P, ld, s, n, np, B, ld, st), "loo_scale_mirror");
  }
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
  return finish_objective(h, (int)sc[1], sc[0], value, grad);
}
