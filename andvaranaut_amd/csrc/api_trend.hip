// The GP trend with marginalised coefficients (option 50 of mi_gp_set_option, include/mi_gp.h): a constant or linear prior mean
// h(x)^T beta whose coefficients carry a vague prior and are integrated out in closed form (universal kriging; Rasmussen &
// Williams section 2.7, eqs. 2.41-2.45).  theta, its length and every caller of mi_gp_lml_grad stay as they are.
//
// Fit (the tail of mi_gp_lml_grad, a consumer of resident state like the objectives of api_loo.hip): the ordinary evaluation has
// left K^-1 in the lower triangle of W_dev and alpha = K^-1 y.  With H (n x p, rows h(x_i)^T)
//   V = K^-1 H,  A = H^T V,  C_A = chol(A),  Q = V C_A^-T,  c = Q^T y = C_A^-1 H^T alpha,  beta^ = C_A^-T c
//   L_T = LML + 1/2 |c|^2 - sum_j log (C_A)_jj + p/2 log 2 pi                                              (R & W eq. 2.45)
//   P~ = K^-1 - Q Q^T,   alpha~ = alpha - V beta^  (= P~ y)
//   dL_T/dtheta_k = 1/2 sum_ij (alpha~_i alpha~_j - P~_ij) dK_ij/dtheta_k
// which is the LML gradient's contraction with P~ in the place of K^-1 and alpha~ in the place of alpha: launch_grad_contract as it
// is.  V is the symmetric thin multiply of trend_f64.hip (the lower triangle of W alone); A is a 128 x 128 product over k = np, formed
// in k segments (a single output tile over all of k would run on four workgroups) that are added in index order; the rank-128
// update W -= Q Q^T runs over the lower trapezoid on the GEMM.
//
// Predict (behind mi_gp_factor, conditional form, L in K_dev and b = L^-1 y in its beta row):
//   G = L^-1 H (G^T = H^T L^-T: the blocked solve of mi_gp_predict on 128 rows),  A = G^T G = C_A C_A^T,
//   beta^ = A^-1 G^T b,  b~ = b - G beta^
// and per point, with a* = L^-1 k(X, x*) the row mi_gp_predict forms in work_dev,
//   r = h(x*) - G^T a*,   mean = a* . b~ + h(x*)^T beta^,   var = kdiag - |a*|^2 + |C_A^-1 r|^2 (+ gv)      (R & W eqs. 2.41-2.42)
#include "gp_handle.h"

namespace {

// The handle's scratch for up to cap points (vl = cap padded to 128, ldg = vl + 16): G^T / H^T (128 rows, ldg apart), V and Q
// (vl x 128), the partial products of A (at most 65 blocks), the block A -> C_A, the leaf's inverse in operand order, C_A^-1
// row-major, then u = H^T alpha or G^T b, c, beta^ (128 each), b~ and alpha~ (vl each), three scalars and the bad-pivot word.
// Every element a launch reads is written earlier in the same call (G^T, C_A^-1, beta^ and b~: by the mi_gp_factor in front of
// mi_gp_predict).
struct TrendScratch {
  long ldg;
  double *GT, *V, *Q, *parts, *A, *minv, *Cinv, *u, *c, *beta, *bt, *at, *scal;
  int* info;
};
TrendScratch trend_layout(double* base, int cap) {
  const long vl = (cap + 127) / 128 * 128;
  TrendScratch t;
  t.ldg = vl + 16;
  t.GT = base;
  t.V = t.GT + 128 * t.ldg;
  t.Q = t.V + vl * 128;
  t.parts = t.Q + vl * 128;
  t.A = t.parts + (long)TREND_PARTS * MINV_ELEMS;
  t.minv = t.A + MINV_ELEMS;
  t.Cinv = t.minv + MINV_ELEMS;
  t.u = t.Cinv + MINV_ELEMS;
  t.c = t.u + 128;
  t.beta = t.c + 128;
  t.bt = t.beta + 128;
  t.at = t.bt + vl;
  t.scal = t.at + vl;
  t.info = reinterpret_cast<int*>(t.scal + 8);
  return t;
}
TrendScratch trend_scratch(const mi_gp_handle* h) { return trend_layout(h->blocks[BLK_TREND].p, h->blocks[BLK_TREND].cap); }

// A = sum over k segments of GT[:, seg] B[seg]^T (B = V stored [k][x] for the fit, G^T itself for the conditional), C_A = chol(A)
// in place, its row-major inverse, then u = GT x, c, beta^ and the scalars
int trend_block(mi_gp_handle* h, const Eval& E, const TrendScratch& t, bool fit, const double* x) {
  const int n = h->n, p = trend_columns(h);
  const hipStream_t st = h->stream;
  int nparts = 0;
  if (fit) HCK(gram_segments(h, E, {t.GT, t.ldg}, {t.V, 128}, 1, t.parts, &nparts), "trend gram segments");
  else HCK(gram_segments(h, E, {t.GT, t.ldg}, {t.GT, t.ldg}, 0, t.parts, &nparts), "trend gram segments");
  HCK(launch_trend_gram_sum(t.parts, nparts, p, t.A, st), "trend_gram_sum");
  HCK(hipMemsetAsync(t.info, 0x7f, sizeof(int), st), "info reset");
  HCK(launch_potrf_leaf128(t.A, 128, t.minv, 0, t.info, st), "trend leaf");
  HCK(launch_tile_inverse_rows(t.A, 128, 0, t.Cinv, 0, 0, 1, 1, st), "trend inverse");
  HCK(launch_trend_rowdot(t.GT, t.ldg, x, n, t.u, st), "trend_rowdot");
  HCK(launch_trend_solve(t.A, t.Cinv, t.u, t.info, p, t.c, t.beta, t.scal, st), "trend_solve");
  return 0;
}

}  // namespace

int trend_objective(mi_gp_handle* h, double* value, double* grad) {
  const int n = h->n, np = h->np, ntc = h->ntc, p = trend_columns(h);
  const long ld = h->buf.lda;
  HCK(hipSetDevice(h->device), "hipSetDevice");
  if (int r = ensure_block(h, BLK_TREND, trend_scratch_len(h->cap), "trend scratch")) return r;
  const TrendScratch t = trend_scratch(h);
  const hipStream_t st = h->stream;
  const Eval E = one_eval(h);
  double* W = h->buf.W_dev;
  HCK(launch_trend_basis(h->buf.X_dev, n, h->cfg.d, p, np, t.GT, t.ldg, st), "trend_basis");
  HCK(launch_trend_symm(W, ld, t.GT, t.ldg, n, np, p, t.V, t.Q, st), "trend_symm");  // (Q: the slices' partial products)
  if (int r = trend_block(h, E, t, true, h->one.alpha_dev)) return r;
  HCK(launch_trend_project(h->one.alpha_dev, t.V, 128, 1, t.beta, p, n, np, t.at, st), "trend_project");
  // Q = V C_A^-T (the columns from p on stay zero), then P~ = K^-1 - Q Q^T over the lower tiles (the padding rows of Q are zero)
  HCK(gemm_call(h, E, 0, 0, {t.V, 128}, {t.Cinv, 128}, {t.Q, 128}, ntc, 1, 128, 0, 0, 1.0, 0.0, 1), "trend Q");
  HCK(gemm_call(h, E, 0, 0, {t.Q, 128}, {t.Q, 128}, {W, ld}, ntc, ntc, 128, 1, 0, -1.0, 1.0, 1), "trend rank-128 update");
  HCK(launch_grad_contract(h->spec, h->one.theta_dev, h->buf.X_dev, n, W, ld, t.at, h->one.part_dev, h->one.grad_host, st),
      "grad_contract");
  double sc[3] = {0.0, 0.0, 0.0};
  HCK(hipMemcpyAsync(sc, t.scal, sizeof(sc), hipMemcpyDeviceToHost, st), "scalar download");
  HCK(hipStreamSynchronize(st), "stream sync");
  const int info = (int)sc[2];
  if (info != INFO_OK) {
    snprintf(h->err, sizeof(h->err), "the trend's block H^T K^-1 H is not positive definite (pivot %d of the basis)", info);
  }
  return finish_objective(h, info != INFO_OK ? n + info : 0, h->one.out_host[0] + sc[0] - sc[1] + 0.5 * (double)p * LOG_2PI, value, grad);
}

int trend_factor(mi_gp_handle* h) {
  const int n = h->n, np = h->np, p = trend_columns(h);
  const long ld = h->buf.lda;
  HCK(hipSetDevice(h->device), "hipSetDevice");
  if (int r = ensure_block(h, BLK_TREND, trend_scratch_len(h->cap), "trend scratch")) return r;
  const TrendScratch t = trend_scratch(h);
  const hipStream_t st = h->stream;
  const Eval E = one_eval(h);
  const double* b = h->buf.K_dev + (long)np * ld;
  HCK(launch_trend_basis(h->buf.X_dev, n, h->cfg.d, p, np, t.GT, t.ldg, st), "trend_basis");
  HCK(trsm_rec(h, E, t.GT, t.ldg, 128, 0, h->ntc), "trend trsm");
  if (int r = trend_block(h, E, t, false, b)) return r;
  HCK(launch_trend_project(b, t.GT, 1, t.ldg, t.beta, p, n, np, t.bt, st), "trend_project");
  double sc[3] = {0.0, 0.0, 0.0};
  HCK(hipMemcpyAsync(sc, t.scal, sizeof(sc), hipMemcpyDeviceToHost, st), "scalar download");
  HCK(hipStreamSynchronize(st), "stream sync");
  const int info = (int)sc[2];
  if (info != INFO_OK) {
    snprintf(h->err, sizeof(h->err), "the trend's block H^T K^-1 H is not positive definite (pivot %d of the basis)", info);
    return n + info;
  }
  return 0;
}

hipError_t trend_predict_reduce(mi_gp_handle* h, const double* Xnew_dev, const double* work_dev, long ldw, int m, double* mean_dev,
                                double* var_dev, int pred_noise) {
  if (!h->blocks[BLK_TREND].p) return hipErrorInvalidValue;  // (mi_gp_factor under a trend allocates it; mi_gp_reserve ends `factored`)
  const TrendScratch t = trend_scratch(h);
  double kd, noise;
  predict_scalars(h, pred_noise, &kd, &noise);
  return launch_trend_predict_reduce(work_dev, ldw, Xnew_dev, h->cfg.d, trend_columns(h), t.GT, t.ldg, t.bt, t.beta, t.Cinv, h->n, m, kd,
                                     noise, mean_dev, var_dev, h->stream);
}

// mi_gp_reserve: the scratch for `capacity` points.  What outlives a call -- the conditional's G^T, C_A^-1, beta^ and b~ behind
// mi_gp_factor -- moves into the new block (the layout depends on the capacity), as mi_gp_reserve moves the leaf inverses and
// alpha; everything else is written by the next call before it is read.  The handle's stream is idle (mi_gp_reserve).
hipError_t trend_reserve(mi_gp_handle* h, int capacity) {
  if (!h->blocks[BLK_TREND].p) return hipSuccess;
  double* fresh = nullptr;
  hipError_t e = hipMalloc(&fresh, sizeof(double) * trend_scratch_len(capacity));
  if (e != hipSuccess) return e;
  const TrendScratch a = trend_scratch(h), b = trend_layout(fresh, capacity);
  const hipStream_t st = h->stream;
  e = hipMemcpy2DAsync(b.GT, sizeof(double) * b.ldg, a.GT, sizeof(double) * a.ldg, sizeof(double) * h->np, 128, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(b.Cinv, a.Cinv, sizeof(double) * MINV_ELEMS, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(b.beta, a.beta, sizeof(double) * 128, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(b.bt, a.bt, sizeof(double) * h->np, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    (void)hipFree(fresh);
    return e;
  }
  (void)hipFree(h->blocks[BLK_TREND].p);
  h->blocks[BLK_TREND] = {fresh, capacity, trend_scratch_len(capacity)};
  return hipSuccess;
}
