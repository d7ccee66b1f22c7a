// Several outputs under one shared kernel (option 51 of mi_gp_set_option, include/mi_gp.h): Y is n x q, 2 <= q <= 128, output o in
// y_dev[o * lda .. o * lda + n).  One kernel, one noise, the outputs independent given theta, their log marginal likelihoods
// summed (what sklearn's GaussianProcessRegressor does for a 2-D y).  theta, its length and every caller of mi_gp_lml_grad stay as
// they are; the factorisation sees output 0 as its y and is not touched.
//
// Fit (the tail of mi_gp_lml_grad, a consumer of resident state like the trend of api_trend.hip): the ordinary evaluation has left
// K^-1 in the lower triangle of W_dev and sum_i log L_ii among its scalars.  With V = K^-1 Y
//   L_MO = sum_o LML(y_o) = -q sum_i log L_ii - q n/2 log 2 pi - 1/2 sum_o y_o . V[:, o]
//   dL_MO/dtheta_k = 1/2 sum_ij (V V^T - q K^-1)_ij dK_ij/dtheta_k
// which is the LML gradient's contraction with q K^-1 - V V^T in the place of K^-1 and a zero vector in the place of alpha:
// launch_grad_contract as it is.  V is the symmetric thin multiply of trend_f64.hip (the lower triangle of W alone) on Y^T staged
// like the trend's H^T; the update W <- q W - V V^T runs over the lower trapezoid on the GEMM.
//
// Predict (behind mi_gp_factor, conditional form, L in K_dev): B^T = Y^T L^-T, the blocked solve of mi_gp_predict on 128 rows, and
// per point, with a* = L^-1 k(X, x*) the row mi_gp_predict forms in work_dev,
//   mean_o = a* . b_o,   var = kdiag - |a*|^2 (+ gv)
// from one pass over the row (multi_f64.hip).
//
// Option 52 = 1: the between-output covariance integrated out.  vec(Y) ~ N(0, Sigma (x) K_y) with Sigma q x q under the Jeffreys
// prior |Sigma|^-(q+1)/2 (the separable emulator of Conti & O'Hagan 2010).  With S = Y^T V = C_S C_S^T
//   L_S = -q sum_i log L_ii - n sum_j log (C_S)_jj + log Gamma_q(n/2) - n q/2 log pi
//   dL_S/dtheta_k = 1/2 sum_ij (n V S^-1 V^T - q K^-1)_ij dK_ij/dtheta_k
// -- S as the trend's A (k-segmented Gram product, the 128 x 128 leaf, its row-major inverse), Q = sqrt(n) V C_S^-T on the GEMM
// and W <- q W - Q Q^T in the place of W <- q W - V V^T.  Predict: the same means, and a variance per output,
//   var_o = (kdiag - |a*|^2 (+ gv)) s_o,   s_o = |b_o|^2 / (n - q - 1)
// (the predictive multivariate t with n - q + 1 degrees of freedom), from the same pass.
#include "gp_handle.h"

namespace {

// The handle's scratch for up to cap points (vl = cap padded to 128, ldg = vl + 16): Y^T / B^T (128 rows, ldg apart), V and the
// thin multiply's partial products (vl x 128 each; under option 52 = 1 the second holds Q once the products are summed), the zero
// vector (vl) and the q quads (128).  Under option 52 = 1 (cov) these follow: the partial products of S (one per k segment of
// gram_segments: at most vl / 128 and at most TREND_PARTS), the block S -> C_S, the leaf's inverse in operand order, C_S^-1
// row-major, the scales s_o (128), two scalars (in 8) and the bad-pivot word.  The option's value is part of the layout:
// mi_gp_set_option drops the block when it changes.  Every element a launch reads is written earlier in the same call (B^T and
// s_o: by the mi_gp_factor in front of mi_gp_predict).
// The layout is written once, as offsets: multi_layout() places the arrays in a block, multi_scratch_len() is where the last ends.
struct MultiOffsets {
  long ldg, vl;
  size_t YT, V, parts, zero, quad, gparts, S, minv, Cinv, svar, scal, info, len;
};
MultiOffsets multi_offsets(int cap, bool cov) {
  MultiOffsets o;
  o.vl = (cap + 127) / 128 * 128;
  o.ldg = o.vl + 16;
  size_t at = 0;
  const auto take = [&at](size_t n) { const size_t here = at; at += n; return here; };
  o.YT = take(128 * (size_t)o.ldg);
  o.V = take((size_t)o.vl * 128);
  o.parts = take((size_t)o.vl * 128);
  o.zero = take((size_t)o.vl);
  o.quad = take(128);
  o.gparts = o.S = o.minv = o.Cinv = o.svar = o.scal = o.info = at;
  if (cov) {
    const size_t segs = (size_t)(o.vl / 128 < TREND_PARTS ? o.vl / 128 : TREND_PARTS);
    o.gparts = take(segs * MINV_ELEMS);
    o.S = take(MINV_ELEMS);
    o.minv = take(MINV_ELEMS);
    o.Cinv = take(MINV_ELEMS);
    o.svar = take(128);
    o.scal = take(8);
    o.info = take(2);
  }
  o.len = at;
  return o;
}
struct MultiScratch {
  long ldg, vl;
  double *YT, *V, *parts, *zero, *quad, *gparts, *S, *minv, *Cinv, *svar, *scal;
  int* info;
};
MultiScratch multi_layout(double* base, int cap, bool cov) {
  const MultiOffsets o = multi_offsets(cap, cov);
  return {o.ldg, o.vl, base + o.YT, base + o.V, base + o.parts, base + o.zero, base + o.quad, base + o.gparts, base + o.S,
          base + o.minv, base + o.Cinv, base + o.svar, base + o.scal, reinterpret_cast<int*>(base + o.info)};
}
size_t multi_scratch_len(int cap, bool cov) { return multi_offsets(cap, cov).len; }
MultiScratch multi_scratch(const mi_gp_handle* h) {
  return multi_layout(h->blocks[BLK_MULTI].p, h->blocks[BLK_MULTI].cap, h->outcov != 0);
}

// log Gamma_q(a) = q (q - 1) / 4 log pi + sum_{j = 1 .. q} lgamma(a + (1 - j) / 2)
double log_multigamma(double a, int q) {
  double s = 0.25 * (double)q * (double)(q - 1) * std::log(M_PI);
  for (int j = 1; j <= q; ++j) s += std::lgamma(a + 0.5 * (double)(1 - j));
  return s;
}

// option 52 = 1, behind V = K^-1 Y: S = Y^T V in k segments added in index order (identity in the padding), C_S = chol(S) in
// place, its row-major inverse, the two scalars, Q = sqrt(n) V C_S^-T (in t.parts; the columns from q on stay zero) and
// W <- q K^-1 - Q Q^T over the lower tiles (the padding rows of Q are zero)
int cov_update(mi_gp_handle* h, const Eval& E, const MultiScratch& t) {
  const int n = h->n, ntc = h->ntc, q = h->nout;
  const hipStream_t st = h->stream;
  int nparts = 0;
  HCK(gram_segments(h, E, {t.YT, t.ldg}, {t.V, 128}, 1, t.gparts, &nparts), "outputs gram segments");
  HCK(launch_trend_gram_sum(t.gparts, nparts, q, t.S, st), "outputs gram sum");
  HCK(hipMemsetAsync(t.info, 0x7f, sizeof(int), st), "info reset");
  HCK(launch_potrf_leaf128(t.S, 128, t.minv, 0, t.info, st), "outputs leaf");
  HCK(launch_tile_inverse_rows(t.S, 128, 0, t.Cinv, 0, 0, 1, 1, st), "outputs inverse");
  HCK(launch_multi_cov_scal(t.S, t.info, q, t.scal, st), "multi_cov_scal");
  HCK(gemm_call(h, E, 0, 0, {t.V, 128}, {t.Cinv, 128}, {t.parts, 128}, ntc, 1, 128, 0, 0, std::sqrt((double)n), 0.0, 1), "outputs Q");
  HCK(gemm_call(h, E, 0, 0, {t.parts, 128}, {t.parts, 128}, {h->buf.W_dev, h->buf.lda}, ntc, ntc, 128, 1, 0, -1.0, (double)q, 1),
      "outputs rank-128 update");
  return 0;
}

}  // namespace

int multi_objective(mi_gp_handle* h, double* value, double* grad) {
  const int n = h->n, np = h->np, ntc = h->ntc, q = h->nout;
  const long ld = h->buf.lda;
  const bool cov = h->outcov != 0;
  HCK(hipSetDevice(h->device), "hipSetDevice");
  if (int r = ensure_block(h, BLK_MULTI, multi_scratch_len(h->cap, cov), "outputs scratch")) return r;
  const MultiScratch t = multi_scratch(h);
  const hipStream_t st = h->stream;
  const Eval E = one_eval(h);
  double* W = h->buf.W_dev;
  HCK(launch_multi_stage(h->buf.y_dev, ld, q, n, np, t.YT, t.ldg, st), "multi_stage");
  HCK(launch_trend_symm(W, ld, t.YT, t.ldg, n, np, q, t.V, t.parts, st), "outputs symm");
  if (cov) {
    if (int r = cov_update(h, E, t)) return r;
  } else {
    HCK(launch_multi_quad(t.YT, t.ldg, t.V, q, n, t.quad, st), "multi_quad");
    // W <- q K^-1 - V V^T over the lower tiles (the padding rows of V and its columns from q on are zero)
    HCK(gemm_call(h, E, 0, 0, {t.V, 128}, {t.V, 128}, {W, ld}, ntc, ntc, 128, 1, 0, -1.0, (double)q, 1), "outputs rank-128 update");
  }
  HCK(hipMemsetAsync(t.zero, 0, sizeof(double) * np, st), "zero vector");
  HCK(launch_grad_contract(h->spec, h->one.theta_dev, h->buf.X_dev, n, W, ld, t.zero, h->one.part_dev, h->one.grad_host, st),
      "grad_contract");
  double rec[128];
  HCK(hipMemcpyAsync(rec, cov ? t.scal : t.quad, sizeof(double) * (cov ? 2 : q), hipMemcpyDeviceToHost, st), "quad download");
  HCK(hipStreamSynchronize(st), "stream sync");
  if (cov) {
    const int info = (int)rec[1];
    if (info != INFO_OK) {
      snprintf(h->err, sizeof(h->err), "the outputs' block Y^T K^-1 Y is not positive definite (pivot %d of the outputs, option 52 = 1)",
               info);
    }
    const double v = -(double)q * h->one.out_host[1] - (double)n * rec[0] + log_multigamma(0.5 * (double)n, q) -
                     0.5 * (double)n * (double)q * std::log(M_PI);
    return finish_objective(h, info != INFO_OK ? n + info : 0, v, value, grad);
  }
  double s = 0.0;
  for (int o = 0; o < q; ++o) s += rec[o];
  const double v = (double)q * (-h->one.out_host[1] - 0.5 * (double)n * LOG_2PI) - 0.5 * s;
  return finish_objective(h, 0, v, value, grad);
}

int multi_factor(mi_gp_handle* h) {
  HCK(hipSetDevice(h->device), "hipSetDevice");
  if (int r = ensure_block(h, BLK_MULTI, multi_scratch_len(h->cap, h->outcov != 0), "outputs scratch")) return r;
  const MultiScratch t = multi_scratch(h);
  const Eval E = one_eval(h);
  HCK(launch_multi_stage(h->buf.y_dev, h->buf.lda, h->nout, h->n, h->np, t.YT, t.ldg, h->stream), "multi_stage");
  HCK(trsm_rec(h, E, t.YT, t.ldg, 128, 0, h->ntc), "outputs trsm");
  // option 52 = 1: s_o = |b_o|^2 / (n - q - 1), the diagonal of S in the conditional form (n >= q + 2: mi_gp_factor)
  if (h->outcov) HCK(launch_multi_rowsq(t.YT, t.ldg, h->nout, h->n, (double)(h->n - h->nout - 1), t.svar, h->stream), "multi_rowsq");
  HCK(hipStreamSynchronize(h->stream), "stream sync");
  return 0;
}

hipError_t multi_predict_reduce(mi_gp_handle* h, const double* work_dev, long ldw, int m, double* mean_dev, double* var_dev,
                                int pred_noise) {
  if (!h->blocks[BLK_MULTI].p) return hipErrorInvalidValue;  // (mi_gp_factor under option 51 allocates it)
  const MultiScratch t = multi_scratch(h);
  double kd, noise;
  predict_scalars(h, pred_noise, &kd, &noise);
  return launch_multi_predict(work_dev, ldw, t.YT, t.ldg, h->nout, h->n, m, kd, noise, h->outcov ? t.svar : nullptr, mean_dev, var_dev,
                              h->stream);
}

// mi_gp_reserve: the scratch for `capacity` points.  What outlives a call -- the conditional's B^T behind mi_gp_factor, and s_o
// under option 52 = 1 -- moves into the new block (the layout depends on the capacity), as trend_reserve moves G^T; everything
// else is written by the next call before it is read.  The handle's stream is idle (mi_gp_reserve).  A block that is large enough
// stays; without a factored state under q >= 2 there is no B^T to keep, and the block is dropped like the objectives' (its next
// use re-sizes it).
hipError_t multi_reserve(mi_gp_handle* h, int capacity) {
  CapBlock& blk = h->blocks[BLK_MULTI];
  if (!blk.p || blk.cap >= capacity) return hipSuccess;
  if (!(h->factored && h->nout > 1)) {
    drop_block(blk);
    return hipSuccess;
  }
  const bool cov = h->outcov != 0;
  double* fresh = nullptr;
  hipError_t e = hipMalloc(&fresh, sizeof(double) * multi_scratch_len(capacity, cov));
  if (e != hipSuccess) return e;
  const MultiScratch a = multi_scratch(h), b = multi_layout(fresh, capacity, cov);
  e = hipMemcpy2DAsync(b.YT, sizeof(double) * b.ldg, a.YT, sizeof(double) * a.ldg, sizeof(double) * h->np, 128, hipMemcpyDeviceToDevice,
                       h->stream);
  if (e == hipSuccess && cov) e = hipMemcpyAsync(b.svar, a.svar, sizeof(double) * 128, hipMemcpyDeviceToDevice, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) {
    (void)hipFree(fresh);
    return e;
  }
  (void)hipFree(blk.p);
  blk = {fresh, capacity, multi_scratch_len(capacity, cov)};
  return hipSuccess;
}
