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
#include "gp_handle.h"

namespace {

// The handle's scratch for up to cap points (vl = cap padded to 128, ldg = vl + 16): Y^T / B^T (128 rows, ldg apart), V and the
// thin multiply's partial products (vl x 128 each), the zero vector (vl) and the q quads (128).  Every element a launch reads is
// written earlier in the same call (B^T: by the mi_gp_factor in front of mi_gp_predict).
// The layout is written once, as offsets: multi_layout() places the arrays in a block, multi_scratch_len() is where the last ends.
struct MultiOffsets {
  long ldg, vl;
  size_t YT, V, parts, zero, quad, len;
};
MultiOffsets multi_offsets(int cap) {
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
  o.len = at;
  return o;
}
struct MultiScratch {
  long ldg, vl;
  double *YT, *V, *parts, *zero, *quad;
};
MultiScratch multi_layout(double* base, int cap) {
  const MultiOffsets o = multi_offsets(cap);
  return {o.ldg, o.vl, base + o.YT, base + o.V, base + o.parts, base + o.zero, base + o.quad};
}
size_t multi_scratch_len(int cap) { return multi_offsets(cap).len; }
MultiScratch multi_scratch(const mi_gp_handle* h) { return multi_layout(h->multi_blk.p, h->multi_blk.cap); }

}  // namespace

int multi_objective(mi_gp_handle* h, double* value, double* grad) {
  const int n = h->n, np = h->np, ntc = h->ntc, q = h->nout;
  const long ld = h->buf.lda;
  HCK(hipSetDevice(h->device), "hipSetDevice");
  if (stale_block(h, h->multi_blk)) HCK(resize_block(h->multi_blk, h->cap, multi_scratch_len(h->cap)), "outputs scratch");
  const MultiScratch t = multi_scratch(h);
  const hipStream_t st = h->stream;
  const Eval E = one_eval(h);
  double* W = h->buf.W_dev;
  HCK(launch_multi_stage(h->buf.y_dev, ld, q, n, np, t.YT, t.ldg, st), "multi_stage");
  HCK(launch_trend_symm(W, ld, t.YT, t.ldg, n, np, q, t.V, t.parts, st), "outputs symm");
  HCK(launch_multi_quad(t.YT, t.ldg, t.V, q, n, t.quad, st), "multi_quad");
  // W <- q K^-1 - V V^T over the lower tiles (the padding rows of V and its columns from q on are zero)
  HCK(gemm_call(h, E, 0, 0, {t.V, 128}, {t.V, 128}, {W, ld}, ntc, ntc, 128, 1, 0, -1.0, (double)q, 1), "outputs rank-128 update");
  HCK(hipMemsetAsync(t.zero, 0, sizeof(double) * np, st), "zero vector");
  HCK(launch_grad_contract(h->spec, h->one.theta_dev, h->buf.X_dev, n, W, ld, t.zero, h->one.part_dev, h->one.grad_host, st),
      "grad_contract");
  double quad[128];
  HCK(hipMemcpyAsync(quad, t.quad, sizeof(double) * q, hipMemcpyDeviceToHost, st), "quad download");
  HCK(hipStreamSynchronize(st), "stream sync");
  double s = 0.0;
  for (int o = 0; o < q; ++o) s += quad[o];
  const double v = (double)q * (-h->one.out_host[1] - 0.5 * (double)n * LOG_2PI) - 0.5 * s;
  return finish_objective(h, 0, v, value, grad);
}

int multi_factor(mi_gp_handle* h) {
  HCK(hipSetDevice(h->device), "hipSetDevice");
  if (stale_block(h, h->multi_blk)) HCK(resize_block(h->multi_blk, h->cap, multi_scratch_len(h->cap)), "outputs scratch");
  const MultiScratch t = multi_scratch(h);
  const Eval E = one_eval(h);
  HCK(launch_multi_stage(h->buf.y_dev, h->buf.lda, h->nout, h->n, h->np, t.YT, t.ldg, h->stream), "multi_stage");
  HCK(trsm_rec(h, E, t.YT, t.ldg, 128, 0, h->ntc), "outputs trsm");
  HCK(hipStreamSynchronize(h->stream), "stream sync");
  return 0;
}

hipError_t multi_predict_reduce(mi_gp_handle* h, const double* work_dev, long ldw, int m, double* mean_dev, double* var_dev,
                                int pred_noise) {
  if (!h->multi_blk.p) return hipErrorInvalidValue;  // (mi_gp_factor under option 51 allocates it)
  const MultiScratch t = multi_scratch(h);
  double kd, noise;
  predict_scalars(h, pred_noise, &kd, &noise);
  return launch_multi_predict(work_dev, ldw, t.YT, t.ldg, h->nout, h->n, m, kd, noise, mean_dev, var_dev, h->stream);
}

// mi_gp_reserve: the scratch for `capacity` points.  What outlives a call -- the conditional's B^T behind mi_gp_factor -- moves into
// the new block (the layout depends on the capacity), as trend_reserve moves G^T; everything else is written by the next call
// before it is read.  The handle's stream is idle (mi_gp_reserve).  A block that is large enough stays; without a factored state
// under q >= 2 there is no B^T to keep, and the block is dropped like the objectives' (its next use re-sizes it).
hipError_t multi_reserve(mi_gp_handle* h, int capacity) {
  if (!h->multi_blk.p || h->multi_blk.cap >= capacity) return hipSuccess;
  if (!(h->factored && h->nout > 1)) return resize_block(h->multi_blk, 0, 0);
  double* fresh = nullptr;
  hipError_t e = hipMalloc(&fresh, sizeof(double) * multi_scratch_len(capacity));
  if (e != hipSuccess) return e;
  const MultiScratch a = multi_scratch(h), b = multi_layout(fresh, capacity);
  e = hipMemcpy2DAsync(b.YT, sizeof(double) * b.ldg, a.YT, sizeof(double) * a.ldg, sizeof(double) * h->np, 128, hipMemcpyDeviceToDevice,
                       h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) {
    (void)hipFree(fresh);
    return e;
  }
  (void)hipFree(h->multi_blk.p);
  h->multi_blk = {fresh, capacity};
  return hipSuccess;
}
