// Host side of the path sweep (options 54 / 55 of mi_gp_set_option; include/mi_gp.h has the contract, paths_f64.hip the kernels):
// mi_gp_predict_grad under option 54 = S >= 1.  Linked weakly from api_gp.hip (gp_handle.h), as api_sweep.hip is.
#include "gp_handle.h"

static int path_refuse(mi_gp_handle* h, const char* why) {
  snprintf(h->err, sizeof(h->err), "mi_gp_predict_grad under option 54 = %d (the path sweep): %s", h->npaths, why);
  return -1;
}

// V <- K_y^-1 (y - Phi(X) W - V) for the S columns of the block: the prior part from the feature half of the sweep kernel at the
// training points, the residual as R^T (128 rows, zeros from S and from column n on), then R^T U and (R^T U) U^T on the GEMM
// (K_y^-1 = U U^T with U = L^-T resident: mi_gp_predict_u's and mi_gp_append's launches), and the rows go back as columns
static int path_condition(mi_gp_handle* h, const PathScratch& t, const double* bph, double* V, long ldw) {
  const int n = h->n, S = h->npaths;
  const hipStream_t st = h->stream;
  const Eval E = one_eval(h);
  HCK(launch_path_sweep(h->spec, h->one.theta_dev, n, h->nfeat, S, bph, t, h->buf.X_dev, n, t.ldr, t.R1, nullptr, true, st), "path prior");
  HCK(launch_path_residual(h->buf.y_dev, V, ldw, n, S, t, st), "path residual");
  HCK(gemm_call(h, E, 0, 1, {t.R1, t.ldr}, {h->buf.Z_dev, h->buf.lda}, {t.R2, t.ldr}, 1, h->ntc, h->np, 0, 4, 1.0, 0.0, 1), "R^T U");
  HCK(gemm_call(h, E, 0, 0, {t.R2, t.ldr}, {h->buf.Z_dev, h->buf.lda}, {t.R1, t.ldr}, 1, h->ntc, h->np, 0, 1, 1.0, 0.0, 1), "R^T U U^T");
  HCK(launch_path_scatter(V, ldw, n, S, t, st), "path weights");
  return 0;
}

int path_sweep(mi_gp_handle* h, const double* Xnew_dev, int m, double* block_dev, long ldw, double* mean_dev, int condition,
               double* dmean_dev) {
  static const char* entry = "mi_gp_predict_grad under option 54 >= 1 (the path sweep)";
  const int S = h->npaths, F = h->nfeat, d = h->cfg.d;
  if (int r = refuse_plain_model(h, entry)) return r;
  if (!h->have_data || !h->buf.Z_dev || !h->buf.W_dev) return path_refuse(h, "needs Z_dev and W_dev in mi_gp_set_data");
  if (d > PATH_MAX_D) {
    snprintf(h->err, sizeof(h->err), "%s: d <= %d, got %d", entry, PATH_MAX_D, d);
    return -1;
  }
  if (!h->factored) return path_refuse(h, "call mi_gp_factor first");
  if (!block_dev) return path_refuse(h, "work_dev, the path block, is required");
  if (ldw < S || (ldw & 1)) return path_refuse(h, "ldw must be even and >= the number of paths");
  if (m < 0 || (m == 0 && !condition)) return path_refuse(h, "m = 0 is the conditioning call alone (pred_noise = 1); m >= 1 otherwise");
  if (m > 0 && !Xnew_dev) return path_refuse(h, "Xnew_dev is required with m >= 1");
  if (m > 0 && !mean_dev && !dmean_dev) return path_refuse(h, "at least one of mean_dev and dmean_dev is required");
  HCK(hipSetDevice(h->device), "hipSetDevice");
  if (int r = make_u_resident(h)) return r;
  if (int r = ensure_block(h, BLK_PATH, path_scratch_len(h->cap, d, F), "path sweep scratch")) return r;
  const PathScratch t = path_scratch(h->blocks[BLK_PATH].p, h->blocks[BLK_PATH].cap, d, F);
  // the path block: Omega [F][d], b [F], W [F][ldw], V [n][ldw]
  const double* Om = block_dev;
  const double* bph = Om + (size_t)F * d;
  double* W = block_dev + (size_t)F * d + F;
  double* V = W + (size_t)F * ldw;
  HCK(launch_path_stage(h->spec, h->one.theta_dev, h->buf.X_dev, h->n, Om, W, ldw, F, S, t, h->stream), "path stage");
  if (condition)
    if (int r = path_condition(h, t, bph, V, ldw)) return r;
  if (m > 0) {
    HCK(launch_path_stage_v(V, ldw, h->n, S, t, h->stream), "path stage V");
    HCK(launch_path_sweep(h->spec, h->one.theta_dev, h->n, F, S, bph, t, Xnew_dev, m, m, mean_dev, dmean_dev, false, h->stream),
        "path_sweep");
  }
  HCK(hipStreamSynchronize(h->stream), "stream sync");
  return 0;
}
