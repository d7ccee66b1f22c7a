// Host side of the design call (options 56 / 57 of mi_gp_set_option; include/mi_gp.h has the contract, design_f64.hip the kernels):
// mi_gp_predict_cov under option 56 = b >= 1.  Linked weakly from api_gp.hip (gp_handle.h), as api_sweep.hip is.
#include "gp_handle.h"

static int design_refuse(mi_gp_handle* h, const char* why) {
  snprintf(h->err, sizeof(h->err), "mi_gp_predict_cov under option 56 = %d (the design call): %s", h->design_b, why);
  return -1;
}

int design_select(mi_gp_handle* h, const double* Xnew_dev, int m, double* work_dev, long ldw, double* out_dev, double* G_dev, long ldc,
                  int pred_noise) {
  const int b = h->design_b, Mr = h->design_nref, Mc = m - Mr, d = h->cfg.d;
  const long Mcp = ((long)Mc + 127) / 128 * 128, Mrp = ((long)Mr + 127) / 128 * 128;
  if (h->trend != 0) return design_refuse(h, "no form under a trend (option 50): set option 50 to 0 first");
  if (h->nout > 1) return design_refuse(h, "no form under several outputs (option 51): set option 51 to 1 first");
  if (h->diag_dev) return design_refuse(h, "no form under a per-point diagonal (mi_gp_set_diag): remove it first");
  if (!h->factored) return design_refuse(h, "call mi_gp_factor first");
  if (!Xnew_dev || !work_dev || !out_dev) return design_refuse(h, "null buffer (Xnew_dev, work_dev and mean_dev are required)");
  if (m <= 0 || Mc < 1) return design_refuse(h, "m = Mc + Mr with Mc >= 1 candidates in front of the Mr reference points of option 57");
  if (Mcp + Mrp > 0x7fffff80L) return design_refuse(h, "too many points");
  if (ldw < h->np || (ldw & 1)) return design_refuse(h, "ldw must be even and >= padded n");
  if (Mr > 0 && !G_dev) return design_refuse(h, "null buffer (cov_dev is required with option 57 >= 1)");
  if (Mr > 0 && (ldc < Mrp || (ldc & 1))) return design_refuse(h, "ldc must be even and >= ceil(Mr/128)*128");
  HCK(hipSetDevice(h->device), "hipSetDevice");
  if (int r = ensure_block(h, BLK_DESIGN, design_scratch_len(Mc, b), "design scratch")) return r;
  const DesignScratch t = design_scratch(h->blocks[BLK_DESIGN].p, Mc, b);
  const hipStream_t st = h->stream;
  const Eval E = one_eval(h);
  const double* theta = h->one.theta_dev;
  const double* Xr = Xnew_dev + (size_t)Mc * d;
  double* Ar = work_dev + Mcp * ldw;
  // A = L^-1 K(X, .): mi_gp_predict's cross-assembly for both point sets, one blocked solve over the rows of both
  HCK(launch_assemble(h->spec, theta, Xnew_dev, Mc, h->buf.X_dev, h->n, work_dev, ldw, (int)Mcp, h->np, 0, 0, st), "assemble cross");
  if (Mr > 0) HCK(launch_assemble(h->spec, theta, Xr, Mr, h->buf.X_dev, h->n, Ar, ldw, (int)Mrp, h->np, 0, 0, st), "assemble cross");
  HCK(trsm_rec(h, E, work_dev, ldw, (int)(Mcp + Mrp), 0, h->ntc), "trsm");
  // v = var_latent + jitter (+ gv): what K_y's diagonal adds to a new observation's variance
  double kd, gvn;
  predict_scalars(h, pred_noise, &kd, &gvn);
  const double noise = h->one.theta_host[h->spec.nkern * d + 2 * h->spec.nkern + 1] + gvn;
  HCK(launch_predict_reduce(work_dev, ldw, h->buf.K_dev + (long)h->np * h->buf.lda, h->n, Mc, kd, noise, t.mean, t.v, st), "row reduction");
  if (Mr > 0) {  // G = K(C, R) - A_C A_R^T and its rows' sums of squares
    HCK(launch_assemble(h->spec, theta, Xnew_dev, Mc, Xr, Mr, G_dev, ldc, (int)Mcp, (int)Mrp, 0, 0, st), "assemble K(C, R)");
    HCK(gemm_call(h, E, 0, 0, {work_dev, ldw}, {Ar, ldw}, {G_dev, ldc}, (int)(Mcp / 128), (int)(Mrp / 128), h->np, 0, 0, -1.0, 1.0, 1),
        "G update");
    HCK(launch_design_rowsq(G_dev, ldc, Mc, Mr, t.rowsq, st), "row sums");
  }
  // the greedy loop: no host synchronisation, the pivot stays on the device
  for (int step = 0; step < b; ++step)
    HCK(launch_design_step(h->spec, theta, Xnew_dev, Mc, Mr, b, step, work_dev, ldw, h->n, G_dev, ldc, noise, t, out_dev, st), "design step");
  HCK(hipStreamSynchronize(st), "stream sync");
  return 0;
}
