// Host side of the mean sweep (option 53 of mi_gp_set_option; include/mi_gp.h has the contract, sweep_f64.hip the kernels):
// mi_gp_predict_grad under option 53 = 1.  Linked weakly from api_gp.hip (gp_handle.h), as api_loo.hip is.
#include "gp_handle.h"

static int sweep_refuse(mi_gp_handle* h, const char* why) {
  snprintf(h->err, sizeof(h->err), "mi_gp_predict_grad under option 53 = 1 (the mean sweep): %s", why);
  return -1;
}

int mean_sweep(mi_gp_handle* h, const double* Xnew_dev, int m, double* mean_dev, double* dmean_dev) {
  static const char* entry = "mi_gp_predict_grad under option 53 = 1 (the mean sweep)";
  if (int r = refuse_plain_model(h, entry)) return r;
  if (!h->have_data || !h->buf.Z_dev || !h->buf.W_dev) return sweep_refuse(h, "needs Z_dev and W_dev in mi_gp_set_data");
  if (h->cfg.d > SWEEP_MAX_D) {
    snprintf(h->err, sizeof(h->err), "%s: d <= %d, got %d", entry, SWEEP_MAX_D, h->cfg.d);
    return -1;
  }
  if (!h->factored) return sweep_refuse(h, "call mi_gp_factor first");
  if (!Xnew_dev || m <= 0) return sweep_refuse(h, "Xnew_dev and m >= 1 are required");
  if (!mean_dev && !dmean_dev) return sweep_refuse(h, "at least one of mean_dev and dmean_dev is required");
  HCK(hipSetDevice(h->device), "hipSetDevice");
  if (int r = make_u_resident(h)) return r;
  if (int r = ensure_block(h, BLK_SWEEP, sweep_scratch_len(h->cap, h->cfg.d), "mean sweep scratch")) return r;
  HCK(launch_mean_sweep(h->spec, h->one.theta_dev, h->buf.X_dev, h->n, Xnew_dev, m, h->one.alpha_dev, h->blocks[BLK_SWEEP].p, mean_dev,
                        dmean_dev, h->stream), "mean_sweep");
  HCK(hipStreamSynchronize(h->stream), "stream sync");
  return 0;
}
