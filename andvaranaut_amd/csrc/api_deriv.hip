// The gradient binding of a GP handle and the block-level access to its two kernels (include/mi_gp_deriv.h; kernels: deriv_f64.hip).
// Linked into libmi_gp_deriv.so alone: gp_sched.hip and api_gp.hip reach the three functions below through weak symbols, at the
// training assembly, the contraction and mi_gp_predict's cross-covariance, and only on a handle whose deriv_npts this file set.
#include "gp_handle.h"
#include "../../include/mi_gp_deriv.h"

hipError_t deriv_assemble_train(mi_gp_handle* h, const Eval& E, int noise_form, hipStream_t st) {
  const int q = 1 + h->cfg.d;
  return launch_assemble_deriv(h->spec.kid[0], h->cfg.d, E.s.theta_dev, h->buf.X_dev, h->deriv_npts, q, h->buf.X_dev, h->deriv_npts, q,
                               E.K, h->buf.lda, h->np, h->np, 1, noise_form, st, h->diag_dev);
}

hipError_t deriv_grad_contract(mi_gp_handle* h, const Eval& E) {
  return launch_grad_contract_deriv(h->spec.kid[0], h->cfg.d, E.s.theta_dev, h->buf.X_dev, h->deriv_npts, E.W, h->buf.lda, E.s.alpha_dev,
                                    E.s.part_dev, E.s.grad_host, h->stream, E.s.lr_sync_dev + E.bt.nb, E.s.out_host + 5, h->eval_seq);
}

// cov(f(x*_p), [f ; grad f](X)): one prediction point per row, zeros in the padding
hipError_t deriv_assemble_cross(mi_gp_handle* h, const double* Xnew_dev, int m, double* work_dev, long ldw, int mp) {
  return launch_assemble_deriv(h->spec.kid[0], h->cfg.d, h->one.theta_dev, Xnew_dev, m, 1, h->buf.X_dev, h->deriv_npts, 1 + h->cfg.d,
                               work_dev, ldw, mp, h->np, 0, 0, h->stream);
}

extern "C" int mi_gp_deriv_bind(mi_gp_handle* h, int npts) {
  if (!h) { set_global_error("mi_gp_deriv_bind: null handle"); return -1; }
  if (npts != 0) {
    const int d = h->cfg.d;
    char why[160] = "";
    if (npts < 0) snprintf(why, sizeof(why), "npts must be >= 0, got %d", npts);
    else if (h->cfg.nkern != 1) snprintf(why, sizeof(why), "one kernel component is required, the handle has %d", h->cfg.nkern);
    else if (h->spec.kid[0] != KID_RBF && h->spec.kid[0] != KID_MATERN52)
      snprintf(why, sizeof(why), "the kernel must be RBF (0) or Matern-5/2 (1), the handle's is %d", h->spec.kid[0]);
    else if (d > DERIV_MAX_D) snprintf(why, sizeof(why), "d <= %d is required, the handle has d = %d", DERIV_MAX_D, d);
    else if ((long)npts * (1 + d) != (long)h->cfg.n)
      snprintf(why, sizeof(why), "the handle's n = %d must be npts (1 + d) = %ld", h->cfg.n, (long)npts * (1 + d));
    else if (h->n != h->cfg.n) snprintf(why, sizeof(why), "the handle has grown by mi_gp_append (n = %d)", h->n);
    else if (!modes_at_default(h)) snprintf(why, sizeof(why), "every mode option (48-57) must be at its default");
    if (why[0]) {
      snprintf(h->err, sizeof(h->err), "mi_gp_deriv_bind: %s", why);
      return -1;
    }
  }
  h->deriv_npts = npts;
  drop_resident(h);  // (as mi_gp_set_data: the factor, U and K^-1 belong to the covariance they were computed for)
  h->have_parts = false;
  return 0;
}

static thread_local char g_why[200];
static int refuse(const char* entry, const char* why) {
  snprintf(g_why, sizeof(g_why), "%s: %s", entry, why);
  set_global_error(g_why);
  return -1;
}
static int launch_failed(const char* entry, hipError_t e) {
  snprintf(g_why, sizeof(g_why), "%s: %s", entry, hipGetErrorString(e));
  set_global_error(g_why);
  return -2;
}

extern "C" int mi_gp_deriv_assemble(int d, int kernel_id, const double* theta_dev, const double* X1_dev, int n1, int comp1,
                                    const double* X2_dev, int n2, int comp2, double* K_dev, long ldk, int rows_pad, int cols_pad,
                                    int sym, int noise_form, const double* extra_diag_dev, void* stream) {
  const char* const me = "mi_gp_deriv_assemble";
  if (d < 1 || d > DERIV_MAX_D) return refuse(me, "1 <= d <= 32");
  if (kernel_id != KID_RBF && kernel_id != KID_MATERN52) return refuse(me, "kernel_id must be 0 (RBF) or 1 (Matern-5/2)");
  if (!theta_dev || !X1_dev || !X2_dev || !K_dev) return refuse(me, "null buffer");
  if (n1 < 1 || n2 < 1 || (comp1 != 1 && comp1 != 1 + d) || (comp2 != 1 && comp2 != 1 + d))
    return refuse(me, "n1, n2 >= 1 and component counts of 1 or 1 + d");
  if (rows_pad < 64 || cols_pad < 64 || rows_pad % 64 || cols_pad % 64 || (long)n1 * comp1 > rows_pad || (long)n2 * comp2 > cols_pad ||
      ldk < cols_pad || (ldk & 1))
    return refuse(me, "rows_pad / cols_pad must be multiples of 64 that cover the components, ldk even and >= cols_pad");
  if (sym && (X1_dev != X2_dev || n1 != n2 || comp1 != comp2 || rows_pad != cols_pad))
    return refuse(me, "sym = 1 takes one point set, component count and padding on both sides");
  if (noise_form < 0 || noise_form > 4) return refuse(me, "noise_form must be 0..4");
  const hipError_t e = launch_assemble_deriv(kernel_id, d, theta_dev, X1_dev, n1, comp1, X2_dev, n2, comp2, K_dev, ldk, rows_pad, cols_pad,
                                             sym ? 1 : 0, noise_form, (hipStream_t)stream, extra_diag_dev);
  return e == hipSuccess ? 0 : launch_failed(me, e);
}

extern "C" int mi_gp_deriv_contract(int d, int kernel_id, const double* theta_dev, const double* X_dev, int npts, const double* W_dev,
                                    long ldw, const double* alpha_dev, double* part_dev, long part_len, double* grad_dev, void* stream) {
  const char* const me = "mi_gp_deriv_contract";
  if (d < 1 || d > DERIV_MAX_D) return refuse(me, "1 <= d <= 32");
  if (kernel_id != KID_RBF && kernel_id != KID_MATERN52) return refuse(me, "kernel_id must be 0 (RBF) or 1 (Matern-5/2)");
  if (!theta_dev || !X_dev || !W_dev || !alpha_dev || !part_dev || !grad_dev) return refuse(me, "null buffer");
  if (npts < 1 || (long)npts * (1 + d) > 2147483647L / 2) return refuse(me, "npts >= 1 and npts (1 + d) < 2^30");
  const int N = npts * (1 + d);
  if (ldw < N) return refuse(me, "ldw must be >= npts (1 + d)");
  if (part_len < (long)grad_contract_blocks(N) * (d + 4)) return refuse(me, "scratch shorter than T (T + 1) / 2 * (d + 4), T = ceil(N / 64)");
  const hipError_t e = launch_grad_contract_deriv(kernel_id, d, theta_dev, X_dev, npts, W_dev, ldw, alpha_dev, part_dev, grad_dev,
                                                  (hipStream_t)stream);
  return e == hipSuccess ? 0 : launch_failed(me, e);
}
