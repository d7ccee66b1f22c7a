#ifndef MI_GP_DERIV_H
#define MI_GP_DERIV_H
#include "mi_gp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Gradient observations (gradient-enhanced kriging; Rasmussen & Williams 9.4): the C-ABI of libmi_gp_deriv.so, a library beside
 * libmi_gp.so that is linked from the same objects, exports the same entry points (include/mi_gp.h: the same code, the same bits
 * on a handle without a binding) and three more.
 *
 * A joint GP over f and grad f.  One stationary component k(s), s = sum_m a_m dl_m^2, a_m = l_m^-2, dl = x_i - x_j, with
 * r = sqrt(s + 1e-12) inside Matern and theta = [l(d), kv, alpha, gv, jitter] as in include/mi_gp.h.  With k1, k2, k3 the first
 * three derivatives of k by s:
 *   cov(f_i, f_j)            = kv k
 *   cov(d_c f_i, f_j)        =  2 kv k1 a_c dl_c            cov(f_i, d_c' f_j) = -2 kv k1 a_c' dl_c'
 *   cov(d_c f_i, d_c' f_j)   = kv (-4 k2 a_c a_c' dl_c dl_c' - 2 k1 a_c [c = c'])
 *   RBF: k_m = (-1/2)^m k.   Matern-5/2: k1 = -(5/6)(1 + sqrt5 r) e^(-sqrt5 r), k2 = (25/12) e^(-sqrt5 r),
 *                                        k3 = -(25 sqrt5 / 24) e^(-sqrt5 r) / r.
 * The observation vector is [y ; G[:,0] ; .. ; G[:,d-1]]: row a = c n + i holds component c (0: the value, c >= 1: d f / d x_c) at
 * point i, N = n (1 + d).  The diagonal: value rows get theta's gv and jitter as the noise_form of include/mi_gp.h says, derivative
 * rows the jitter alone, and mi_gp_set_diag's vector (N doubles under a binding) is added to both: a fixed gradient-noise variance
 * goes there.  d/dgv counts the value rows only.
 * d/dl_p = (-2 a_p / l_p) d/da_p with
 *   dK00/da_p  = kv k1 dl_p^2
 *   dKc0/da_p  = 2 kv dl_c (k2 dl_p^2 a_c + k1 [c = p])                        (K0c' by antisymmetry)
 *   dKcc'/da_p = kv (-4 k3 dl_p^2 a_c a_c' dl_c dl_c' - 4 k2 dl_c dl_c' (a_c' [c = p] + a_c [c' = p])
 *                    - 2 k2 dl_p^2 a_c [c = c'] - 2 k1 [c = c' = p])
 * and d/dkv = K~ / kv (without the diagonal terms).  dl and s are formed directly from the coordinates, never from the expansion
 * |x|^2 + |x'|^2 - 2 x.x': the derivative blocks are proportional to dl. */

/* Binds the handle to gradient observations at npts points: mi_gp_create's n must be npts (1 + d), with one component that is RBF
 * (kernel id 0) or Matern-5/2 (1), d <= 32 and every mode option (48-57) at its default.  From then on X_dev of mi_gp_set_data holds
 * npts x d, y_dev the N observations in the layout above, and mi_gp_lml, mi_gp_lml_grad, mi_gp_lml_parts, mi_gp_factor,
 * mi_gp_predict (the VALUE at new points; the prior variance is kv), mi_gp_set_diag and mi_gp_set_data work on the joint
 * covariance: the same factorisation, solves and reductions behind another assembly, contraction and cross-covariance.  Every
 * other entry point that takes the handle, and mi_gp_set_option of a mode option away from its default, returns -1 before any
 * device call with a text that names mi_gp_deriv_bind, the handle unchanged.  npts = 0 unbinds.  Every successful call ends the
 * resident state like mi_gp_set_data; a refused one changes nothing.  Makes no HIP call.
 * Returns 0, or -1 with the text behind mi_gp_last_error. */
MI_GP_API int mi_gp_deriv_bind(mi_gp_handle* h, int npts);

/* Block-level: the covariance of the components of X1 (n1 x d, comp1 components: 1 or 1 + d) with those of X2 (n2 x d, comp2), for
 * kernel_id 0 or 1 and d <= 32, into K_dev (rows ldk apart, ldk even).  sym = 1 (X2 = X1, comp2 = comp1): the lower 64x64 tiles with
 * the diagonal above (noise_form 0 marginal, 1 conditional, 2 explicit; extra_diag_dev: N1 doubles or NULL) and the identity in
 * the padding up to rows_pad = cols_pad; sym = 0: the full rows_pad x cols_pad rectangle, zeros in the padding, no diagonal.
 * rows_pad / cols_pad: multiples of 64 that cover n1 comp1 / n2 comp2.  Asynchronous on `stream`.
 * Returns 0, -1 (text behind mi_gp_last_global_error) or -2. */
MI_GP_API int mi_gp_deriv_assemble(int d, int kernel_id, const double* theta_dev, const double* X1_dev, int n1, int comp1,
                                   const double* X2_dev, int n2, int comp2, double* K_dev, long ldk, int rows_pad, int cols_pad,
                                   int sym, int noise_form, const double* extra_diag_dev, void* stream);

/* Block-level: grad_dev[d + 4] = 1/2 sum_ab (alpha_a alpha_b - W_ab) dK~_ab/dtheta over the N = npts (1 + d) observations, from the
 * LOWER triangle of W_dev (rows ldw apart) and alpha_dev[N], in mi_gp_lml_grad's parameter order (the alpha slot receives 0).
 * part_dev: scratch of part_len >= T (T + 1) / 2 * (d + 4) doubles, T = ceil(N / 64).  One 64x64 tile of W per workgroup, the
 * tiles' partial sums added in tile order: no atomics on the sums, a repeat returns the same bits.  Asynchronous on `stream`.
 * Returns 0, -1 (text behind mi_gp_last_global_error) or -2. */
MI_GP_API int mi_gp_deriv_contract(int d, int kernel_id, const double* theta_dev, const double* X_dev, int npts, const double* W_dev,
                                   long ldw, const double* alpha_dev, double* part_dev, long part_len, double* grad_dev,
                                   void* stream);

#ifdef __cplusplus
}
#endif
#endif
