#ifndef MI_GP_SPARSE_H
#define MI_GP_SPARSE_H
#include "mi_gp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sparse inducing-point bound: the C-ABI of libmi_gp_sparse.so, a library of its own beside libmi_gp.so (include/mi_gp.h), built
 * from the same kernels.  Titsias' collapsed variational bound (SGPR) over m << n inducing points Z, for data sets
 * whose n x n covariance one card cannot hold: the bound F(theta) <= log marginal likelihood, its exact theta gradient and the
 * sparse predictive.  The n data points are streamed in chunks; no n x n and no n x m matrix is ever held.  O(n m^2) on the fp64
 * matrix cores plus O(n m (d + P)) in one contraction kernel, memory O(m^2 + chunk m).
 * theta is the C-ABI's [ls | kv | alpha | gv | jitter].  s = gv + jitter is the noise variance (s > 0 is required),
 * Kuu = K(Z, Z) + jitter I, Kuf = K(Z, X), kdiag the prior variance of mi_gp_predict, kappa = n kdiag.  The B-form:
 *   L = chol(Kuu),  A = L^-1 Kuf (m x n),  Psi = A A^T,  v = A y,  yy = y^T y
 *   B = I + Psi/s = LB LB^T,  c = LB^-1 v / s,  a^ = B^-1 v / s = LB^-T c
 *   F = -n/2 log(2 pi s) - sum log LB_ii - yy/(2s) + |c|^2/2 - (kappa - tr Psi)/(2s)
 *   H = I - B^-1 - a^ a^^T,  T^T = A^T (H L^-1 / s) + y (L^-T a^)^T / s  (= dF/dKuf, transposed: one row per data point)
 *   Guu = -1/2 L^-T (Psi/s - H) L^-1  (= dF/dKuu)
 *   dF/ds = -n/(2s) + yy/(2s^2) + (kappa - tr Psi)/(2s^2) + (m - tr B^-1)/(2s) - (|c|^2 + |a^|^2)/(2s)
 *   dF/dtheta_k = sum_ui T_ui dKuf_ui/dtheta_k + sum_uv Guu_uv dK(Z,Z)_uv/dtheta_k - n/(2s) dkdiag/dtheta_k + [theta_k = gv] dF/ds
 * (Psi = s (B - I) turns tr(B^-1 Psi) and a^^T Psi a^ of the textbook dF/ds into the last two terms: sums of one sign.)
 * The gradient's jitter slot is written as 0: jitter is a constant of the fit, a stabiliser, not a parameter of the bound.
 * Predictive at x*, a* = L^-1 k(Z, x*), b* = LB^-1 a*:  mean = b* . c,  var = kdiag - |a*|^2 + |b*|^2 (+ s with pred_noise).
 *
 * Pass 1 walks the data in chunks of `chunk` points in index order: K(X_c, Z) into chunk work rows, the blocked solve against L,
 * Psi += A_c A_c^T on the GEMM, v and yy in fixed-order sums.  Then the m-sized algebra (both factorisations, L^-T, LB^-T, B^-1 and
 * the m x m products on the GEMM).  Pass 2 (gradient only) rebuilds A_c^T chunk by chunk -- it is never stored --, forms T_c^T with
 * one GEMM and contracts it with dKuf/dtheta in one kernel; Kuu's term goes through the symmetric contraction of mi_gp_lml_grad
 * (include/mi_gp.h).
 * The gradient by the inducing locations (zgrad_slabs >= 1).  Every base kernel is stationary ARD, so kdiag and the jitter on Kuu's
 * diagonal do not depend on Z, and with k_c' = dk_c/dr2 and coef_c the fold's dK/dK_c
 *   dF/dz_ud =   sum_i T_ui sum_c coef_c(i,u) kv_c k_c'(r2_c(i,u)) 2 (z_ud - x_id) / l_cd^2      (Kuf's term)
 *            + 2 sum_v Guu_uv sum_c coef_c(u,v) kv_c k_c'(r2_c(u,v)) 2 (z_ud - z_vd) / l_cd^2    (Kuu's term)
 * with r2 in the direct form: z_u = x_i gives a zero term exactly, despite the 1e-12 under Matern-3/2's and Exponential's root.
 * Kuf's term is one more kernel per chunk of pass 2 on the weights the theta contraction reads (T_c^T and the rank-one part
 * formed in the kernel): workgroup (ub, sl) of a grid (ceil(m / 64), slabs) owns 64 inducing points and walks the chunk's 64-row
 * data blocks sl, sl + slabs, ...; each slab's m x d partial goes to scratch and a reduction adds the slabs in slab order, the
 * first chunk overwriting dF/dZ and later chunks adding to it in chunk order.  slabs = min(row blocks of the chunk, zgrad_slabs,
 * ceil(1024 / column blocks)), lowered until the slab scratch is at most 64 MB: a function of (chunk's points, m, d, zgrad_slabs)
 * alone.  Kuu's term is the kernel of mi_gp_grad_x (include/mi_gp.h) over Z with the weight 2 Guu and a zero alpha.  No atomics;
 * dF/dZ's bits depend on (Z, X, y, theta, chunk, slabs) and nothing else; another slab count regroups sums.  dF/dZ, Kuu's part and
 * the slab scratch live in the object's own allocation (sized by the first mi_gp_sparse_set_data), not in the caller's work block.
 * Z stays a borrowed buffer that every call reads afresh: a caller that overwrites it (an optimiser's step) may evaluate the bound
 * at once, but must call mi_gp_sparse_set_data again before mi_gp_sparse_predict -- that resets the factored state and, after the
 * first time, allocates nothing.
 * Every sum runs in a fixed order and nothing uses atomics: the same call in the same state returns the same bits.  Every element
 * a launch reads is written earlier in the same call: what the work block held before does not matter.  Another chunk size
 * regroups sums: agreement to rounding, not bit for bit.
 * The object owns one stream; every call returns synchronised.  Returns: 0; -1 a bad argument (refused before any HIP call,
 * text in mi_gp_sparse_last_error); -2 a HIP failure; info > 0 a bad pivot -- the 1-based pivot in Kuu, or m + the pivot in B --
 * with F = -inf and a zero gradient; the object stays usable.
 * Limits: 1 <= m <= 2048 (16 tile columns, the widest panel the factorisation uses), m <= n, chunk a multiple of 128 (0: 8192).
 * Replaces nothing of the reference: "Sparse regression for large datasets" is an open item of its to-do list. */
typedef struct mi_gp_sparse mi_gp_sparse;
typedef struct {
  int n, m, d, nkern;
  int kernel_ids[MI_GP_MAX_KERN];
  int ops[MI_GP_MAX_KERN];
  int device;
  int chunk;               /* data points per pass step, a multiple of 128; 0: the default, 8192 */
  int zgrad_slabs;         /* 0: no dF/dZ, every call bit for bit what it is without the field; s >= 1: mi_gp_sparse_bound_grad also
                              writes dF/dZ, its kernel with at most s slabs per chunk (1: one slab walks every row block); < 0 refused */
} mi_gp_sparse_config;
/* validates and records the configuration; makes no HIP call (the stream and the object's small scratch come with the first
 * mi_gp_sparse_set_data).  With a null object the text of a refusal is behind mi_gp_sparse_last_error(NULL). */
MI_GP_API int mi_gp_sparse_create(const mi_gp_sparse_config* cfg, mi_gp_sparse** out);
MI_GP_API int mi_gp_sparse_destroy(mi_gp_sparse* s);
MI_GP_API const char* mi_gp_sparse_last_error(mi_gp_sparse* s);
/* doubles of caller scratch for m inducing points and chunks of `chunk` points (the configured value, not 0):
 * 9 mp^2 + 2 chunk mp + 264 mp with mp = m rounded up to a multiple of 128 -- nine mp x mp blocks (L, Psi, LB, L^-T, LB^-T and
 * four of the gradient's), two blocks of chunk work rows, both sets of leaf inverses and eight vectors.  -1 on a bad argument. */
MI_GP_API long mi_gp_sparse_work(int m, int chunk);
/* binds borrowed fp64 row-major device buffers: X (n x d), y (n), Z (m x d, converted inputs like X) and work_dev (work_len >=
 * mi_gp_sparse_work(m, chunk) doubles, work_len even, the address 16-byte aligned).  n must be the configured n. */
MI_GP_API int mi_gp_sparse_set_data(mi_gp_sparse* s, const double* X_dev, const double* y_dev, int n, const double* Z_dev,
                                    double* work_dev, long work_len);
/* *bound = F(theta) and grad_out[ntheta] = dF/dtheta (theta_host: nkern * d + 2 * nkern + 2 host doubles).  A null grad_out
 * means the value only: pass 1 and the algebra of F alone, and the same bits for F as with the gradient.  With zgrad_slabs >= 1
 * grad_out takes ntheta + m * d doubles: dF/dtheta as without it (the same bits), then dF/dZ row-major (m x d); a bad pivot
 * zeroes both. */
MI_GP_API int mi_gp_sparse_bound_grad(mi_gp_sparse* s, const double* theta_host, double* bound, double* grad_out);
/* the state of the predictive at theta: L, LB, c and both sets of leaf inverses stay in the work block until the next
 * mi_gp_sparse_bound_grad, _factor or _set_data */
MI_GP_API int mi_gp_sparse_factor(mi_gp_sparse* s, const double* theta_host);
/* mean_dev[mq], var_dev[mq] at the mq rows of Xnew_dev behind a successful mi_gp_sparse_factor (-1 without one): two blocked
 * solves on the query rows, in passes of `chunk` rows through the work block, and one reduction.  Xnew_dev, mean_dev and var_dev
 * may be any device-visible address. */
MI_GP_API int mi_gp_sparse_predict(mi_gp_sparse* s, const double* Xnew_dev, int mq, double* mean_dev, double* var_dev, int pred_noise);


#ifdef __cplusplus
}
#endif
#endif
