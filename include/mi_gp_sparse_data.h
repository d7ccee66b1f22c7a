#ifndef MI_GP_SPARSE_DATA_H
#define MI_GP_SPARSE_DATA_H
#include "mi_gp_sparse.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Data-side gradients of the sparse inducing-point bound: the C-ABI of libmi_gp_sparse_data.so, a library beside
 * libmi_gp_sparse.so that is linked from the same objects, exports the same eight entry points (include/mi_gp_sparse.h: the same
 * code, the same bits) and one more.  With dF/dy and dF/dX the bound can be pulled back onto whatever produced the data: the
 * parameters of input and output warps that are fitted with the hyper-parameters, as mi_gp_alpha and mi_gp_grad_x
 * (include/mi_gp.h) serve the dense log marginal likelihood.
 * The notation is that of include/mi_gp_sparse.h.  Every base kernel is stationary, so kdiag and kappa do not depend on X, and
 *   dF/dy_i  = -y_i / s + sum_u K(x_i, z_u) t_u,   t = L^-T a^ / s
 *            = -y_i / s + (A_c^T a^)_i / s                                    (the same number from the chunk's resident rows)
 *   dF/dx_id = sum_u w_iu sum_c coef_c(i,u) kv_c k_c'(r2_c(i,u)) 2 (x_id - z_ud) / l_cd^2,   w_iu = T_c^T[i][u] + y_i t_u
 * with r2 in the direct form: x_i = z_u gives a zero term exactly.  w is the weight the theta contraction and dF/dZ's kernel read.
 * Both are steps of pass 2, per chunk behind the contraction.  dF/dy is one small kernel on the rows A_c^T, every row's sum in a
 * fixed order.  dF/dX is dF/dZ's kernel with the two sets exchanged: workgroup (rb, sl) of a grid (ceil(cnt / 64), slabs) owns
 * 64 data points of the chunk and walks the 64-column blocks of Z sl, sl + slabs, ...; each slab's partial goes to scratch and a
 * reduction writes the slabs' sum in slab order.  A data row belongs to one chunk: nothing is summed across chunks, the
 * reduction overwrites.  slabs = min(column blocks of m, xgrad_slabs, ceil(1024 / row blocks of the chunk)), lowered until the
 * slab scratch is at most 64 MB: a function of (chunk's points, m, d, xgrad_slabs) alone.  No atomics; the bits of dF/dX depend
 * on (Z, X, y, theta, chunk, slabs) and nothing else; another slab count regroups sums.  The slab scratch is an allocation of the
 * object's own, made by the first gradient call that needs it. */

/* binds device outputs for the data-side gradients: every later mi_gp_sparse_bound_grad with a non-null grad_out also writes
 * dF/dy into gy_dev[n] and, if gx_dev is non-null, dF/dX into gx_dev[n x d] (row-major).  gy_dev == NULL unbinds (gx_dev must
 * then be NULL).  xgrad_slabs >= 1 caps the slabs of the X kernel (as zgrad_slabs does for Z); < 1 is refused.  Makes no HIP
 * call before the next mi_gp_sparse_set_data / bound_grad; survives set_data.  A bad pivot zeroes both outputs.
 * F, dF/dtheta and dF/dZ are bit for bit what they are without a binding; a null grad_out (the value only) writes nothing.
 * Returns 0, or -1 with the text behind mi_gp_sparse_last_error. */
MI_GP_API int mi_gp_sparse_bind_data_grad(mi_gp_sparse* s, double* gy_dev, double* gx_dev, int xgrad_slabs);

#ifdef __cplusplus
}
#endif
#endif
