// Exact k-fold cross-validation from the resident K^-1 (mi_gp_kfold, api_kfold.hip).  For a fold I the hold-out predictive of
// the noisy observations given every other point is Sigma_I = (K^-1_II)^-1, y_I - mu_I = Sigma_I alpha_I.  The kernels here
// gather K^-1_II out of the lower triangle of W into a 128 x 128 block per fold (the leaf of leaf_f64.hip factorises the blocks
// of a pass, one workgroup per fold) and turn the leaf's C = chol(K^-1_II) and M = C^-1 into the fold's moments and density;
// leave-one-out has a closed form and a kernel of its own.
#include <cmath>
#include "migp_kernels.h"

namespace migp {

// Workgroup (f, g): rows 16 g .. 16 g + 15 of fold f0 + f's block: element (a, b) = W[max(i_a, i_b)][min(i_a, i_b)] -- never the
// strict upper triangle of W, which is scratch -- and the identity in the padding.  Group 0 also gathers alpha_I and y_I (zeros in
// the padding) and resets the fold's bad-pivot word.
__global__ __launch_bounds__(256) void kfold_gather_kernel(const double* __restrict__ W, long ld, const double* __restrict__ alpha,
                                                           const double* __restrict__ y, const int* __restrict__ idx,
                                                           const int* __restrict__ ptr, int f0, double* __restrict__ blocks,
                                                           double* __restrict__ vecs, int* __restrict__ info) {
  const int f = blockIdx.x, g = blockIdx.y, t = threadIdx.x;
  const int p0 = ptr[f0 + f], s = ptr[f0 + f + 1] - p0;
  __shared__ int ii[128];
  if (t < 128) ii[t] = t < s ? idx[p0 + t] : -1;
  __syncthreads();
  double* blk = blocks + (long)f * MINV_ELEMS;
  for (int e = t; e < 16 * 128; e += 256) {
    const int a = 16 * g + (e >> 7), b = e & 127;
    double v = a == b ? 1.0 : 0.0;
    if (a < s && b < s) {
      const int ia = ii[a], ib = ii[b];
      v = W[(long)(ia > ib ? ia : ib) * ld + (ia > ib ? ib : ia)];
    }
    blk[a * 128 + b] = v;
  }
  if (g == 0) {
    if (t < 128) {
      vecs[(long)f * 256 + t] = t < s ? alpha[ii[t]] : 0.0;
      vecs[(long)f * 256 + 128 + t] = t < s ? y[ii[t]] : 0.0;
    }
    if (t == 0) info[f0 + f] = INFO_OK;
  }
}

// One workgroup per fold, thread j = position j of the fold.  With C = chol(K^-1_II) in the fold's block and M = C^-1 in minv
// (minv_index order; only the lower triangle is read): t = M alpha_I, r = M^T t = Sigma_I alpha_I, mean = y_I - r,
// var_j = sum_r M[r][j]^2, logp = -1/2 |t|^2 + sum log C_ii - |I|/2 log 2 pi (kfold_fold_logp, migp_kernels.h: the k-fold
// objective's fold kernel returns the same bits through it).  Every sum runs in a fixed order.  A fold whose block was not
// positive definite gets logp = -inf and NaN moments.
__global__ __launch_bounds__(128) void kfold_moments_kernel(const double* __restrict__ blocks, const double* __restrict__ minv,
                                                            const double* __restrict__ vecs, const int* __restrict__ ptr,
                                                            const int* __restrict__ info, int f0, double* __restrict__ logp,
                                                            double* __restrict__ mean, double* __restrict__ var) {
  const int f = blockIdx.x, j = threadIdx.x;
  const int p0 = ptr[f0 + f], s = ptr[f0 + f + 1] - p0;
  if (info[f0 + f] != INFO_OK) {
    if (j == 0) logp[f0 + f] = -INFINITY;
    if (mean != nullptr && j < s) mean[p0 + j] = var[p0 + j] = NAN;
    return;
  }
  const double* C = blocks + (long)f * MINV_ELEMS;
  const double* M = minv + (long)f * MINV_ELEMS;
  const double* al = vecs + (long)f * 256;
  __shared__ double tv[128], s1[128], s2[128];
  const double lp = kfold_fold_logp(C, M, al, j, s, tv, s1, s2);
  if (mean != nullptr && j < s) {
    double r = 0.0, v = 0.0;
    for (int i = j; i < s; ++i) {
      const double m = M[minv_index(i, j)];
      r = __builtin_fma(m, tv[i], r);
      v = __builtin_fma(m, m, v);
    }
    mean[p0 + j] = al[128 + j] - r;
    var[p0 + j] = v;
  }
  if (j == 0) logp[f0 + f] = lp;
}

// Leave-one-out, fold f = the point i = idx[f]: with k = K^-1_ii, var = 1 / k, mean = y_i - alpha_i / k,
// logp = 1/2 log k - 1/2 alpha_i^2 / k - 1/2 log 2 pi; k <= 0 (or NaN): info 1, logp = -inf, NaN moments.
__global__ __launch_bounds__(256) void kfold_loo_kernel(const double* __restrict__ W, long ld, const double* __restrict__ alpha,
                                                        const double* __restrict__ y, const int* __restrict__ idx, int nfolds,
                                                        double* __restrict__ logp, double* __restrict__ mean, double* __restrict__ var,
                                                        int* __restrict__ info) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= nfolds) return;
  const int i = idx[f];
  const double k = W[(long)i * ld + i], a = alpha[i];
  const bool ok = k > 0.0;
  const double v = 1.0 / k;
  info[f] = ok ? 0 : 1;
  logp[f] = ok ? 0.5 * log(k) - 0.5 * a * a * v - 0.5 * LOG_2PI : -INFINITY;
  if (mean != nullptr) {
    mean[f] = ok ? y[i] - a * v : NAN;
    var[f] = ok ? v : NAN;
  }
}

hipError_t launch_kfold_gather(const double* W, long ld, const double* alpha, const double* y, const int* idx, const int* ptr, int f0,
                               int nf, double* blocks, double* vecs, int* info, hipStream_t stream) {
  kfold_gather_kernel<<<dim3(nf, 8), 256, 0, stream>>>(W, ld, alpha, y, idx, ptr, f0, blocks, vecs, info);
  return hipGetLastError();
}

hipError_t launch_kfold_moments(const double* blocks, const double* minv, const double* vecs, const int* ptr, const int* info, int f0,
                                int nf, double* logp, double* mean, double* var, hipStream_t stream) {
  kfold_moments_kernel<<<nf, 128, 0, stream>>>(blocks, minv, vecs, ptr, info, f0, logp, mean, var);
  return hipGetLastError();
}

hipError_t launch_kfold_loo(const double* W, long ld, const double* alpha, const double* y, const int* idx, int nfolds, double* logp,
                            double* mean, double* var, int* info, hipStream_t stream) {
  kfold_loo_kernel<<<(nfolds + 255) / 256, 256, 0, stream>>>(W, ld, alpha, y, idx, nfolds, logp, mean, var, info);
  return hipGetLastError();
}

}  // namespace migp
