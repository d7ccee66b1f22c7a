// Kernels of the k-fold cross-validation objective (option 49 of mi_gp_set_option, api_loo.hip): the leave-one-out tail of
// loo_f64.hip with diag(s) replaced by a block-diagonal matrix of fold factors.  For the contiguous folds I_f of b points, with
// P = K^-1 (lower triangle of W), C = chol(P_II) and M = C^-1 from the batched leaf (the pass of api_kfold.hip),
//   t = M alpha_I,  tau = |t|^2,  e_I = M^T t  (= Sigma_I alpha_I),  q_I = t / sqrt(1 + tau)
//   R_f = M^T + e t^T / (1 + sqrt(1 + tau))     so that R R^T = Sigma_I + e e^T = 2 dL/dP_II and R q = e
//   B[:, I_f] = Pfull[:, I_f] R_f               (full np x np, zeros in the padding),  w = P e = B q
// and from B on the tail is the leave-one-out one.  The fold kernel is memory-bound; the multiply runs on
// v_mfma_f64_16x16x4_f64 (2 * 128 * np * n flops whatever b is).  Every sum runs in a fixed order.
#include <cmath>
#include "symm_chunk.h"

namespace migp {

// One workgroup per fold, thread j = position j of the fold (kfold_moments_kernel's layout, and its density: kfold_fold_logp).
// Row i of R_f goes to row p0 + i of R (128 columns, zeros from the fold's size on).
__global__ __launch_bounds__(128) void cv_fold_kernel(const double* __restrict__ blocks, const double* __restrict__ minv,
                                                      const double* __restrict__ vecs, const int* __restrict__ ptr,
                                                      const int* __restrict__ info, int f0, double* __restrict__ flogp,
                                                      double* __restrict__ e, double* __restrict__ q, double* __restrict__ R) {
  const int f = blockIdx.x, j = threadIdx.x;
  const int p0 = ptr[f0 + f], s = ptr[f0 + f + 1] - p0;
  double* Rf = R + (long)p0 * 128;
  if (info[f0 + f] != INFO_OK) {
    if (j == 0) flogp[f0 + f] = -INFINITY;
    if (j < s) e[p0 + j] = q[p0 + j] = 0.0;
    for (int i = 0; i < s; ++i) Rf[i * 128 + j] = 0.0;
    return;
  }
  const double* C = blocks + (long)f * MINV_ELEMS;
  const double* M = minv + (long)f * MINV_ELEMS;
  const double* al = vecs + (long)f * 256;
  __shared__ double tv[128], s1[128], s2[128], ev[128];
  const double lp = kfold_fold_logp(C, M, al, j, s, tv, s1, s2);
  const double t = tv[j], root = sqrt(1.0 + s2[0]);
  double r = 0.0;
  if (j < s)
    for (int i = j; i < s; ++i) r = __builtin_fma(M[minv_index(i, j)], tv[i], r);
  ev[j] = r;
  __syncthreads();
  if (j < s) {
    e[p0 + j] = r;
    q[p0 + j] = t / root;
  }
  if (j == 0) flogp[f0 + f] = lp;
  const double ct = t / (1.0 + root);
  for (int i = 0; i < s; ++i) Rf[i * 128 + j] = j < s ? (j >= i ? M[minv_index(j, i)] : 0.0) + ev[i] * ct : 0.0;
}

// One workgroup: thread t takes the folds t, t + 256, ... in order, the 256 partial sums meet in a fixed tree (loo_weights_kernel's
// reduction over folds).
__global__ __launch_bounds__(256) void cv_reduce_kernel(const double* __restrict__ flogp, const int* __restrict__ ptr,
                                                        const int* __restrict__ info, int nfolds, double* __restrict__ scal) {
  const int t = threadIdx.x;
  double acc = 0.0;
  int first = 0x7fffffff;
  for (int f = t; f < nfolds; f += 256) {
    acc += flogp[f];
    if (info[f] != INFO_OK) first = min(first, ptr[f] + info[f]);
  }
  tree_sum_first_256(acc, first);
  if (t == 0) {
    scal[0] = acc;
    scal[1] = first == 0x7fffffff ? 0.0 : (double)first;
  }
}

// Workgroup (g, rb): rows 64 rb .. 64 rb + 63 of B in the columns of fold group g -- as many whole folds as fit 128 columns
// (gb = max(1, 128 / b) * b columns from c0 = g gb; the last group is ragged), which are not aligned to tiles.  The group's factor
// is the block-diagonal matrix of its folds' R_f, so B[rows, c0 .. c0 + cw) = Pfull[rows, c0 .. c0 + cw) blockdiag(R_f): k runs in
// chunks of 32 through LDS (symm_chunk.h), As = the chunk's columns of Pfull for the 64 rows (zeros in the rows from n on and in
// the k padding), Rs = the chunk's rows of the block-diagonal factor.  Every 16-column block is a candidate; one whose folds do
// not meet the chunk adds nothing and is passed over.  Rs has rows of 144 doubles (two k rows of a half-wave's B read 16 bank
// pairs apart).  The group one past the last (np > n) writes the zero columns n .. np - 1.
constexpr int CV_RLD = 144;
__global__ __launch_bounds__(256) void cv_mirror_multiply_kernel(const double* __restrict__ W, long ldw, const double* __restrict__ R,
                                                                 int b, int gb, int ngroups, int n, double* __restrict__ B, long ldb) {
  __shared__ double As[64 * SYMM_ALD];
  __shared__ double Rs[SYMM_KC * CV_RLD];
  const int g = blockIdx.x, i0 = blockIdx.y * 64, t = threadIdx.x;
  if (g == ngroups) {
    const int cw = gridDim.y * 64 - n;
    for (int x = t; x < 64 * cw; x += 256) B[(long)(i0 + x / cw) * ldb + n + x % cw] = 0.0;
    return;
  }
  const int c0 = g * gb, cw = min(gb, n - c0), ncb = (cw + 15) >> 4;
  const int lane = t & 63, wv = t >> 6, l15 = lane & 15, l4 = lane >> 4;
  // this thread's column of Rs: its fold's first column and its column inside the fold
  const int rc = t & 127, rlo = rc / b * b;
  const bool rlive = rc < cw;
  double4_t acc[8];
#pragma unroll
  for (int cb = 0; cb < 8; ++cb) acc[cb] = double4_t{0.0, 0.0, 0.0, 0.0};
  for (int kc = 0; kc < cw; kc += SYMM_KC) {
    symm_stage_chunk(W, ldw, n, i0, c0 + kc, c0 + cw, As);
    for (int x = t; x < SYMM_KC * 128; x += 256) {
      const int kk = x >> 7, k = kc + kk;
      if (rc < ncb * 16)
        Rs[kk * CV_RLD + rc] = (rlive && k < cw && k >= rlo && k < rlo + b) ? R[(long)(c0 + k) * 128 + (rc - rlo)] : 0.0;
    }
    __syncthreads();
    symm_chunk_mfma(As, Rs, CV_RLD, [&](int cb) {
      // the k range of the folds that meet this column block
      const int klo = 16 * cb / b * b, khi = ((16 * cb + 15) / b + 1) * b;
      return cb < ncb && khi > kc && klo < kc + SYMM_KC;
    }, acc);
    __syncthreads();
  }
#pragma unroll
  for (int cb = 0; cb < 8; ++cb) {
    const int col = 16 * cb + l15;
    if (cb < ncb && col < cw) {
#pragma unroll
      for (int r = 0; r < 4; ++r) B[(long)(i0 + 16 * wv + l4 + 4 * r) * ldb + c0 + col] = acc[cb][r];
    }
  }
}

hipError_t launch_cv_fold(const double* blocks, const double* minv, const double* vecs, const int* ptr, const int* info, int f0,
                          int nf, double* flogp, double* e, double* q, double* R, hipStream_t stream) {
  cv_fold_kernel<<<nf, 128, 0, stream>>>(blocks, minv, vecs, ptr, info, f0, flogp, e, q, R);
  return hipGetLastError();
}

hipError_t launch_cv_reduce(const double* flogp, const int* ptr, const int* info, int nfolds, double* scal, hipStream_t stream) {
  cv_reduce_kernel<<<1, 256, 0, stream>>>(flogp, ptr, info, nfolds, scal);
  return hipGetLastError();
}

hipError_t launch_cv_mirror_multiply(const double* W, long ldw, const double* R, int b, int n, int np, double* B, long ldb,
                                     hipStream_t stream) {
  const int gb = (b >= 128 ? 1 : 128 / b) * b, ngroups = (n + gb - 1) / gb;
  cv_mirror_multiply_kernel<<<dim3(ngroups + (np > n ? 1 : 0), np / 64), 256, 0, stream>>>(W, ldw, R, b, gb, ngroups, n, B, ldb);
  return hipGetLastError();
}

}  // namespace migp
