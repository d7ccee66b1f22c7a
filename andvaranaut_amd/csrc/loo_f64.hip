// Kernels of the leave-one-out objective (option 48 of mi_gp_set_option, api_loo.hip): from the resident P = K^-1 (lower triangle
// of W) and alpha = P y they build, with p_i = P_ii,
//   logp_i = 1/2 log p_i - 1/2 alpha_i^2 / p_i - 1/2 log 2 pi     (mi_gp_kfold's singleton density)
//   e_i = alpha_i / p_i,  s_i = sqrt((1 + alpha_i^2 / p_i) / p_i),  q_i = e_i / s_i
//   B = P diag(s)  (full np x np, zeros in the padding),  w = P e = B q
//   G' = -(alpha w^T + w alpha^T)  over the lower 128 x 128 tiles (the GEMM adds B B^T to it)
// so that dL_LOO/dtheta_k = -1/2 sum_ij G'_ij dK_ij/dtheta_k: the LML gradient's contraction with a zero alpha vector.
// Everything is memory-bound; every sum runs in a fixed order.
#include <cmath>
#include "migp_kernels.h"

namespace migp {

constexpr int LT = 64;  // tile of the mirror / rank-2 kernels

// One workgroup: thread t takes the points t, t + 256, ... in order, the 256 partial sums meet in a fixed tree.
// scal[0] = sum_i logp_i, scal[1] = 1-based index of the first p_i that is not a positive finite number (0: none); such a point
// gets logp = -inf and zero weights.
__global__ __launch_bounds__(256) void loo_weights_kernel(const double* __restrict__ W, long ld, const double* __restrict__ alpha,
                                                          int n, double* __restrict__ e, double* __restrict__ s,
                                                          double* __restrict__ q, double* __restrict__ logp,
                                                          double* __restrict__ scal) {
  const int t = threadIdx.x;
  double acc = 0.0;
  int first = 0x7fffffff;
  for (int i = t; i < n; i += 256) {
    const double k = W[(long)i * ld + i], a = alpha[i];
    const bool ok = k > 0.0 && k < INFINITY;
    const double v = 1.0 / k;
    const double lp = ok ? 0.5 * log(k) - 0.5 * a * a * v - 0.5 * LOG_2PI : -INFINITY;
    const double ei = a * v, si = sqrt((1.0 + a * a * v) * v);
    e[i] = ok ? ei : 0.0;
    s[i] = ok ? si : 0.0;
    q[i] = ok ? ei / si : 0.0;
    logp[i] = lp;
    acc += lp;
    if (!ok && i < first) first = i;
  }
  tree_sum_first_256(acc, first);
  if (t == 0) {
    scal[0] = acc;
    scal[1] = first == 0x7fffffff ? 0.0 : (double)(first + 1);
  }
}

// Workgroup (bj, bi): the 64 x 64 tile of B at tile row bi, tile column bj.  Its source is the tile (max, min) of the LOWER
// triangle of W, read row by row into LDS (512 B per wave load) and taken out straight (bi > bj), transposed (bi < bj) or
// mirrored about its diagonal (bi = bj: the strict upper triangle of W is scratch and is not read).  Rows of 65 doubles: the
// transposed read's lanes land on distinct bank pairs.
__global__ __launch_bounds__(256) void loo_scale_mirror_kernel(const double* __restrict__ W, long ldw, const double* __restrict__ s,
                                                               int n, double* __restrict__ B, long ldb) {
  __shared__ double T[LT][LT + 1];
  const int bj = blockIdx.x, bi = blockIdx.y;
  const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
  const int hi = bi > bj ? bi : bj, lo = bi > bj ? bj : bi;
  const double* src = W + (long)hi * LT * ldw + (long)lo * LT;
  for (int r = r0; r < LT; r += 4) T[r][c] = (hi != lo || c <= r) ? src[(long)r * ldw + c] : 0.0;
  __syncthreads();
  const int j = bj * LT + c;
  const double sj = j < n ? s[j] : 0.0;
  double* dst = B + (long)bi * LT * ldb + (long)bj * LT;
  for (int r = r0; r < LT; r += 4) {
    const int i = bi * LT + r;
    const double p = bi > bj ? T[r][c] : bi < bj ? T[c][r] : (r >= c ? T[r][c] : T[c][r]);
    dst[(long)r * ldb + c] = (i < n && j < n) ? p * sj : 0.0;
  }
}

// w[i] = sum_{k < n} B[i][k] q[k] for the rows i < n: one wave per row, lane l takes k = l, l + 64, ... in order, then the
// wave's fixed shuffle tree.
__global__ __launch_bounds__(256) void loo_gemv_kernel(const double* __restrict__ B, long ld, const double* __restrict__ q, int n,
                                                       double* __restrict__ w) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  const double* b = B + (long)row * ld;
  double acc = 0.0;
  for (int k = lane; k < n; k += 64) acc += b[k] * q[k];
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane == 0) w[row] = acc;
}

// G'[i][j] = -(alpha_i w_j + w_i alpha_j) over every 128 x 128 tile on or below the block diagonal of G (whole tiles: the GEMM
// behind it reads and writes whole tiles), zeros in the padding.  Workgroup (bj, bi) = one 64 x 64 tile.
__global__ __launch_bounds__(256) void loo_rank2_init_kernel(const double* __restrict__ alpha, const double* __restrict__ w, int n,
                                                             double* __restrict__ G, long ld) {
  const int bj = blockIdx.x, bi = blockIdx.y;
  if ((bj >> 1) > (bi >> 1)) return;
  const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
  const int j = bj * LT + c;
  const bool jl = j < n;
  const double aj = jl ? alpha[j] : 0.0, wj = jl ? w[j] : 0.0;
  for (int r = r0; r < LT; r += 4) {
    const int i = bi * LT + r;
    const bool live = jl && i < n;
    const double ai = live ? alpha[i] : 0.0, wi = live ? w[i] : 0.0;
    G[(long)i * ld + j] = live ? -(ai * wj + wi * aj) : 0.0;
  }
}

hipError_t launch_loo_weights(const double* W, long ld, const double* alpha, int n, double* e, double* s, double* q, double* logp,
                              double* scal, hipStream_t stream) {
  loo_weights_kernel<<<1, 256, 0, stream>>>(W, ld, alpha, n, e, s, q, logp, scal);
  return hipGetLastError();
}

hipError_t launch_loo_scale_mirror(const double* W, long ldw, const double* s, int n, int np, double* B, long ldb,
                                   hipStream_t stream) {
  loo_scale_mirror_kernel<<<dim3(np / LT, np / LT), 256, 0, stream>>>(W, ldw, s, n, B, ldb);
  return hipGetLastError();
}

hipError_t launch_loo_gemv(const double* B, long ld, const double* q, int n, double* w, hipStream_t stream) {
  loo_gemv_kernel<<<(n + 3) / 4, 256, 0, stream>>>(B, ld, q, n, w);
  return hipGetLastError();
}

hipError_t launch_loo_rank2_init(const double* alpha, const double* w, int n, int np, double* G, long ld, hipStream_t stream) {
  loo_rank2_init_kernel<<<dim3(np / LT, np / LT), 256, 0, stream>>>(alpha, w, n, G, ld);
  return hipGetLastError();
}

}  // namespace migp
