// Appending k <= 128 points to a resident conditional-form factorisation (mi_gp_append, api_gp.hip).  The O(n^2 k) bulk --
// K21, L21 = K21 L11^-T, the partial products of L21 L21^T, U11 L21^T -- runs on the existing assembly, strip-solve and GEMM
// kernels; the kernels here handle the appended 128 x 128 tile: the Schur complement S and the right-hand side of beta2 in
// front of the leaf, the scalar increments behind it, the new rows of L / U in place, and the rebuilt diagonal-block inverses.
#include <cmath>
#include "migp_kernels.h"

namespace migp {

// Block b (of 128): row b of S -= sum over the nparts partial products (in part order), lower part only; and
// r[b] = y2[b] - L21[b, :] . beta1 (b < k; 0 in the padding) into row 128 of the S block.
__global__ __launch_bounds__(256) void append_schur_kernel(double* __restrict__ S, const double* __restrict__ parts, int nparts,
                                                           const double* __restrict__ L21, long ldw,
                                                           const double* __restrict__ beta1, int np, const double* __restrict__ y2,
                                                           int k) {
  const int b = blockIdx.x, t = threadIdx.x;
  if (t <= b && t < 128) {
    double acc = 0.0;
    for (int s = 0; s < nparts; ++s) acc += parts[(long)s * MINV_ELEMS + b * 128 + t];
    S[b * 128 + t] -= acc;
  }
  __shared__ double red[256];
  double a = 0.0;
  if (b < k)
    for (int c = t; c < np; c += 256) a = __builtin_fma(L21[(long)b * ldw + c], beta1[c], a);
  red[t] = a;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t == 0) S[128 * 128 + b] = b < k ? y2[b] - red[0] : 0.0;
}

// stats[0] = sum log L22_ii, stats[1] = |beta2|^2 over the k appended entries, stats[2] = the bad-pivot word (as a double)
__global__ void append_stats_kernel(const double* __restrict__ S, int k, const int* __restrict__ info, double* __restrict__ stats) {
  __shared__ double s1[128], s2[128];
  const int t = threadIdx.x;
  const double d = t < k ? S[t * 129] : 1.0, bv = t < k ? S[128 * 128 + t] : 0.0;
  s1[t] = log(d);
  s2[t] = bv * bv;
  __syncthreads();
  for (int w = 64; w > 0; w >>= 1) {
    if (t < w) { s1[t] += s1[t + w]; s2[t] += s2[t + w]; }
    __syncthreads();
  }
  if (t == 0) { stats[0] = s1[0]; stats[1] = s2[0]; stats[2] = (double)info[0]; }
}

// New beta row at row np_new of K: beta1 (columns < n, read from row np_old), beta2 (columns n .. n + k - 1, row 128 of the
// S block), zeros up to np_new; when the factor grew by a tile the 127 rows below it are zeroed too (the y^T block's layout).
// (np_new == np_old: the row is read and written element by element by the same thread.)
__global__ void append_beta_kernel(double* __restrict__ K, long ld, int np_old, int np_new, int n, int k, const double* __restrict__ S) {
  const int rows = np_new > np_old ? 128 : 1;
  const long total = (long)rows * np_new;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int r = (int)(e / np_new), c = (int)(e % np_new);
    double v = 0.0;
    if (r == 0) v = c < n ? K[(long)np_old * ld + c] : c < n + k ? S[128 * 128 + (c - n)] : 0.0;
    K[(long)(np_new + r) * ld + c] = v;
  }
}

// Rows [n, row_end) of K over columns [0, np_new): appended row p = i - n is [L21[p, :n], L22[p, :p + 1], 0 ...];
// rows beyond n + k (the padding of a new tile) are identity rows.
__global__ void append_rows_kernel(double* __restrict__ K, long ld, int n, int k, int row_end, int np_new,
                                   const double* __restrict__ L21, long ldw, const double* __restrict__ S) {
  const long total = (long)(row_end - n) * np_new;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int i = n + (int)(e / np_new), c = (int)(e % np_new);
    const int p = i - n;
    double v;
    if (p < k) v = c < n ? L21[(long)p * ldw + c] : c <= i ? S[p * 128 + (c - n)] : 0.0;
    else v = c == i ? 1.0 : 0.0;
    K[(long)i * ld + c] = v;
  }
}

// Inverse of the lower-triangular 128 x 128 tile T (rows ldt apart), rows [i0, 128) by forward substitution: rows < i0 are
// those of the resident inverse (inv([A 0; B C]) = [A^-1 0; -C^-1 B A^-1  C^-1]).  One workgroup per column j (blockIdx.y:
// tile; rows [i0_first, 128) of the first, all rows of a second), the dot product of a row split over the wave.  plain == 0: out in the strip kernel's operand order (minv_index,
// zeros above the diagonal); plain == 1: row-major 128 x 128, i0 must be 0.
__global__ __launch_bounds__(64) void tile_inverse_rows_kernel(const double* __restrict__ T, long ldt, long sT, double* __restrict__ out,
                                                               long sout, int i0_first, int plain) {
  T += blockIdx.y * sT;
  out += blockIdx.y * sout;
  const int i0 = blockIdx.y == 0 ? i0_first : 0;  // (a second tile is a new one: no resident rows)
  const int j = blockIdx.x, lane = threadIdx.x;
  __shared__ double x[128];
  for (int l = lane; l < 128; l += 64) x[l] = l < i0 ? out[plain ? l * 128 + j : minv_index(l, j)] : 0.0;
  __syncthreads();
  for (int i = i0 < j ? j : i0; i < 128; ++i) {
    double a = 0.0;
    for (int l = j + lane; l < i; l += 64) a = __builtin_fma(T[(long)i * ldt + l], x[l], a);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    if (lane == 0) x[i] = ((i == j ? 1.0 : 0.0) - a) / T[(long)i * ldt + i];
    __syncthreads();
  }
  for (int l = lane; l < 128; l += 64)  // (the resident rows l < i0 stay as they are)
    if (l >= i0) out[plain ? l * 128 + j : minv_index(l, j)] = l < j ? 0.0 : x[l];
}

// U = L^-T grown by the appended points: columns [n, np_new) of every row r < np_new -- U12 = -U11 L21^T U22 (r < n, from
// Qt = -L22^-1 L21 U11^T, row p = column n + p), U22 = L22^-T (upper), identity in the padding -- and, when a tile was added,
// zeros in columns [0, n) of its rows.
__global__ void append_u_kernel(double* __restrict__ Z, long ld, int n, int k, int np_old, int np_new, const double* __restrict__ Qt,
                                long ldw, const double* __restrict__ Linv22) {
  const int wc = np_new - n;
  const long total_a = (long)np_new * wc;
  const long total_b = np_new > np_old ? (long)(np_new - np_old) * n : 0;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total_a + total_b; e += (long)gridDim.x * blockDim.x) {
    if (e < total_a) {
      const int r = (int)(e / wc), c = n + (int)(e % wc);
      const int q = c - n;
      double v;
      if (r < n) v = q < k ? Qt[(long)q * ldw + r] : 0.0;
      else if (r < n + k) v = (q < k && c >= r) ? Linv22[q * 128 + (r - n)] : 0.0;
      else v = c == r ? 1.0 : 0.0;
      Z[(long)r * ld + c] = v;
    } else {
      const long f = e - total_a;
      Z[(long)(np_old + f / n) * ld + f % n] = 0.0;
    }
  }
}

static int grid_for(long total) {
  long b = (total + 255) / 256;
  return (int)(b < 1 ? 1 : b > 4096 ? 4096 : b);
}

hipError_t launch_append_schur(double* S, const double* parts, int nparts, const double* L21, long ldw, const double* beta1, int np,
                               const double* y2, int k, hipStream_t stream) {
  append_schur_kernel<<<128, 256, 0, stream>>>(S, parts, nparts, L21, ldw, beta1, np, y2, k);
  return hipGetLastError();
}

hipError_t launch_append_stats(const double* S, int k, const int* info, double* stats, hipStream_t stream) {
  append_stats_kernel<<<1, 128, 0, stream>>>(S, k, info, stats);
  return hipGetLastError();
}

hipError_t launch_append_commit(double* K, long ld, int n, int k, int np_old, int np_new, const double* L21, long ldw, const double* S,
                                hipStream_t stream) {
  append_beta_kernel<<<grid_for((long)(np_new > np_old ? 128 : 1) * np_new), 256, 0, stream>>>(K, ld, np_old, np_new, n, k, S);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int row_end = np_new > np_old ? np_new : n + k;
  append_rows_kernel<<<grid_for((long)(row_end - n) * np_new), 256, 0, stream>>>(K, ld, n, k, row_end, np_new, L21, ldw, S);
  return hipGetLastError();
}

hipError_t launch_tile_inverse_rows(const double* T, long ldt, long sT, double* out, long sout, int i0_first, int ntiles, int plain,
                                    hipStream_t stream) {
  tile_inverse_rows_kernel<<<dim3(128, ntiles), 64, 0, stream>>>(T, ldt, sT, out, sout, i0_first, plain);
  return hipGetLastError();
}

hipError_t launch_append_u(double* Z, long ld, int n, int k, int np_old, int np_new, const double* Qt, long ldw, const double* Linv22,
                           hipStream_t stream) {
  const long total = (long)np_new * (np_new - n) + (np_new > np_old ? (long)(np_new - np_old) * n : 0);
  append_u_kernel<<<grid_for(total), 256, 0, stream>>>(Z, ld, n, k, np_old, np_new, Qt, ldw, Linv22);
  return hipGetLastError();
}

}  // namespace migp
