// Device code shared by the kernels that multiply the symmetric K^-1, of which only the LOWER triangle of W is kept, by a thin
// operand on v_mfma_f64_16x16x4_f64 (cv_mirror_multiply_kernel, trend_symm_kernel): 64 rows per workgroup of 256 threads, k in
// chunks of 32 through LDS.  Pfull[i][j] = W[max(i, j)][min(i, j)]; the strict upper triangle of W is scratch and never read.
#pragma once
#include "migp_kernels.h"

namespace migp {

typedef double double4_t __attribute__((ext_vector_type(4)));

// k per chunk, and the doubles between rows of the staged chunk (the 16 rows x 2 k of a half-wave's A read land on 32 distinct
// bank pairs)
constexpr int SYMM_KC = 32, SYMM_ALD = 34;

// As[r * SYMM_ALD + kk] = Pfull[i0 + r][j0 + kk] for the 64 rows r and the 32 columns kk of one chunk, zero where the row is >= n
// or the column >= jend (jend <= n).  The elements on and below the diagonal are read straight, 32 consecutive doubles per row
// of W; those above it are the mirror image and are read along the rows of W again, 64 consecutive doubles per row.  A chunk
// wholly left of the row block takes the first loop alone, one wholly right of it the second; only a chunk that crosses the
// diagonal runs both, each masked to its side.  Every element of As is written once; the caller synchronises.
__device__ __forceinline__ void symm_stage_chunk(const double* __restrict__ W, long ldw, int n, int i0, int j0, int jend,
                                                 double* __restrict__ As) {
  const int t = threadIdx.x;
  if (j0 <= i0 + 63) {
    for (int x = t; x < 64 * SYMM_KC; x += 256) {
      const int r = x >> 5, kk = x & 31, i = i0 + r, j = j0 + kk;
      if (i >= j) As[r * SYMM_ALD + kk] = (i < n && j < jend) ? W[(long)i * ldw + j] : 0.0;
    }
  }
  if (j0 + SYMM_KC - 1 > i0) {
    for (int x = t; x < 64 * SYMM_KC; x += 256) {
      const int kk = x >> 6, r = x & 63, i = i0 + r, j = j0 + kk;
      if (i < j) As[r * SYMM_ALD + kk] = (i < n && j < jend) ? W[(long)j * ldw + i] : 0.0;
    }
  }
}

// acc[cb] += As (this wave's 16 rows, the chunk's 32 k) * Bs[:, 16 cb .. 16 cb + 15] for every column block cb < 8 with live(cb):
// the chunk's rows of the thin operand are in Bs, bld doubles apart.  Wave w takes the rows 16 w .. 16 w + 15.  Lane maps
// (gemm_f64.hip): A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15], D[(l >> 4) + 4 r][l & 15].
template <class Live>
__device__ __forceinline__ void symm_chunk_mfma(const double* __restrict__ As, const double* __restrict__ Bs, int bld, Live live,
                                                double4_t (&acc)[8]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
  double a[SYMM_KC / 4];
#pragma unroll
  for (int ks = 0; ks < SYMM_KC / 4; ++ks) a[ks] = As[(16 * wv + l15) * SYMM_ALD + 4 * ks + l4];
#pragma unroll
  for (int cb = 0; cb < 8; ++cb) {
    if (live(cb)) {
#pragma unroll
      for (int ks = 0; ks < SYMM_KC / 4; ++ks)
        acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], Bs[(4 * ks + l4) * bld + 16 * cb + l15], acc[cb], 0, 0, 0);
    }
  }
}

}  // namespace migp
