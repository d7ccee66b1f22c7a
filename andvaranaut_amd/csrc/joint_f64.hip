// Joint predictive covariance and posterior draws (mi_gp_predict_cov / mi_gp_sample_cov, api_gp.hip).  The O(M^3) work --
// Sigma = K** - A^T A, its Cholesky factor, the draw product Z L^T -- runs on the existing assembly, leaf, strip and GEMM
// kernels; the kernels here are the pieces around them: the counter-based normal generator that writes Z straight into the
// padded GEMM operand, the diagonal shift / identity padding in front of the factorisation, the zeroed upper halves of the
// diagonal tiles behind it (the draw product reads them under kmode 4), and the epilogue that adds the mean.
#include <cmath>
#include "migp_kernels.h"

namespace migp {

// Philox4x64-10 (Salmon et al., SC'11; the generator of numpy.random.Philox): ten rounds over the 256-bit counter c under the
// 128-bit key (k0, k1), the key bumped by the Weyl constants between rounds.
__device__ __forceinline__ void philox4x64_10(unsigned long long (&c)[4], unsigned long long k0, unsigned long long k1) {
  constexpr unsigned long long M0 = 0xD2E7470EE14C6C93ull, M1 = 0xCA5A826395121157ull;
  constexpr unsigned long long W0 = 0x9E3779B97F4A7C15ull, W1 = 0xBB67AE8584CAA73Bull;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long lo0 = M0 * c[0], hi0 = __umul64hi(M0, c[0]);
    const unsigned long long lo1 = M1 * c[2], hi1 = __umul64hi(M1, c[2]);
    const unsigned long long n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += W0;
    k1 += W1;
  }
}

// (0, 1) from the top 53 bits of a word: ((w >> 11) + 1/2) 2^-53, never 0 or 1
__device__ __forceinline__ double unit_open(unsigned long long w) { return ((double)(w >> 11) + 0.5) * 0x1.0p-53; }

// One thread per Philox block q: block b = offset + q is Philox4x64-10 of the counter b + 1 (256-bit, carried) under key
// (seed, 0) -- numpy.random.Philox(key=seed, counter=b).random_raw(4).  Words (w0, w1) give normals 4q, 4q + 1 and (w2, w3)
// give 4q + 2, 4q + 3 by Box-Muller: rho = sqrt(-2 log u0), (rho cos 2 pi u1, rho sin 2 pi u1).  Normal j = r m + i (draw r,
// point i) goes to Z[r * ldz + i]; the padding of Z is zeroed by the caller.
__global__ __launch_bounds__(256) void philox_normal_kernel(double* __restrict__ Z, long ldz, int m, long total, long nblocks,
                                                            unsigned long long seed, unsigned long long offset) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= nblocks) return;
  const unsigned long long b = offset + (unsigned long long)q;
  unsigned long long c[4] = {b + 1ull, b + 1ull == 0ull ? 1ull : 0ull, 0ull, 0ull};
  philox4x64_10(c, seed, 0ull);
#pragma unroll
  for (int pr = 0; pr < 2; ++pr) {
    const double u0 = unit_open(c[2 * pr]), u1 = unit_open(c[2 * pr + 1]);
    const double rho = sqrt(-2.0 * log(u0));
    double sn, cs;
    sincospi(2.0 * u1, &sn, &cs);
    const double v[2] = {rho * cs, rho * sn};
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const long j = 4 * q + 2 * pr + t;
      if (j < total) {
        const long r = j / m, i = j - r * m;
        Z[r * ldz + i] = v[t];
      }
    }
  }
}

hipError_t launch_philox_normals(double* Z, long ldz, int m, int s, unsigned long long seed, unsigned long long offset,
                                 hipStream_t stream) {
  const long total = (long)s * m, nblocks = (total + 3) / 4;
  philox_normal_kernel<<<(unsigned)((nblocks + 255) / 256), 256, 0, stream>>>(Z, ldz, m, total, nblocks, seed, offset);
  return hipGetLastError();
}

// Sigma (mp x mp, lower) in front of its factorisation: + shift on the m leading diagonal entries, identity in the lower
// triangle of the padding rows m .. mp - 1.  Thread t < m: diagonal entry t; beyond: element (m + e / mp, e % mp).
__global__ __launch_bounds__(256) void cov_prepare_kernel(double* __restrict__ C, long ldc, int m, int mp, double shift) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t < m) {
    C[t * ldc + t] += shift;
    return;
  }
  const long e = t - m;
  if (e >= (long)(mp - m) * mp) return;
  const long i = m + e / mp, j = e % mp;
  if (j <= i) C[i * ldc + j] = (i == j) ? 1.0 : 0.0;
}

hipError_t launch_cov_prepare(double* C, long ldc, int m, int mp, double shift, hipStream_t stream) {
  const long total = m + (long)(mp - m) * mp;
  cov_prepare_kernel<<<(unsigned)((total + 255) / 256), 256, 0, stream>>>(C, ldc, m, mp, shift);
  return hipGetLastError();
}

// zeros in the strict upper triangle of the ntiles diagonal 128 x 128 tiles of L (blockIdx.y = tile; 64 threads per row pair)
__global__ __launch_bounds__(256) void zero_diag_upper_kernel(double* __restrict__ L, long ld) {
  const int tile = blockIdx.y;
  const int e = blockIdx.x * 256 + threadIdx.x;  // < 128 * 128
  const int r = e >> 7, c = e & 127;
  if (c > r) L[(long)(128 * tile + r) * ld + 128 * tile + c] = 0.0;
}

hipError_t launch_zero_diag_upper(double* L, long ld, int ntiles, hipStream_t stream) {
  zero_diag_upper_kernel<<<dim3(128 * 128 / 256, ntiles), 256, 0, stream>>>(L, ld);
  return hipGetLastError();
}

// draws[r * ldd + i] = mean[i] + D[r * ldp + i] for r < s, i < m
__global__ __launch_bounds__(256) void draw_epilogue_kernel(const double* __restrict__ D, long ldp, const double* __restrict__ mean,
                                                            int m, long total, double* __restrict__ draws, long ldd) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const long r = t / m, i = t - r * m;
  draws[r * ldd + i] = mean[i] + D[r * ldp + i];
}

hipError_t launch_draw_epilogue(const double* D, long ldp, const double* mean, int m, int s, double* draws, long ldd,
                                hipStream_t stream) {
  const long total = (long)s * m;
  draw_epilogue_kernel<<<(unsigned)((total + 255) / 256), 256, 0, stream>>>(D, ldp, mean, m, total, draws, ldd);
  return hipGetLastError();
}

}  // namespace migp
