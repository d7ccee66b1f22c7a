// Kernels of the multi-output GP under one shared kernel (option 51 of mi_gp_set_option, api_multi.hip): q <= 128 outputs kept as
// Y^T -- 128 rows of ldg doubles, zeros in the rows from q on and in the columns from n on, the layout of the trend's H^T --, the q
// quadratic forms y_o . (K^-1 y_o) behind the symmetric thin multiply, and mi_gp_predict's reduction, which takes the q means
// and the variance of a point from ONE pass over its row of the work block on v_mfma_f64_16x16x4_f64.  Under option 52 = 1 (the
// between-output covariance integrated out) two one-workgroup reductions join them -- sum_j log (C_S)_jj with the bad-pivot word
// of S = Y^T K^-1 Y, and the q scales s_o = |b_o|^2 / (n - q - 1) -- and the reduction's epilogue writes a variance per output.
// Every sum runs in a fixed order; nothing is accumulated with atomics.
#include "symm_chunk.h"

namespace migp {

// YT[o][i] = y[o * ldy + i] for o < q, i < n; zeros up to row 127 and column np - 1
__global__ __launch_bounds__(256) void multi_stage_kernel(const double* __restrict__ y, long ldy, int q, int n, int np,
                                                          double* __restrict__ YT, long ldg) {
  const long e = blockIdx.x * 256L + threadIdx.x;
  if (e >= 128L * np) return;
  const int o = (int)(e / np), i = (int)(e % np);
  YT[o * ldg + i] = (i < n && o < q) ? y[o * ldy + i] : 0.0;
}

// quad[o] = sum_{i < n} YT[o][i] V[i][o]: one workgroup per output (the workgroups from q on write zero).  A thread adds its
// points in index order, the 256 partial sums meet by butterfly inside each wave and the four waves in index order.
__global__ __launch_bounds__(256) void multi_quad_kernel(const double* __restrict__ YT, long ldg, const double* __restrict__ V, int q,
                                                         int n, double* __restrict__ quad) {
  __shared__ double red[4];
  const int o = blockIdx.x, t = threadIdx.x;
  double s = 0.0;
  if (o < q)
    for (int i = t; i < n; i += 256) s = __builtin_fma(YT[o * ldg + i], V[(long)i * 128 + o], s);
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) s += __shfl_xor(s, w);
  if ((t & 63) == 0) red[t >> 6] = s;
  __syncthreads();
  if (t == 0) quad[o] = ((red[0] + red[1]) + red[2]) + red[3];
}

// scal[0] = sum_{j < q} log C[j][j] (C: the factored 128 x 128 block of S, row-major lower), added in index order by one thread;
// scal[1] = the bad-pivot word of that factorisation
__global__ __launch_bounds__(128) void multi_cov_scal_kernel(const double* __restrict__ C, const int* __restrict__ info, int q,
                                                             double* __restrict__ scal) {
  __shared__ double ls[128];
  const int a = threadIdx.x;
  ls[a] = a < q ? log(C[a * 129]) : 0.0;
  __syncthreads();
  if (a == 0) {
    double l = 0.0;
    for (int k = 0; k < q; ++k) l += ls[k];
    scal[0] = l;
    scal[1] = (double)info[0];
  }
}

// s[o] = sum_{i < n} BT[o][i]^2 / dof: one workgroup per output (the workgroups from q on write zero), summed as multi_quad_kernel
// sums
__global__ __launch_bounds__(256) void multi_rowsq_kernel(const double* __restrict__ BT, long ldg, int q, int n, double dof,
                                                          double* __restrict__ s_out) {
  __shared__ double red[4];
  const int o = blockIdx.x, t = threadIdx.x;
  double s = 0.0;
  if (o < q)
    for (int i = t; i < n; i += 256) {
      const double b = BT[o * ldg + i];
      s = __builtin_fma(b, b, s);
    }
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) s += __shfl_xor(s, w);
  if ((t & 63) == 0) red[t >> 6] = s;
  __syncthreads();
  if (t == 0) s_out[o] = (((red[0] + red[1]) + red[2]) + red[3]) / dof;
}

// mi_gp_predict's reduction under q outputs.  Workgroup b owns the 16 points 16 b .. 16 b + 15: their rows a* = L^-1 k(X, x*) of
// the work block are read ONCE, in chunks of 32 k through LDS (As: 16 rows x 32 k, Bs: the chunk's 32 columns of B^T for the
// 16 ncb leading outputs, rows of trend_hld-like odd group counts apart).  Wave w forms the 16 x 16 blocks of outputs cb = w and
// cb = w + 4 over all of k on the fp64 matrix core -- no two waves share an accumulator, so there is nothing to add across waves
// -- with two accumulators per block (a dependent fp64 MFMA issues after ~250 cycles, an independent one after 64).  |a*|^2:
// thread t adds the squares of row t >> 4 at the chunk positions (t & 15) and (t & 15) + 16, chunk by chunk; the 16 partial sums
// of a row meet by butterfly.  The next chunk's loads are in flight while the current one is multiplied.  Rows from m on,
// columns from n on and outputs from q on are staged as zeros whatever the buffers hold.
// svar (option 52 = 1; else nullptr): the q scales s_o.  The 16 variances then go through LDS (As is free behind the last chunk)
// and var[o * m + i] = ((kdiag - |a*_i|^2) + noise) * s_o is written for every output, 16 points of an output side by side.
// Lane maps (gemm_f64.hip): A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15], D[(l >> 4) + 4 r][l & 15].
constexpr int MULTI_PTS = 16;
__host__ __device__ inline int multi_hld(int ncb) { return 16 * ncb + ((ncb & 1) ? 32 : 16); }
__global__ __launch_bounds__(256) void multi_predict_kernel(const double* __restrict__ A, long lda, const double* __restrict__ BT,
                                                            long ldg, int q, int n, int m, double kdiag, double noise,
                                                            const double* __restrict__ svar, double* __restrict__ mean,
                                                            double* __restrict__ var) {
  extern __shared__ double mp_lds[];
  double* As = mp_lds;
  double* Bs = mp_lds + MULTI_PTS * SYMM_ALD;
  const int ncb = (q + 15) / 16, hld = multi_hld(ncb);
  const int p0 = blockIdx.x * MULTI_PTS, t = threadIdx.x;
  const int lane = t & 63, wv = t >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int nch = (n + SYMM_KC - 1) / SYMM_KC;
  // what this thread stages of a chunk: two elements of As (x = t, t + 256: row x >> 5, k x & 31) and up to sixteen of Bs
  // (x = t + 256 j < 16 ncb * 32: output x >> 5, k x & 31)
  const int ar0 = t >> 5, ar1 = ar0 + 8, kk = t & 31;
  double ra[2], rb[16];
  auto fetch = [&](int ch) {
    const int k = ch * SYMM_KC + kk;
    const bool kin = k < n;
    ra[0] = (kin && p0 + ar0 < m) ? A[(long)(p0 + ar0) * lda + k] : 0.0;
    ra[1] = (kin && p0 + ar1 < m) ? A[(long)(p0 + ar1) * lda + k] : 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int c = (t >> 5) + 8 * j;
      if (j < 2 * ncb) rb[j] = (kin && c < q) ? BT[c * ldg + k] : 0.0;
    }
  };
  const double4_t zero4 = {0.0, 0.0, 0.0, 0.0};
  double4_t acc[2][2] = {{zero4, zero4}, {zero4, zero4}};
  double sq = 0.0;
  fetch(0);
  for (int ch = 0; ch < nch; ++ch) {
    As[ar0 * SYMM_ALD + kk] = ra[0];
    As[ar1 * SYMM_ALD + kk] = ra[1];
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (j < 2 * ncb) Bs[kk * hld + (t >> 5) + 8 * j] = rb[j];
    __syncthreads();
    if (ch + 1 < nch) fetch(ch + 1);
    {
      const double u = As[(t >> 4) * SYMM_ALD + (t & 15)], v = As[(t >> 4) * SYMM_ALD + (t & 15) + 16];
      sq = __builtin_fma(u, u, sq);
      sq = __builtin_fma(v, v, sq);
    }
    double a[SYMM_KC / 4];
#pragma unroll
    for (int ks = 0; ks < SYMM_KC / 4; ++ks) a[ks] = As[l15 * SYMM_ALD + 4 * ks + l4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int cb = wv + 4 * h;
      if (cb < ncb) {
#pragma unroll
        for (int ks = 0; ks < SYMM_KC / 4; ++ks)
          acc[h][ks & 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], Bs[(4 * ks + l4) * hld + 16 * cb + l15], acc[h][ks & 1], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // the 16 lanes t & 15 of a row are neighbours inside one wave
#pragma unroll
  for (int w = 8; w > 0; w >>= 1) sq += __shfl_xor(sq, w);
  if (svar) {
    if ((t & 15) == 0) As[t >> 4] = (kdiag - sq) + noise;
    __syncthreads();
    for (int x = t; x < MULTI_PTS * q; x += 256) {
      const int o = x >> 4, pt = p0 + (x & 15);
      if (pt < m) var[(long)o * m + pt] = As[x & 15] * svar[o];
    }
  } else if ((t & 15) == 0 && p0 + (t >> 4) < m) {
    var[p0 + (t >> 4)] = (kdiag - sq) + noise;
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int cb = wv + 4 * h, o = 16 * cb + l15;
    if (cb < ncb && o < q) {
      const double4_t s = acc[h][0] + acc[h][1];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int pt = p0 + l4 + 4 * r;
        if (pt < m) mean[(long)o * m + pt] = s[r];
      }
    }
  }
}

hipError_t launch_multi_stage(const double* y, long ldy, int q, int n, int np, double* YT, long ldg, hipStream_t stream) {
  multi_stage_kernel<<<(unsigned)((128L * np + 255) / 256), 256, 0, stream>>>(y, ldy, q, n, np, YT, ldg);
  return hipGetLastError();
}

hipError_t launch_multi_quad(const double* YT, long ldg, const double* V, int q, int n, double* quad, hipStream_t stream) {
  multi_quad_kernel<<<128, 256, 0, stream>>>(YT, ldg, V, q, n, quad);
  return hipGetLastError();
}

hipError_t launch_multi_cov_scal(const double* C, const int* info, int q, double* scal, hipStream_t stream) {
  multi_cov_scal_kernel<<<1, 128, 0, stream>>>(C, info, q, scal);
  return hipGetLastError();
}

hipError_t launch_multi_rowsq(const double* BT, long ldg, int q, int n, double dof, double* s, hipStream_t stream) {
  multi_rowsq_kernel<<<128, 256, 0, stream>>>(BT, ldg, q, n, dof, s);
  return hipGetLastError();
}

hipError_t launch_multi_predict(const double* A, long lda, const double* BT, long ldg, int q, int n, int m, double kdiag, double noise,
                                const double* svar, double* mean, double* var, hipStream_t stream) {
  if (q < 1 || q > 128 || m < 1) return hipErrorInvalidValue;
  const int ncb = (q + 15) / 16;
  const size_t lds = sizeof(double) * (MULTI_PTS * SYMM_ALD + SYMM_KC * multi_hld(ncb));
  multi_predict_kernel<<<(m + MULTI_PTS - 1) / MULTI_PTS, 256, lds, stream>>>(A, lda, BT, ldg, q, n, m, kdiag, noise, svar, mean, var);
  return hipGetLastError();
}

}  // namespace migp
