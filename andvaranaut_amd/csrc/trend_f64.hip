// Kernels of the GP trend with marginalised coefficients (option 50 of mi_gp_set_option, api_trend.hip): the basis
// h(x) = [1] (constant) or [1, x_1 .. x_d] (linear) with p <= 128 columns, kept as H^T -- 128 rows of ldg doubles, zeros in the rows
// from p on and in the columns from n on --, the symmetric thin multiply V = K^-1 H from the LOWER triangle of W alone, and the
// small reductions behind the p x p block A = H^T K^-1 H.  The multiply moves ~8 np^2 bytes (it streams the np x np matrix once,
// each lower element once straight and once mirrored) for 2 * 16 ceil(p/16) np^2 flops on v_mfma_f64_16x16x4_f64.  Every sum runs in a
// fixed order; nothing is accumulated with atomics.
#include <cmath>
#include "symm_chunk.h"

namespace migp {

// HT[c][i] = h_c(x_i) for c < p, i < n; zeros up to row 127 and column np - 1
__global__ __launch_bounds__(256) void trend_basis_kernel(const double* __restrict__ X, int n, int d, int p, int np,
                                                          double* __restrict__ HT, long ldg) {
  const long e = blockIdx.x * 256L + threadIdx.x;
  if (e >= 128L * np) return;
  const int c = (int)(e / np), i = (int)(e % np);
  HT[c * ldg + i] = (i < n && c < p) ? (c == 0 ? 1.0 : X[(long)i * d + (c - 1)]) : 0.0;
}

// Workgroup (rb, s): rows 64 rb .. 64 rb + 63 of slice s of V = Pfull H in the 16 ncb leading columns, Pfull[i][j] =
// W[max(i, j)][min(i, j)] for i, j < n and zero beyond.  k runs in chunks of 32 through LDS (symm_chunk.h): As = the chunk's
// columns of Pfull for the 64 rows, Hs = the chunk's rows of H (columns of HT), in rows of 16 ncb + 16 or + 32 doubles (an odd
// number of 16-double groups: the two k rows of a half-wave's B read land on disjoint banks).
// The kernel is bound by the latency of its loads, so the k range is cut into nslice slices of whole chunks that run side by
// side (a workgroup keeps 16 KB in flight; four or five of them fit a CU): slice s writes its partial product, 16 ncb columns
// wide, to out + s np ldo, and trend_slice_sum_kernel adds the slices in index order.  nslice == 1 writes V itself (ldo = 128),
// with zeros in the columns from 16 ncb on: all of the np x 128 block is written either way.
__host__ __device__ inline int trend_hld(int ncb) { return 16 * ncb + ((ncb & 1) ? 32 : 16); }
__global__ __launch_bounds__(256) void trend_symm_kernel(const double* __restrict__ W, long ldw, const double* __restrict__ HT,
                                                         long ldg, int n, int np, int ncb, int nslice, double* __restrict__ out,
                                                         int ldo) {
  extern __shared__ double tr_lds[];
  double* As = tr_lds;
  double* Hs = tr_lds + 64 * SYMM_ALD;
  const int hld = trend_hld(ncb);
  const int i0 = blockIdx.x * 64, t = threadIdx.x;
  const int lane = t & 63, wv = t >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int nch = np / SYMM_KC, sl = blockIdx.y;
  const int ch0 = (int)((long)sl * nch / nslice), ch1 = (int)((long)(sl + 1) * nch / nslice);
  out += (long)sl * np * ldo;
  double4_t acc[8];
#pragma unroll
  for (int cb = 0; cb < 8; ++cb) acc[cb] = double4_t{0.0, 0.0, 0.0, 0.0};
  for (int ch = ch0; ch < ch1; ++ch) {
    const int kc = ch * SYMM_KC;
    symm_stage_chunk(W, ldw, n, i0, kc, n, As);
    for (int x = t; x < 16 * ncb * SYMM_KC; x += 256) {
      const int c = x >> 5, kk = x & 31;
      Hs[kk * hld + c] = HT[c * ldg + kc + kk];
    }
    __syncthreads();
    symm_chunk_mfma(As, Hs, hld, [&](int cb) { return cb < ncb; }, acc);
    __syncthreads();
  }
#pragma unroll
  for (int cb = 0; cb < 8; ++cb) {
    if (16 * cb < ldo) {
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(long)(i0 + 16 * wv + l4 + 4 * r) * ldo + 16 * cb + l15] = cb < ncb ? acc[cb][r] : 0.0;
    }
  }
}

// V[i][c] = the sum over the slices, in index order, of parts[s][i][c] (rows of wc = 16 ncb doubles) for c < wc, zero up to column 127
__global__ __launch_bounds__(256) void trend_slice_sum_kernel(const double* __restrict__ parts, int nslice, int np, int wc,
                                                              double* __restrict__ V) {
  const long e = blockIdx.x * 256L + threadIdx.x;
  if (e >= 128L * np) return;
  const int i = (int)(e >> 7), c = (int)(e & 127);
  double s = 0.0;
  if (c < wc)
    for (int q = 0; q < nslice; ++q) s += parts[((long)q * np + i) * wc + c];
  V[e] = s;
}

// A = the sum of nparts 128 x 128 partial products in index order over the leading p x p block, the identity beyond it
__global__ __launch_bounds__(256) void trend_gram_sum_kernel(const double* __restrict__ parts, int nparts, int p,
                                                             double* __restrict__ A) {
  const int e = blockIdx.x * 256 + threadIdx.x, a = e >> 7, b = e & 127;
  double s = 0.0;
  if (a < p && b < p) {
    for (int q = 0; q < nparts; ++q) s += parts[(long)q * MINV_ELEMS + e];
  } else {
    s = a == b ? 1.0 : 0.0;
  }
  A[e] = s;
}

// the 256 values of a workgroup summed in a fixed order: inside each wave by butterfly, the four waves in index order
__device__ __forceinline__ double block_sum_256(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();  // (red may still be read from the call before)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// u[c] = sum_{i < n} M[c][i] x[i] for the 128 rows of M (ld apart): one workgroup per row
__global__ __launch_bounds__(256) void trend_rowdot_kernel(const double* __restrict__ M, long ld, const double* __restrict__ x, int n,
                                                           double* __restrict__ u) {
  __shared__ double red[4];
  const double* row = M + blockIdx.x * ld;
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s = __builtin_fma(row[i], x[i], s);
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) u[blockIdx.x] = s;
}

// One workgroup, thread a = basis column a: c = C^-1 u, beta = C^-T c (zeros from p on), scal[0] = 1/2 |c|^2,
// scal[1] = sum_{j < p} log C_jj, scal[2] = the bad-pivot word of the factorisation of A.  C: the factored block (row-major, lower),
// Cinv its inverse (row-major, zeros above the diagonal).
__global__ __launch_bounds__(128) void trend_solve_kernel(const double* __restrict__ C, const double* __restrict__ Cinv,
                                                          const double* __restrict__ u, const int* __restrict__ info, int p,
                                                          double* __restrict__ cvec, double* __restrict__ beta,
                                                          double* __restrict__ scal) {
  __shared__ double us[128], cs[128], ls[128];
  const int a = threadIdx.x;
  us[a] = a < p ? u[a] : 0.0;
  __syncthreads();
  double c = 0.0;
  if (a < p)
    for (int k = 0; k <= a; ++k) c = __builtin_fma(Cinv[a * 128 + k], us[k], c);
  cs[a] = c;
  ls[a] = a < p ? log(C[a * 129]) : 0.0;
  __syncthreads();
  double b = 0.0;
  if (a < p)
    for (int k = a; k < p; ++k) b = __builtin_fma(Cinv[k * 128 + a], cs[k], b);
  cvec[a] = c;
  beta[a] = b;
  if (a == 0) {
    double q = 0.0, l = 0.0;
    for (int k = 0; k < p; ++k) {
      q = __builtin_fma(cs[k], cs[k], q);
      l += ls[k];
    }
    scal[0] = 0.5 * q;
    scal[1] = l;
    scal[2] = (double)info[0];
  }
}

// out[i] = base[i] - sum_{a < p} M[i * si + a * sa] beta[a] for i < n, zeros up to np
__global__ __launch_bounds__(256) void trend_project_kernel(const double* __restrict__ base, const double* __restrict__ M, long si,
                                                            long sa, const double* __restrict__ beta, int p, int n, int np,
                                                            double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= np) return;
  double s = 0.0;
  if (i < n) {
    for (int a = 0; a < p; ++a) s = __builtin_fma(M[i * si + a * sa], beta[a], s);
    s = base[i] - s;
  }
  out[i] = s;
}

// mi_gp_predict's reduction under a trend: one workgroup per point, ONE pass over its row a* = L^-1 k(X, x*) of the work block
// for a* . b~, |a*|^2 and the first eight products a* . G_c, further passes (the row is in cache) for eight more columns each;
// then r = h(x*) - G^T a*, t = C^-1 r and
//   mean = a* . b~ + h(x*)^T beta^,   var = kdiag - |a*|^2 + |t|^2 + noise.
// C^-1 is read from memory: with one point per workgroup a copy in LDS would cost the loads it saves.
__global__ __launch_bounds__(256) void trend_predict_reduce_kernel(const double* __restrict__ A, long lda, const double* __restrict__ Xnew,
                                                                   int d, int p, const double* __restrict__ GT, long ldg,
                                                                   const double* __restrict__ bt, const double* __restrict__ beta,
                                                                   const double* __restrict__ Cinv, int n, double kdiag, double noise,
                                                                   double* __restrict__ mean, double* __restrict__ var) {
  __shared__ double red[4], rs[128], hs[128], tq[128];
  const int pt = blockIdx.x, t = threadIdx.x;
  const double* row = A + (long)pt * lda;
  double sm = 0.0, sq = 0.0;
  for (int c0 = 0; c0 < p; c0 += 8) {
    double acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = 0.0;
    for (int j = t; j < n; j += 256) {
      const double a = row[j];
      if (c0 == 0) {
        sm = __builtin_fma(a, bt[j], sm);
        sq = __builtin_fma(a, a, sq);
      }
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (c0 + c < p) acc[c] = __builtin_fma(a, GT[(c0 + c) * ldg + j], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const double s = block_sum_256(acc[c], red);
      if (t == 0 && c0 + c < p) rs[c0 + c] = s;
    }
  }
  sm = block_sum_256(sm, red);
  sq = block_sum_256(sq, red);
  if (t < 128) hs[t] = t < p ? (t == 0 ? 1.0 : Xnew[(long)pt * d + (t - 1)]) : 0.0;
  __syncthreads();
  if (t < 128) rs[t] = t < p ? hs[t] - rs[t] : 0.0;
  __syncthreads();
  if (t < 128) {
    double v = 0.0;
    if (t < p)
      for (int k = 0; k <= t; ++k) v = __builtin_fma(Cinv[t * 128 + k], rs[k], v);
    tq[t] = v * v;
  }
  __syncthreads();
  if (t == 0) {
    double q = 0.0, hb = 0.0;
    for (int k = 0; k < p; ++k) {
      q += tq[k];
      hb = __builtin_fma(hs[k], beta[k], hb);
    }
    mean[pt] = sm + hb;
    var[pt] = (kdiag - sq) + q + noise;
  }
}

hipError_t launch_trend_basis(const double* X, int n, int d, int p, int np, double* HT, long ldg, hipStream_t stream) {
  trend_basis_kernel<<<(unsigned)((128L * np + 255) / 256), 256, 0, stream>>>(X, n, d, p, np, HT, ldg);
  return hipGetLastError();
}

// slices of the k range: enough workgroups for about five per CU of a 256-CU device, as many as `parts` (np x 128 doubles) holds
int trend_symm_slices(int np, int p) {
  const int ncb = (p + 15) / 16, fit = 128 / (16 * ncb), want = (1280 + np / 64 - 1) / (np / 64);
  const int s = want < fit ? want : fit;
  return s < 1 ? 1 : s > np / SYMM_KC ? np / SYMM_KC : s;
}

hipError_t launch_trend_symm(const double* W, long ldw, const double* HT, long ldg, int n, int np, int p, double* V, double* parts,
                             hipStream_t stream) {
  const int ncb = (p + 15) / 16, ns = trend_symm_slices(np, p);
  const size_t lds = sizeof(double) * (64 * SYMM_ALD + SYMM_KC * trend_hld(ncb));
  if (ns == 1) {
    trend_symm_kernel<<<dim3(np / 64, 1), 256, lds, stream>>>(W, ldw, HT, ldg, n, np, ncb, 1, V, 128);
    return hipGetLastError();
  }
  trend_symm_kernel<<<dim3(np / 64, ns), 256, lds, stream>>>(W, ldw, HT, ldg, n, np, ncb, ns, parts, 16 * ncb);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  trend_slice_sum_kernel<<<(unsigned)((128L * np + 255) / 256), 256, 0, stream>>>(parts, ns, np, 16 * ncb, V);
  return hipGetLastError();
}

hipError_t launch_trend_gram_sum(const double* parts, int nparts, int p, double* A, hipStream_t stream) {
  trend_gram_sum_kernel<<<MINV_ELEMS / 256, 256, 0, stream>>>(parts, nparts, p, A);
  return hipGetLastError();
}

hipError_t launch_trend_rowdot(const double* M, long ld, const double* x, int n, double* u, hipStream_t stream) {
  trend_rowdot_kernel<<<128, 256, 0, stream>>>(M, ld, x, n, u);
  return hipGetLastError();
}

hipError_t launch_trend_solve(const double* C, const double* Cinv, const double* u, const int* info, int p, double* cvec, double* beta,
                              double* scal, hipStream_t stream) {
  trend_solve_kernel<<<1, 128, 0, stream>>>(C, Cinv, u, info, p, cvec, beta, scal);
  return hipGetLastError();
}

hipError_t launch_trend_project(const double* base, const double* M, long si, long sa, const double* beta, int p, int n, int np,
                                double* out, hipStream_t stream) {
  trend_project_kernel<<<(np + 255) / 256, 256, 0, stream>>>(base, M, si, sa, beta, p, n, np, out);
  return hipGetLastError();
}

hipError_t launch_trend_predict_reduce(const double* A, long lda, const double* Xnew, int d, int p, const double* GT, long ldg,
                                       const double* bt, const double* beta, const double* Cinv, int n, int m, double kdiag,
                                       double noise, double* mean, double* var, hipStream_t stream) {
  trend_predict_reduce_kernel<<<m, 256, 0, stream>>>(A, lda, Xnew, d, p, GT, ldg, bt, beta, Cinv, n, kdiag, noise, mean, var);
  return hipGetLastError();
}

}  // namespace migp
