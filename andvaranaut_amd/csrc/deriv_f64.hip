// The joint GP over f and grad f (include/mi_gp_deriv.h has the blocks and their theta derivatives): the covariance of
// [f ; d_1 f ; .. ; d_d f] at two point sets and the contraction 1/2 sum (alpha alpha^T - K^-1) dK~/dtheta over it.
// Row a = c n + i of the joint matrix is component c (0: the value) at point i, so a 64x64 tile covers up to 64 points per side
// whatever components its rows and columns belong to -- a component boundary may fall anywhere inside it.  A workgroup stages
// the (unscaled) coordinates of its rows' and columns' points and each row's and column's component in LDS; thread (ty, tx) owns
// the 4x4 strided micro-tile rows ty + 16 a, columns tx + 16 b (grad_contract_kernel's split).  dl = x_i - x_j and
// s = sum_m a_m dl_m^2 are formed directly from the coordinates: the derivative blocks are proportional to dl and would lose their
// leading digits through |x|^2 + |x'|^2 - 2 x.x'.  Every entry costs O(d): O(N^2 d) in all, as the plain contraction.
// d <= DERIV_MAX_D: one LDS block holds every dimension.
#include "migp_kernels.h"
#include "migp_math.h"

namespace migp {

constexpr int VT = 64;                  // tile
constexpr int VLD = DERIV_MAX_D + 1;    // LDS row stride in doubles (odd: the 16 rows a wave reads at once fall in different banks)

// Tile e of the lower triangle counted row by row (grad_predict.hip's tri_tile, its twin)
struct DerivTile { int ti, tj; };
__device__ __forceinline__ DerivTile deriv_tri_tile(int e) {
  int t = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
  while ((t + 1) * (t + 2) / 2 <= e) ++t;
  while (t * (t + 1) / 2 > e) --t;
  return {t, e - t * (t + 1) / 2};
}

// The 64 joint rows from row0 on: the coordinates of each row's point (zeros beyond d and beyond the last row) and its component
// (-1 beyond the last row).  256 threads; the caller synchronises
__device__ __forceinline__ void deriv_stage(const double* __restrict__ X, int n, int q, int d, int row0, double* Xs, int* comp) {
  const int tid = threadIdx.x;
  const int m = tid % DERIV_MAX_D;
  const long N = (long)n * q;
  for (int r = tid / DERIV_MAX_D; r < VT; r += 256 / DERIV_MAX_D) {
    const long a = (long)row0 + r;
    double v = 0.0;
    if (a < N && m < d) v = X[(a % n) * d + m];
    Xs[r * VLD + m] = v;
  }
  if (tid < VT) {
    const long a = (long)row0 + tid;
    comp[tid] = a < N ? (int)(a / n) : -1;
  }
}

// One 64x64 tile per workgroup: sym = 1 the tiles of the lower triangle (blockIdx.x counts them row by row), else
// blockIdx.x = ti * tcols + tj over the rectangle
template <int KID>
__global__ __launch_bounds__(256) void deriv_assemble_kernel(int d, const double* __restrict__ theta, const double* __restrict__ X1, int n1,
                                                             int q1, const double* __restrict__ X2, int n2, int q2,
                                                             double* __restrict__ K, long ldk, int tcols, int sym, int noise_form,
                                                             const double* __restrict__ extra_diag) {
  __shared__ double Xi[VT * VLD];
  __shared__ double Xj[VT * VLD];
  __shared__ double av[DERIV_MAX_D];
  __shared__ int ci[VT], cj[VT];
  const int tid = threadIdx.x;
  int ti, tj;
  if (sym) {
    const DerivTile t = deriv_tri_tile(blockIdx.x);
    ti = t.ti;
    tj = t.tj;
  } else {
    ti = blockIdx.x / tcols;
    tj = blockIdx.x % tcols;
  }
  const int i0 = ti * VT, j0 = tj * VT;
  deriv_stage(X1, n1, q1, d, i0, Xi, ci);
  deriv_stage(X2, n2, q2, d, j0, Xj, cj);
  if (tid < DERIV_MAX_D) av[tid] = tid < d ? 1.0 / (theta[tid] * theta[tid]) : 0.0;
  __syncthreads();
  const int tx = tid & 15, ty = tid >> 4;
  const double kv = theta[d];
  const double gv = theta[d + 2], jitter = theta[d + 3];
  const double sg = sqrt(gv);

  double s[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) s[a][b] = 0.0;
  for (int m = 0; m < d; ++m) {
    double xi[4], xj[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) xi[a] = Xi[(ty + 16 * a) * VLD + m];
#pragma unroll
    for (int b = 0; b < 4; ++b) xj[b] = Xj[(tx + 16 * b) * VLD + m];
    const double am = av[m];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const double df = xi[a] - xj[b];
        s[a][b] = __builtin_fma(am * df, df, s[a][b]);
      }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int ra = ty + 16 * a;
    const long ga = (long)i0 + ra;
    const int c = ci[ra];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int rb = tx + 16 * b;
      const long gb = (long)j0 + rb;
      const int cp = cj[rb];
      double x;
      if (c < 0 || cp < 0) {
        x = (sym && ga == gb) ? 1.0 : 0.0;
      } else {
        double k, k1, k2, k3;
        base_kernel_val_der3(KID, s[a][b], k, k1, k2, k3);
        // (dl_c and a_c of the row's component, dl_c' and a_c' of the column's; index 0 stands in for the value component, unused)
        const int mc = c > 0 ? c - 1 : 0, mp = cp > 0 ? cp - 1 : 0;
        const double dc = Xi[ra * VLD + mc] - Xj[rb * VLD + mc];
        const double dp = Xi[ra * VLD + mp] - Xj[rb * VLD + mp];
        const double ac = av[mc], ap = av[mp];
        if (c == 0 && cp == 0) x = kv * k;
        else if (cp == 0) x = 2.0 * kv * k1 * (ac * dc);
        else if (c == 0) x = -2.0 * kv * k1 * (ap * dp);
        else {
          x = -4.0 * k2 * ((ac * dc) * (ap * dp));
          if (c == cp) x -= 2.0 * k1 * ac;
          x *= kv;
        }
        if (sym && ga == gb) {
          if (c == 0) {  // the value rows: launch_assemble's forms, operation for operation
            if (noise_form == 0) { x += sg * sg; x += jitter; }
            else if (noise_form == 1) { x += jitter; x += sg * sg; }
            else if (noise_form == 3) { x += sg * sg; }
            else if (noise_form == 4) { x += jitter; }
            else { x += jitter + gv; }
          } else {
            x += jitter;  // a derivative is observed without the value's noise
          }
          if (extra_diag) x += extra_diag[ga];
        }
      }
      K[ga * ldk + gb] = x;
    }
  }
}

// One 64x64 tile of the lower triangle of W per workgroup; part[blockIdx.x][p] receives the tile's partial sums, p in the order
// l(d), kv, alpha (0), gv, jitter.  Per entry (row component c, column component c'), with w the weight:
//   the coefficient A of dl_p^2 in dK~/da_p for EVERY p, and the two single-p terms T1 (p = c) and T2 (p = c')
//   (0, 0):   A = kv k1                                                    T1 = T2 = 0
//   (c, 0):   A = 2 kv dl_c k2 a_c                                         T1 = 2 kv dl_c k1
//   (0, c'):  A = -2 kv dl_c' k2 a_c'                                      T2 = -2 kv dl_c' k1
//   (c, c'):  A = kv (-4 k3 a_c a_c' dl_c dl_c' - 2 k2 a_c [c = c'])       T1 = kv (-4 k2 dl_c dl_c' a_c' - 2 k1 [c = c'])
//                                                                          T2 = kv (-4 k2 dl_c dl_c' a_c)
// The length-scale pass then is grad_contract_kernel's: per dimension the micro-tile's sum, a wave tree, the four waves' partials
// in LDS, one barrier, thread p adds its four.  The single-p terms ride in that pass under a comparison (registers are not indexed).
template <int KID>
__global__ __launch_bounds__(256) void deriv_contract_kernel(int d, const double* __restrict__ theta, const double* __restrict__ X, int n,
                                                             const double* __restrict__ W, long ldw,
                                                             const double* __restrict__ alpha_v, double* __restrict__ part) {
  __shared__ double Xi[VT * VLD];
  __shared__ double Xj[VT * VLD];
  __shared__ double av[DERIV_MAX_D];
  __shared__ int ci[VT], cj[VT];
  __shared__ double red[4 * DERIV_MAX_D];
  const int tid = threadIdx.x;
  const int q = 1 + d;
  const long N = (long)n * q;
  const int P = d + 4;
  double* out = part + (long)blockIdx.x * P;
  const DerivTile t = deriv_tri_tile(blockIdx.x);
  const int i0 = t.ti * VT, j0 = t.tj * VT;
  deriv_stage(X, n, q, d, i0, Xi, ci);
  deriv_stage(X, n, q, d, j0, Xj, cj);
  if (tid < DERIV_MAX_D) av[tid] = tid < d ? 1.0 / (theta[tid] * theta[tid]) : 0.0;
  __syncthreads();
  const int tx = tid & 15, ty = tid >> 4;
  const double kv = theta[d];

  double s[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) s[a][b] = 0.0;
  for (int m = 0; m < d; ++m) {
    double xi[4], xj[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) xi[a] = Xi[(ty + 16 * a) * VLD + m];
#pragma unroll
    for (int b = 0; b < 4; ++b) xj[b] = Xj[(tx + 16 * b) * VLD + m];
    const double am = av[m];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const double df = xi[a] - xj[b];
        s[a][b] = __builtin_fma(am * df, df, s[a][b]);
      }
  }

  // per entry: the weight (1 below the diagonal, 1/2 on it, 0 above and in the padding: grad_contract_kernel's) times A, T1, T2
  double A[4][4], T1[4][4], T2[4][4];
  int mrow[4], mcol[4];  // the dimension of the row's / column's component, -1 for the value component
  double skv = 0.0, sgv = 0.0, sjit = 0.0;
#pragma unroll
  for (int a = 0; a < 4; ++a) mrow[a] = ci[ty + 16 * a] - 1;
#pragma unroll
  for (int b = 0; b < 4; ++b) mcol[b] = cj[tx + 16 * b] - 1;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int ra = ty + 16 * a;
    const long ga = (long)i0 + ra;
    const int c = ci[ra];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int rb = tx + 16 * b;
      const long gb = (long)j0 + rb;
      const int cp = cj[rb];
      double w = 0.0;
      if (ga < N && gb < N && gb <= ga) {
        w = alpha_v[ga] * alpha_v[gb] - W[ga * ldw + gb];
        if (ga == gb) w *= 0.5;
      }
      double k, k1, k2, k3;
      base_kernel_val_der3(KID, s[a][b], k, k1, k2, k3);
      const int mc = c > 0 ? c - 1 : 0, mp = cp > 0 ? cp - 1 : 0;
      const double dc = Xi[ra * VLD + mc] - Xj[rb * VLD + mc];
      const double dp = Xi[ra * VLD + mp] - Xj[rb * VLD + mp];
      const double ac = av[mc], ap = av[mp];
      double kt, ca, t1 = 0.0, t2 = 0.0;  // K~ / kv and the three coefficients over kv
      if (c <= 0 && cp <= 0) {
        kt = k;
        ca = k1;
      } else if (cp <= 0) {
        kt = 2.0 * k1 * (ac * dc);
        ca = 2.0 * dc * k2 * ac;
        t1 = 2.0 * dc * k1;
      } else if (c <= 0) {
        kt = -2.0 * k1 * (ap * dp);
        ca = -2.0 * dp * k2 * ap;
        t2 = -2.0 * dp * k1;
      } else {
        const double dd = dc * dp;
        kt = -4.0 * k2 * ((ac * dc) * (ap * dp));
        ca = -4.0 * k3 * ((ac * ap) * dd);
        t1 = -4.0 * k2 * dd * ap;
        t2 = -4.0 * k2 * dd * ac;
        if (c == cp) {
          kt -= 2.0 * k1 * ac;
          ca -= 2.0 * k2 * ac;
          t1 -= 2.0 * k1;
        }
      }
      const double wk = w * kv;
      A[a][b] = wk * ca;
      T1[a][b] = wk * t1;
      T2[a][b] = wk * t2;
      skv += w * kt;
      if (ga == gb) {  // (w already carries the 1/2; 0 in the padding)
        sjit += w;
        if (c == 0) sgv += w;
      }
    }
  }

  auto block_sum = [&](double v) -> double {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
  };
  skv = block_sum(skv);
  sgv = block_sum(sgv);
  sjit = block_sum(sjit);
  if (tid == 0) {
    out[d] = skv;
    out[d + 1] = 0.0;
    out[d + 2] = sgv;
    out[d + 3] = sjit;
  }
  __syncthreads();  // red is written again below
  for (int m = 0; m < d; ++m) {
    double xi[4], xj[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) xi[a] = Xi[(ty + 16 * a) * VLD + m];
#pragma unroll
    for (int b = 0; b < 4; ++b) xj[b] = Xj[(tx + 16 * b) * VLD + m];
    double sm = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const double df = xi[a] - xj[b];
        double v = A[a][b] * (df * df);
        v += mrow[a] == m ? T1[a][b] : 0.0;
        v += mcol[b] == m ? T2[a][b] : 0.0;
        sm += v;
      }
    for (int off = 32; off > 0; off >>= 1) sm += __shfl_down(sm, off, 64);
    if ((tid & 63) == 0) red[4 * m + (tid >> 6)] = sm;
  }
  __syncthreads();
  if (tid < d) {
    const double sm = red[4 * tid] + red[4 * tid + 1] + red[4 * tid + 2] + red[4 * tid + 3];
    out[tid] = sm * (-2.0 * av[tid] / theta[tid]);  // d/dl_p = (-2 a_p / l_p) d/da_p
  }
}

// grad[p] = sum_b part[b][p] in a fixed order, and the evaluation's sequence number behind it (grad_predict.hip's grad_final_kernel
// for one problem, its twin: a change to the publication goes into both)
__global__ void deriv_final_kernel(const double* __restrict__ part, int nblk, int P, double* __restrict__ grad,
                                   unsigned* __restrict__ done, double* __restrict__ flag, double seq) {
  const int p = blockIdx.x;
  __shared__ double red[256];
  double s = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) s += part[(long)b * P + p];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    grad[p] = red[0];
    if (done && seq != 0.0) {
      __threadfence_system();
      if (atomicAdd(done, 1u) == (unsigned)P - 1u) {
        *done = 0u;  // ready for the next evaluation
        __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}

hipError_t launch_assemble_deriv(int kid, int d, const double* theta, const double* X1, int n1, int q1, const double* X2, int n2, int q2,
                                 double* K, long ldk, int rows_pad, int cols_pad, int sym, int noise_form, hipStream_t stream,
                                 const double* extra_diag) {
  if ((kid != KID_RBF && kid != KID_MATERN52) || d < 1 || d > DERIV_MAX_D || (q1 != 1 && q1 != 1 + d) || (q2 != 1 && q2 != 1 + d) ||
      rows_pad % VT || cols_pad % VT || (long)n1 * q1 > rows_pad || (long)n2 * q2 > cols_pad || n1 < 1 || n2 < 1)
    return hipErrorInvalidValue;
  const int tr = rows_pad / VT, tc = cols_pad / VT;
  if (sym && (tr != tc || n1 != n2 || q1 != q2)) return hipErrorInvalidValue;
  const int nblk = sym ? tr * (tr + 1) / 2 : tr * tc;
  if (kid == KID_RBF)
    deriv_assemble_kernel<KID_RBF><<<nblk, 256, 0, stream>>>(d, theta, X1, n1, q1, X2, n2, q2, K, ldk, tc, sym, noise_form,
                                                             sym ? extra_diag : nullptr);
  else
    deriv_assemble_kernel<KID_MATERN52><<<nblk, 256, 0, stream>>>(d, theta, X1, n1, q1, X2, n2, q2, K, ldk, tc, sym, noise_form,
                                                                  sym ? extra_diag : nullptr);
  return hipGetLastError();
}

hipError_t launch_grad_contract_deriv(int kid, int d, const double* theta, const double* X, int n, const double* W, long ldw,
                                      const double* alpha, double* part, double* grad, hipStream_t stream, unsigned* done, double* flag,
                                      double seq) {
  if ((kid != KID_RBF && kid != KID_MATERN52) || d < 1 || d > DERIV_MAX_D || n < 1) return hipErrorInvalidValue;
  const int nblk = grad_contract_blocks(n * (1 + d));
  const int P = d + 4;
  if (kid == KID_RBF) deriv_contract_kernel<KID_RBF><<<nblk, 256, 0, stream>>>(d, theta, X, n, W, ldw, alpha, part);
  else deriv_contract_kernel<KID_MATERN52><<<nblk, 256, 0, stream>>>(d, theta, X, n, W, ldw, alpha, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  deriv_final_kernel<<<P, 256, 0, stream>>>(part, nblk, P, grad, done, flag, seq);
  return hipGetLastError();
}

}  // namespace migp
