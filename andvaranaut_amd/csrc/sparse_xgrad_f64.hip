// The data-side gradients of the sparse inducing-point bound (api_sparse_data.hip; include/mi_gp_sparse_data.h has the algebra),
// the kernels behind mi_gp_sparse_bind_data_grad -- in a file of their own beside sparse_zgrad_f64.hip, whose kernels they leave
// as they are:
//   sparse_xgrad : sum_u w_iu dK(x_i, z_u)/dx_i over the inducing points, per data point of one chunk -- sparse_zgrad_kernel with
//                  the owned and the walked set exchanged, the third of the family grad_x_kernel (grad_predict.hip) began
//   sparse_ygrad : dF/dy of one chunk from its resident rows A_c^T
// The slabs of sparse_xgrad are added by sparse_zgrad_f64.hip's reduction.  Every sum runs in a fixed order; nothing here uses
// atomics.
#include <algorithm>
#include "migp_kernels.h"
#include "migp_math.h"

namespace migp {

constexpr int ST = 64;  // tile (sparse_zgrad_f64.hip's ST, grad_x_kernel's GT)

// dF/dX over one chunk of data points (include/mi_gp_sparse_data.h):
//   g_id = sum_u w_iu sum_c coef_c(i,u) kv_c k_c'(r2_c(i,u)) * 2 (x_id - z_ud) / l_cd^2,   w_iu = T[i][u] + y_i t_u
// -- sparse_zgrad_kernel's sum taken per data point instead of per inducing point: the OWNED set is the chunk's data points, the
// WALKED set the inducing points, and since a data row belongs to one chunk nothing is summed across chunks.  Workgroup
// (blockIdx.x, blockIdx.y) owns the 64 data points from 64 blockIdx.x and walks the 64-column blocks of Z jb = blockIdx.y,
// blockIdx.y + gridDim.y, ...; its 64 x d partial goes to slab blockIdx.y of gx ([gridDim.y][slab] doubles, rows of d), and
// sparse_zgrad_reduce_kernel writes the slabs' sum in slab order.
// Per block of Z: the weight tile is staged with its owned index first -- T is row-major over the data points, so here the reads
// run along u, its contiguous direction, and so do the LDS writes; padding of either set gives zero; pass 1 builds the
// per-component r2 in the direct form on 4x4 micro-tiles (rows ty+16a of the owned set, columns tx+16b of the walked one) --
// x_i = z_u gives r2 = 0 and a zero term exactly -- and the coefficient tile cf_c = w coef_c kv_c k_c', parked in LDS; pass 2 is
// the small dense product with thread (i = tid & 63, dimensions = tid >> 6 mod 4).  The staging, the micro-tile reads,
// coef_elem, the window scheme (w0) beyond XG_MAXD dimensions and the LDS budget are grad_x_kernel's and sparse_zgrad_kernel's,
// word for word: a change to the fold goes into all three.
constexpr int XGCH = 16;  // input dimensions per LDS chunk (grad_x_kernel's GXCH)
constexpr int XGLD = XGCH + 1;
constexpr int XG_MAXD = 128;  // output dimensions per pass (grad_x_kernel's GX_MAXD)

template <int NK, int NCH>  // NCH: chunks of 16 input dimensions covered by one window (dw <= 16 * NCH)
__global__ __launch_bounds__(256) void sparse_xgrad_kernel(KernSpec spec, const double* __restrict__ theta,
                                                           const double* __restrict__ X, int cnt, const double* __restrict__ Z, int m,
                                                           const double* __restrict__ T, long ldt, const double* __restrict__ yv,
                                                           const double* __restrict__ tv, double* __restrict__ gx, long slab, int w0) {
  __shared__ double Xi[ST * XGLD];  // the owned data points
  __shared__ double Xj[ST * XGLD];  // the walked inducing points
  __shared__ double Ct[ST * (ST + 1)];
  __shared__ double ils[NK * XG_MAXD];  // 1 / l_cm of the window's dimensions
  __shared__ double ilc[NK * XGCH];     // 1 / l_cm of the pass-1 chunk being staged
  const int tid = threadIdx.x;
  const int d = spec.d;
  const int nk = RUNTIME_NK<NK> ? spec.nkern : NK;
  const int dw = min(XG_MAXD, d - w0);  // this pass's output dimensions
  const int nt = (m + ST - 1) / ST;
  const int i0 = blockIdx.x * ST;
  const int tx = tid & 15, ty = tid >> 4;  // pass-1 micro-tile: rows ty+16a, cols tx+16b
  const int pr = tid & 63, pq = tid >> 6;  // pass-2: row pr, dimensions m = pq (mod 4)
  const double* kv = theta + nk * d;
  const double* al = kv + nk;
  for (int e = tid; e < nk * dw; e += 256) ils[(e / dw) * XG_MAXD + e % dw] = 1.0 / theta[(e / dw) * d + w0 + e % dw];
  double acc[NCH][XGCH / 4];
#pragma unroll
  for (int mc = 0; mc < NCH; ++mc)
#pragma unroll
    for (int u = 0; u < XGCH / 4; ++u) acc[mc][u] = 0.0;

  gx += (long)blockIdx.y * slab;
  for (int jb = blockIdx.y; jb < nt; jb += gridDim.y) {
    const int j0 = jb * ST;
    __syncthreads();  // previous block's pass 2 is done with Ct / Xj
    // weight tile w = T[i][u] + y_i t_u, read along u and stored with the owned index first; zero in the padding of either set
    // (counted by k, a scalar, not by e = tid, tid + 256, ... as in the twins: with the owned index on the slow side the
    // compiler folded gi < cnt into that loop's exit, which made it a divergent loop left at EXEC == 0, and in <4, 8> it placed
    // the accumulators' spill copies above the EXEC restore -- the defect of DESIGN.md section 5.6, which
    // tests/test_isa_uninit.py finds in the listing.  A scalar trip count leaves no such exit.)
#pragma unroll 4
    for (int k = 0; k < ST * ST / 256; ++k) {
      const int e = tid + 256 * k;
      const int r = e >> 6, c = e & 63;
      const int gi = i0 + r, gj = j0 + c;
      double w = 0.0;
      if (gi < cnt && gj < m) w = T[(long)gi * ldt + gj] + yv[gi] * tv[gj];
      Ct[r * (ST + 1) + c] = w;
    }
    // pass 1: scaled squared distances per component
    double r2[NK][4][4];
#pragma unroll
    for (int c = 0; c < nk; ++c)
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) r2[c][a][b] = 0.0;
    for (int m0 = 0; m0 < d; m0 += XGCH) {
      const int dc = min(XGCH, d - m0);
      if (m0 > 0) __syncthreads();
      for (int e = tid; e < ST * XGCH; e += 256) {
        const int r = e / XGCH, mm = e % XGCH;
        double vi = 0.0, vj = 0.0;
        if (mm < dc) {
          if (i0 + r < cnt) vi = X[(long)(i0 + r) * d + m0 + mm];
          if (j0 + r < m) vj = Z[(long)(j0 + r) * d + m0 + mm];
        }
        Xi[r * XGLD + mm] = vi;
        Xj[r * XGLD + mm] = vj;
      }
      if (tid < nk * XGCH) {
        const int c = tid / XGCH, mm = tid % XGCH;
        ilc[tid] = (mm < dc) ? 1.0 / theta[c * d + m0 + mm] : 0.0;
      }
      __syncthreads();
      for (int mm = 0; mm < dc; ++mm) {
        double xi[4], xj[4];  // the micro-tile's coordinates (grad_x_kernel's reads)
#pragma unroll
        for (int a = 0; a < 4; ++a) xi[a] = Xi[(ty + 16 * a) * XGLD + mm];
#pragma unroll
        for (int b = 0; b < 4; ++b) xj[b] = Xj[(tx + 16 * b) * XGLD + mm];
#pragma unroll
        for (int c = 0; c < nk; ++c) {
          const double il = ilc[c * XGCH + mm];
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
              const double df = (xi[a] - xj[b]) * il;
              r2[c][a][b] += df * df;
            }
        }
      }
    }
    // coefficient tiles cf[c] = w * (dK/dK_c of the fold) * kv_c dk_c/dr2
    double cf[NK][4][4];
    auto coef_elem = [&](int a, int b) {
      double kval[NK], dkv[NK], da;
#pragma unroll
      for (int c = 0; c < nk; ++c) comp_val_der<false>(spec.kid[c], r2[c][a][b], al[c], kv[c], kval[c], dkv[c], da);
      double pref[NK];  // dK/dK_c of the fold: grad_contract_kernel's recurrence, per element
      double Tf = kval[0];
      pref[0] = 1.0;
#pragma unroll
      for (int c = 1; c < nk; ++c) {
        pref[c] = (spec.op[c - 1] == 0) ? 1.0 : Tf;
        Tf = (spec.op[c - 1] == 0) ? Tf + kval[c] : Tf * kval[c];
      }
      const double w = Ct[(ty + 16 * a) * (ST + 1) + tx + 16 * b];
#pragma unroll
      for (int c = 0; c < nk; ++c) {
        double coef = pref[c];
#pragma unroll
        for (int c2 = c + 1; c2 < nk; ++c2)
          if (spec.op[c2 - 1] == 1) coef *= kval[c2];
        cf[c][a][b] = w * coef * dkv[c];
      }
    };
    if constexpr (NK >= 2) {
      // NOT unrolled for composite kernels: grad_x_kernel's precaution (its comment records nondeterministic results of the
      // fully unrolled form -- sixteen elements x NK families in one giant basic block -- under this toolchain, a
      // code-generation problem and no race in the source).  The rolled loop keeps the block small;
      // tests/test_gpu_sparse_data_grad.py repeats the evaluation and demands identical bits.
#pragma unroll 1
      for (int a = 0; a < 4; ++a)
#pragma unroll 1
        for (int b = 0; b < 4; ++b) coef_elem(a, b);
    } else {
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) coef_elem(a, b);
    }
    // pass 2, one component at a time through the LDS tile
#pragma unroll
    for (int c = 0; c < nk; ++c) {
      __syncthreads();  // everyone has read the weights (c == 0) / finished the previous component
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) Ct[(ty + 16 * a) * (ST + 1) + tx + 16 * b] = cf[c][a][b];
#pragma unroll
      for (int mc = 0; mc < NCH; ++mc) {
        const int m0 = mc * XGCH;
        if (m0 >= dw) break;
        const int dc = min(XGCH, dw - m0);
        if (NCH > 1) {  // several chunks: bring this one back (a single chunk -- d <= 16, w0 = 0 -- is still resident)
          __syncthreads();
          for (int e = tid; e < ST * XGCH; e += 256) {
            const int r = e / XGCH, mm = e % XGCH;
            double vi = 0.0, vj = 0.0;
            if (mm < dc) {
              if (i0 + r < cnt) vi = X[(long)(i0 + r) * d + w0 + m0 + mm];
              if (j0 + r < m) vj = Z[(long)(j0 + r) * d + w0 + m0 + mm];
            }
            Xi[r * XGLD + mm] = vi;
            Xj[r * XGLD + mm] = vj;
          }
        }
        __syncthreads();
        double t[XGCH / 4], xr[XGCH / 4];
#pragma unroll
        for (int u = 0; u < XGCH / 4; ++u) {
          t[u] = 0.0;
          xr[u] = Xi[pr * XGLD + pq + 4 * u];
        }
        for (int j = 0; j < ST; ++j) {
          const double cj = Ct[pr * (ST + 1) + j];
#pragma unroll
          for (int u = 0; u < XGCH / 4; ++u) t[u] += cj * (xr[u] - Xj[j * XGLD + pq + 4 * u]);
        }
#pragma unroll
        for (int u = 0; u < XGCH / 4; ++u) {
          const int mm = m0 + pq + 4 * u;
          if (pq + 4 * u < dc) {
            const double il = ils[c * XG_MAXD + mm];
            acc[mc][u] += 2.0 * il * il * t[u];
          }
        }
      }
    }
  }
  if (i0 + pr < cnt) {
#pragma unroll
    for (int mc = 0; mc < NCH; ++mc)
#pragma unroll
      for (int u = 0; u < XGCH / 4; ++u) {
        const int mm = mc * XGCH + pq + 4 * u;
        if (mm < dw) gx[(long)(i0 + pr) * d + w0 + mm] = acc[mc][u];
      }
  }
}

// gy[i] = -y[i] / s + (sum_{u < m} At[i][u] ahat[u]) / s for the cnt rows of one chunk: one wave per row, lane l sums the entries
// u = l, l + 64, ... in that order and the 64 partial sums are folded by halves -- the same tree at every call
__global__ __launch_bounds__(256) void sparse_ygrad_kernel(const double* __restrict__ At, long ld, int m, const double* __restrict__ ahat,
                                                           const double* __restrict__ yv, int cnt, double sv, double* __restrict__ gy) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= cnt) return;  // (whole waves leave together: the shuffles below stay within one row's wave)
  const double* a = At + (long)row * ld;
  double sum = 0.0;
  for (int u = lane; u < m; u += 64) sum += a[u] * ahat[u];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
  if (lane == 0) gy[row] = -yv[row] / sv + sum / sv;
}

// (SPARSE_ZGRAD_KERNELS' table: [slot][window of 1, 2, XG_MAXD / XGCH = 8 chunks])
static const decltype(&sparse_xgrad_kernel<1, 1>) SPARSE_XGRAD_KERNELS[5][3] = {
    {sparse_xgrad_kernel<1, 1>, sparse_xgrad_kernel<1, 2>, sparse_xgrad_kernel<1, 8>},
    {sparse_xgrad_kernel<2, 1>, sparse_xgrad_kernel<2, 2>, sparse_xgrad_kernel<2, 8>},
    {sparse_xgrad_kernel<3, 1>, sparse_xgrad_kernel<3, 2>, sparse_xgrad_kernel<3, 8>},
    {sparse_xgrad_kernel<4, 1>, sparse_xgrad_kernel<4, 2>, sparse_xgrad_kernel<4, 8>},
    {sparse_xgrad_kernel<8, 1>, sparse_xgrad_kernel<8, 2>, sparse_xgrad_kernel<8, 8>}};
static_assert(XG_MAXD / XGCH == 8, "SPARSE_XGRAD_KERNELS' last column is the full window");

constexpr long XG_SCRATCH_BYTES = 64L << 20;  // the most the slabs of one chunk may take

static long sparse_xgrad_slab_len(int cnt, int d) { return (long)((cnt + ST - 1) / ST) * ST * d; }

int sparse_xgrad_slabs(int cnt, int m, int d, int cap) {
  const int nrb = (cnt + ST - 1) / ST, ncb = (m + ST - 1) / ST;
  int s = std::min(ncb, std::min(cap, (1024 + nrb - 1) / nrb));
  while (s > 1 && (long)s * sparse_xgrad_slab_len(cnt, d) * (long)sizeof(double) > XG_SCRATCH_BYTES) --s;
  return s < 1 ? 1 : s;
}

long sparse_xgrad_scratch(int cnt, int m, int d, int cap) { return (long)sparse_xgrad_slabs(cnt, m, d, cap) * sparse_xgrad_slab_len(cnt, d); }

hipError_t launch_sparse_xgrad(const KernSpec& spec, const double* theta, const double* X, int cnt, const double* Z, int m,
                               const double* T, long ldt, const double* y, const double* tv, int cap, double* scratch, double* gx,
                               hipStream_t stream) {
  const int d = spec.d, nslab = sparse_xgrad_slabs(cnt, m, d, cap);
  const long slab = sparse_xgrad_slab_len(cnt, d);
  const dim3 grid((cnt + ST - 1) / ST, nslab);
  const int slot = spec.nkern >= 1 && spec.nkern <= 4 ? spec.nkern - 1 : 4;
  const auto kern = SPARSE_XGRAD_KERNELS[slot][d <= XGCH ? 0 : d <= 2 * XGCH ? 1 : 2];
  // one pass per window of XG_MAXD output dimensions (a single pass up to d = 128)
  for (int w0 = 0; w0 < d; w0 += XG_MAXD) kern<<<grid, 256, 0, stream>>>(spec, theta, X, cnt, Z, m, T, ldt, y, tv, scratch, slab, w0);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // the slabs' sum in slab order: it overwrites, a data row belongs to this chunk alone
  return launch_sparse_zgrad_add(scratch, nslab, slab, (long)cnt * d, gx, 1, stream);
}

hipError_t launch_sparse_ygrad(const double* At, long ld, int m, const double* ahat, const double* y, int cnt, double sv, double* gy,
                               hipStream_t stream) {
  sparse_ygrad_kernel<<<(cnt + 3) / 4, 256, 0, stream>>>(At, ld, m, ahat, y, cnt, sv, gy);
  return hipGetLastError();
}

}  // namespace migp
