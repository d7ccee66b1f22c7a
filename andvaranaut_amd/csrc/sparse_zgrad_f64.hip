// dF/dZ of the sparse inducing-point bound (api_sparse.hip; include/mi_gp_sparse.h has the algebra), the kernels behind
// zgrad_slabs >= 1 -- in a file of their own beside sparse_f64.hip, whose kernels they leave as they are:
//   sparse_zgrad        : sum_i T_iu dK(x_i, z_u)/dz_u over one chunk of data points, per inducing point -- the rectangular twin of
//                         grad_x_kernel (grad_predict.hip)
//   sparse_zgrad_reduce : its slabs added in slab order onto the chunks before
// Every sum runs in a fixed order; nothing here uses atomics.
#include <algorithm>
#include "migp_kernels.h"
#include "migp_math.h"

namespace migp {

constexpr int ST = 64;  // tile (sparse_f64.hip's ST, grad_x_kernel's GT)

// dF/dZ's Kuf term over one chunk of data points (include/mi_gp_sparse.h):
//   g_ud = sum_i w_iu sum_c coef_c(i,u) kv_c k_c'(r2_c(i,u)) * 2 (z_ud - x_id) / l_cd^2,   w_iu = T[i][u] + y_i t_u
// -- sparse_contract_kernel's weights against dk/dz instead of dk/dtheta, so the outputs are per inducing point (m x d numbers,
// not P scalars): the rectangular twin of grad_x_kernel (grad_predict.hip), the OWNED set the inducing points and the WALKED
// set the chunk's data points.  Workgroup (blockIdx.x, blockIdx.y) owns the 64 inducing points from 64 blockIdx.x and walks
// the chunk's 64-row data blocks jb = blockIdx.y, blockIdx.y + gridDim.y, ...; its 64 x d partial goes to slab blockIdx.y of gz
// ([gridDim.y][slab] doubles, rows of d), and sparse_zgrad_reduce_kernel adds the slabs in slab order.
// Per data block: the weight tile is staged with its owned index first (T is row-major over the data points, so the reads run
// along u; padding of either set gives zero); pass 1 builds the per-component r2 in the direct form on 4x4 micro-tiles (rows
// ty+16a of the owned set, columns tx+16b of the walked one) -- z_u = x_i gives r2 = 0 and a zero term exactly -- and the
// coefficient tile cf_c = w coef_c kv_c k_c', parked in LDS; pass 2 is the small dense product with thread (u = tid & 63,
// dimensions = tid >> 6 mod 4).  The staging, the micro-tile reads, coef_elem, the window scheme (w0) beyond ZG_MAXD dimensions
// and the LDS budget are grad_x_kernel's, word for word: a change to the fold goes into both.
constexpr int ZGCH = 16;  // input dimensions per LDS chunk (grad_x_kernel's GXCH)
constexpr int ZGLD = ZGCH + 1;
constexpr int ZG_MAXD = 128;  // output dimensions per pass (grad_x_kernel's GX_MAXD)

template <int NK, int NCH>  // NCH: chunks of 16 input dimensions covered by one window (dw <= 16 * NCH)
__global__ __launch_bounds__(256) void sparse_zgrad_kernel(KernSpec spec, const double* __restrict__ theta,
                                                           const double* __restrict__ X, int cnt, const double* __restrict__ Z, int m,
                                                           const double* __restrict__ T, long ldt, const double* __restrict__ yv,
                                                           const double* __restrict__ tv, double* __restrict__ gz, long slab, int w0) {
  __shared__ double Xi[ST * ZGLD];  // the owned inducing points
  __shared__ double Xj[ST * ZGLD];  // the walked data points
  __shared__ double Ct[ST * (ST + 1)];
  __shared__ double ils[NK * ZG_MAXD];  // 1 / l_cm of the window's dimensions
  __shared__ double ilc[NK * ZGCH];     // 1 / l_cm of the pass-1 chunk being staged
  const int tid = threadIdx.x;
  const int d = spec.d;
  const int nk = RUNTIME_NK<NK> ? spec.nkern : NK;
  const int dw = min(ZG_MAXD, d - w0);  // this pass's output dimensions
  const int nt = (cnt + ST - 1) / ST;
  const int i0 = blockIdx.x * ST;
  const int tx = tid & 15, ty = tid >> 4;  // pass-1 micro-tile: rows ty+16a, cols tx+16b
  const int pr = tid & 63, pq = tid >> 6;  // pass-2: row pr, dimensions m = pq (mod 4)
  const double* kv = theta + nk * d;
  const double* al = kv + nk;
  for (int e = tid; e < nk * dw; e += 256) ils[(e / dw) * ZG_MAXD + e % dw] = 1.0 / theta[(e / dw) * d + w0 + e % dw];
  double acc[NCH][ZGCH / 4];
#pragma unroll
  for (int mc = 0; mc < NCH; ++mc)
#pragma unroll
    for (int u = 0; u < ZGCH / 4; ++u) acc[mc][u] = 0.0;

  gz += (long)blockIdx.y * slab;
  for (int jb = blockIdx.y; jb < nt; jb += gridDim.y) {
    const int j0 = jb * ST;
    __syncthreads();  // previous block's pass 2 is done with Ct / Xj
    // weight tile w = T[i][u] + y_i t_u, read along u and stored with the owned index first; zero in the padding of either set
    for (int e = tid; e < ST * ST; e += 256) {
      const int c = e >> 6, r = e & 63;
      const int gi = i0 + r, gj = j0 + c;
      double w = 0.0;
      if (gi < m && gj < cnt) w = T[(long)gj * ldt + gi] + yv[gj] * tv[gi];
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
    for (int m0 = 0; m0 < d; m0 += ZGCH) {
      const int dc = min(ZGCH, d - m0);
      if (m0 > 0) __syncthreads();
      for (int e = tid; e < ST * ZGCH; e += 256) {
        const int r = e / ZGCH, mm = e % ZGCH;
        double vi = 0.0, vj = 0.0;
        if (mm < dc) {
          if (i0 + r < m) vi = Z[(long)(i0 + r) * d + m0 + mm];
          if (j0 + r < cnt) vj = X[(long)(j0 + r) * d + m0 + mm];
        }
        Xi[r * ZGLD + mm] = vi;
        Xj[r * ZGLD + mm] = vj;
      }
      if (tid < nk * ZGCH) {
        const int c = tid / ZGCH, mm = tid % ZGCH;
        ilc[tid] = (mm < dc) ? 1.0 / theta[c * d + m0 + mm] : 0.0;
      }
      __syncthreads();
      for (int mm = 0; mm < dc; ++mm) {
        double xi[4], xj[4];  // the micro-tile's coordinates (grad_x_kernel's reads)
#pragma unroll
        for (int a = 0; a < 4; ++a) xi[a] = Xi[(ty + 16 * a) * ZGLD + mm];
#pragma unroll
        for (int b = 0; b < 4; ++b) xj[b] = Xj[(tx + 16 * b) * ZGLD + mm];
#pragma unroll
        for (int c = 0; c < nk; ++c) {
          const double il = ilc[c * ZGCH + mm];
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
      // tests/test_gpu_sparse_zgrad.py repeats the evaluation and demands identical bits.
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
        const int m0 = mc * ZGCH;
        if (m0 >= dw) break;
        const int dc = min(ZGCH, dw - m0);
        if (NCH > 1) {  // several chunks: bring this one back (a single chunk -- d <= 16, w0 = 0 -- is still resident)
          __syncthreads();
          for (int e = tid; e < ST * ZGCH; e += 256) {
            const int r = e / ZGCH, mm = e % ZGCH;
            double vi = 0.0, vj = 0.0;
            if (mm < dc) {
              if (i0 + r < m) vi = Z[(long)(i0 + r) * d + w0 + m0 + mm];
              if (j0 + r < cnt) vj = X[(long)(j0 + r) * d + w0 + m0 + mm];
            }
            Xi[r * ZGLD + mm] = vi;
            Xj[r * ZGLD + mm] = vj;
          }
        }
        __syncthreads();
        double t[ZGCH / 4], xr[ZGCH / 4];
#pragma unroll
        for (int u = 0; u < ZGCH / 4; ++u) {
          t[u] = 0.0;
          xr[u] = Xi[pr * ZGLD + pq + 4 * u];
        }
        for (int j = 0; j < ST; ++j) {
          const double cj = Ct[pr * (ST + 1) + j];
#pragma unroll
          for (int u = 0; u < ZGCH / 4; ++u) t[u] += cj * (xr[u] - Xj[j * ZGLD + pq + 4 * u]);
        }
#pragma unroll
        for (int u = 0; u < ZGCH / 4; ++u) {
          const int mm = m0 + pq + 4 * u;
          if (pq + 4 * u < dc) {
            const double il = ils[c * ZG_MAXD + mm];
            acc[mc][u] += 2.0 * il * il * t[u];
          }
        }
      }
    }
  }
  if (i0 + pr < m) {
#pragma unroll
    for (int mc = 0; mc < NCH; ++mc)
#pragma unroll
      for (int u = 0; u < ZGCH / 4; ++u) {
        const int mm = mc * ZGCH + pq + 4 * u;
        if (mm < dw) gz[(long)(i0 + pr) * d + w0 + mm] = acc[mc][u];
      }
  }
}

// gz[e] = (first ? 0 : gz[e]) + sum_k part[k][e], e < len: the slabs of one chunk in slab order onto the chunks before it, the
// chunks in the order of the launches on the stream (gx_reduce_kernel's scheme, one thread per output element)
__global__ void sparse_zgrad_reduce_kernel(const double* __restrict__ part, int nslab, long slab, long len, double* __restrict__ gz,
                                           int first) {
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < len; e += (long)gridDim.x * blockDim.x) {
    double s = part[e];
    for (int k = 1; k < nslab; ++k) s += part[(long)k * slab + e];
    gz[e] = first ? s : gz[e] + s;
  }
}

// (GRAD_X_KERNELS' table: [slot][window of 1, 2, ZG_MAXD / ZGCH = 8 chunks])
static const decltype(&sparse_zgrad_kernel<1, 1>) SPARSE_ZGRAD_KERNELS[5][3] = {
    {sparse_zgrad_kernel<1, 1>, sparse_zgrad_kernel<1, 2>, sparse_zgrad_kernel<1, 8>},
    {sparse_zgrad_kernel<2, 1>, sparse_zgrad_kernel<2, 2>, sparse_zgrad_kernel<2, 8>},
    {sparse_zgrad_kernel<3, 1>, sparse_zgrad_kernel<3, 2>, sparse_zgrad_kernel<3, 8>},
    {sparse_zgrad_kernel<4, 1>, sparse_zgrad_kernel<4, 2>, sparse_zgrad_kernel<4, 8>},
    {sparse_zgrad_kernel<8, 1>, sparse_zgrad_kernel<8, 2>, sparse_zgrad_kernel<8, 8>}};
static_assert(ZG_MAXD / ZGCH == 8, "SPARSE_ZGRAD_KERNELS' last column is the full window");

constexpr long ZG_SCRATCH_BYTES = 64L << 20;  // the most the slabs of one chunk may take

static long sparse_zgrad_slab_len(int m, int d) { return (long)((m + ST - 1) / ST) * ST * d; }

int sparse_zgrad_slabs(int cnt, int m, int d, int cap) {
  const int nrb = (cnt + ST - 1) / ST, ncb = (m + ST - 1) / ST;
  int s = std::min(nrb, std::min(cap, (1024 + ncb - 1) / ncb));
  while (s > 1 && (long)s * sparse_zgrad_slab_len(m, d) * (long)sizeof(double) > ZG_SCRATCH_BYTES) --s;
  return s < 1 ? 1 : s;
}

long sparse_zgrad_scratch(int cnt, int m, int d, int cap) { return (long)sparse_zgrad_slabs(cnt, m, d, cap) * sparse_zgrad_slab_len(m, d); }

hipError_t launch_sparse_zgrad(const KernSpec& spec, const double* theta, const double* X, int cnt, const double* Z, int m,
                               const double* T, long ldt, const double* y, const double* tv, int cap, double* scratch, double* gz,
                               int first, hipStream_t stream) {
  const int d = spec.d, nslab = sparse_zgrad_slabs(cnt, m, d, cap);
  const long slab = sparse_zgrad_slab_len(m, d);
  const dim3 grid((m + ST - 1) / ST, nslab);
  const int slot = spec.nkern >= 1 && spec.nkern <= 4 ? spec.nkern - 1 : 4;
  const auto kern = SPARSE_ZGRAD_KERNELS[slot][d <= ZGCH ? 0 : d <= 2 * ZGCH ? 1 : 2];
  // one pass per window of ZG_MAXD output dimensions (a single pass up to d = 128)
  for (int w0 = 0; w0 < d; w0 += ZG_MAXD) kern<<<grid, 256, 0, stream>>>(spec, theta, X, cnt, Z, m, T, ldt, y, tv, scratch, slab, w0);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_sparse_zgrad_add(scratch, nslab, slab, (long)m * d, gz, first, stream);
}

hipError_t launch_sparse_zgrad_add(const double* part, int nslab, long slab, long len, double* gz, int first, hipStream_t stream) {
  sparse_zgrad_reduce_kernel<<<(int)std::min<long>((len + 255) / 256, 1024), 256, 0, stream>>>(part, nslab, slab, len, gz, first);
  return hipGetLastError();
}

}  // namespace migp
