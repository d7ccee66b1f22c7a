// Kernels around the factorisation for the hyper-parameter gradient and
// the posterior conditional (K8):
//   set_identity_blocks : identity into the 128x128 diagonal blocks of U (input of the leaf inverses)
//   trmv_upper          : alpha = U beta  with U = L^-T upper triangular  (== L^-T L^-1 y, gpmcmc.py:315)
//   grad_contract       : dLML/dtheta_k = 1/2 sum_ij (alpha_i alpha_j - Kinv_ij) dK_ij/dtheta_k, all
//                         parameters in one pass over the lower triangle ("assembly shaped": the
//                         covariance and its derivatives are recomputed from X, only Kinv is read)
//   predict_reduce      : mu_i = A_i . beta,  var_i = kdiag - |A_i|^2 (+ gv)   (gpmcmc.py:766-778)
// The reference obtains the gradient by reverse-mode autodiff through the PyTensor graph inside
// pm.find_MAP / pm.sample (gpmcmc.py:345,351); the analytic form is restated in oracle/gp_oracle.py.
#include "migp_kernels.h"
#include "migp_math.h"

namespace migp {

constexpr int GT = 64;  // contraction tile
constexpr int GDCH = 32;
constexpr int GDLD = GDCH + 1;

__global__ void set_identity_blocks_kernel(double* __restrict__ U, long ld, long sZ) {
  double* blk = U + (long)blockIdx.z * sZ + (long)blockIdx.x * 128 * ld + (long)blockIdx.x * 128;
  for (int e = threadIdx.x; e < 128 * 128; e += blockDim.x) {
    const int r = e >> 7, c = e & 127;
    blk[(long)r * ld + c] = (r == c) ? 1.0 : 0.0;
  }
}

// alpha[i] = sum_{k >= i} U[i][k] * beta[k], one wave per row, rows [0, n); U is np x ld, columns
// beyond n hold the padding (identity diagonal / zeros) and beta is zero there by construction.
__global__ __launch_bounds__(256) void trmv_upper_kernel(const double* __restrict__ U, long ld,
                                                         const double* __restrict__ beta, int n,
                                                         double* __restrict__ alpha, long sZ, long sK, long salpha) {
  U += (long)blockIdx.z * sZ;  // batched evaluation: problem blockIdx.z
  beta += (long)blockIdx.z * sK;
  alpha += (long)blockIdx.z * salpha;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  const double* u = U + (long)row * ld;
  double s = 0.0;
  const int k0 = row & ~63;
  for (int k = k0 + lane; k < n; k += 64) {
    if (k >= row) s += u[k] * beta[k];
  }
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) alpha[row] = s;
}

// out[i] = sum_{k <= i} U[k][i] * x[k]  (U^T x = L^-1 x for U = L^-T), columns [0, n).  One workgroup per 64 columns;
// wave g walks rows k = g (mod 4), 8 independent loads in flight per lane: consecutive lanes read consecutive doubles of
// one row of U (512 B per wave load), x[k] is a broadcast; the four partial sums meet in LDS in a fixed order.
__global__ __launch_bounds__(256) void trmv_upper_t_kernel(const double* __restrict__ U, long ld,
                                                           const double* __restrict__ x, int n,
                                                           double* __restrict__ out) {
  __shared__ double part[4][64];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + c;
  const int kmax = min(n - 1, blockIdx.x * 64 + 63);
  const bool live = i < n;
  double s[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) s[u] = 0.0;
  int k = g;
  for (; k + 28 <= kmax; k += 32) {
    double uv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int kk = k + 4 * u;
      uv[u] = (live && kk <= i) ? U[(long)kk * ld + i] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) s[u] += uv[u] * x[k + 4 * u];
  }
  for (; k <= kmax; k += 4)
    if (live && k <= i) s[0] += U[(long)k * ld + i] * x[k];
  part[g][c] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  __syncthreads();
  if (g == 0 && live) out[i] = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
}

// (base_kernel_val_der, RUNTIME_NK and comp_val_der: migp_math.h, shared with sweep_f64.hip)

// What the three kernels that differentiate through the composite covariance (grad_contract, grad_x, predict_grad) share.
// They hold further copies of one another's code -- the fold's derivative, the micro-tile reads, grad_contract's staging --
// because this toolchain compiles those to other instructions once they are functions (profiles/NOTES_grad_refactor.md);
// each such copy names its twins.

// Tile e of the lower triangle counted row by row: e = ti (ti + 1) / 2 + tj with tj <= ti (sqrt, then corrected to be exact)
struct TriTile { int ti, tj; };
__device__ __forceinline__ TriTile tri_tile(int e) {
  int t = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
  while ((t + 1) * (t + 2) / 2 <= e) ++t;
  while (t * (t + 1) / 2 > e) --t;
  return {t, e - t * (t + 1) / 2};
}

// One 64x64 tile of the lower triangle per workgroup; thread (ty, tx) owns the 4x4 strided
// micro-tile rows ty+16a, cols tx+16b.  part[blockIdx.x][p] receives the block's partial sums.
// Parameter order p: ls(nk*d), kv(nk), alpha(nk), gv, jitter.
// Occupancy (round 6): the kernel is bound by LDS / exp latency, not by issue -- at 176 VGPRs (two waves per SIMD) the N = 16384 pass
// took 2.0 ms against ~0.6 ms of fp64 issue.  One and two components are built for three waves per SIMD (<= 168 VGPRs: the
// weights' products with dk/dr2 are formed once, G = wc * dkv, and the five per-element arrays of the fold die before the
// length-scale pass; RQ = false: no component is a rational quadratic, so d k / d alpha -- identically zero then -- is not carried);
// N = 16384 LML + gradient 70.6 -> 69.9 ms on one box.  Same arithmetic, same bits.
template <int NK, bool RQ>
__global__ __launch_bounds__(256, NK == 1 ? 3 : (NK == 2 && !RQ) ? 2 : 1) void grad_contract_kernel(KernSpec spec, const double* __restrict__ theta,
                                                            const double* __restrict__ X, int n,
                                                            const double* __restrict__ W, long ldw,
                                                            const double* __restrict__ alpha_v,
                                                            double* __restrict__ part, int rect_tw, int tj0,
                                                            long wrow0, long wcol0, int stheta, long sW, long salpha,
                                                            long spart) {
  theta += (long)blockIdx.z * stheta;  // batched evaluation: problem blockIdx.z
  W += (long)blockIdx.z * sW;
  alpha_v += (long)blockIdx.z * salpha;
  part += (long)blockIdx.z * spart;
  __shared__ double Xi[GT * GDLD];
  __shared__ double Xj[GT * GDLD];
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const int d = spec.d;
  const int nk = RUNTIME_NK<NK> ? spec.nkern : NK;
  const int P = nk * d + 2 * nk + 2;
  double* out = part + (long)blockIdx.x * P;
  int ti, tj;
  if (rect_tw > 0) {
    // column slab of a distributed K^-1: tile columns [tj0, tj0 + rect_tw), tile rows from tj0 down; W holds the slab
    // with its element (wrow0, wcol0) first.  Tiles above the diagonal contribute nothing.
    ti = tj0 + blockIdx.x / rect_tw;
    tj = tj0 + blockIdx.x % rect_tw;
    if (ti < tj) {
      for (int p = tid; p < P; p += 256) out[p] = 0.0;
      return;
    }
    W -= wrow0 * ldw + wcol0;
  } else {
    const TriTile t = tri_tile(blockIdx.x);
    ti = t.ti;
    tj = t.tj;
  }
  const int i0 = ti * GT, j0 = tj * GT;
  const int tx = tid & 15, ty = tid >> 4;
  const double* ls = theta;
  const double* kv = theta + nk * d;
  const double* al = kv + nk;

  // weights: w_ab = (alpha_i alpha_j - W_ij) * (1 below the diagonal, 1/2 on it, 0 above / padding)
  double wgt[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int gi = i0 + ty + 16 * a, gj = j0 + tx + 16 * b;
      double w = 0.0;
      if (gi < n && gj < n && gj <= gi) {
        w = alpha_v[gi] * alpha_v[gj] - W[(long)gi * ldw + gj];
        if (gi == gj) w *= 0.5;
      }
      wgt[a][b] = w;
    }

  // pass 1: per-component scaled squared distances r2[c] (direct form) -> value, derivative, fold
  double kval[NK][4][4], dkv[NK][4][4], dal[RQ ? NK : 1][4][4];
#pragma unroll
  for (int c = 0; c < nk; ++c) {
    double r2[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) r2[a][b] = 0.0;
    for (int m0 = 0; m0 < d; m0 += GDCH) {
      const int dc = min(GDCH, d - m0);
      __syncthreads();
      {  // 256 % GDCH == 0: a thread always stages the same input dimension, one division per chunk (again in the length-scale pass)
        const int m = tid % GDCH;
        const double il = (m < dc) ? 1.0 / ls[c * d + m0 + m] : 0.0;
        for (int r = tid / GDCH; r < GT; r += 256 / GDCH) {
          double vi = 0.0, vj = 0.0;
          if (m < dc) {
            if (i0 + r < n) vi = X[(long)(i0 + r) * d + m0 + m] * il;
            if (j0 + r < n) vj = X[(long)(j0 + r) * d + m0 + m] * il;
          }
          Xi[r * GDLD + m] = vi;
          Xj[r * GDLD + m] = vj;
        }
      }
      __syncthreads();
      for (int m = 0; m < dc; ++m) {
        double xi[4], xj[4];  // the micro-tile's coordinates (same reads: both passes here, grad_x_kernel's pass 1)
#pragma unroll
        for (int a = 0; a < 4; ++a) xi[a] = Xi[(ty + 16 * a) * GDLD + m];
#pragma unroll
        for (int b = 0; b < 4; ++b) xj[b] = Xj[(tx + 16 * b) * GDLD + m];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const double df = xi[a] - xj[b];
            r2[a][b] += df * df;
          }
      }
    }
    const int kid = spec.kid[c];
    const double kvc = kv[c], alc = al[c];
    // (comp_val_der<RQ>, written out: through the function the NK = 4 and NK = 8 instantiations without a rational quadratic
    // come out with other vector registers)
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        double k, dk, da;
        base_kernel_val_der(kid, r2[a][b], alc, k, dk, da);
        kval[c][a][b] = kvc * k;
        dkv[c][a][b] = kvc * dk;
        if constexpr (RQ) dal[c][a][b] = kvc * da;
      }
  }
  // coefficient dK/dK_c of the left-to-right fold, times the weight (the same recurrence is in grad_x_kernel's coef_elem and
  // in predict_grad_kernel: a change to the fold goes into all three, and into assemble.hip's forward fold)
  double wc[NK][4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      double pref[NK];
      double T = kval[0][a][b];
      pref[0] = 1.0;
#pragma unroll
      for (int c = 1; c < nk; ++c) {
        pref[c] = (spec.op[c - 1] == 0) ? 1.0 : T;
        T = (spec.op[c - 1] == 0) ? T + kval[c][a][b] : T * kval[c][a][b];
      }
#pragma unroll
      for (int c = 0; c < nk; ++c) {
        double coef = pref[c];
#pragma unroll
        for (int c2 = c + 1; c2 < nk; ++c2)
          if (spec.op[c2 - 1] == 1) coef *= kval[c2][a][b];
        wc[c][a][b] = wgt[a][b] * coef;
      }
    }

  // block reduction helper
  auto block_sum = [&](double v) -> double {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
  };

  // kv, alpha, gv, jitter
#pragma unroll
  for (int c = 0; c < nk; ++c) {
    double skv = 0.0, sal = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        skv += wc[c][a][b] * kval[c][a][b];
        if constexpr (RQ) sal += wc[c][a][b] * dal[c][a][b];
      }
    skv = block_sum(skv);
    if constexpr (RQ) sal = block_sum(sal);
    if (tid == 0) {
      out[nk * d + c] = skv / kv[c];
      out[nk * d + nk + c] = sal;
    }
  }
  {
    double sd = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (i0 + ty + 16 * a == j0 + tx + 16 * b) sd += wgt[a][b];  // already carries the 1/2
    sd = block_sum(sd);
    if (tid == 0) {
      out[nk * d + 2 * nk] = sd;
      out[nk * d + 2 * nk + 1] = sd;
    }
  }
  // length scales: dK/dl_{c,m} = wc * kv dk/dr2 * (-2/l_m) * ((x_im - x_jm)/l_m)^2; G = wc * kv dk/dr2 once per element
#pragma unroll
  for (int c = 0; c < nk; ++c)
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) dkv[c][a][b] *= wc[c][a][b];
  // (one component with d <= GDCH: the scaled coordinates of pass 1 are still in LDS -- nothing to stage again)
  const bool staged = NK == 1 && d <= GDCH;
#pragma unroll
  for (int c = 0; c < nk; ++c) {
    for (int m0 = 0; m0 < d; m0 += GDCH) {
      const int dc = min(GDCH, d - m0);
      __syncthreads();
      if (!staged) {  // (pass 1's staging block, word for word)
        const int m = tid % GDCH;
        const double il = (m < dc) ? 1.0 / ls[c * d + m0 + m] : 0.0;
        for (int r = tid / GDCH; r < GT; r += 256 / GDCH) {
          double vi = 0.0, vj = 0.0;
          if (m < dc) {
            if (i0 + r < n) vi = X[(long)(i0 + r) * d + m0 + m] * il;
            if (j0 + r < n) vj = X[(long)(j0 + r) * d + m0 + m] * il;
          }
          Xi[r * GDLD + m] = vi;
          Xj[r * GDLD + m] = vj;
        }
        __syncthreads();
      }
      // per-dimension sums: wave partials of all dimensions of the chunk go to LDS, ONE barrier, then thread m adds
      // its four (same order as a per-dimension block sum, two barriers per dimension less)
      for (int m = 0; m < dc; ++m) {
        double xi[4], xj[4];  // the micro-tile's coordinates (same reads: both passes here, grad_x_kernel's pass 1)
#pragma unroll
        for (int a = 0; a < 4; ++a) xi[a] = Xi[(ty + 16 * a) * GDLD + m];
#pragma unroll
        for (int b = 0; b < 4; ++b) xj[b] = Xj[(tx + 16 * b) * GDLD + m];
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const double df = xi[a] - xj[b];
            s += dkv[c][a][b] * (df * df);
          }
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if ((tid & 63) == 0) red[4 * m + (tid >> 6)] = s;
      }
      __syncthreads();
      if (tid < dc) {
        const double s = red[4 * tid] + red[4 * tid + 1] + red[4 * tid + 2] + red[4 * tid + 3];
        out[c * d + m0 + tid] = s * (-2.0 / ls[c * d + m0 + tid]);
      }
    }
  }
}

// dLML/dX (n x d, row-major) for the inputs-as-parameters consumers (input warping, gpmcmc.py:211-233; the
// free observation rows of inverse_opt, gpmcmc.py:1096-1101):
//   dLML/dx_im = sum_j (alpha_i alpha_j - Kinv_ij) dK_ij/dx_im
//              = sum_c sum_j Wsym_ij coef_c kv_c k_c'(r2_c) * 2 (x_im - x_jm) / l_cm^2
// (row i and column i of the symmetric sum 1/2 tr(W dK) contribute equally).  One workgroup per block of
// 64 rows walks all 64-column blocks: pass 1 builds the coefficient tile C_c (same 4x4 micro-tiles as
// grad_contract) and parks it in LDS, pass 2 is the small dense product C_c (64x64) . (x_i - X_j) with
// thread (row, m mod 4).  Kinv is stored as its lower triangle only; the upper part is read transposed.
constexpr int GXCH = 16;  // input dimensions per LDS chunk
constexpr int GXLD = GXCH + 1;
constexpr int GX_MAXD = 128;  // output dimensions per grad_x pass (window)

// Input dimensions beyond GX_MAXD: the host launches one pass per WINDOW of up to 128 output dimensions [w0, w0 + dw); every
// pass recomputes the coefficient tiles from all d dimensions (pass 1) and contracts them with its window (pass 2).
template <int NK, int NCH>  // NCH: chunks of 16 input dimensions covered by one window (dw <= 16 * NCH)
__global__ __launch_bounds__(256) void grad_x_kernel(KernSpec spec, const double* __restrict__ theta,
                                                     const double* __restrict__ X, int n,
                                                     const double* __restrict__ W, long ldw,
                                                     const double* __restrict__ alpha_v, double* __restrict__ gx, int w0) {
  // gridDim.y > 1: this workgroup walks column blocks blockIdx.y, blockIdx.y + gridDim.y, ... and writes its partial
  // result to slab blockIdx.y of gx ([gridDim.y][n][d]); gx_reduce_kernel adds the slabs in order
  __shared__ double Xi[GT * GXLD];
  __shared__ double Xj[GT * GXLD];
  __shared__ double Ct[GT * (GT + 1)];
  __shared__ double ils[NK * GX_MAXD];  // 1 / l_cm of the window's dimensions
  __shared__ double ilc[NK * GXCH];     // 1 / l_cm of the pass-1 chunk being staged
  const int tid = threadIdx.x;
  const int d = spec.d;
  const int nk = RUNTIME_NK<NK> ? spec.nkern : NK;
  const int dw = min(GX_MAXD, d - w0);  // this pass's output dimensions
  const int nt = (n + GT - 1) / GT;
  const int ib = blockIdx.x, i0 = ib * GT;
  const int tx = tid & 15, ty = tid >> 4;  // pass-1 micro-tile: rows ty+16a, cols tx+16b
  const int pr = tid & 63, pq = tid >> 6;  // pass-2: row pr, dimensions m = pq (mod 4)
  const double* kv = theta + nk * d;
  const double* al = kv + nk;
  for (int e = tid; e < nk * dw; e += 256) ils[(e / dw) * GX_MAXD + e % dw] = 1.0 / theta[(e / dw) * d + w0 + e % dw];
  double acc[NCH][GXCH / 4];
#pragma unroll
  for (int mc = 0; mc < NCH; ++mc)
#pragma unroll
    for (int u = 0; u < GXCH / 4; ++u) acc[mc][u] = 0.0;

  gx += (long)blockIdx.y * n * d;
  for (int jb = blockIdx.y; jb < nt; jb += gridDim.y) {
    const int j0 = jb * GT;
    __syncthreads();  // previous block's pass 2 is done with Ct / Xj
    // symmetric weight tile, coalesced along whichever index is contiguous in the stored lower triangle
    for (int e = tid; e < GT * GT; e += 256) {
      int r, c;
      if (jb <= ib) { r = e >> 6; c = e & 63; } else { c = e >> 6; r = e & 63; }
      const int gi = i0 + r, gj = j0 + c;
      double w = 0.0;
      if (gi < n && gj < n) {
        const double kin = (gj <= gi) ? W[(long)gi * ldw + gj] : W[(long)gj * ldw + gi];
        w = alpha_v[gi] * alpha_v[gj] - kin;
      }
      Ct[r * (GT + 1) + c] = w;
    }
    // pass 1: scaled squared distances per component
    double r2[NK][4][4];
#pragma unroll
    for (int c = 0; c < nk; ++c)
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) r2[c][a][b] = 0.0;
    for (int m0 = 0; m0 < d; m0 += GXCH) {
      const int dc = min(GXCH, d - m0);
      if (m0 > 0) __syncthreads();
      for (int e = tid; e < GT * GXCH; e += 256) {
        const int r = e / GXCH, m = e % GXCH;
        double vi = 0.0, vj = 0.0;
        if (m < dc) {
          if (i0 + r < n) vi = X[(long)(i0 + r) * d + m0 + m];
          if (j0 + r < n) vj = X[(long)(j0 + r) * d + m0 + m];
        }
        Xi[r * GXLD + m] = vi;
        Xj[r * GXLD + m] = vj;
      }
      if (tid < nk * GXCH) {
        const int c = tid / GXCH, m = tid % GXCH;
        ilc[tid] = (m < dc) ? 1.0 / theta[c * d + m0 + m] : 0.0;
      }
      __syncthreads();
      for (int m = 0; m < dc; ++m) {
        double xi[4], xj[4];  // the micro-tile's coordinates (grad_contract_kernel's reads, leading dimension GXLD)
#pragma unroll
        for (int a = 0; a < 4; ++a) xi[a] = Xi[(ty + 16 * a) * GXLD + m];
#pragma unroll
        for (int b = 0; b < 4; ++b) xj[b] = Xj[(tx + 16 * b) * GXLD + m];
#pragma unroll
        for (int c = 0; c < nk; ++c) {
          const double il = ilc[c * GXCH + m];
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
    // coefficient tiles cf[c] = Wsym * (dK/dK_c of the fold) * kv_c dk_c/dr2
    double cf[NK][4][4];
    auto coef_elem = [&](int a, int b) {
      double kval[NK], dkv[NK], da;
#pragma unroll
      for (int c = 0; c < nk; ++c) comp_val_der<false>(spec.kid[c], r2[c][a][b], al[c], kv[c], kval[c], dkv[c], da);
      double pref[NK];  // dK/dK_c of the fold: grad_contract_kernel's recurrence, per element
      double T = kval[0];
      pref[0] = 1.0;
#pragma unroll
      for (int c = 1; c < nk; ++c) {
        pref[c] = (spec.op[c - 1] == 0) ? 1.0 : T;
        T = (spec.op[c - 1] == 0) ? T + kval[c] : T * kval[c];
      }
      const double w = Ct[(ty + 16 * a) * (GT + 1) + tx + 16 * b];
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
      // NOT unrolled for composite kernels.  Round 3: with the inlined exp / sqrt sequences of migp_math.h the fully unrolled
      // form (sixteen elements x NK families, 80-150 KB of code, 256 VGPRs) returned NONDETERMINISTIC dLML/dX for
      // four-component kernels -- entries of 1e13 that changed from call to call on identical inputs, while the same
      // source at -O1, with this loop rolled, or with exp behind a call is bit-reproducible and matches the oracle to
      // 2e-12; neither extra barriers nor SGPR spilling to memory changed it, so it is a code-generation problem of
      // this toolchain on the giant basic block, not a race in the source.  The rolled loop keeps the block small;
      // tests/test_gpu_data_grad.py repeats the evaluation and demands identical bits.
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
        for (int b = 0; b < 4; ++b) Ct[(ty + 16 * a) * (GT + 1) + tx + 16 * b] = cf[c][a][b];
#pragma unroll
      for (int mc = 0; mc < NCH; ++mc) {
        const int m0 = mc * GXCH;
        if (m0 >= dw) break;
        const int dc = min(GXCH, dw - m0);
        if (NCH > 1) {  // several chunks: bring this one back (a single chunk -- d <= 16, w0 = 0 -- is still resident)
          __syncthreads();
          for (int e = tid; e < GT * GXCH; e += 256) {
            const int r = e / GXCH, m = e % GXCH;
            double vi = 0.0, vj = 0.0;
            if (m < dc) {
              if (i0 + r < n) vi = X[(long)(i0 + r) * d + w0 + m0 + m];
              if (j0 + r < n) vj = X[(long)(j0 + r) * d + w0 + m0 + m];
            }
            Xi[r * GXLD + m] = vi;
            Xj[r * GXLD + m] = vj;
          }
        }
        __syncthreads();
        double t[GXCH / 4], xr[GXCH / 4];
#pragma unroll
        for (int u = 0; u < GXCH / 4; ++u) {
          t[u] = 0.0;
          xr[u] = Xi[pr * GXLD + pq + 4 * u];
        }
        for (int j = 0; j < GT; ++j) {
          const double cj = Ct[pr * (GT + 1) + j];
#pragma unroll
          for (int u = 0; u < GXCH / 4; ++u) t[u] += cj * (xr[u] - Xj[j * GXLD + pq + 4 * u]);
        }
#pragma unroll
        for (int u = 0; u < GXCH / 4; ++u) {
          const int m = m0 + pq + 4 * u;
          if (pq + 4 * u < dc) {
            const double il = ils[c * GX_MAXD + m];
            acc[mc][u] += 2.0 * il * il * t[u];
          }
        }
      }
    }
  }
  if (i0 + pr < n) {
#pragma unroll
    for (int mc = 0; mc < NCH; ++mc)
#pragma unroll
      for (int u = 0; u < GXCH / 4; ++u) {
        const int m = mc * GXCH + pq + 4 * u;
        if (m < dw) gx[(long)(i0 + pr) * d + w0 + m] = acc[mc][u];
      }
  }
}

// grad[p] = sum_b part[b][p] in a fixed order (the weights already are 1 below the diagonal and 1/2
// on it, which is 1/2 sum over the full symmetric matrix).
__global__ void grad_final_kernel(const double* __restrict__ part, int nblk, int P, double* __restrict__ grad, long spart,
                                  int sgrad, unsigned* __restrict__ done, double* __restrict__ flag, int sflag, double seq) {
  part += (long)blockIdx.z * spart;  // batched evaluation: problem blockIdx.z
  grad += (long)blockIdx.z * sgrad;
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
      // LAST kernel of an LML + gradient evaluation: the workgroup that completes the gradient publishes the evaluation's
      // sequence number, released at system scope (the host may spin on it instead of synchronising the stream)
      __threadfence_system();
      done += blockIdx.z;
      if (atomicAdd(done, 1u) == (unsigned)P - 1u) {
        *done = 0u;  // ready for the next evaluation
        __hip_atomic_store(flag + (long)blockIdx.z * sflag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}

// s1 = A_i . beta, s2 = |A_i|^2 of one row, one wave: lane-strided partial sums, then a wave64 tree (every entry point that
// predicts reduces its rows through this one sequence, so a batched row has the bits of a single one)
__device__ __forceinline__ void predict_row_sums(const double* __restrict__ a, const double* __restrict__ beta, int n, int lane,
                                                 double& s1, double& s2) {
  s1 = 0.0;
  s2 = 0.0;
  for (int k = lane; k < n; k += 64) {
    const double v = a[k];
    s1 += v * beta[k];
    s2 += v * v;
  }
  for (int off = 32; off > 0; off >>= 1) {
    s1 += __shfl_down(s1, off, 64);
    s2 += __shfl_down(s2, off, 64);
  }
}

// mean[i] = A_i . beta ; var[i] = kdiag - |A_i|^2 (+ noise), one wave per prediction point
__global__ __launch_bounds__(256) void predict_reduce_kernel(const double* __restrict__ A, long lda,
                                                             const double* __restrict__ beta, int n, int m,
                                                             double kdiag, double noise, double* __restrict__ mean,
                                                             double* __restrict__ var) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= m) return;
  double s1, s2;
  predict_row_sums(A + (long)row * lda, beta, n, lane, s1, s2);
  if (lane == 0) {
    mean[row] = s1;
    var[row] = kdiag - s2 + noise;
  }
}

// The prior diagonal and the predictive noise of one theta, as mi_gp_predict folds them on the host: Stationary.diag == 1, so
// the composite diagonal is the +/* fold of kv; the noise is sqrt(gv)^2.  Contraction off: the host has no FMA here, and
// kd * kv_c + kv_(c+1) fused would be another rounding.
__device__ __forceinline__ void prior_diag_noise(const KernSpec& spec, const double* __restrict__ th, int pred_noise, double& kd,
                                                 double& noise) {
#pragma clang fp contract(off)
  const int nk = spec.nkern, d = spec.d;
  kd = th[nk * d];
  for (int c = 1; c < nk; ++c) kd = (spec.op[c - 1] == 0) ? kd + th[nk * d + c] : kd * th[nk * d + c];
  noise = 0.0;
  if (pred_noise) {
    const double sg = sqrt(th[nk * d + 2 * nk]);  // (correctly rounded, as std::sqrt on the host)
    noise = sg * sg;
  }
}

// predict_reduce_kernel for problem blockIdx.z of a batch (mi_gp_predict_batch); rows of a problem without a positive-definite
// factor are NaN
__global__ __launch_bounds__(256) void predict_reduce_batch_kernel(KernSpec spec, const double* __restrict__ theta, int stheta,
                                                                   const double* __restrict__ A, long lda, long sA,
                                                                   const double* __restrict__ beta, long sbeta,
                                                                   const int* __restrict__ info, int sinfo, int n, int m,
                                                                   int pred_noise, double* __restrict__ mean,
                                                                   double* __restrict__ var) {
  const int z = blockIdx.z;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= m) return;
  mean += (long)z * m;
  var += (long)z * m;
  if (info[(long)z * sinfo] != INFO_OK) {
    if (lane == 0) mean[row] = var[row] = __builtin_nan("");
    return;
  }
  double s1, s2;
  predict_row_sums(A + (long)z * sA + (long)row * lda, beta + (long)z * sbeta, n, lane, s1, s2);
  if (lane == 0) {
    double kd, noise;
    prior_diag_noise(spec, theta + (long)z * stheta, pred_noise, kd, noise);
    mean[row] = s1;
    var[row] = kd - s2 + noise;
  }
}

// Equal-weight mixture of the k problems' moments at each point, one thread per point: two passes over the problems in index
// order (the bits do not depend on the launch), the sums taken relative to the first member's moments -- the same quantities,
// no cancellation in the sums, and draws that all agree return that draw's moments exactly.  Reads 3 k m doubles (the means
// twice), writes 2 m: bandwidth-bound; the threads of a wave read consecutive points of one problem.
__global__ __launch_bounds__(256) void mixture_moments_kernel(const double* __restrict__ mean, const double* __restrict__ var,
                                                              int m, int k, const int* __restrict__ info, int sinfo,
                                                              double* __restrict__ mix_mean, double* __restrict__ mix_var) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  int cnt = 0, p0 = -1;
  double mu0 = 0.0, s = 0.0;
  for (int p = 0; p < k; ++p)
    if (info[(long)p * sinfo] == INFO_OK) {
      const double v = mean[(long)p * m + i];
      if (p0 < 0) { p0 = p; mu0 = v; }
      s += v - mu0;
      ++cnt;
    }
  if (cnt == 0) {
    mix_mean[i] = mix_var[i] = __builtin_nan("");
    return;
  }
  const double mu = mu0 + s / cnt;
  const double v0 = var[(long)p0 * m + i];
  double sv = 0.0, sd = 0.0;
  for (int p = p0; p < k; ++p)
    if (info[(long)p * sinfo] == INFO_OK) {
      const double dl = mean[(long)p * m + i] - mu;
      sv += var[(long)p * m + i] - v0;
      sd += dl * dl;
    }
  mix_mean[i] = mu;
  mix_var[i] = v0 + sv / cnt + sd / cnt;
}

hipError_t launch_set_identity_blocks(double* U, long ld, int nblocks, hipStream_t stream, const Batch* bt) {
  set_identity_blocks_kernel<<<dim3(nblocks, 1, bt ? bt->nb : 1), 256, 0, stream>>>(U, ld, bt ? bt->sZ : 0);
  return hipGetLastError();
}

hipError_t launch_trmv_upper(const double* U, long ld, const double* beta, int n, double* alpha, hipStream_t stream,
                             const Batch* bt) {
  trmv_upper_kernel<<<dim3((n + 3) / 4, 1, bt ? bt->nb : 1), 256, 0, stream>>>(U, ld, beta, n, alpha, bt ? bt->sZ : 0, bt ? bt->sK : 0,
                                                                               bt ? bt->salpha : 0);
  return hipGetLastError();
}

int grad_contract_blocks(int n) {
  const int nt = (n + GT - 1) / GT;
  return nt * (nt + 1) / 2;
}

static bool has_ratquad(const KernSpec& spec) {
  for (int c = 0; c < spec.nkern; ++c)
    if (spec.kid[c] == KID_RATQUAD) return true;
  return false;
}

// Every instantiation of the three gradient kernels stands in one table per kernel (GRAD_CONTRACT_KERNELS here,
// GRAD_X_KERNELS and PREDICT_GRAD_KERNELS ahead of their launchers).  One to four components have an instantiation of their
// own, five to eight share <8>: slot nk_slot(nkern) of each table.
static int nk_slot(int nkern) { return nkern >= 1 && nkern <= 4 ? nkern - 1 : 4; }

static const decltype(&grad_contract_kernel<1, false>) GRAD_CONTRACT_KERNELS[5][2] = {  // [slot][a component is a rational quadratic]
    {grad_contract_kernel<1, false>, grad_contract_kernel<1, true>}, {grad_contract_kernel<2, false>, grad_contract_kernel<2, true>},
    {grad_contract_kernel<3, false>, grad_contract_kernel<3, true>}, {grad_contract_kernel<4, false>, grad_contract_kernel<4, true>},
    {grad_contract_kernel<8, false>, grad_contract_kernel<8, true>}};

// The contraction over grid.x tiles (grid.z problems) with the kernel's eight trailing arguments, then the fixed-order sum
// of the tiles' partials
static hipError_t launch_contract(const KernSpec& spec, const double* theta, const double* X, int n, const double* W, long ldw,
                                  const double* alpha, double* part, double* grad, hipStream_t stream, dim3 grid,
                                  int rect_tw, int tj0, long wrow0, long wcol0, int stheta, long sW, long salpha, long spart,
                                  unsigned* done, double* flag, int sflag, double seq) {
  const int P = spec.nkern * spec.d + 2 * spec.nkern + 2;
  GRAD_CONTRACT_KERNELS[nk_slot(spec.nkern)][has_ratquad(spec)]<<<grid, 256, 0, stream>>>(
      spec, theta, X, n, W, ldw, alpha, part, rect_tw, tj0, wrow0, wcol0, stheta, sW, salpha, spart);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  grad_final_kernel<<<dim3(P, 1, grid.z), 256, 0, stream>>>(part, (int)grid.x, P, grad, spart, stheta, done, flag, sflag, seq);
  return hipGetLastError();
}

hipError_t launch_grad_contract(const KernSpec& spec, const double* theta, const double* X, int n, const double* W,
                                long ldw, const double* alpha, double* part, double* grad, hipStream_t stream, const Batch* bt,
                                unsigned* done, double* flag, double seq) {
  const int nblk = grad_contract_blocks(n);
  return launch_contract(spec, theta, X, n, W, ldw, alpha, part, grad, stream, dim3(nblk, 1, bt ? bt->nb : 1), 0, 0, 0, 0,
                         bt ? bt->stheta : 0, bt ? bt->sW : 0, bt ? bt->salpha : 0, bt ? bt->spart : 0, done, flag,
                         bt ? bt->sout : 0, seq);
}

// Column slab [col0, col0 + cols) of the lower triangle (rows >= col0): W points at element (row0, col0) of K^-1,
// row0 <= col0, both multiples of 64.  Its tiles: columns [tj0, tj0 + tw), rows from tj0 down; tw <= 0: beyond the last column.
struct SlabTiles {
  int tj0, tw, nblk;
  SlabTiles(int n, int col0, int cols) {
    const int nt = (n + GT - 1) / GT;
    tj0 = col0 / GT;
    tw = min((cols + GT - 1) / GT, nt - tj0);
    nblk = tw <= 0 ? 0 : (nt - tj0) * tw;
  }
};

// part: grad_contract_slab_blocks() x ntheta doubles
int grad_contract_slab_blocks(int n, int col0, int cols) { return SlabTiles(n, col0, cols).nblk; }

hipError_t launch_grad_contract_slab(const KernSpec& spec, const double* theta, const double* X, int n, const double* W,
                                     long ldw, int row0, int col0, int cols, const double* alpha, double* part,
                                     double* grad, hipStream_t stream) {
  const SlabTiles sl(n, col0, cols);
  if (sl.tw <= 0) return hipMemsetAsync(grad, 0, sizeof(double) * (spec.nkern * spec.d + 2 * spec.nkern + 2), stream);
  return launch_contract(spec, theta, X, n, W, ldw, alpha, part, grad, stream, dim3(sl.nblk), sl.tw, sl.tj0, row0, col0,
                         0, 0, 0, 0, nullptr, nullptr, 0, 0.0);
}

// Gradient of the posterior conditional w.r.t. ONE prediction point x* (converted inputs):
//   d mu / d x*_m  =  sum_i alpha_i dk(x_i, x*)/dx*_m,     d var / d x*_m = -2 sum_i w_i dk(x_i, x*)/dx*_m,
// with alpha = K^-1 y, w = K^-1 k(X, x*) and dk/dx*_m = sum_c coef_c kv_c k_c'(r2_c) 2 (x*_m - x_im) / l_cm^2
// (Stationary.diag is constant, so the prior variance does not move).  This is the differentiable single-point
// predictive that BO's refinement step builds in PyTensor at gpmcmc.py:766-778 and maximises with pm.find_MAP.
// One workgroup per point; dimensions in chunks of 16 held in registers, block-reduced through LDS.
template <int NK>
__global__ __launch_bounds__(256) void predict_grad_kernel(KernSpec spec, const double* __restrict__ theta,
                                                           const double* __restrict__ X, int n,
                                                           const double* __restrict__ xstar,
                                                           const double* __restrict__ alpha_v,
                                                           const double* __restrict__ wv, long ldwv,
                                                           double* __restrict__ dmean, double* __restrict__ dvar) {
  extern __shared__ double pg_dyn[];  // xs[d], then ils[NK][d]: sized by the launcher (any d that fits 64 KB of LDS)
  __shared__ double red[2][GXCH][4];
  const int tid = threadIdx.x;
  const int d = spec.d;
  const int nk = RUNTIME_NK<NK> ? spec.nkern : NK;
  double* xs = pg_dyn;
  double* ils = pg_dyn + d;
  const int p = blockIdx.x;
  const double* kv = theta + nk * d;
  const double* al = kv + nk;
  const double* w = wv + (long)p * ldwv;
  for (int e = tid; e < d; e += 256) xs[e] = xstar[(long)p * d + e];
  for (int e = tid; e < nk * d; e += 256) ils[e] = 1.0 / theta[e];
  __syncthreads();
  for (int m0 = 0; m0 < d; m0 += GXCH) {
    const int dc = min(GXCH, d - m0);
    double am[GXCH], av[GXCH];
#pragma unroll
    for (int u = 0; u < GXCH; ++u) am[u] = av[u] = 0.0;
    for (int i = tid; i < n; i += 256) {
      const double* xi = X + (long)i * d;
      double kval[NK], dkv[NK];
#pragma unroll
      for (int c = 0; c < nk; ++c) {
        double r2 = 0.0;
        for (int m = 0; m < d; ++m) {
          const double df = (xs[m] - xi[m]) * ils[c * d + m];
          r2 += df * df;
        }
        double da;
        comp_val_der<false>(spec.kid[c], r2, al[c], kv[c], kval[c], dkv[c], da);
      }
      double pref[NK];  // dK/dK_c of the fold: grad_contract_kernel's recurrence, per training point
      double T = kval[0];
      pref[0] = 1.0;
#pragma unroll
      for (int c = 1; c < nk; ++c) {
        pref[c] = (spec.op[c - 1] == 0) ? 1.0 : T;
        T = (spec.op[c - 1] == 0) ? T + kval[c] : T * kval[c];
      }
      const double ai = alpha_v[i], wi = -2.0 * w[i];
#pragma unroll
      for (int c = 0; c < nk; ++c) {
        double coef = pref[c];
#pragma unroll
        for (int c2 = c + 1; c2 < nk; ++c2)
          if (spec.op[c2 - 1] == 1) coef *= kval[c2];
        const double g = coef * dkv[c];
#pragma unroll
        for (int u = 0; u < GXCH; ++u) {
          if (u < dc) {
            const double il = ils[c * d + m0 + u];
            const double dkx = g * 2.0 * (xs[m0 + u] - xi[m0 + u]) * il * il;
            am[u] += ai * dkx;
            av[u] += wi * dkx;
          }
        }
      }
    }
    // fixed-order block reduction: wave shuffle, then the four wave sums
#pragma unroll
    for (int u = 0; u < GXCH; ++u) {
      double a = am[u], b = av[u];
      for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off, 64);
        b += __shfl_down(b, off, 64);
      }
      if ((tid & 63) == 0) { red[0][u][tid >> 6] = a; red[1][u][tid >> 6] = b; }
    }
    __syncthreads();
    if (tid < dc) {
      dmean[(long)p * d + m0 + tid] = red[0][tid][0] + red[0][tid][1] + red[0][tid][2] + red[0][tid][3];
      dvar[(long)p * d + m0 + tid] = red[1][tid][0] + red[1][tid][1] + red[1][tid][2] + red[1][tid][3];
    }
    __syncthreads();
  }
}

static const decltype(&predict_grad_kernel<1>) PREDICT_GRAD_KERNELS[5] = {  // [slot]
    predict_grad_kernel<1>, predict_grad_kernel<2>, predict_grad_kernel<3>, predict_grad_kernel<4>, predict_grad_kernel<8>};

hipError_t launch_predict_grad(const KernSpec& spec, const double* theta, const double* X, int n, const double* xstar,
                               int m, const double* alpha, const double* w, long ldw, double* dmean, double* dvar,
                               hipStream_t stream) {
  const size_t lds = sizeof(double) * (size_t)(spec.nkern + 1) * spec.d;
  if (lds > PREDICT_GRAD_MAX_LDS) return hipErrorInvalidValue;  // (mi_gp_predict_grad says which d fit)
  PREDICT_GRAD_KERNELS[nk_slot(spec.nkern)]<<<m, 256, lds, stream>>>(spec, theta, X, n, xstar, alpha, w, ldw, dmean, dvar);
  return hipGetLastError();
}

// ---- mi_gp_logpdf's gradient: dx_im = sum_j C_ij dk(x*_i, x_j)/dx*_im + sum_j D_ij dk(x*_i, x*_j)/dx*_im (api_gp.hip)

// Row i of S^-1 = L22^-T L22^-1 per workgroup (thread j: sum over l >= max(i, j) in index order), and gamma_i = (L22^-T beta2)_i
// by its thread 0.  Linv is lower triangular with the identity in the padding, beta2 zero there: so are Sinv and gamma.
__global__ __launch_bounds__(128) void logpdf_sinv_kernel(const double* __restrict__ Linv, const double* __restrict__ beta2,
                                                          double* __restrict__ Sinv, double* __restrict__ gamma) {
  const int i = blockIdx.x, j = threadIdx.x;
  double s = 0.0;
  for (int l = max(i, j); l < 128; ++l) s = __builtin_fma(Linv[l * 128 + i], Linv[l * 128 + j], s);
  Sinv[i * 128 + j] = s;
  if (j == 0) {
    double g = 0.0;
    for (int l = i; l < 128; ++l) g = __builtin_fma(Linv[l * 128 + i], beta2[l], g);
    gamma[i] = g;
  }
}

// One thread per training point j: C[i][j] = gamma_i (alpha_j - sum_l gamma_l P[l][j]) + Q[i][j] over Q, in place
__global__ __launch_bounds__(256) void logpdf_weights_kernel(double* __restrict__ Cw, const double* __restrict__ P, long ldw,
                                                             const double* __restrict__ alpha_v, const double* __restrict__ gamma,
                                                             int n, int k, double* __restrict__ dy) {
  __shared__ double g[128];
  const int tid = threadIdx.x;
  if (tid < 128) g[tid] = tid < k ? gamma[tid] : 0.0;
  __syncthreads();
  if (dy && blockIdx.x == 0 && tid < k) dy[tid] = -g[tid];
  const int j = blockIdx.x * 256 + tid;
  if (j >= n) return;
  double t = 0.0;
  for (int l = 0; l < k; ++l) t = __builtin_fma(g[l], P[(long)l * ldw + j], t);
  const double a = alpha_v[j] - t;
  for (int i = 0; i < k; ++i) Cw[(long)i * ldw + j] = __builtin_fma(g[i], a, Cw[(long)i * ldw + j]);
}

// Twin of predict_grad_kernel (its dimension chunks, fold derivative and fixed-order block reduction, word for word where the
// two agree): one workgroup per trial point p, ONE accumulator set over two point segments -- the n training points with the
// weights of row p of C, then the kk trial points with D_pj = gamma_p gamma_j - Sinv[p][j].  A coincident point (the trial
// point itself, duplicates, a training point) contributes 0 through its zero coordinate difference.
template <int NK>
__global__ __launch_bounds__(256) void logpdf_grad_kernel(KernSpec spec, const double* __restrict__ theta,
                                                          const double* __restrict__ X, int n,
                                                          const double* __restrict__ xstar, int kk,
                                                          const double* __restrict__ Cw, long ldw,
                                                          const double* __restrict__ gamma, const double* __restrict__ Sinv,
                                                          double* __restrict__ dx) {
  extern __shared__ double pg_dyn[];  // xs[d], then ils[NK][d]: sized by the launcher (any d that fits 64 KB of LDS)
  __shared__ double red[GXCH][4];
  const int tid = threadIdx.x;
  const int d = spec.d;
  const int nk = RUNTIME_NK<NK> ? spec.nkern : NK;
  double* xs = pg_dyn;
  double* ils = pg_dyn + d;
  const int p = blockIdx.x;
  const double* kv = theta + nk * d;
  const double* al = kv + nk;
  const double* crow = Cw + (long)p * ldw;
  const double* srow = Sinv + p * 128;
  const double gp = gamma[p];
  for (int e = tid; e < d; e += 256) xs[e] = xstar[(long)p * d + e];
  for (int e = tid; e < nk * d; e += 256) ils[e] = 1.0 / theta[e];
  __syncthreads();
  for (int m0 = 0; m0 < d; m0 += GXCH) {
    const int dc = min(GXCH, d - m0);
    double am[GXCH];
#pragma unroll
    for (int u = 0; u < GXCH; ++u) am[u] = 0.0;
    for (int i = tid; i < n + kk; i += 256) {
      const bool trial = i >= n;
      const double* xi = trial ? xstar + (long)(i - n) * d : X + (long)i * d;
      const double wi = trial ? gp * gamma[i - n] - srow[i - n] : crow[i];
      double kval[NK], dkv[NK];
#pragma unroll
      for (int c = 0; c < nk; ++c) {
        double r2 = 0.0;
        for (int m = 0; m < d; ++m) {
          const double df = (xs[m] - xi[m]) * ils[c * d + m];
          r2 += df * df;
        }
        double da;
        comp_val_der<false>(spec.kid[c], r2, al[c], kv[c], kval[c], dkv[c], da);
      }
      double pref[NK];  // dK/dK_c of the fold: grad_contract_kernel's recurrence, per point
      double T = kval[0];
      pref[0] = 1.0;
#pragma unroll
      for (int c = 1; c < nk; ++c) {
        pref[c] = (spec.op[c - 1] == 0) ? 1.0 : T;
        T = (spec.op[c - 1] == 0) ? T + kval[c] : T * kval[c];
      }
#pragma unroll
      for (int c = 0; c < nk; ++c) {
        double coef = pref[c];
#pragma unroll
        for (int c2 = c + 1; c2 < nk; ++c2)
          if (spec.op[c2 - 1] == 1) coef *= kval[c2];
        const double g = coef * dkv[c];
#pragma unroll
        for (int u = 0; u < GXCH; ++u) {
          if (u < dc) {
            const double il = ils[c * d + m0 + u];
            const double dkx = g * 2.0 * (xs[m0 + u] - xi[m0 + u]) * il * il;
            am[u] += wi * dkx;
          }
        }
      }
    }
    // fixed-order block reduction: wave shuffle, then the four wave sums
#pragma unroll
    for (int u = 0; u < GXCH; ++u) {
      double a = am[u];
      for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
      if ((tid & 63) == 0) red[u][tid >> 6] = a;
    }
    __syncthreads();
    if (tid < dc) dx[(long)p * d + m0 + tid] = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
    __syncthreads();
  }
}

static const decltype(&logpdf_grad_kernel<1>) LOGPDF_GRAD_KERNELS[5] = {  // [slot]
    logpdf_grad_kernel<1>, logpdf_grad_kernel<2>, logpdf_grad_kernel<3>, logpdf_grad_kernel<4>, logpdf_grad_kernel<8>};

hipError_t launch_logpdf_sinv(const double* Linv, const double* beta2, double* Sinv, double* gamma, hipStream_t stream) {
  logpdf_sinv_kernel<<<128, 128, 0, stream>>>(Linv, beta2, Sinv, gamma);
  return hipGetLastError();
}

hipError_t launch_logpdf_weights(double* Cw, const double* P, long ldw, const double* alpha, const double* gamma, int n, int k,
                                 double* dy, hipStream_t stream) {
  logpdf_weights_kernel<<<(n + 255) / 256, 256, 0, stream>>>(Cw, P, ldw, alpha, gamma, n, k, dy);
  return hipGetLastError();
}

hipError_t launch_logpdf_grad(const KernSpec& spec, const double* theta, const double* X, int n, const double* xstar, int k,
                              const double* Cw, long ldw, const double* gamma, const double* Sinv, double* dx, hipStream_t stream) {
  const size_t lds = sizeof(double) * (size_t)(spec.nkern + 1) * spec.d;
  if (lds > PREDICT_GRAD_MAX_LDS) return hipErrorInvalidValue;  // (mi_gp_logpdf says which d fit)
  LOGPDF_GRAD_KERNELS[nk_slot(spec.nkern)]<<<k, 256, lds, stream>>>(spec, theta, X, n, xstar, k, Cw, ldw, gamma, Sinv, dx);
  return hipGetLastError();
}

hipError_t launch_trmv_upper_t(const double* U, long ld, const double* x, int n, double* out, hipStream_t stream) {
  trmv_upper_t_kernel<<<(n + 63) / 64, 256, 0, stream>>>(U, ld, x, n, out);
  return hipGetLastError();
}

__global__ void gx_reduce_kernel(const double* __restrict__ part, int nsplit, long len, double* __restrict__ gx) {
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < len; e += (long)gridDim.x * blockDim.x) {
    double s = part[e];
    for (int k = 1; k < nsplit; ++k) s += part[(long)k * len + e];
    gx[e] = s;
  }
}

int grad_x_splits(int n, int d) {
  const int nrb = (n + GT - 1) / GT;
  int s = (512 + nrb - 1) / nrb;
  if (s > 8) s = 8;
  if (s > nrb) s = nrb;
  while (s > 1 && (size_t)s * n * d * sizeof(double) > ((size_t)256 << 20)) --s;
  return s < 1 ? 1 : s;
}

static const decltype(&grad_x_kernel<1, 1>) GRAD_X_KERNELS[5][3] = {  // [slot][window of 1, 2, GX_MAXD / GXCH = 8 chunks]
    {grad_x_kernel<1, 1>, grad_x_kernel<1, 2>, grad_x_kernel<1, 8>}, {grad_x_kernel<2, 1>, grad_x_kernel<2, 2>, grad_x_kernel<2, 8>},
    {grad_x_kernel<3, 1>, grad_x_kernel<3, 2>, grad_x_kernel<3, 8>}, {grad_x_kernel<4, 1>, grad_x_kernel<4, 2>, grad_x_kernel<4, 8>},
    {grad_x_kernel<8, 1>, grad_x_kernel<8, 2>, grad_x_kernel<8, 8>}};
static_assert(GX_MAXD / GXCH == 8, "GRAD_X_KERNELS' last column is the full window");

// scratch: [grad_x_splits(n, d)][n][d] doubles when more than one split is used (may be null otherwise)
hipError_t launch_grad_x(const KernSpec& spec, const double* theta, const double* X, int n, const double* W, long ldw,
                         const double* alpha, double* gx_out, double* scratch, hipStream_t stream) {
  const int nsplit = scratch ? grad_x_splits(n, spec.d) : 1;
  double* gx = nsplit > 1 ? scratch : gx_out;
  const dim3 nblk((n + GT - 1) / GT, nsplit);
  // one pass per window of GX_MAXD output dimensions (a single pass up to d = 128)
  const auto kern = GRAD_X_KERNELS[nk_slot(spec.nkern)][spec.d <= GXCH ? 0 : spec.d <= 2 * GXCH ? 1 : 2];
  for (int w0 = 0; w0 < spec.d; w0 += GX_MAXD) kern<<<nblk, 256, 0, stream>>>(spec, theta, X, n, W, ldw, alpha, gx, w0);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || nsplit == 1) return e;
  const long len = (long)n * spec.d;
  gx_reduce_kernel<<<(int)((len + 255) / 256 < 1024 ? (len + 255) / 256 : 1024), 256, 0, stream>>>(scratch, nsplit, len, gx_out);
  return hipGetLastError();
}

hipError_t launch_predict_reduce(const double* A, long lda, const double* beta, int n, int m, double kdiag,
                                 double noise, double* mean, double* var, hipStream_t stream) {
  predict_reduce_kernel<<<(m + 3) / 4, 256, 0, stream>>>(A, lda, beta, n, m, kdiag, noise, mean, var);
  return hipGetLastError();
}

hipError_t launch_predict_reduce_batched(const KernSpec& spec, const double* theta, const double* A, long lda, const double* beta,
                                         const int* info, int n, int m, int pred_noise, double* mean, double* var,
                                         hipStream_t stream, const Batch& bt) {
  predict_reduce_batch_kernel<<<dim3((m + 3) / 4, 1, bt.nb), 256, 0, stream>>>(spec, theta, bt.stheta, A, lda, bt.swork, beta, bt.sK,
                                                                              info, bt.sinfo, n, m, pred_noise, mean, var);
  return hipGetLastError();
}

hipError_t launch_mixture_moments(const double* mean, const double* var, int m, int k, const int* info, int sinfo,
                                  double* mix_mean, double* mix_var, hipStream_t stream) {
  mixture_moments_kernel<<<(m + 255) / 256, 256, 0, stream>>>(mean, var, m, k, info, sinfo, mix_mean, mix_var);
  return hipGetLastError();
}

}  // namespace migp
