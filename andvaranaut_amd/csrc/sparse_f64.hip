// Kernels of the sparse inducing-point bound (api_sparse.hip; include/mi_gp_sparse.h has the algebra):
//   sparse_contract : sum_iu T_iu dK(x_i, z_u)/dtheta_k over one chunk of data points, all parameters in one pass -- the
//                     rectangular twin of grad_contract_kernel (grad_predict.hip)
//   sparse_grad_accum : the tiles' partial sums of a chunk added in a fixed order onto the chunks before it
//   the m-sized helpers around the factorisations of Kuu and B (v and y^T y, B = I + Psi / s, the scalars of F, H and G0) and
//   the reduction of a block of query rows to mean and variance
// Every sum runs in a fixed order; nothing here uses atomics.
#include "migp_kernels.h"
#include "migp_math.h"

namespace migp {

constexpr int ST = 64;    // contraction tile (grad_contract_kernel's GT)
constexpr int SDCH = 32;  // input dimensions per LDS chunk (its GDCH)
constexpr int SDLD = SDCH + 1;

// One 64 x 64 tile of the cnt x m cross-covariance K(X_c, Z) per workgroup: tile row blockIdx.x / ntu over the chunk's points,
// tile column blockIdx.x % ntu over the inducing points; thread (ty, tx) owns the 4x4 strided micro-tile rows ty+16a, cols
// tx+16b.  part[blockIdx.x][p] receives the block's partial sums in the C-ABI's parameter order ls(nk*d), kv(nk), alpha(nk), gv,
// jitter; the last two are zero, a cross-covariance has no diagonal term.
// The rectangular twin of grad_contract_kernel (grad_predict.hip): two point sets instead of one, FULL weights
// w_iu = T[i][u] + y_i t_u (the rank-one part of T_c^T is formed here instead of in a pass of its own), no symmetric halving and
// no alpha_i alpha_j term.  The per-component r2 in the direct form, the value / derivative of the base kernels, the fold's
// derivative, the micro-tile reads, the staging and the per-dimension sums are that kernel's, word for word; its occupancy note
// (bound by LDS and exp latency, not by issue) holds here too, so the launch bounds are the same.
template <int NK, bool RQ>
__global__ __launch_bounds__(256, NK == 1 ? 3 : (NK == 2 && !RQ) ? 2 : 1) void sparse_contract_kernel(
    KernSpec spec, const double* __restrict__ theta, const double* __restrict__ X, int cnt, const double* __restrict__ Z, int m,
    const double* __restrict__ T, long ldt, const double* __restrict__ yv, const double* __restrict__ tv, int ntu,
    double* __restrict__ part) {
  __shared__ double Xi[ST * SDLD];
  __shared__ double Xj[ST * SDLD];
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const int d = spec.d;
  const int nk = RUNTIME_NK<NK> ? spec.nkern : NK;
  const int P = nk * d + 2 * nk + 2;
  double* out = part + (long)blockIdx.x * P;
  const int ti = blockIdx.x / ntu, tj = blockIdx.x % ntu;
  const int i0 = ti * ST, j0 = tj * ST;
  const int tx = tid & 15, ty = tid >> 4;
  const double* ls = theta;
  const double* kv = theta + nk * d;
  const double* al = kv + nk;

  // weights: w_ab = T_iu + y_i t_u, zero in the padding of either set
  double wgt[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int gi = i0 + ty + 16 * a, gj = j0 + tx + 16 * b;
      double w = 0.0;
      if (gi < cnt && gj < m) w = T[(long)gi * ldt + gj] + yv[gi] * tv[gj];
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
    for (int m0 = 0; m0 < d; m0 += SDCH) {
      const int dc = min(SDCH, d - m0);
      __syncthreads();
      {  // (grad_contract_kernel's staging block with the second set read from Z)
        const int mm = tid % SDCH;
        const double il = (mm < dc) ? 1.0 / ls[c * d + m0 + mm] : 0.0;
        for (int r = tid / SDCH; r < ST; r += 256 / SDCH) {
          double vi = 0.0, vj = 0.0;
          if (mm < dc) {
            if (i0 + r < cnt) vi = X[(long)(i0 + r) * d + m0 + mm] * il;
            if (j0 + r < m) vj = Z[(long)(j0 + r) * d + m0 + mm] * il;
          }
          Xi[r * SDLD + mm] = vi;
          Xj[r * SDLD + mm] = vj;
        }
      }
      __syncthreads();
      for (int mm = 0; mm < dc; ++mm) {
        double xi[4], xj[4];  // the micro-tile's coordinates (grad_contract_kernel's reads)
#pragma unroll
        for (int a = 0; a < 4; ++a) xi[a] = Xi[(ty + 16 * a) * SDLD + mm];
#pragma unroll
        for (int b = 0; b < 4; ++b) xj[b] = Xj[(tx + 16 * b) * SDLD + mm];
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
    // (comp_val_der<RQ>, written out as in grad_contract_kernel)
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
  // coefficient dK/dK_c of the left-to-right fold, times the weight (grad_contract_kernel's recurrence: a change to the fold
  // goes into it, grad_x_kernel's coef_elem, predict_grad_kernel, this kernel and assemble.hip's forward fold)
  double wc[NK][4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      double pref[NK];
      double Tf = kval[0][a][b];
      pref[0] = 1.0;
#pragma unroll
      for (int c = 1; c < nk; ++c) {
        pref[c] = (spec.op[c - 1] == 0) ? 1.0 : Tf;
        Tf = (spec.op[c - 1] == 0) ? Tf + kval[c][a][b] : Tf * kval[c][a][b];
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

  // block reduction helper (grad_contract_kernel's)
  auto block_sum = [&](double v) -> double {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
  };

  // kv, alpha; gv and jitter do not enter a cross-covariance
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
  if (tid == 0) {
    out[nk * d + 2 * nk] = 0.0;
    out[nk * d + 2 * nk + 1] = 0.0;
  }
  // length scales: dK/dl_{c,m} = wc * kv dk/dr2 * (-2/l_m) * ((x_im - z_um)/l_m)^2; G = wc * kv dk/dr2 once per element
#pragma unroll
  for (int c = 0; c < nk; ++c)
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) dkv[c][a][b] *= wc[c][a][b];
  // (one component with d <= SDCH: the scaled coordinates of pass 1 are still in LDS -- nothing to stage again)
  const bool staged = NK == 1 && d <= SDCH;
#pragma unroll
  for (int c = 0; c < nk; ++c) {
    for (int m0 = 0; m0 < d; m0 += SDCH) {
      const int dc = min(SDCH, d - m0);
      __syncthreads();
      if (!staged) {  // (pass 1's staging block, word for word)
        const int mm = tid % SDCH;
        const double il = (mm < dc) ? 1.0 / ls[c * d + m0 + mm] : 0.0;
        for (int r = tid / SDCH; r < ST; r += 256 / SDCH) {
          double vi = 0.0, vj = 0.0;
          if (mm < dc) {
            if (i0 + r < cnt) vi = X[(long)(i0 + r) * d + m0 + mm] * il;
            if (j0 + r < m) vj = Z[(long)(j0 + r) * d + m0 + mm] * il;
          }
          Xi[r * SDLD + mm] = vi;
          Xj[r * SDLD + mm] = vj;
        }
        __syncthreads();
      }
      // per-dimension sums: wave partials of all dimensions of the chunk go to LDS, ONE barrier, then thread mm adds its four
      for (int mm = 0; mm < dc; ++mm) {
        double xi[4], xj[4];  // the micro-tile's coordinates (grad_contract_kernel's reads)
#pragma unroll
        for (int a = 0; a < 4; ++a) xi[a] = Xi[(ty + 16 * a) * SDLD + mm];
#pragma unroll
        for (int b = 0; b < 4; ++b) xj[b] = Xj[(tx + 16 * b) * SDLD + mm];
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const double df = xi[a] - xj[b];
            s += dkv[c][a][b] * (df * df);
          }
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if ((tid & 63) == 0) red[4 * mm + (tid >> 6)] = s;
      }
      __syncthreads();
      if (tid < dc) {
        const double s = red[4 * tid] + red[4 * tid + 1] + red[4 * tid + 2] + red[4 * tid + 3];
        out[c * d + m0 + tid] = s * (-2.0 / ls[c * d + m0 + tid]);
      }
    }
  }
}

// acc[p] = (first ? 0 : acc[p]) + sum_b part[b][p]: the tiles of one chunk in grad_final_kernel's fixed tree, the chunks in the
// order of the launches on the stream
__global__ __launch_bounds__(256) void sparse_grad_accum_kernel(const double* __restrict__ part, int nblk, int P,
                                                                double* __restrict__ acc, int first) {
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
  if (threadIdx.x == 0) acc[p] = first ? red[0] : acc[p] + red[0];
}

// v[u] (+)= sum_{i < cnt} At[i][u] y[i] for the 64 columns of workgroup blockIdx.x < gridDim.x - 1 (wave g walks the rows
// i = g mod 4, eight sums in flight; the partial sums meet in a fixed order: trmv_upper_t_kernel's scheme over a rectangle);
// the last workgroup adds sum y_i^2 onto yy[0]
__global__ __launch_bounds__(256) void sparse_accum_vy_kernel(const double* __restrict__ At, long ld, const double* __restrict__ y,
                                                              int cnt, double* __restrict__ v, double* __restrict__ yy, int first) {
  __shared__ double part[4][64];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  if (blockIdx.x == gridDim.x - 1) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < cnt; i += 256) s += y[i] * y[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) yy[0] = first ? red[0] : yy[0] + red[0];
    return;
  }
  const int u = blockIdx.x * 64 + c;
  double s[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) s[q] = 0.0;
  int i = g;
  for (; i + 28 < cnt; i += 32) {
#pragma unroll
    for (int q = 0; q < 8; ++q) s[q] += At[(long)(i + 4 * q) * ld + u] * y[i + 4 * q];
  }
  for (; i < cnt; i += 4) s[0] += At[(long)i * ld + u] * y[i];
  part[g][c] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  __syncthreads();
  if (g == 0) {
    const double t = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
    v[u] = first ? t : v[u] + t;
  }
}

// B = I + Psi / s over the whole mp x mp block (Psi holds its lower triangle and zeros above it)
__global__ void sparse_make_b_kernel(const double* __restrict__ Psi, double* __restrict__ B, int mp, double s) {
  const long total = (long)mp * mp;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int i = (int)(e / mp), j = (int)(e % mp);
    B[e] = Psi[e] / s + (i == j ? 1.0 : 0.0);
  }
}

// out[i] = in[i] / s, i < n
__global__ void sparse_scale_kernel(const double* __restrict__ in, double* __restrict__ out, int n, double s) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[i] / s;
}

// out[0] = sum_{i < m} log LB_ii, out[1] = tr Psi, out[2] = |c|^2, out[3] = |a^|^2 (0 without ahat), out[4] = tr B^-1 (0 without
// Binv): one workgroup, thread-strided sums and a fixed tree
__global__ __launch_bounds__(256) void sparse_scalars_kernel(const double* __restrict__ LB, const double* __restrict__ Psi, long ld,
                                                             const double* __restrict__ cvec, const double* __restrict__ ahat,
                                                             const double* __restrict__ Binv, int m, double* __restrict__ out) {
  __shared__ double red[5][256];
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < m; i += 256) {
    s[0] += log(LB[(long)i * ld + i]);
    s[1] += Psi[(long)i * ld + i];
    s[2] += cvec[i] * cvec[i];
    if (ahat) s[3] += ahat[i] * ahat[i];
    if (Binv) s[4] += Binv[(long)i * ld + i];
  }
  for (int q = 0; q < 5; ++q) red[q][threadIdx.x] = s[q];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w)
      for (int q = 0; q < 5; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x < 5) out[threadIdx.x] = red[threadIdx.x][0];
}

// H = I - B^-1 - a^ a^^T and G0 = Psi / s - H over the whole mp x mp block (Psi mirrored from its lower triangle, a^ zero from m
// on: both come out zero in the padding)
__global__ void sparse_hg_kernel(const double* __restrict__ Psi, const double* __restrict__ Binv, const double* __restrict__ ahat,
                                 int mp, double s, double* __restrict__ H, double* __restrict__ G0) {
  const long total = (long)mp * mp;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int i = (int)(e / mp), j = (int)(e % mp);
    const double psi = j <= i ? Psi[e] : Psi[(long)j * mp + i];
    const double h = (i == j ? 1.0 : 0.0) - Binv[e] - ahat[i] * ahat[j];
    H[e] = h;
    G0[e] = psi / s - h;
  }
}

// mean[i] = b*_i . c, var[i] = kdiag - |a*_i|^2 + |b*_i|^2 + noise over the rows a* = L^-1 k(Z, x*) of A and b* = LB^-1 a* of
// Bq, one wave per query point (predict_reduce_kernel's lane-strided sums and wave tree)
__global__ __launch_bounds__(256) void sparse_predict_reduce_kernel(const double* __restrict__ A, const double* __restrict__ Bq,
                                                                    long ld, const double* __restrict__ cvec, int m, int mq,
                                                                    double kdiag, double noise, double* __restrict__ mean,
                                                                    double* __restrict__ var) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= mq) return;
  const double* a = A + (long)row * ld;
  const double* b = Bq + (long)row * ld;
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int k = lane; k < m; k += 64) {
    const double av = a[k], bv = b[k];
    s1 += bv * cvec[k];
    s2 += av * av;
    s3 += bv * bv;
  }
  for (int off = 32; off > 0; off >>= 1) {
    s1 += __shfl_down(s1, off, 64);
    s2 += __shfl_down(s2, off, 64);
    s3 += __shfl_down(s3, off, 64);
  }
  if (lane == 0) {
    mean[row] = s1;
    var[row] = kdiag - s2 + s3 + noise;
  }
}

static bool sparse_has_ratquad(const KernSpec& spec) {
  for (int c = 0; c < spec.nkern; ++c)
    if (spec.kid[c] == KID_RATQUAD) return true;
  return false;
}

// (GRAD_CONTRACT_KERNELS' table: one to four components have an instantiation of their own, five to eight share <8>)
static const decltype(&sparse_contract_kernel<1, false>) SPARSE_CONTRACT_KERNELS[5][2] = {
    {sparse_contract_kernel<1, false>, sparse_contract_kernel<1, true>}, {sparse_contract_kernel<2, false>, sparse_contract_kernel<2, true>},
    {sparse_contract_kernel<3, false>, sparse_contract_kernel<3, true>}, {sparse_contract_kernel<4, false>, sparse_contract_kernel<4, true>},
    {sparse_contract_kernel<8, false>, sparse_contract_kernel<8, true>}};

int sparse_contract_blocks(int cnt, int m) { return ((cnt + ST - 1) / ST) * ((m + ST - 1) / ST); }

hipError_t launch_sparse_contract(const KernSpec& spec, const double* theta, const double* X, int cnt, const double* Z, int m,
                                  const double* T, long ldt, const double* y, const double* tv, double* part, double* acc, int first,
                                  hipStream_t stream) {
  const int P = spec.nkern * spec.d + 2 * spec.nkern + 2;
  const int ntu = (m + ST - 1) / ST, nblk = sparse_contract_blocks(cnt, m);
  const int slot = spec.nkern >= 1 && spec.nkern <= 4 ? spec.nkern - 1 : 4;
  SPARSE_CONTRACT_KERNELS[slot][sparse_has_ratquad(spec)]<<<nblk, 256, 0, stream>>>(spec, theta, X, cnt, Z, m, T, ldt, y, tv, ntu, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  sparse_grad_accum_kernel<<<P, 256, 0, stream>>>(part, nblk, P, acc, first);
  return hipGetLastError();
}

hipError_t launch_sparse_accum_vy(const double* At, long ld, int mp, const double* y, int cnt, double* v, double* yy, int first,
                                  hipStream_t stream) {
  sparse_accum_vy_kernel<<<mp / 64 + 1, 256, 0, stream>>>(At, ld, y, cnt, v, yy, first);
  return hipGetLastError();
}

static int elementwise_blocks(long total) { return (int)std::min<long>((total + 255) / 256, 4096); }

hipError_t launch_sparse_make_b(const double* Psi, double* B, int mp, double s, hipStream_t stream) {
  sparse_make_b_kernel<<<elementwise_blocks((long)mp * mp), 256, 0, stream>>>(Psi, B, mp, s);
  return hipGetLastError();
}

hipError_t launch_sparse_scale(const double* in, double* out, int n, double s, hipStream_t stream) {
  sparse_scale_kernel<<<(n + 255) / 256, 256, 0, stream>>>(in, out, n, s);
  return hipGetLastError();
}

hipError_t launch_sparse_scalars(const double* LB, const double* Psi, long ld, const double* cvec, const double* ahat,
                                 const double* Binv, int m, double* out, hipStream_t stream) {
  sparse_scalars_kernel<<<1, 256, 0, stream>>>(LB, Psi, ld, cvec, ahat, Binv, m, out);
  return hipGetLastError();
}

hipError_t launch_sparse_hg(const double* Psi, const double* Binv, const double* ahat, int mp, double s, double* H, double* G0,
                            hipStream_t stream) {
  sparse_hg_kernel<<<elementwise_blocks((long)mp * mp), 256, 0, stream>>>(Psi, Binv, ahat, mp, s, H, G0);
  return hipGetLastError();
}

hipError_t launch_sparse_predict_reduce(const double* A, const double* Bq, long ld, const double* cvec, int m, int mq, double kdiag,
                                        double noise, double* mean, double* var, hipStream_t stream) {
  sparse_predict_reduce_kernel<<<(mq + 3) / 4, 256, 0, stream>>>(A, Bq, ld, cvec, m, mq, kdiag, noise, mean, var);
  return hipGetLastError();
}

}  // namespace migp
