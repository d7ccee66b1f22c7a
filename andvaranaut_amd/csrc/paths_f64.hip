// The matrix-free sweep of S posterior sample paths and their input gradients (option 54 of mi_gp_set_option, api_paths.hip):
//   f_s(x*) = sum_i W[i,s] cos(om_i . x* + b_i) + sum_j k(x*, x_j) V[j,s]
// -- a prior function draw from random Fourier features plus the pathwise update, one weight per training point (Wilson et al.
// 2020).  The second sum is the mean sweep of sweep_f64.hip with S weight vectors, and the design is the same: a thread owns ONE
// QUERY POINT, x* and the accumulators in registers; everything read inside the loops -- x_j, 1 / l, 2 / l^2, a row of V, om_i,
// b_i, a row of W -- is the same for all lanes of a wave at a contiguous address and arrives through the scalar cache; no LDS, no
// barrier, no atomics.  What changes: a thread carries T path accumulators, so the pair's kernel value -- r2, exp / root and the
// + / * fold, ~40 operations -- is formed once and used T times at 2 operations each.  With the gradient a thread holds T x DW
// gradient accumulators, so T is small there (path_tile()).  blockIdx.z is the path tile, blockIdx.y the part: the training range
// is cut into PATH_PARTS_N parts by a rule of n alone, the feature range into PATH_PARTS_F parts by a rule of F alone; a wave sums
// one part for 64 points and T paths, and path_reduce_kernel adds the partial sums in part order.  Every accumulation is an
// explicit fma in a fixed order, so the bits of path s at point p depend on the point, column s of V and W, Omega, b and the
// resident state and on nothing else: not on m, the position of p, S, the other columns, the tile width or the gradient.
// The weights are staged per call into rows of 128 doubles, zeros up to S rounded up to 16 (path_stage_kernel): the tiles read
// whole runs without a bound check, and the caller's padding columns are never touched.  cos / sin are the device library's:
// Matern and Exponential frequencies are heavy-tailed (Exponential's are Cauchy), and these reduce arguments of any size exactly.
#include "migp_kernels.h"
#include "migp_math.h"

namespace migp {

int path_window(int d) { return d <= 4 ? 4 : d <= 16 ? 16 : 32; }
int path_tile(int d, bool grad) { return !grad ? PATH_TILE_VALUE : d <= 4 ? 8 : d <= 16 ? 2 : 1; }

template <bool GRAD, int DW>
constexpr int PATH_T = !GRAD ? PATH_TILE_VALUE : DW == 4 ? 8 : DW == 16 ? 2 : 1;

// doubles of the partial sums: PATH_PARTS_N + PATH_PARTS_F parts of PATH_CHUNK points and 128 value columns -- with the gradient
// a tile holds T (1 + d) <= 40 columns, three tiles to a group
constexpr size_t PATH_PART_LEN = (size_t)(PATH_PARTS_N + PATH_PARTS_F) * PATH_CHUNK * PATH_MAX_S;

static long path_ldr(int cap) { return ((long)cap + 127) / 128 * 128; }

PathScratch path_scratch(double* base, int cap, int d, int F) {
  const size_t DW = path_window(d);
  PathScratch t;
  t.ldr = path_ldr(cap);
  t.Xp = base;
  t.il = t.Xp + (size_t)cap * DW;
  t.il2 = t.il + MAX_KERN * DW;
  t.Om = t.il2 + MAX_KERN * DW;
  t.Wp = t.Om + (size_t)F * DW;
  t.Vp = t.Wp + (size_t)F * PATH_MAX_S;
  t.part = t.Vp + (size_t)cap * PATH_MAX_S;
  t.R1 = t.part + PATH_PART_LEN;
  t.R2 = t.R1 + (size_t)128 * t.ldr;
  return t;
}
size_t path_scratch_len(int cap, int d, int F) {
  const size_t DW = path_window(d);
  return ((size_t)cap + 2 * MAX_KERN + (size_t)F) * DW + ((size_t)F + cap) * PATH_MAX_S + PATH_PART_LEN + (size_t)256 * path_ldr(cap);
}

// Xp[j][DW] = x_j, il[c][DW] = 1 / l_c, il2[c][DW] = 2 / l_c^2, Om[i][DW] = om_i, each with zeros from d on (a padded dimension
// adds (x - 0) * 0 to r2 and om * x = 0 to the phase); Wp[i][128] = W[i][.], zeros in the columns S .. Sp - 1
__global__ __launch_bounds__(256) void path_stage_kernel(const double* __restrict__ theta, const double* __restrict__ X, int n, int d,
                                                         int nk, int DW, const double* __restrict__ Om, const double* __restrict__ W,
                                                         long ldw, int F, int S, int Sp, double* __restrict__ Xp,
                                                         double* __restrict__ il, double* __restrict__ il2, double* __restrict__ Omp,
                                                         double* __restrict__ Wp) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long j = i / DW;
  const int u = (int)(i % DW);
  if (j < n) Xp[i] = u < d ? X[j * d + u] : 0.0;
  if (j < nk) {
    const double v = u < d ? 1.0 / theta[j * d + u] : 0.0;
    il[i] = v;
    il2[i] = 2.0 * v * v;
  }
  if (j < F) Omp[i] = u < d ? Om[j * d + u] : 0.0;
  const long r = i / Sp;
  const int s = (int)(i % Sp);
  if (r < F) Wp[r * PATH_MAX_S + s] = s < S ? W[r * ldw + s] : 0.0;
}

// Vp[j][128] = V[j][.], zeros in the columns S .. Sp - 1
__global__ __launch_bounds__(256) void path_stage_v_kernel(const double* __restrict__ V, long ldw, int n, int S, int Sp,
                                                           double* __restrict__ Vp) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long r = i / Sp;
  const int s = (int)(i % Sp);
  if (r < n) Vp[r * PATH_MAX_S + s] = s < S ? V[r * ldw + s] : 0.0;
}

// With the gradient a thread holds the gradient window GW: the dimensions [w0, w0 + GW) of the gradient.  The window of 32
// dimensions runs as two gradient windows of 16, and the 5..8-component instantiation (its component arrays live in registers
// too) in windows of 8: every window forms r2 and the phase from all d dimensions, window 0 writes the value, and x*, T x GW
// gradient accumulators and the temporaries of exp / pow / cos stay below 256 VGPRs without a spill.
template <int NK, bool GRAD, int DW>
constexpr int PATH_GW = !GRAD ? 1 : DW == 4 ? 4 : RUNTIME_NK<NK> ? 8 : 16;
static int path_grad_windows(int nkern, int d) { return d <= 4 ? 1 : path_window(d) / (nkern > 4 ? 8 : 16); }
// the component loops: unrolled for 1..4 components, rolled for the run-time count of the 5..8 instantiation (its arrays are
// indexed at run time)
template <int NK>
constexpr int PATH_UNROLL_C = RUNTIME_NK<NK> ? 1 : NK;

// 0 in an SGPR, through an empty asm: an offset the optimiser cannot see through.  `row + path_opaque_zero()` is still a
// wave-uniform global address (a scalar load), but the load is neither hoisted out of a loop nor merged with an earlier load
// of the same row -- where that would keep 32 or 64 doubles live in VGPRs
__device__ __forceinline__ int path_opaque_zero() {
  int z = 0;
  asm volatile("" : "+s"(z));
  return z;
}

// One part of the sums of one point: the training points [jbeg, jend) (TRAIN) or the features [jbeg, jend), for the T paths
// whose staged weights start at vw (a row is PATH_MAX_S doubles), gradient dimensions [W0, W0 + GW)
template <int NK, bool GRAD, int DW, int W0, bool TRAIN>
__device__ __forceinline__ void path_part(const KernSpec& spec, const double* __restrict__ theta, const double* __restrict__ rows,
                                          const double* __restrict__ il, const double* __restrict__ il2,
                                          const double* __restrict__ vw, const double* __restrict__ bph, int jbeg, int jend,
                                          const double (&xs)[DW], double (&mu)[PATH_T<GRAD, DW>],
                                          double (&g)[PATH_T<GRAD, DW>][PATH_GW<NK, GRAD, DW>]) {
  constexpr int T = PATH_T<GRAD, DW>;
  constexpr int GW = PATH_GW<NK, GRAD, DW>;
  if constexpr (TRAIN) {
    const int d = spec.d;
    const int nk = RUNTIME_NK<NK> ? spec.nkern : NK;
    const double* kv = theta + nk * d;
    const double* al = kv + nk;
    for (int j = jbeg; j < jend; ++j) {
      const double* xj = rows + (long)j * DW;
      const double* vr = vw + (long)j * PATH_MAX_S;
      // 1 / l and 2 / l^2 are re-read per training point, through the scalar cache like x_j: hoisted out of the loop they would
      // not fit the SGPR file, and the compiler would park NK x DW doubles of them in VGPRs
      const double *ilj = il + path_opaque_zero(), *il2j = il2 + path_opaque_zero();
      double kval[NK], dkv[NK];  // kv_c k_c; kv_c k_c' times dK/dK_c of the fold
      double Tk = 0.0;
#pragma unroll PATH_UNROLL_C<NK>
      for (int c = 0; c < nk; ++c) {
        const double* ilc = ilj + c * DW;
        // (the window of 32, and of 16 under 5..8 components: x_j is re-read per component, or the 32 differences x* - x_j would stay live across the components)
        const double* xjc = (DW == 32 || (RUNTIME_NK<NK> && DW == 16)) ? xj + path_opaque_zero() : xj;
        double r2 = 0.0;
#pragma unroll
        for (int u = 0; u < DW; ++u) {
          const double df = (xs[u] - xjc[u]) * ilc[u];
          r2 = __builtin_fma(df, df, r2);
        }
        double da, dk;
        comp_val_der<false>(spec.kid[c], r2, al[c], kv[c], kval[c], dk, da);
        // the fold so far multiplies a component that joins by '*' (mean_sweep_kernel's recurrence)
        const bool mul = c > 0 && spec.op[c > 0 ? c - 1 : 0] == 1;
        dkv[c] = mul ? Tk * dk : dk;
        Tk = c == 0 ? kval[0] : mul ? Tk * kval[c] : Tk + kval[c];
      }
#pragma unroll
      for (int t = 0; t < T; ++t) mu[t] = __builtin_fma(Tk, vr[t], mu[t]);
      if constexpr (GRAD) {
        // ... and every later '*' multiplies it: the suffix products, from the last component down
        double suf = 1.0;
#pragma unroll PATH_UNROLL_C<NK>
        for (int c = nk - 1; c >= 0; --c) {
          dkv[c] *= suf;
          if (c > 0 && spec.op[c - 1] == 1) suf *= kval[c];
        }
        // the DIFFERENCES are accumulated (mean_sweep_kernel); a coincident training point adds v * 0
        const double* xjg = (DW == 32 || (RUNTIME_NK<NK> && DW == 16)) ? xj + path_opaque_zero() : xj;
#pragma unroll
        for (int u = 0; u < GW; ++u) {
          double s = dkv[0] * il2j[W0 + u];
#pragma unroll PATH_UNROLL_C<NK>
          for (int c = 1; c < nk; ++c) s = __builtin_fma(dkv[c], il2j[c * DW + W0 + u], s);
          const double base = s * (xs[W0 + u] - xjg[W0 + u]);
#pragma unroll
          for (int t = 0; t < T; ++t) g[t][u] = __builtin_fma(vr[t], base, g[t][u]);
        }
      }
    }
  } else {
    for (int i = jbeg; i < jend; ++i) {
      const double* om = rows + (long)i * DW;
      const double* wr = vw + (long)i * PATH_MAX_S;
      double ph = bph[i];
#pragma unroll
      for (int u = 0; u < DW; ++u) ph = __builtin_fma(om[u], xs[u], ph);
      const double cs = cos(ph);
#pragma unroll
      for (int t = 0; t < T; ++t) mu[t] = __builtin_fma(wr[t], cs, mu[t]);
      if constexpr (GRAD) {
        const double sn = sin(ph);
#pragma unroll
        for (int t = 0; t < T; ++t) {
          const double ws = -(wr[t] * sn);
#pragma unroll
          for (int u = 0; u < GW; ++u) g[t][u] = __builtin_fma(ws, om[W0 + u], g[t][u]);
        }
      }
    }
  }
}

// path_part for the gradient window w of NW = DW / GW: the window's first dimension is a template argument, so that x* and
// the accumulators are indexed at compile time (w is wave-uniform)
template <int NK, bool GRAD, int DW, bool TRAIN, int W = 0, class... Args>
__device__ __forceinline__ void path_window_part(int w, Args&&... args) {
  constexpr int GW = PATH_GW<NK, GRAD, DW>;
  constexpr int NW = GRAD ? DW / GW : 1;
  if constexpr (W + 1 < NW) {
    if (w == W)
      path_part<NK, GRAD, DW, W * GW, TRAIN>(args...);
    else
      path_window_part<NK, GRAD, DW, TRAIN, W + 1>(w, args...);
  } else {
    path_part<NK, GRAD, DW, W * GW, TRAIN>(args...);
  }
}

// Part y = y0 + blockIdx.y: y < PATH_PARTS_N the training points [y q, min((y + 1) q, n)), q = ceil(n / PATH_PARTS_N); otherwise
// the features [f F / PATH_PARTS_F, (f + 1) F / PATH_PARTS_F), f = y - PATH_PARTS_N.  blockIdx.z = tile * NW + w: the paths are the
// columns [tile T, (tile + 1) T) of Vp / Wp (the host has added the group's first column), w the gradient window (NW = DW / GW).
// part[((blockIdx.y * tiles + tile) * T + t) * m * E + p * E + e]: e = 0 the value, e = 1 + k the gradient's dimension k
// (E = 1 + d with GRAD, else 1).  Two waves per SIMD: the register allocator stays at or below 256 VGPRs, the occupancy cliff.
template <int NK, bool GRAD, int DW>
__global__ __launch_bounds__(64, 2) void path_sweep_kernel(KernSpec spec, const double* __restrict__ theta, const double* __restrict__ Xp,
                                                           const double* __restrict__ il, const double* __restrict__ il2, int n,
                                                           const double* __restrict__ Vp, const double* __restrict__ Omp,
                                                           const double* __restrict__ bph, const double* __restrict__ Wp, int F,
                                                           const double* __restrict__ xstar, int m, int y0, double* __restrict__ part) {
  constexpr int T = PATH_T<GRAD, DW>;
  constexpr int GW = PATH_GW<NK, GRAD, DW>;
  constexpr int NW = GRAD ? DW / GW : 1;
  const long p = (long)blockIdx.x * 64 + threadIdx.x;
  if (p >= m) return;
  const int d = spec.d;
  const int y = y0 + (int)blockIdx.y;
  const int tile = (int)blockIdx.z / NW, tiles = (int)gridDim.z / NW;
  const int w0 = ((int)blockIdx.z % NW) * GW;  // (wave-uniform)
  const int s0 = tile * T;
  const double* xp = xstar + p * d;
  double xs[DW], mu[T], g[T][GW];
#pragma unroll
  for (int u = 0; u < DW; ++u) xs[u] = u < d ? xp[u] : 0.0;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    mu[t] = 0.0;
#pragma unroll
    for (int u = 0; u < GW; ++u) g[t][u] = 0.0;
  }
  const int w = (int)blockIdx.z % NW;
  if (y < PATH_PARTS_N) {
    const int jq = (n + PATH_PARTS_N - 1) / PATH_PARTS_N;
    const int jbeg = y * jq, jend = min(n, jbeg + jq);
    path_window_part<NK, GRAD, DW, true>(w, spec, theta, Xp, il, il2, Vp + s0, bph, jbeg, jend, xs, mu, g);
  } else {
    const int fq = F / PATH_PARTS_F;
    const int ibeg = (y - PATH_PARTS_N) * fq, iend = ibeg + fq;
    path_window_part<NK, GRAD, DW, false>(w, spec, theta, Omp, il, il2, Wp + s0, bph, ibeg, iend, xs, mu, g);
  }
  const int E = GRAD ? 1 + d : 1;
  double* out = part + (((long)blockIdx.y * tiles + tile) * T * m + p) * E;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    double* o = out + (long)t * m * E;
    if (w0 == 0) o[0] = mu[t];
    if constexpr (GRAD) {
#pragma unroll
      for (int u = 0; u < GW; ++u)
        if (w0 + u < d) o[1 + w0 + u] = g[t][u];
    }
  }
}

// One thread per (column, point, element) of a pass: the sum of its ny partial sums in part order goes to
// mean[(col0 + col) * ldo + p] (e = 0) or dmean[((col0 + col) * ldo + p) * d + e - 1]; the tile columns from S on are dropped
__global__ __launch_bounds__(256) void path_reduce_kernel(const double* __restrict__ part, int ny, int cols, int mc, int E, int d, int col0,
                                                          int S, long ldo, double* __restrict__ mean, double* __restrict__ dmean) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long per = (long)mc * E, all = per * cols;
  if (i >= all) return;
  const int col = (int)(i / per);
  const long rem = i % per;
  const long p = rem / E;
  const int e = (int)(rem % E);
  if (col0 + col >= S) return;
  double s = part[i];
  for (int y = 1; y < ny; ++y) s += part[(long)y * all + i];
  const long o = (long)(col0 + col) * ldo + p;
  if (e == 0) {
    if (mean) mean[o] = s;
  } else {
    dmean[o * d + e - 1] = s;
  }
}

__global__ __launch_bounds__(256) void path_residual_kernel(const double* __restrict__ y, const double* __restrict__ V, long ldw, int n,
                                                            int S, long ldr, double* __restrict__ R) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= 128 * ldr) return;
  const int s = (int)(i / ldr);
  const long j = i % ldr;
  R[i] = (s < S && j < n) ? (y[j] - R[i]) - V[j * ldw + s] : 0.0;
}

__global__ __launch_bounds__(256) void path_scatter_kernel(double* __restrict__ V, long ldw, int n, int S, long ldr,
                                                           const double* __restrict__ R) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)n * S) return;
  const long j = i / S;
  const int s = (int)(i % S);
  V[j * ldw + s] = R[s * ldr + j];
}

static int path_nk_slot(int nkern) { return nkern >= 1 && nkern <= 4 ? nkern - 1 : 4; }

#define PATH_ROW(NK, G) { path_sweep_kernel<NK, G, 4>, path_sweep_kernel<NK, G, 16>, path_sweep_kernel<NK, G, 32> }
static const decltype(&path_sweep_kernel<1, false, 4>) PATH_SWEEP_KERNELS[5][2][3] = {  // [slot][gradient][window]
    {PATH_ROW(1, false), PATH_ROW(1, true)}, {PATH_ROW(2, false), PATH_ROW(2, true)}, {PATH_ROW(3, false), PATH_ROW(3, true)},
    {PATH_ROW(4, false), PATH_ROW(4, true)}, {PATH_ROW(8, false), PATH_ROW(8, true)}};
#undef PATH_ROW

hipError_t launch_path_stage(const KernSpec& spec, const double* theta, const double* X, int n, const double* Om, const double* W, long ldw,
                             int F, int S, const PathScratch& t, hipStream_t stream) {
  const int DW = path_window(spec.d), Sp = (S + 15) / 16 * 16;
  long rows = n > F ? n : F;
  if (rows < spec.nkern) rows = spec.nkern;
  const long threads = rows * DW > (long)F * Sp ? rows * DW : (long)F * Sp;
  path_stage_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, stream>>>(theta, X, n, spec.d, spec.nkern, DW, Om, W, ldw, F, S, Sp, t.Xp,
                                                                           t.il, t.il2, t.Om, t.Wp);
  return hipGetLastError();
}

hipError_t launch_path_stage_v(const double* V, long ldw, int n, int S, const PathScratch& t, hipStream_t stream) {
  const int Sp = (S + 15) / 16 * 16;
  path_stage_v_kernel<<<(unsigned)(((long)n * Sp + 255) / 256), 256, 0, stream>>>(V, ldw, n, S, Sp, t.Vp);
  return hipGetLastError();
}

hipError_t launch_path_sweep(const KernSpec& spec, const double* theta, int n, int F, int S, const double* bph, const PathScratch& t,
                             const double* xstar, int m, long ldo, double* mean, double* dmean, bool features_only, hipStream_t stream) {
  const int d = spec.d;
  if (d > PATH_MAX_D || S < 1 || S > PATH_MAX_S || (!mean && !dmean)) return hipErrorInvalidValue;
  const bool grad = dmean != nullptr;
  const int T = path_tile(d, grad), E = grad ? 1 + d : 1;
  const int form = d <= 4 ? 0 : d <= 16 ? 1 : 2;
  const int nw = grad ? path_grad_windows(spec.nkern, d) : 1;  // (PATH_GW)
  const int tiles = (S + T - 1) / T;
  int group = PATH_MAX_S / (T * E);  // tiles whose partial sums fit the scratch
  if (group < 1) group = 1;
  const int y0 = features_only ? PATH_PARTS_N : 0;
  const int ny = PATH_PARTS_N + PATH_PARTS_F - y0;
  const auto kern = PATH_SWEEP_KERNELS[path_nk_slot(spec.nkern)][grad ? 1 : 0][form];
  hipError_t e = hipSuccess;
  // a pass of few columns takes more points, up to 8 PATH_CHUNK: the partial sums still fit, and a launch has the same
  // number of waves whatever S is (the bits of a point do not depend on the pass it falls into)
  const int cols = min(group, tiles) * T * E;
  const int chunk = PATH_CHUNK * min(8, PATH_MAX_S / cols);
  for (int s = 0; s < m && e == hipSuccess; s += chunk) {
    const int mc = min(chunk, m - s);
    for (int z = 0; z < tiles && e == hipSuccess; z += group) {
      const int nz = min(group, tiles - z), col0 = z * T;
      const dim3 grid((unsigned)((mc + 63) / 64), ny, nz * nw);
      kern<<<grid, 64, 0, stream>>>(spec, theta, t.Xp, t.il, t.il2, n, t.Vp + col0, t.Om, bph, t.Wp + col0, F, xstar + (size_t)s * d, mc, y0,
                                    t.part);
      e = hipGetLastError();
      if (e != hipSuccess) break;
      const long all = (long)nz * T * mc * E;
      path_reduce_kernel<<<(unsigned)((all + 255) / 256), 256, 0, stream>>>(t.part, ny, nz * T, mc, E, d, col0, S, ldo,
                                                                            mean ? mean + s : nullptr,
                                                                            dmean ? dmean + (size_t)s * d : nullptr);
      e = hipGetLastError();
    }
  }
  return e;
}

hipError_t launch_path_residual(const double* y, const double* V, long ldw, int n, int S, const PathScratch& t, hipStream_t stream) {
  path_residual_kernel<<<(unsigned)((128 * t.ldr + 255) / 256), 256, 0, stream>>>(y, V, ldw, n, S, t.ldr, t.R1);
  return hipGetLastError();
}

hipError_t launch_path_scatter(double* V, long ldw, int n, int S, const PathScratch& t, hipStream_t stream) {
  path_scatter_kernel<<<(unsigned)(((long)n * S + 255) / 256), 256, 0, stream>>>(V, ldw, n, S, t.ldr, t.R1);
  return hipGetLastError();
}

}  // namespace migp
