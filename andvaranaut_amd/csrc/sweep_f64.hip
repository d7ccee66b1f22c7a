// The matrix-free sweep of the posterior mean and its input gradient (option 53 of mi_gp_set_option, api_sweep.hip):
//   mu(x*) = sum_j k(x*, x_j) alpha_j,      d mu / d x*_m = sum_j alpha_j sum_c coef_c kv_c k_c'(r2_c) 2 (x*_m - x_jm) / l_cm^2
// with alpha = K^-1 y resident: O(n d) per point, no m x n matrix -- the route of Saltelli designs, active subspaces and
// mean-only y_dist samples of 1e5 .. 1e7 points, where mi_gp_predict_u pays O(n^2) per point for a variance nobody reads.
// The n-body form: a thread owns ONE QUERY POINT, x* and the accumulators mu, g[.] in registers, and walks training points in
// index order.  The training range is cut into SWEEP_PARTS parts by a rule of n alone; a wave (one workgroup) sums ONE part
// for 64 points and writes the partial sums to scratch, and sweep_reduce_kernel adds a point's partial sums in part order.
// Every sum runs in a fixed order and a point's bits depend on nothing but the point and the resident state: not on m, not on
// its position, not on the other points.  The parts are there because a wave's loop is a chain of dependent steps: a call of
// m points is only m / 64 point sets on a chip of 1024 SIMDs, and the parts multiply the waves in flight by sixteen.
// Everything a thread reads inside the loop -- x_j, 1 / l, 2 / l^2, alpha_j -- is the same for all lanes of a wave.  The training
// points are staged once per call, zero-padded to the register window (sweep_stage_kernel), so that a row is one contiguous
// run of doubles at a wave-uniform address: the compiler fetches it through the scalar cache into SGPRs, and the vector ALU
// -- fp64 MFMA buys no flops over it on this chip (assemble.hip) -- does nothing but the arithmetic.  No LDS, no barrier.
// r2 in the DIRECT form sum_m ((x*_m - x_jm) (1 / l_cm))^2 of predict_grad_kernel, never the assembly's expansion: its residue
// of a few eps |x / l|^2 is amplified by Exponential's dk/dr2 ~ 1 / r near r = 0 (tests/grad_refs.py: alpha_reference).
#include "migp_kernels.h"
#include "migp_math.h"

namespace migp {

// Xp[j][S] = x_j, zeros from d on; il[c][S] = 1 / l_cm, il2[c][S] = 2 / l_cm^2 (as 2 il il), zeros from d on: a padded
// dimension adds (x - 0) * 0 = 0 to r2 and 0 to its gradient entry, which is not stored
__global__ __launch_bounds__(256) void sweep_stage_kernel(const double* __restrict__ theta, const double* __restrict__ X, int n, int d,
                                                          int nk, int S, double* __restrict__ Xp, double* __restrict__ il,
                                                          double* __restrict__ il2) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long j = i / S;
  const int u = (int)(i % S);
  if (j < n) Xp[i] = u < d ? X[j * d + u] : 0.0;
  if (j < nk) {
    const double v = u < d ? 1.0 / theta[j * d + u] : 0.0;
    il[i] = v;
    il2[i] = 2.0 * v * v;
  }
}

// DW: the register window, dimensions of x* and of the gradient a thread holds.  !WIDE: d <= DW = S, one window, r2 from the
// registers.  WIDE (32 < d <= 128, S = d rounded up to 32): blockIdx.z is the window [w0, w0 + 32) of the gradient; every window
// forms r2 from all d dimensions of its point, read from memory (device memory: the host side stages the points of the wide
// form) -- the same T for each of them, window 0 writes the mean's partial sum.
// blockIdx.y is the part: training points [y q, min((y + 1) q, n)), q = ceil(n / SWEEP_PARTS).  part[(y * m + p) * E + e] receives
// the partial sum of point p: e = 0 the mean, e = 1 + k the gradient's dimension k (E = 1 + d with GRAD, else 1).
template <int NK, bool GRAD, int DW, bool WIDE>
__global__ __launch_bounds__(64) void mean_sweep_kernel(KernSpec spec, const double* __restrict__ theta,
                                                        const double* __restrict__ Xp, const double* __restrict__ il,
                                                        const double* __restrict__ il2, int S, int n,
                                                        const double* __restrict__ alpha_v, const double* __restrict__ xstar,
                                                        int m, double* __restrict__ part) {
  const long p = (long)blockIdx.x * 64 + threadIdx.x;
  if (p >= m) return;
  const int jq = (n + SWEEP_PARTS - 1) / SWEEP_PARTS;
  const int jbeg = (int)blockIdx.y * jq, jend = min(n, jbeg + jq);
  const int d = spec.d;
  const int nk = RUNTIME_NK<NK> ? spec.nkern : NK;
  const int w0 = WIDE ? (int)blockIdx.z * DW : 0;
  const double* kv = theta + nk * d;
  const double* al = kv + nk;
  const double* xp = xstar + p * d;
  double xs[DW], g[DW];
#pragma unroll
  for (int u = 0; u < DW; ++u) {
    xs[u] = (w0 + u < d) ? xp[w0 + u] : 0.0;
    g[u] = 0.0;
  }
  double mu = 0.0;
  for (int j = jbeg; j < jend; ++j) {
    const double* xj = Xp + (long)j * S;
    double kval[NK], dkv[NK];
#pragma unroll
    for (int c = 0; c < nk; ++c) {
      const double* ilc = il + c * S;
      double r2 = 0.0;
      if constexpr (WIDE) {
        for (int q = 0; q < d; ++q) {
          const double df = (xp[q] - xj[q]) * ilc[q];
          r2 += df * df;
        }
      } else {
#pragma unroll
        for (int u = 0; u < DW; ++u) {
          const double df = (xs[u] - xj[u]) * ilc[u];
          r2 += df * df;
        }
      }
      double da;
      comp_val_der<false>(spec.kid[c], r2, al[c], kv[c], kval[c], dkv[c], da);
    }
    double pref[NK];  // dK/dK_c of the fold: grad_contract_kernel's recurrence (grad_predict.hip), per training point
    double T = kval[0];
    pref[0] = 1.0;
#pragma unroll
    for (int c = 1; c < nk; ++c) {
      pref[c] = (spec.op[c - 1] == 0) ? 1.0 : T;
      T = (spec.op[c - 1] == 0) ? T + kval[c] : T * kval[c];
    }
    const double a = alpha_v[j];
    mu += T * a;
    if constexpr (GRAD) {
      double gc[NK];  // alpha_j coef_c kv_c k_c'
#pragma unroll
      for (int c = 0; c < nk; ++c) {
        double coef = pref[c];
#pragma unroll
        for (int c2 = c + 1; c2 < nk; ++c2)
          if (spec.op[c2 - 1] == 1) coef *= kval[c2];
        gc[c] = a * (coef * dkv[c]);
      }
      // the DIFFERENCES are accumulated, never x* sum C - sum C x_j: that form cancels for short length scales
#pragma unroll
      for (int u = 0; u < DW; ++u) {
        double s = gc[0] * il2[w0 + u];
#pragma unroll
        for (int c = 1; c < nk; ++c) s += gc[c] * il2[c * S + w0 + u];
        g[u] += s * (xs[u] - xj[w0 + u]);
      }
    }
  }
  const int E = GRAD ? 1 + d : 1;
  double* out = part + ((long)blockIdx.y * m + p) * E;
  if (w0 == 0) out[0] = mu;
  if constexpr (GRAD) {
#pragma unroll
    for (int u = 0; u < DW; ++u)
      if (w0 + u < d) out[1 + w0 + u] = g[u];
  }
}

// mean[p] = sum_y part[(y m + p) E], dmean[p d + k] = sum_y part[(y m + p) E + 1 + k], y = 0 .. SWEEP_PARTS - 1 in index order (a
// part beyond the training range holds zeros); one thread per output element (gx_reduce_kernel's scheme, grad_predict.hip)
__global__ __launch_bounds__(256) void sweep_reduce_kernel(const double* __restrict__ part, int m, int E, int d, double* __restrict__ mean,
                                                           double* __restrict__ dmean) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)m * E) return;
  const long p = i / E;
  const int e = (int)(i % E);
  double s = part[i];
#pragma unroll
  for (int y = 1; y < SWEEP_PARTS; ++y) s += part[(long)y * m * E + i];
  if (e == 0) {
    if (mean) mean[p] = s;
  } else {
    dmean[p * d + e - 1] = s;
  }
}

// the padded row length of the staged training points for d <= SWEEP_MAX_D input dimensions: the register window of the
// instantiation that runs (4, 16 or 32), or d rounded up to the 32-dimension windows of the wide form
int sweep_stride(int d) { return d <= 4 ? 4 : d <= 16 ? 16 : d <= 32 ? 32 : (d + 31) / 32 * 32; }
// query points per pass: enough waves (points / 64 * SWEEP_PARTS) for every SIMD's share at full occupancy
int sweep_chunk(int d) { return d <= 32 ? 16384 : 4096; }
// the staged points, 1 / l and 2 / l^2, the partial sums of one pass and, for the wide form, the pass's query points
size_t sweep_scratch_len(int cap, int d) {
  return ((size_t)cap + 2 * MAX_KERN) * sweep_stride(d) + (size_t)SWEEP_PARTS * sweep_chunk(d) * (1 + d) +
         (d > 32 ? (size_t)sweep_chunk(d) * d : 0);
}

static int nk_slot(int nkern) { return nkern >= 1 && nkern <= 4 ? nkern - 1 : 4; }

#define SWEEP_ROW(NK, G) \
  { mean_sweep_kernel<NK, G, 4, false>, mean_sweep_kernel<NK, G, 16, false>, mean_sweep_kernel<NK, G, 32, false>, \
    mean_sweep_kernel<NK, G, 32, true> }
static const decltype(&mean_sweep_kernel<1, false, 4, false>) MEAN_SWEEP_KERNELS[5][2][4] = {  // [slot][gradient][window form]
    {SWEEP_ROW(1, false), SWEEP_ROW(1, true)}, {SWEEP_ROW(2, false), SWEEP_ROW(2, true)}, {SWEEP_ROW(3, false), SWEEP_ROW(3, true)},
    {SWEEP_ROW(4, false), SWEEP_ROW(4, true)}, {SWEEP_ROW(8, false), SWEEP_ROW(8, true)}};
#undef SWEEP_ROW

hipError_t launch_mean_sweep(const KernSpec& spec, const double* theta, const double* X, int n, const double* xstar, int m,
                             const double* alpha, double* scratch, double* mean, double* dmean, hipStream_t stream) {
  const int d = spec.d, S = sweep_stride(d), chunk = sweep_chunk(d);
  if (d > SWEEP_MAX_D) return hipErrorInvalidValue;  // (mi_gp_predict_grad names the limit)
  double* Xp = scratch;
  double* il = Xp + (size_t)n * S;
  double* il2 = il + (size_t)MAX_KERN * S;
  double* part = il2 + (size_t)MAX_KERN * S;
  double* xq = part + (size_t)SWEEP_PARTS * chunk * (1 + d);  // (wide form only)
  const long rows = n > spec.nkern ? n : spec.nkern;
  sweep_stage_kernel<<<(unsigned)((rows * S + 255) / 256), 256, 0, stream>>>(theta, X, n, d, spec.nkern, S, Xp, il, il2);
  hipError_t e = hipGetLastError();
  const int form = d <= 4 ? 0 : d <= 16 ? 1 : d <= 32 ? 2 : 3;
  const int E = dmean ? 1 + d : 1;
  for (int s = 0; s < m && e == hipSuccess; s += chunk) {
    const int mc = min(chunk, m - s);
    const double* xs = xstar + (size_t)s * d;
    if (form == 3) {
      // the wide form reads x* inside its innermost loop: from device memory, wherever the caller keeps the points
      e = hipMemcpyAsync(xq, xs, sizeof(double) * (size_t)mc * d, hipMemcpyDefault, stream);
      if (e != hipSuccess) break;
      xs = xq;
    }
    const dim3 grid((unsigned)((mc + 63) / 64), SWEEP_PARTS, (form == 3 && dmean) ? S / 32 : 1);
    MEAN_SWEEP_KERNELS[nk_slot(spec.nkern)][dmean ? 1 : 0][form]<<<grid, 64, 0, stream>>>(spec, theta, Xp, il, il2, S, n, alpha, xs, mc,
                                                                                          part);
    e = hipGetLastError();
    if (e != hipSuccess) break;
    sweep_reduce_kernel<<<(unsigned)(((long)mc * E + 255) / 256), 256, 0, stream>>>(part, mc, E, d, mean ? mean + s : nullptr,
                                                                                    dmean ? dmean + (size_t)s * d : nullptr);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace migp
