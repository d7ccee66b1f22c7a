// The greedy loop of the design call (option 56 of mi_gp_set_option, api_design.hip; include/mi_gp.h has the contract): b steps of a
// pivoted elimination on the resident Mc x Mr cross-covariance block G = cov(C, R) between the candidates and the reference points.
// A step is three launches on one stream -- pick, column, update -- and the pivot index stays in device memory between them:
//   pick    score(c) = rowsq[c] / (Mr v[c]) (Mr = 0: v[c] - noise) over the alive candidates with a finite v > 0, the arg-max with
//           ties to the lowest index, the pivot marked dead; one workgroup
//   column  g[c] = cov_t(c, c*) = k(x_c, x_c*) - A_c . A_c* - sum_{s < t} g_s[c] g_s[c*] / v*_s, one wave per candidate: one pass
//           over the candidates' rows of A = L^-1 K(X, .), the memory-bound part that grows with n
//   update  G[c, :] -= (g[c] / v*) G[c*, :] with the row's new sum of squares in the same pass, v[c] -= g[c]^2 / v*; one wave per
//           ALIVE row: 16 bytes of traffic per element of G.  The pivot's row is dead from the pick on, so no wave writes the row
//           that every wave reads.
// No atomics.  Every row sum is the lane-strided partial sums and the wave64 tree of predict_row_sums (grad_predict.hip): a row's
// bits do not depend on the grid.  Every element a launch reads was written earlier in the same call.
#include "migp_kernels.h"
#include "migp_math.h"

namespace migp {

size_t design_scratch_len(int Mc, int b) {
  const size_t mcp = ((size_t)Mc + 127) / 128 * 128;
  return (4 + (size_t)b) * mcp + 128 + 2;
}

DesignScratch design_scratch(double* base, int Mc, int b) {
  DesignScratch t;
  t.mcp = ((long)Mc + 127) / 128 * 128;
  t.v = base;
  t.rowsq = t.v + t.mcp;
  t.mean = t.rowsq + t.mcp;
  t.hist = t.mean + t.mcp;
  t.vs = t.hist + (long)b * t.mcp;
  t.alive = reinterpret_cast<int*>(t.vs + 128);  // mcp ints in mcp doubles
  t.piv = reinterpret_cast<int*>(t.vs + 128 + t.mcp);
  return t;
}

typedef double double2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double wave_sum(double s) {
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  return s;
}

// The rows of A and G start 16-byte aligned (ldw and ldc are even, as the assembly's stores require): a lane walks a row in pairs,
// pair q = lane, lane + 64, ... (16 bytes per lane and load), lane 0 takes the last element of an odd length.  The order of a
// lane's sum is fixed by the length alone.

// rowsq[c] = sum_r G[c][r]^2 for c < Mc, one wave per row
__global__ __launch_bounds__(256) void design_rowsq_kernel(const double* __restrict__ G, long ldc, int Mc, int Mr,
                                                           double* __restrict__ rowsq) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= Mc) return;
  const double* __restrict__ a = G + (long)row * ldc;
  const double2_t* a2 = reinterpret_cast<const double2_t*>(a);
  double s = 0.0;
  for (int q = lane; q < (Mr >> 1); q += 64) {
    const double2_t x = a2[q];
    s = __builtin_fma(x.x, x.x, s);
    s = __builtin_fma(x.y, x.y, s);
  }
  if ((Mr & 1) && lane == 0) s = __builtin_fma(a[Mr - 1], a[Mr - 1], s);
  s = wave_sum(s);
  if (lane == 0) rowsq[row] = s;
}

// out: the call's mean_dev -- [Mc] round-0 gains, [b] chosen indices (-1 beyond the count), [b] their gains (0 beyond), the count.
// A step finds the count of the steps before it there: fewer than `step` means the selection has stopped, and piv stays -1.
__global__ __launch_bounds__(256) void design_pick_kernel(int step, int Mc, int Mr, int b, double noise, const double* __restrict__ v,
                                                          const double* __restrict__ rowsq, int* __restrict__ alive,
                                                          int* __restrict__ piv, double* __restrict__ vs, double* __restrict__ out) {
  __shared__ double bs[256];
  __shared__ int bi[256];
  const int t = threadIdx.x;
  double* gains0 = out;
  double* idx = out + Mc;
  double* gains = idx + b;
  double* count = gains + b;
  const bool stopped = step > 0 && (int)count[0] < step;
  if (stopped) {
    if (t == 0) piv[0] = -1;
    return;
  }
  if (step == 0)
    for (int s = t; s < b; s += 256) { idx[s] = -1.0; gains[s] = 0.0; }
  double best = -INFINITY;
  int at = 0x7fffffff;
  for (int c = t; c < Mc; c += 256) {
    const bool live = step == 0 || alive[c] != 0;
    const double vc = v[c];
    const bool ok = live && vc > 0.0 && vc < INFINITY;
    const double sc = Mr > 0 ? rowsq[c] / ((double)Mr * vc) : vc - noise;
    if (step == 0) {
      alive[c] = 1;
      gains0[c] = ok ? sc : NAN;
    }
    if (ok && sc > best) { best = sc; at = c; }  // (c ascends: the first of equal scores stays)
  }
  bs[t] = best;
  bi[t] = at;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w && (bs[t + w] > bs[t] || (bs[t + w] == bs[t] && bi[t + w] < bi[t]))) { bs[t] = bs[t + w]; bi[t] = bi[t + w]; }
    __syncthreads();
  }
  if (t == 0) {
    const int p = bi[0];
    if (p < Mc && bs[0] > 0.0) {
      piv[0] = p;
      idx[step] = (double)p;
      gains[step] = bs[0];
      count[0] = (double)(step + 1);
      vs[step] = v[p];
      alive[p] = 0;
    } else {
      piv[0] = -1;
      if (step == 0) count[0] = 0.0;
    }
  }
}

// the candidate column hist[step][c] = g[c] for c < Mc at the pivot p = piv[0] (p < 0: nothing).  r2 in the direct form of the gradient kernels,
// value per component and the + / * fold of the assembly.  theta: [ls(nkern * d), kv(nkern), alpha(nkern), gv, jitter]
__global__ __launch_bounds__(256) void design_column_kernel(KernSpec spec, const double* __restrict__ theta, const double* __restrict__ Xc,
                                                            int Mc, const double* __restrict__ A, long ldw, int n, int step,
                                                            double* __restrict__ hist, long mcp, const double* __restrict__ vs,
                                                            const int* __restrict__ piv) {
  const int p = piv[0];
  if (p < 0) return;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= Mc) return;
  const double* __restrict__ a = A + (long)row * ldw;
  const double* __restrict__ ap = A + (long)p * ldw;
  const double2_t* a2 = reinterpret_cast<const double2_t*>(a);
  const double2_t* __restrict__ p2 = reinterpret_cast<const double2_t*>(ap);
  const int n2 = n >> 1;
  double dot = 0.0;
  int q = lane;
  for (; q + 192 < n2; q += 256) {  // eight independent loads in flight; the sum keeps the order of q
    const double2_t x0 = a2[q], x1 = a2[q + 64], x2 = a2[q + 128], x3 = a2[q + 192];
    const double2_t y0 = p2[q], y1 = p2[q + 64], y2 = p2[q + 128], y3 = p2[q + 192];
    dot = __builtin_fma(x0.x, y0.x, dot);
    dot = __builtin_fma(x0.y, y0.y, dot);
    dot = __builtin_fma(x1.x, y1.x, dot);
    dot = __builtin_fma(x1.y, y1.y, dot);
    dot = __builtin_fma(x2.x, y2.x, dot);
    dot = __builtin_fma(x2.y, y2.y, dot);
    dot = __builtin_fma(x3.x, y3.x, dot);
    dot = __builtin_fma(x3.y, y3.y, dot);
  }
  for (; q < n2; q += 64) {
    const double2_t x = a2[q], y = p2[q];
    dot = __builtin_fma(x.x, y.x, dot);
    dot = __builtin_fma(x.y, y.y, dot);
  }
  if ((n & 1) && lane == 0) dot = __builtin_fma(a[n - 1], ap[n - 1], dot);
  dot = wave_sum(dot);
  double hs = 0.0;
  for (int s = lane; s < step; s += 64) hs = __builtin_fma(hist[s * mcp + row], hist[s * mcp + p] / vs[s], hs);
  hs = wave_sum(hs);
  const int d = spec.d, nk = spec.nkern;
  const double* __restrict__ xi = Xc + (long)row * d;
  const double* __restrict__ xj = Xc + (long)p * d;
  double kval = 0.0;
  for (int c = 0; c < nk; ++c) {
    double r2 = 0.0;
    for (int m = lane; m < d; m += 64) {
      const double u = (xi[m] - xj[m]) * (1.0 / theta[c * d + m]);
      r2 = __builtin_fma(u, u, r2);
    }
    r2 = wave_sum(r2);
    double k, dk, da;
    base_kernel_val_der(spec.kid[c], r2, theta[nk * d + nk + c], k, dk, da);
    k *= theta[nk * d + c];
    kval = c == 0 ? k : spec.op[c - 1] == 0 ? kval + k : kval * k;
  }
  if (lane == 0) {
    hist[step * mcp + row] = (kval - dot) - hs;
  }
}

// the fused pass over the alive rows at the pivot p = piv[0] (p < 0: nothing); g: the step's candidate column
__global__ __launch_bounds__(256) void design_update_kernel(double* __restrict__ G, long ldc, int Mc, int Mr, const double* __restrict__ g,
                                                            double* __restrict__ v, const double* __restrict__ vs, int step,
                                                            const int* __restrict__ piv, const int* __restrict__ alive,
                                                            double* __restrict__ rowsq) {
  const int p = piv[0];
  if (p < 0) return;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= Mc || alive[row] == 0) return;
  const double gc = g[row];
  const double f = gc / vs[step];
  double* __restrict__ a = G + (long)row * ldc;
  const double* __restrict__ pr = G + (long)p * ldc;  // (dead: no wave writes it)
  double2_t* a2 = reinterpret_cast<double2_t*>(a);
  const double2_t* __restrict__ p2 = reinterpret_cast<const double2_t*>(pr);
  const int m2 = Mr >> 1;
  double s = 0.0;
  int q = lane;
  for (; q + 192 < m2; q += 256) {  // eight independent loads in flight; the sum keeps the order of q
    double2_t x0 = a2[q], x1 = a2[q + 64], x2 = a2[q + 128], x3 = a2[q + 192];
    const double2_t y0 = p2[q], y1 = p2[q + 64], y2 = p2[q + 128], y3 = p2[q + 192];
    x0.x = __builtin_fma(-f, y0.x, x0.x); x0.y = __builtin_fma(-f, y0.y, x0.y);
    x1.x = __builtin_fma(-f, y1.x, x1.x); x1.y = __builtin_fma(-f, y1.y, x1.y);
    x2.x = __builtin_fma(-f, y2.x, x2.x); x2.y = __builtin_fma(-f, y2.y, x2.y);
    x3.x = __builtin_fma(-f, y3.x, x3.x); x3.y = __builtin_fma(-f, y3.y, x3.y);
    a2[q] = x0;
    a2[q + 64] = x1;
    a2[q + 128] = x2;
    a2[q + 192] = x3;
    s = __builtin_fma(x0.x, x0.x, s);
    s = __builtin_fma(x0.y, x0.y, s);
    s = __builtin_fma(x1.x, x1.x, s);
    s = __builtin_fma(x1.y, x1.y, s);
    s = __builtin_fma(x2.x, x2.x, s);
    s = __builtin_fma(x2.y, x2.y, s);
    s = __builtin_fma(x3.x, x3.x, s);
    s = __builtin_fma(x3.y, x3.y, s);
  }
  for (; q < m2; q += 64) {
    double2_t x = a2[q];
    const double2_t y = p2[q];
    x.x = __builtin_fma(-f, y.x, x.x);
    x.y = __builtin_fma(-f, y.y, x.y);
    a2[q] = x;
    s = __builtin_fma(x.x, x.x, s);
    s = __builtin_fma(x.y, x.y, s);
  }
  if ((Mr & 1) && lane == 0) {
    const double x = __builtin_fma(-f, pr[Mr - 1], a[Mr - 1]);
    a[Mr - 1] = x;
    s = __builtin_fma(x, x, s);
  }
  s = wave_sum(s);
  if (lane == 0) {
    rowsq[row] = s;
    v[row] = __builtin_fma(-gc, f, v[row]);
  }
}

hipError_t launch_design_rowsq(const double* G, long ldc, int Mc, int Mr, double* rowsq, hipStream_t stream) {
  design_rowsq_kernel<<<(Mc + 3) / 4, 256, 0, stream>>>(G, ldc, Mc, Mr, rowsq);
  return hipGetLastError();
}

hipError_t launch_design_step(const KernSpec& spec, const double* theta, const double* Xc, int Mc, int Mr, int b, int step,
                              const double* A, long ldw, int n, double* G, long ldc, double noise, const DesignScratch& t, double* out,
                              hipStream_t stream) {
  const int rows = (Mc + 3) / 4;
  design_pick_kernel<<<1, 256, 0, stream>>>(step, Mc, Mr, b, noise, t.v, t.rowsq, t.alive, t.piv, t.vs, out);
  design_column_kernel<<<rows, 256, 0, stream>>>(spec, theta, Xc, Mc, A, ldw, n, step, t.hist, t.mcp, t.vs, t.piv);
  design_update_kernel<<<rows, 256, 0, stream>>>(G, ldc, Mc, Mr, t.hist + step * t.mcp, t.v, t.vs, step, t.piv, t.alive, t.rowsq);
  return hipGetLastError();
}

}  // namespace migp
