// Device math shared by the covariance assembly (assemble.hip) and the kernels that differentiate it (grad_predict.hip):
// K and dK/dtheta are built from the SAME exp / sqrt sequences, so they are bit-consistent with each other.
#pragma once
#include <hip/hip_runtime.h>
#include "migp_kernels.h"

namespace migp {

// exp(x) for x <= 0 (any magnitude, -inf included): Cody-Waite reduction by ln 2 in two pieces, degree-13 Taylor polynomial
// on |r| <= ln2 / 2 (remainder 4e-18 relative), ldexp.  Max error 1.0 ulp against libm over [-745, 0]; arguments below
// -746 (exp underflows to 0 from -745.13 on) are clamped there, so -inf -- r2 = inf from an underflowing length scale --
// gives 0 like libm, not NaN (the unclamped reduction computed inf - inf).  That holds for the RBF family only: the Matern /
// Exponential argument goes through sqrt_pos first, and sqrt_pos(inf) is NaN.  fmax also turns a NaN argument into -746:
// NaN does NOT propagate through this function, which is why the host rejects non-finite theta (factor_internal) and
// non-finite X / y (MiGP.__init__, MiGP.update_data) before anything reaches the device.
__device__ __forceinline__ double exp_nonpos(double x) {
  x = __builtin_fmax(x, -746.0);
  const double k = __builtin_rint(x * 1.4426950408889634);
  double r = __builtin_fma(-k, 0.6931471803691238, x);
  r = __builtin_fma(-k, 1.9082149292705877e-10, r);
  double p = 1.6059043836821613e-10;                       // 1/13!
  p = __builtin_fma(p, r, 2.08767569878681e-09);          // 1/12!
  p = __builtin_fma(p, r, 2.505210838544172e-08);         // 1/11!
  p = __builtin_fma(p, r, 2.755731922398589e-07);         // 1/10!
  p = __builtin_fma(p, r, 2.7557319223985893e-06);        // 1/9!
  p = __builtin_fma(p, r, 2.48015873015873e-05);          // 1/8!
  p = __builtin_fma(p, r, 0.0001984126984126984);         // 1/7!
  p = __builtin_fma(p, r, 0.001388888888888889);          // 1/6!
  p = __builtin_fma(p, r, 0.008333333333333333);          // 1/5!
  p = __builtin_fma(p, r, 0.041666666666666664);          // 1/4!
  p = __builtin_fma(p, r, 0.16666666666666666);           // 1/3!
  p = __builtin_fma(p, r, 0.5);
  p = __builtin_fma(p, r, 1.0);
  p = __builtin_fma(p, r, 1.0);
  return __builtin_amdgcn_ldexp(p, (int)k);                // k >= -1077: 2^-1077 p rounds to 0
}

// sqrt(t) for normal t > 0: v_rsq_f64 seed (measured 2^-24.2 relative, tools/probe_rcp.hip), ONE Goldschmidt step
// (g, h to ~2^-48) and one Newton correction g + (t - g^2) h, whose error is the PRODUCT of the two (2^-96) plus the
// final rounding: <= 1 ulp against libm (tools/probe_math.hip).  Round 2 ran two Goldschmidt steps (three more FMAs).
__device__ __forceinline__ double sqrt_pos(double t) {
  const double y = __builtin_amdgcn_rsq(t);
  double g = t * y, h = 0.5 * y;
  const double e = __builtin_fma(-h, g, 0.5);
  g = __builtin_fma(g, e, g);
  h = __builtin_fma(h, e, h);
  const double dd = __builtin_fma(-g, g, t);
  return __builtin_fma(dd, h, g);
}

// d k / d r2 of the base kernels (matches oracle base_kernel_dr2) and the value itself
__device__ __forceinline__ void base_kernel_val_der(int kid, double r2, double alpha, double& k, double& dk,
                                                    double& dalpha) {
  dalpha = 0.0;
  if (kid == KID_RATQUAD) {
    const double u = 0.5 * r2 / alpha;
    k = pow(1.0 + u, -alpha);
    dk = -0.5 * k / (1.0 + u);
    dalpha = k * (-log1p(u) + u / (1.0 + u));
    return;
  }
  // the four exponential families share ONE exp evaluation: e = exp(-rate * s), s = r2 (RBF) or r = sqrt(r2 + 1e-12)
  const bool rbf = kid == KID_RBF;
  const double r = rbf ? 0.0 : sqrt_pos(r2 + 1e-12);
  const double rate = rbf ? 0.5 : kid == KID_MATERN52 ? 2.23606797749979 : kid == KID_MATERN32 ? 1.7320508075688772 : 0.5;
  const double e = exp_nonpos(-1.0 * rate * (rbf ? r2 : r));
  if (rbf) {
    k = e;
    dk = -0.5 * e;
  } else if (kid == KID_MATERN52) {
    k = (1.0 + 2.23606797749979 * r + 5.0 / 3.0 * (r * r)) * e;
    dk = -(5.0 / 6.0) * (1.0 + 2.23606797749979 * r) * e;
  } else if (kid == KID_MATERN32) {
    k = (1.0 + 1.7320508075688772 * r) * e;
    dk = -1.5 * e;
  } else {
    k = e;
    dk = -0.25 * e / r;
  }
}

// k and its first three derivatives by s = r2 for the two families a joint GP over f and grad f is built from (deriv_f64.hip):
// k and k1 are base_kernel_val_der's k and dk, from the same exp / sqrt sequences.
//   RBF:        k_m = (-1/2)^m k
//   Matern-5/2: k2 = 25/12 e^(-sqrt5 r), k3 = -(25 sqrt5 / 24) e^(-sqrt5 r) / r with r = sqrt(s + 1e-12) >= 1e-6; every use of k3
//               multiplies it by four differences, so it is finite and its term vanishes at coincident points
__device__ __forceinline__ void base_kernel_val_der3(int kid, double r2, double& k, double& k1, double& k2, double& k3) {
  if (kid == KID_RBF) {
    const double e = exp_nonpos(-0.5 * r2);
    k = e;
    k1 = -0.5 * e;
    k2 = 0.25 * e;
    k3 = -0.125 * e;
    return;
  }
  const double r = sqrt_pos(r2 + 1e-12);
  const double e = exp_nonpos(-1.0 * 2.23606797749979 * r);
  k = (1.0 + 2.23606797749979 * r + 5.0 / 3.0 * (r * r)) * e;
  k1 = -(5.0 / 6.0) * (1.0 + 2.23606797749979 * r) * e;
  k2 = (25.0 / 12.0) * e;
  k3 = -(25.0 * 2.23606797749979 / 24.0) * e / r;
}

// NK = 8 is the one instantiation for 5..8 components: it reads the count at run time, `RUNTIME_NK<NK> ? spec.nkern : NK`
template <int NK>
constexpr bool RUNTIME_NK = NK > 4;

// Component c at scaled squared distance r2: kval = kv_c k, dkv = kv_c dk/dr2 and, only under RQ (some component is a
// rational quadratic), dal = kv_c dk/dalpha -- identically zero otherwise, and then not carried.  kvc is a reference so
// that a caller's kv[c] is read where it is used.
template <bool RQ>
__device__ __forceinline__ void comp_val_der(int kid, double r2, double alpha, const double& kvc, double& kval, double& dkv,
                                             double& dal) {
  double k, dk, da;
  base_kernel_val_der(kid, r2, alpha, k, dk, da);
  kval = kvc * k;
  dkv = kvc * dk;
  if constexpr (RQ) dal = kvc * da;
}

}  // namespace migp
