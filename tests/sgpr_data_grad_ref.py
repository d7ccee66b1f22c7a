"""References of the sparse bound's gradients by the data (include/mi_gp_sparse_data.h), for tests/test_sgpr_data_grad_host.py,
tests/test_gpu_sparse_data_grad.py and the warp tests.  No GPU and no device library; everything the bound itself needs comes from
tests/sgpr_ref.py and tests/sgpr_zgrad_ref.py, which stay as they are.

  data_grads_ld     dF/dy and dF/dX in np.longdouble: the algebra of sgpr_zgrad_ref.zgrad_ld up to T, then
                    gy = -y / s + Kuf^T t with t = L^-T a^ / s, and gx = contract_z(T^T, X, Z) -- the same derivative of the
                    kernel, taken by its first argument, with the data points in that place.  THE reference of the device tests
  device_fp64_data  the device's steps in fp64 NumPy: expansion-form assemblies, T_c^T = A_c^T M2 + y_c t^T per chunk, dF/dy
                    from the chunk's resident rows, A_c^T a^ / s
  CASES             the 30 cases of sgpr_ref.DEVICE_CASES with one change (case_theta below says which and why)
  SparseStandIn     a NumPy object with the methods GPMCMC._warp_likelihood asks of MiSparseGP, backed by the fp64 steps
"""
import numpy as np

import sgpr_ref as R
import sgpr_zgrad_ref as ZR

LD = R.LD
CASES = R.DEVICE_CASES


def case_theta(kernel, d):
    """sgpr_ref.case_theta with one change: Matern52*Exponential at d = 17 takes 300, not 100, times linspace(0.4, 1.5, d).
    The cause is the one sgpr_ref.case_theta describes -- the assemblies' expansion-form r2 leaves a rounding residue where the
    direct form gives 0, and Exponential's sqrt(r2 + 1e-12) magnifies it.  At 100 times the fp64 restatement alone uses 1.77
    tolerances on dF/dX at (257, 130, 17) on the k-means++ case and 0.33 on the subset case; at 300 times it uses 0.02."""
    if kernel == "Matern52*Exponential" and d == 17:
        return R.make_theta(kernel, d, ls=300.0 * np.linspace(0.4, 1.5, d))
    return R.case_theta(kernel, d)


def device_case(case):
    """sgpr_ref.device_case with this file's case_theta"""
    X, y, Z, _, Xnew, chunk = R.device_case(case)
    return X, y, Z, case_theta(case[0], case[3]), Xnew, chunk


def data_grads_ld(X, y, Z, kernel, theta):
    """dict: grad_y (n), grad_x (n, d) in np.longdouble and cond_Kuu (fp64).  The algebra up to T is sgpr_zgrad_ref.zgrad_ld's."""
    kerns, _ = R.split(kernel)
    d, m = X.shape[1], Z.shape[0]
    _, _, _, gv, jitter = R.split_theta(theta, d, len(kerns))
    s = LD(gv) + LD(jitter)
    yl = y.astype(LD)
    Im = np.eye(m, dtype=LD)
    Kuu = R.cov(Z, Z, kernel, theta) + LD(jitter) * Im
    Kuf = R.cov(Z, X, kernel, theta)
    L = R.cholesky_ld(Kuu)
    A = R.forward_ld(L, Kuf)
    B = Im + (A @ A.T) / s
    LB = R.cholesky_ld(B)
    c = R.forward_ld(LB, (A @ yl)[:, None])[:, 0] / s
    LBinv = R.forward_ld(LB, Im)
    Linv = R.forward_ld(L, Im)
    Binv = LBinv.T @ LBinv
    ah = LBinv.T @ c
    T = Linv.T @ (((Im - Binv - np.outer(ah, ah)) @ A + np.outer(ah, yl)) / s)
    t = (Linv.T @ ah) / s
    return {"grad_y": -yl / s + Kuf.T @ t, "grad_x": ZR.contract_z(T.T, X, Z, kernel, theta),
            "cond_Kuu": float(np.linalg.cond(Kuu.astype(np.float64)))}


def device_fp64_data(X, y, Z, kernel, theta, chunk=None, full=False):
    """(dF/dy, dF/dX) by csrc/api_sparse.hip's steps in fp64 NumPy (sgpr_ref.device_fp64's matrices in the same roles); with
    ``full`` also F, dF/dtheta and dF/dZ from sgpr_ref.device_fp64 and sgpr_zgrad_ref.device_fp64_z"""
    import scipy.linalg as sla

    f8 = np.float64
    kerns, _ = R.split(kernel)
    n, d = X.shape
    m = Z.shape[0]
    _, _, _, gv, jitter = R.split_theta(theta, d, len(kerns))
    s = gv + jitter
    chunk = n if chunk is None else chunk
    Kuu = R.cov(Z, Z, kernel, theta, f8, expansion=True)
    Kuu[np.diag_indices(m)] += jitter
    L = np.linalg.cholesky(Kuu)
    Psi, v = np.zeros((m, m)), np.zeros(m)
    rows = []
    for i0 in range(0, n, chunk):
        Xc, yc = X[i0:i0 + chunk], y[i0:i0 + chunk]
        At = sla.solve_triangular(L, R.cov(Z, Xc, kernel, theta, f8, expansion=True), lower=True).T
        rows.append((Xc, yc, At))
        Psi += At.T @ At
        v += At.T @ yc
    LB = np.linalg.cholesky(np.eye(m) + Psi / s)
    UB = sla.solve_triangular(LB, np.eye(m), lower=True).T
    ah = UB @ (UB.T @ (v / s))
    U = sla.solve_triangular(L, np.eye(m), lower=True).T
    H = np.eye(m) - UB @ UB.T - np.outer(ah, ah)
    M2 = (H @ U.T) / s
    tv = (U @ ah) / s
    gy = np.concatenate([-yc / s + (At @ ah) / s for _, yc, At in rows])
    gx = np.concatenate([ZR.contract_z(At @ M2 + np.outer(yc, tv), Xc, Z, kernel, theta, f8) for Xc, yc, At in rows])
    if not full:
        return gy, gx
    out = R.device_fp64(X, y, Z, kernel, theta, chunk=chunk)
    return out["F"], out["grad"], gy, gx, ZR.device_fp64_z(X, y, Z, kernel, theta, chunk=chunk)


_REFERENCES = {}


def reference(X, y, Z, kernel, theta, key):
    """data_grads_ld, computed once per process under `key` and shared (callers must not change it)"""
    if key not in _REFERENCES:
        _REFERENCES[key] = data_grads_ld(X, y, Z, kernel, theta)
    return _REFERENCES[key]


def case_reference(case):
    X, y, Z, theta, _, _ = device_case(case)
    return reference(X, y, Z, case[0], theta, case)


def ratios(gy, gx, ref):
    """(dF/dy's, dF/dX's) largest error against data_grads_ld's, per entry relative to max(|ref|, 1), over the project's gradient
    tolerance max(1e-10, 200 cond(Kuu) eps) (sgpr_ref.tolerances)"""
    ptol = R.tolerances(ref["cond_Kuu"])[1]

    def one(got, g):
        return float(np.max(np.abs(np.asarray(got).astype(LD) - g) / np.maximum(np.abs(g), 1))) / ptol

    return one(gy, ref["grad_y"]), one(gx, ref["grad_x"])


class SparseStandIn:
    """Stands in for andvaranaut_amd.MiSparseGP(data_grad=True, z_grad=True) on the CPU: update_data, set_inducing and
    lml_grad_data, arithmetic by device_fp64_data (tests only; the manner of test_host_logic._OracleGP).  ``precise=True``
    takes the long-double references instead (bound_ld, zgrad_ld, data_grads_ld), rounded to fp64 at the end.  ``cond`` is
    cond(Kuu) at the last evaluation."""

    def __init__(self, X, y, Z, kernel, precise=False):
        self.X, self.y, self.Z, self.kernel, self.precise = np.array(X), np.array(y), np.array(Z), kernel, precise
        self.calls = []
        self.cond = None

    def update_data(self, X=None, y=None):
        if X is not None:
            self.X = np.array(X, dtype=np.float64)
        if y is not None:
            self.y = np.array(y, dtype=np.float64)

    def set_inducing(self, Z):
        self.calls.append("set_inducing")
        self.Z = np.array(Z, dtype=np.float64)

    def lml_grad_data(self, theta, want_x=True, want_z=False):
        self.calls.append((bool(want_x), bool(want_z)))
        theta = np.asarray(theta, dtype=np.float64)
        try:
            if self.precise:
                b = R.bound_ld(self.X, self.y, self.Z, self.kernel, theta)
                dg = data_grads_ld(self.X, self.y, self.Z, self.kernel, theta)
                F, g, gy, gx = b["F"], b["grad"], dg["grad_y"].astype(np.float64), dg["grad_x"].astype(np.float64)
                gz = ZR.zgrad_ld(self.X, self.y, self.Z, self.kernel, theta)["grad_z"].astype(np.float64) if want_z else None
                self.cond = b["cond_Kuu"]
            else:
                F, g, gy, gx, gz = device_fp64_data(self.X, self.y, self.Z, self.kernel, theta, full=True)
        except np.linalg.LinAlgError:
            out = (-np.inf, np.zeros(len(theta)), np.zeros(len(self.y)), np.zeros(self.X.shape) if want_x else None)
            return out + (np.zeros(self.Z.shape),) if want_z else out
        out = (float(F), np.asarray(g, dtype=np.float64), gy, gx if want_x else None)
        return out + (gz,) if want_z else out


def warp_tolerances(cond):
    """(value, gradient, which) for a posterior through the warps: the rule of tests/test_gpu_facade.py's dense counterpart --
    the value within 1e-9 relative, every gradient entry within 1e-7 max(1, max|g|) -- or, where cond(Kuu) makes them looser,
    sgpr_ref.tolerances' pair in the same places"""
    vtol, ptol = R.tolerances(cond)
    return max(1e-9, vtol), max(1e-7, ptol), ("facade" if vtol <= 1e-9 else "cond", "facade" if ptol <= 1e-7 else "cond")


def warp_errors(v, g, vref, gref, cond):
    """the errors of a posterior value and gradient over warp_tolerances' pair"""
    vt, gt, which = warp_tolerances(cond)
    return abs(v - vref) / (vt * abs(vref)), float(np.abs(g - gref).max()) / (gt * max(1.0, float(np.abs(gref).max()))), which
