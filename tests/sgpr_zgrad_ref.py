"""References of the sparse bound's gradient by the inducing locations (include/mi_gp_sparse.h), for
tests/test_sgpr_zgrad_host.py and tests/test_gpu_sparse_zgrad.py.  No GPU and no device library; everything the bound itself needs
comes from tests/sgpr_ref.py, which stays as it is.

  contract_z      g[u, d] = sum_j Wt[u, j] dK(z_u, x_j) / dz_ud for a weight matrix over (inducing point, point): the fold's
                  coefficient times kv_c k_c'(r2_c) times 2 (z_ud - x_jd) / l_cd^2, r2 in the direct form
  zgrad_ld        dF/dZ in np.longdouble: contract_z(T, Z, X) + 2 contract_z(Guu, Z, Z) with the T = dF/dKuf and Guu = dF/dKuu of
                  sgpr_ref.bound_ld (Kuu is symmetric and each z_u moves row u and column u of it: the factor 2).  THE reference
                  of the device tests
  device_fp64_z   the device's steps in fp64 NumPy: expansion-form assemblies, T_c^T = A_c^T M2 + y_c t^T, W = -2 Guu, Kuf's
                  term summed chunk by chunk in chunk order, then Kuu's term with the weight -W
"""
import numpy as np

import sgpr_ref as R

LD = R.LD


def contract_z(Wt, Zs, X2, kernel, theta, dt=LD):
    """(m, d) array: sum over the points X2 of Wt[u, j] dK(z_u, x_j)/dz_u"""
    kerns, ops = R.split(kernel)
    nk, d = len(kerns), Zs.shape[1]
    ls, kv, al, _, _ = R.split_theta(theta, d, nk)
    parts = [R.base_kernel(kerns[c], R._r2(Zs, X2, ls[c], dt, False), al[c]) for c in range(nk)]
    coefs = R.fold_coefs([dt(kv[c]) * parts[c][0] for c in range(nk)], ops)
    g = np.zeros(Zs.shape, dtype=dt)
    Wt = Wt.astype(dt)
    for c in range(nk):
        G = Wt * coefs[c] * dt(kv[c]) * parts[c][1]
        for k in range(d):
            df = Zs[:, k, None].astype(dt) - X2[None, :, k].astype(dt)
            g[:, k] += (G * df).sum(axis=1) * (dt(2) / (dt(ls[c, k]) * dt(ls[c, k])))
    return g


def zgrad_ld(X, y, Z, kernel, theta):
    """dict: grad_z (m, d) in np.longdouble and cond_Kuu (fp64).  The algebra up to T and Guu is sgpr_ref.bound_ld's, literally."""
    kerns, _ = R.split(kernel)
    d, m = X.shape[1], Z.shape[0]
    _, _, _, gv, jitter = R.split_theta(theta, d, len(kerns))
    s = LD(gv) + LD(jitter)
    yl = y.astype(LD)
    Im = np.eye(m, dtype=LD)
    Kuu = R.cov(Z, Z, kernel, theta) + LD(jitter) * Im
    L = R.cholesky_ld(Kuu)
    A = R.forward_ld(L, R.cov(Z, X, kernel, theta))
    B = Im + (A @ A.T) / s
    LB = R.cholesky_ld(B)
    c = R.forward_ld(LB, (A @ yl)[:, None])[:, 0] / s
    LBinv = R.forward_ld(LB, Im)
    Linv = R.forward_ld(L, Im)
    Binv = LBinv.T @ LBinv
    ah = LBinv.T @ c
    T = Linv.T @ (((Im - Binv - np.outer(ah, ah)) @ A + np.outer(ah, yl)) / s)
    Guu = -(Linv.T @ (B - 2 * Im + Binv + np.outer(ah, ah)) @ Linv) / 2
    return {"grad_z": contract_z(T, Z, X, kernel, theta) + 2 * contract_z(Guu, Z, Z, kernel, theta),
            "cond_Kuu": float(np.linalg.cond(Kuu.astype(np.float64)))}


def device_fp64_z(X, y, Z, kernel, theta, chunk=None):
    """dF/dZ by csrc/api_sparse.hip's steps in fp64 NumPy (sgpr_ref.device_fp64's matrices in the same roles)"""
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
    W = U @ ((Psi / s - H) @ U.T)  # -2 Guu
    tv = (U @ ah) / s
    gz = np.zeros((m, d))
    for k, (Xc, yc, At) in enumerate(rows):
        part = contract_z((At @ M2 + np.outer(yc, tv)).T, Z, Xc, kernel, theta, f8)
        gz = part if k == 0 else gz + part
    return gz + contract_z(-W, Z, Z, kernel, theta, f8)


_REFERENCES = {}


def reference(X, y, Z, kernel, theta, key):
    """zgrad_ld, computed once per process under `key` and shared (callers must not change it)"""
    if key not in _REFERENCES:
        _REFERENCES[key] = zgrad_ld(X, y, Z, kernel, theta)
    return _REFERENCES[key]


def case_reference(case):
    """zgrad_ld of a case of sgpr_ref.DEVICE_CASES (or any case tuple sgpr_ref.device_case takes)"""
    X, y, Z, theta, _, _ = R.device_case(case)
    return reference(X, y, Z, case[0], theta, case)


def ratio(got, ref):
    """the largest error of an (m, d) dF/dZ against zgrad_ld's, per entry relative to max(|ref|, 1), over the project's gradient
    tolerance max(1e-10, 200 cond(Kuu) eps) (sgpr_ref.tolerances)"""
    ptol = R.tolerances(ref["cond_Kuu"])[1]
    g = ref["grad_z"]
    return float(np.max(np.abs(np.asarray(got).astype(LD) - g) / np.maximum(np.abs(g), 1))) / ptol
