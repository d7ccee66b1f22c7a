"""References for the GP trend with marginalised coefficients (option 50 of mi_gp_set_option, MiGP.set_trend), in float64
NumPy / SciPy, sharing nothing with the device:

    trend_direct       the device's algebra restated (Rasmussen & Williams eq. 2.45 with V = K^-1 H, A = H^T V, P~, alpha~), its
                       gradient by the contraction 1/2 sum (alpha~ alpha~^T - P~) dK
    trend_projected    the DEFINITION of the value: L_T = log N(C^T y; 0, C^T K_y C) - 1/2 log|H^T H| with C an orthonormal basis
                       of null(H^T) (the density of the data projected off the basis; the last term is the Jacobian of the vague
                       prior's limit, R & W eq. 2.45)
    trend_forward      (value, gradient) in forward mode ON THE PROJECTED DATA: one K_c^-1 (C^T dK/dtheta_k C) per hyper-parameter
    predict_dense      R & W eqs. 2.41-2.42 through dense solves with K_y (conditional form)
    predict_factor     the same through the factor L, G = L^-1 H and b~, as the device forms it

and the cases that tests/test_trend_host.py and tests/test_gpu_trend.py share: loo_ref.CASES[2:] x orders {1, 2}, and loo_ref.BIG
with order 2."""
import functools

import numpy as np
import scipy.linalg as sla

import kfold_ref
import loo_ref
from oracle import gp_oracle as orc

LOG_2PI = kfold_ref.LOG_2PI
ORDERS = (1, 2)
NAMES = {1: "constant", 2: "linear"}


def basis(X, order):
    """H (n x p): rows h(x)^T = [1] (order 1) or [1, x_1 .. x_d] (order 2)"""
    X = np.asarray(X, dtype=np.float64)
    return np.ones((len(X), 1)) if order == 1 else np.hstack([np.ones((len(X), 1)), X])


def _cov(X, kernel, theta, diag, form="marginal"):
    kerns, ops = kfold_ref.split_kernel(kernel)
    return kerns, ops, orc.noisy_cov(X, kerns, ops, theta, form, diag)


def trend_direct(X, y, kernel, theta, order, diag=None, grad=True):
    kerns, ops, K = _cov(X, kernel, theta, diag)
    n = len(y)
    H = basis(X, order)
    p = H.shape[1]
    L = sla.cholesky(K, lower=True)
    Kinv = sla.cho_solve((L, True), np.eye(n))
    Kinv = 0.5 * (Kinv + Kinv.T)
    alpha = Kinv @ y
    lml = -0.5 * y @ alpha - np.sum(np.log(np.diag(L))) - 0.5 * n * LOG_2PI
    V = Kinv @ H
    CA = sla.cholesky(H.T @ V, lower=True)
    Q = sla.solve_triangular(CA, V.T, lower=True).T
    c = Q.T @ y
    val = lml + 0.5 * c @ c - np.sum(np.log(np.diag(CA))) + 0.5 * p * LOG_2PI
    if not grad:
        return float(val), None
    Pt = Kinv - Q @ Q.T
    at = alpha - Q @ c
    return float(val), loo_ref.contract(Pt - np.outer(at, at), X, kerns, ops, theta)


def _projected(X, y, kernel, theta, order, diag):
    kerns, ops, K = _cov(X, kernel, theta, diag)
    H = basis(X, order)
    p = H.shape[1]
    Qf, R = np.linalg.qr(H, mode="complete")
    C = Qf[:, p:]
    return kerns, ops, C, C.T @ K @ C, C.T @ y, -np.sum(np.log(np.abs(np.diag(R))))


def trend_projected(X, y, kernel, theta, order, diag=None):
    _, _, _, Kc, yc, jac = _projected(X, y, kernel, theta, order, diag)
    Lc = sla.cholesky(Kc, lower=True)
    z = sla.solve_triangular(Lc, yc, lower=True)
    return float(-0.5 * z @ z - np.sum(np.log(np.diag(Lc))) - 0.5 * len(yc) * LOG_2PI + jac)


def project_householder(K, y, H):
    """(C^T K C, C^T y, -1/2 log|H^T H|) without forming C: the p Householder reflectors of H's QR factorisation applied to K from
    both sides and to y, O(n^2 p) -- what makes the projected-data value affordable at thousands of points"""
    K, y, R = np.array(K, dtype=np.float64), np.array(y, dtype=np.float64), np.array(H, dtype=np.float64)
    p = R.shape[1]
    for j in range(p):
        x = R[j:, j]
        s = -np.linalg.norm(x) if x[0] >= 0 else np.linalg.norm(x)
        v = x.copy()
        v[0] -= s
        tau = 2.0 / (v @ v)
        R[j:, :] -= tau * np.outer(v, v @ R[j:, :])
        y[j:] -= tau * v * (v @ y[j:])
        K[j:, :] -= tau * np.outer(v, v @ K[j:, :])
        K[:, j:] -= tau * np.outer(K[:, j:] @ v, v)
    return K[p:, p:], y[p:], -np.sum(np.log(np.abs(np.diag(R[:p, :p]))))


def trend_projected_large(X, y, kernel, theta, order, diag=None):
    """trend_projected through project_householder (the same definition, another route to C^T K C)"""
    _, _, K = _cov(X, kernel, theta, diag)
    Kc, yc, jac = project_householder(K, y, basis(X, order))
    Lc = sla.cholesky(Kc, lower=True, overwrite_a=True, check_finite=False)
    z = sla.solve_triangular(Lc, yc, lower=True, check_finite=False)
    return float(-0.5 * z @ z - np.sum(np.log(np.diag(Lc))) - 0.5 * len(yc) * LOG_2PI + jac)


def trend_forward(X, y, kernel, theta, order, diag=None):
    kerns, ops, C, Kc, yc, jac = _projected(X, y, kernel, theta, order, diag)
    Lc = sla.cholesky(Kc, lower=True)
    ac = sla.cho_solve((Lc, True), yc)
    val = -0.5 * yc @ ac - np.sum(np.log(np.diag(Lc))) - 0.5 * len(yc) * LOG_2PI + jac
    dK = orc.dK_dtheta(X, kerns, ops, theta)
    g = np.zeros(len(dK))
    for k in range(len(dK)):
        dKc = C.T @ dK[k] @ C
        g[k] = 0.5 * ac @ dKc @ ac - 0.5 * np.trace(sla.cho_solve((Lc, True), dKc))
    return float(val), g


def _cross(X, Xn, kernel, theta):
    kerns, ops = kfold_ref.split_kernel(kernel)
    return orc.kernel_matrix(X, Xn, kerns, ops, theta), orc.kernel_diag(kerns, ops, theta, X.shape[1])


def predict_dense(X, y, Xn, kernel, theta, order, diag=None, pred_noise=True):
    """(mean, var, the trend's term of var) at Xn"""
    _, _, K = _cov(X, kernel, theta, diag, "conditional")
    Ks, kd = _cross(X, Xn, kernel, theta)
    H, Hs = basis(X, order), basis(Xn, order)
    KiH, Kiy, KiKs = np.linalg.solve(K, H), np.linalg.solve(K, y), np.linalg.solve(K, Ks)
    A = H.T @ KiH
    beta = np.linalg.solve(A, H.T @ Kiy)
    R = Hs.T - H.T @ KiKs
    term = np.sum(R * np.linalg.solve(A, R), axis=0)
    mean = Ks.T @ (Kiy - KiH @ beta) + Hs @ beta
    gv = np.sqrt(theta[-2]) ** 2 if pred_noise else 0.0
    return mean, kd - np.sum(Ks * KiKs, axis=0) + term + gv, term


def predict_factor(X, y, Xn, kernel, theta, order, diag=None, pred_noise=True):
    _, _, K = _cov(X, kernel, theta, diag, "conditional")
    Ks, kd = _cross(X, Xn, kernel, theta)
    H, Hs = basis(X, order), basis(Xn, order)
    L = sla.cholesky(K, lower=True)
    G = sla.solve_triangular(L, H, lower=True)
    b = sla.solve_triangular(L, y, lower=True)
    CA = sla.cholesky(G.T @ G, lower=True)
    beta = sla.cho_solve((CA, True), G.T @ b)
    bt = b - G @ beta
    A = sla.solve_triangular(L, Ks, lower=True)
    T = sla.solve_triangular(CA, Hs.T - G.T @ A, lower=True)
    term = np.sum(T * T, axis=0)
    gv = np.sqrt(theta[-2]) ** 2 if pred_noise else 0.0
    return A.T @ bt + Hs @ beta, kd - np.sum(A * A, axis=0) + term + gv, term


# ------------------------------------------------------------------------------------------------------------------ cases
CASE_IDS = [(i, o) for i in range(2, len(loo_ref.CASES)) for o in ORDERS]
# the share of the variance that the trend's term carries at the outside points of predict_points(), at least (measured on the
# references of every case: the smallest is 0.081 for a constant and 0.422 for a linear trend)
MIN_SHARE = {1: 0.08, 2: 0.42}


# p = 128 coefficients (d = 127, the most option 50 takes): all eight 16-column blocks of the symmetric multiply and sixteen
# passes of the predict reduction; n = 200 leaves 72 projected points
WIDE = ("RBF", 200, 127, False, 1e-2)


@functools.lru_cache(maxsize=None)
def wide_case():
    """(X, y, kernel, theta, cond(K), projected value, forward gradient, points, predict_dense's result) of WIDE, linear trend"""
    kernel, n, d, with_diag, gv = WIDE
    X, y, theta, diag = loo_ref.make_problem(kernel, n, d, with_diag, gv, 123)
    cond = kfold_ref.full_cond(X, kernel, theta, diag)
    _, g = trend_forward(X, y, kernel, theta, 2, diag)
    Xn = predict_points(77, d)
    return X, y, kernel, theta, cond, trend_projected(X, y, kernel, theta, 2, diag), g, Xn, predict_dense(X, y, Xn, kernel, theta, 2, diag)


def predict_points(i, d):
    """5 points inside [0, 1]^d, then 5 outside it at 1 + 2 U(0, 1)^d"""
    rng = np.random.default_rng(i)
    return np.vstack([rng.random((5, d)), 1.0 + 2.0 * rng.random((5, d))])


@functools.lru_cache(maxsize=None)
def case_refs(i, order):
    """(value by the projected-data definition, (value, gradient) in forward mode) of loo_ref.CASES[i] under a trend of the given
    order, once per process"""
    X, y, kernel, theta, diag, _ = loo_ref.case(i)
    out = (trend_projected(X, y, kernel, theta, order, diag), trend_forward(X, y, kernel, theta, order, diag))
    out[1][1].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case_predict(i, order):
    """(points, predict_dense's (mean, var, term)) of loo_ref.CASES[i]"""
    X, y, kernel, theta, diag, _ = loo_ref.case(i)
    Xn = predict_points(i, X.shape[1])
    out = predict_dense(X, y, Xn, kernel, theta, order, diag)
    for a in (Xn,) + out:
        a.setflags(write=False)
    return Xn, out
