"""References for the leave-one-out objective (option 48 of mi_gp_set_option, MiGP.loo_grad): L_LOO = sum_i log p(y_i | y_-i)
and its gradient w.r.t. theta, three ways that share nothing with the device:

    loo_value_refit   the DEFINITION of the value: kfold_ref.kfold_refit on singletons (one factorisation of the complement per
                      point), summed
    loo_forward       Rasmussen & Williams eq. 5.10-5.13 in forward mode: one Z_k = K^-1 dK/dtheta_k per hyper-parameter, with the
                      oracle's dK_dtheta
    loo_reverse       the device's reverse-mode algebra restated in NumPy: G' = M - (alpha w^T + w alpha^T) contracted with dK

and the cases and bounds that tests/test_loo_host.py and tests/test_gpu_loo_objective.py share."""
import functools

import numpy as np
import scipy.linalg as sla

import kfold_ref
from oracle import gp_oracle as orc

EPS = kfold_ref.EPS
LOG_2PI = kfold_ref.LOG_2PI


def _kinv(X, y, kernel, theta, diag):
    kerns, ops = kfold_ref.split_kernel(kernel)
    L = sla.cholesky(orc.noisy_cov(X, kerns, ops, theta, "marginal", diag), lower=True)
    Kinv = sla.cho_solve((L, True), np.eye(len(y)))
    Kinv = 0.5 * (Kinv + Kinv.T)
    return kerns, ops, Kinv, Kinv @ y


def loo_value_refit(X, y, kernel, theta, diag=None):
    logp, _, _ = kfold_ref.kfold_refit(X, y, kernel, theta, [np.array([i]) for i in range(len(y))], diag)
    return float(np.sum(logp))


def loo_forward(X, y, kernel, theta, diag=None):
    """(L_LOO, dL_LOO/dtheta) by R & W eq. 5.13: dL/dtheta_k = sum_i (alpha_i [Z_k alpha]_i - 1/2 (1 + alpha_i^2 / p_i) [Z_k K^-1]_ii) / p_i"""
    kerns, ops, Kinv, alpha = _kinv(X, y, kernel, theta, diag)
    p = np.diag(Kinv).copy()
    val = float(np.sum(0.5 * np.log(p) - 0.5 * alpha * alpha / p - 0.5 * LOG_2PI))
    dK = orc.dK_dtheta(X, kerns, ops, theta)
    g = np.zeros(len(dK))
    for k in range(len(dK)):
        Z = Kinv @ dK[k]
        g[k] = np.sum((alpha * (Z @ alpha) - 0.5 * (1.0 + alpha * alpha / p) * np.einsum("ij,ji->i", Z, Kinv)) / p)
    return val, g


def contract(G, X, kerns, ops, theta, block=1500):
    """-1/2 sum_ij G_ij dK_ij/dtheta_k for a symmetric G, in row / column blocks of at most `block` points (dK_dtheta of the union
    of two blocks: the derivative of an entry depends on its two points alone)"""
    n = len(X)
    cuts = list(range(0, n, block)) + [n]
    g = None
    for a in range(len(cuts) - 1):
        I = np.arange(cuts[a], cuts[a + 1])
        for b in range(a + 1):
            J = np.arange(cuts[b], cuts[b + 1])
            if a == b:
                dK = orc.dK_dtheta(X[I], kerns, ops, theta)
                part = np.array([np.sum(G[np.ix_(I, I)] * d) for d in dK])
            else:
                dK = orc.dK_dtheta(X[np.r_[I, J]], kerns, ops, theta)[:, : len(I), len(I) :]
                part = 2.0 * np.array([np.sum(G[np.ix_(I, J)] * d) for d in dK])
            g = part if g is None else g + part
    return -0.5 * g


def loo_reverse(X, y, kernel, theta, diag=None):
    """(L_LOO, dL_LOO/dtheta) by the algebra of csrc/api_loo.hip, in float64 NumPy"""
    kerns, ops, Kinv, alpha = _kinv(X, y, kernel, theta, diag)
    p = np.diag(Kinv).copy()
    val = float(np.sum(0.5 * np.log(p) - 0.5 * alpha * alpha / p - 0.5 * LOG_2PI))
    e = alpha / p
    s = np.sqrt((1.0 + alpha * alpha / p) / p)
    B = Kinv * s[None, :]
    w = B @ (e / s)
    G = B @ B.T - np.outer(alpha, w) - np.outer(w, alpha)
    return val, contract(G, X, kerns, ops, theta)


def value_ratio(got, want, cond):
    """|got - want| / max(|want|, 1) over the project's bound for a log density, max(1e-10, 20 cond eps)"""
    return abs(got - want) / max(abs(want), 1.0) / max(1e-10, 20.0 * cond * EPS)


def grad_ratio(got, want, cond):
    """the project's gradient rule: per component, floored at 1e-3 of the largest, over max(1e-7, 500 cond eps)"""
    scale = np.maximum(np.abs(want), 1e-3 * max(np.max(np.abs(want)), 1e-300))
    return float(np.max(np.abs(got - want) / scale)) / max(1e-7, 500.0 * cond * EPS)


# ------------------------------------------------------------------------------------------------------------------ cases
# (kernel, n, d, per-point diagonal, gv): every n of {1, 128, 130, 257, 300} (one point; one full tile; two rows in the second
# tile; one row in the third; no multiple of anything), every kernel, d = 2, 3 and 33 (33 crosses the contraction's chunk of 32
# dimensions), each kernel with and without a diagonal
CASES = [
    ("RBF", 1, 2, False, 1e-2),
    ("Matern52", 1, 3, True, 1e-2),
    ("RBF", 128, 3, True, 1e-2),
    ("RBF", 300, 33, False, 1e-3),
    ("Matern52", 130, 2, False, 1e-3),
    ("Matern52", 257, 33, True, 1e-2),
    ("Exponential", 257, 3, False, 1e-3),
    ("Exponential", 300, 2, True, 1e-2),
    ("RBF*Matern32+RatQuad", 130, 3, True, 1e-3),
    ("RBF*Matern32+RatQuad", 300, 2, False, 1e-2),
    ("RBF*Matern32+RatQuad", 128, 33, False, 1e-2),
]
# 46 tile columns: the tail's GEMM takes its 128x128-tile path (1081 tiles of the lower trapezoid >= 1024)
BIG = ("RBF", 5800, 1, False, 1e-2)


def make_problem(kernel, n, d, with_diag, gv, seed):
    if n == 1:  # (synth_problem standardises y: one point has no spread)
        X, y = np.random.default_rng(seed).random((1, d)), np.array([0.7])
    else:
        X, y = orc.synth_problem(n, d, seed=seed)
    diag = np.random.default_rng(seed).uniform(1e-3, 1e-1, n) if with_diag else None
    theta = kfold_ref.make_theta(kernel, d, gv)
    if d > 8:  # (unit length scales in 33 dimensions leave nothing but the diagonal)
        nk = len(kfold_ref.split_kernel(kernel)[0])
        theta[: nk * d] *= np.sqrt(d / 3.0)
    return X, y, theta, diag


@functools.lru_cache(maxsize=None)
def case(i):
    """(X, y, kernel, theta, diag or None, cond(K)) of CASES[i]"""
    kernel, n, d, with_diag, gv = CASES[i]
    X, y, theta, diag = make_problem(kernel, n, d, with_diag, gv, 70 + i)
    return X, y, kernel, theta, diag, kfold_ref.full_cond(X, kernel, theta, diag)


@functools.lru_cache(maxsize=None)
def case_refs(i):
    """(value by refit, (value, gradient) forward mode, (value, gradient) reverse mode) of CASES[i], once per process"""
    X, y, kernel, theta, diag, _ = case(i)
    out = (loo_value_refit(X, y, kernel, theta, diag), loo_forward(X, y, kernel, theta, diag), loo_reverse(X, y, kernel, theta, diag))
    out[1][1].setflags(write=False)
    out[2][1].setflags(write=False)
    return out
