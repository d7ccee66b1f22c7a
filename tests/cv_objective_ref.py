"""References for the k-fold cross-validation objective (option 49 of mi_gp_set_option, MiGP.cv_grad): over the contiguous folds
I_f = [f b, min((f + 1) b, n)), L_CV = sum_f log p(y_I_f | y_-I_f) and its gradient w.r.t. theta, three ways that share nothing
with the device:

    cv_value_refit   the DEFINITION of the value: kfold_ref.kfold_refit on the folds (one factorisation of the complement per
                     fold), summed
    cv_forward       forward mode: with P = K^-1, alpha = P y, Sigma_I = (P_II)^-1, e_I = Sigma_I alpha_I and one
                     Z_k = P dK/dtheta_k per hyper-parameter (the oracle's dK_dtheta),
                     dL/dtheta_k = sum_f [ e_I^T (Z_k alpha)_I - 1/2 tr((e e^T + Sigma_I) (Z_k P)_II) ]
    cv_reverse       the device's reverse-mode algebra restated in NumPy: R = M^T + e t^T / (1 + sqrt(1 + tau)) per fold,
                     B[:, I] = P[:, I] R, w = B q, G' = B B^T - (alpha w^T + w alpha^T) contracted with dK

and the cases that tests/test_cv_objective_host.py and tests/test_gpu_cv_objective.py share: loo_ref.CASES under every block
size of BLOCKS.  The bounds are loo_ref.value_ratio and loo_ref.grad_ratio."""
import functools

import numpy as np
import scipy.linalg as sla

import kfold_ref
import loo_ref
from oracle import gp_oracle as orc

LOG_2PI = kfold_ref.LOG_2PI
# 2: the smallest block; 37: folds across the 64- and the 128-column boundary; 43: 130 = 43 + 43 + 43 + 1; 100: 300 = 3 x 100;
# 128: the largest (257 = 128 + 128 + 1)
BLOCKS = (2, 37, 43, 100, 128)
# (case of loo_ref.CASES, block size): every pair but one point under a block of two or more, where the objective is the LML
PAIRS = [(i, b) for i in range(len(loo_ref.CASES)) for b in BLOCKS if loo_ref.CASES[i][1] > 1]


def folds_of(n, b):
    return [np.arange(a, min(a + b, n)) for a in range(0, n, b)]


def cv_value_refit(X, y, kernel, theta, b, diag=None):
    logp, _, _ = kfold_ref.kfold_refit(X, y, kernel, theta, folds_of(len(y), b), diag)
    return float(np.sum(logp))


def _fold_parts(Kinv, alpha, I):
    """(logp, C^-1, t) of one fold from its block of K^-1"""
    C = sla.cholesky(Kinv[np.ix_(I, I)], lower=True)
    M = sla.solve_triangular(C, np.eye(len(I)), lower=True)
    t = M @ alpha[I]
    return -0.5 * t @ t + np.sum(np.log(np.diag(C))) - 0.5 * len(I) * LOG_2PI, M, t


def cv_forward(X, y, kernel, theta, b, diag=None):
    """(L_CV, dL_CV/dtheta) in forward mode: one N^3 product per hyper-parameter"""
    kerns, ops, Kinv, alpha = loo_ref._kinv(X, y, kernel, theta, diag)
    folds = folds_of(len(y), b)
    val, W = 0.0, []
    for I in folds:
        lp, M, t = _fold_parts(Kinv, alpha, I)
        val += lp
        e = M.T @ t
        W.append((e, np.outer(e, e) + M.T @ M))
    dK = orc.dK_dtheta(X, kerns, ops, theta)
    g = np.zeros(len(dK))
    for k in range(len(dK)):
        Z = Kinv @ dK[k]
        Za, ZP = Z @ alpha, Z @ Kinv
        g[k] = sum(e @ Za[I] - 0.5 * np.sum(S * ZP[np.ix_(I, I)].T) for I, (e, S) in zip(folds, W))
    return float(val), g


def cv_reverse(X, y, kernel, theta, b, diag=None):
    """(L_CV, dL_CV/dtheta) by the algebra of csrc/api_loo.hip under option 49, in float64 NumPy"""
    kerns, ops, Kinv, alpha = loo_ref._kinv(X, y, kernel, theta, diag)
    n = len(y)
    val, B, q = 0.0, np.zeros((n, n)), np.zeros(n)
    for I in folds_of(n, b):
        lp, M, t = _fold_parts(Kinv, alpha, I)
        val += lp
        root = np.sqrt(1.0 + t @ t)
        R = M.T + np.outer(M.T @ t, t) / (1.0 + root)
        B[:, I] = Kinv[:, I] @ R
        q[I] = t / root
    w = B @ q
    G = B @ B.T - np.outer(alpha, w) - np.outer(w, alpha)
    return float(val), loo_ref.contract(G, X, kerns, ops, theta)


@functools.lru_cache(maxsize=None)
def case_refs(i, b):
    """(value by refit, (value, gradient) forward mode, (value, gradient) reverse mode) of loo_ref.CASES[i] under block size b, once
    per process"""
    X, y, kernel, theta, diag, _ = loo_ref.case(i)
    out = (cv_value_refit(X, y, kernel, theta, b, diag), cv_forward(X, y, kernel, theta, b, diag),
           cv_reverse(X, y, kernel, theta, b, diag))
    out[1][1].setflags(write=False)
    out[2][1].setflags(write=False)
    return out
