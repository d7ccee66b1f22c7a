"""References for several outputs under one shared kernel (option 51 of mi_gp_set_option, MiGP.set_outputs): Y is n x q, the
outputs independent given theta, their log marginal likelihoods summed.

    oracle_sum          the DEFINITION: oracle.gp_oracle's LML and gradient per column at the same theta, summed
    oracle_conditional  the oracle's conditional per column (the variance does not depend on y: one column's serves all)
    tail                the device's algebra restated in NumPy: V = K^-1 Y, the q quads, q K^-1 - V V^T contracted with dK and a
                        zero vector in the place of alpha

and the problems that tests/test_multi_output_host.py and tests/test_gpu_multi_output.py share.  The bounds are the project's own
(loo_ref.value_ratio / grad_ratio for L_MO and its gradient, kfold_ref.tolerances for the moments)."""
import functools

import numpy as np
import scipy.linalg as sla

import kfold_ref
import loo_ref
from oracle import gp_oracle as orc

LOG_2PI = kfold_ref.LOG_2PI


def oracle_sum(X, Y, kernel, theta, diag=None):
    """(L_MO, dL_MO/dtheta): the oracle's (LML, gradient) of every column of Y, added in column order"""
    kerns, ops = kfold_ref.split_kernel(kernel)
    val, grad = 0.0, 0.0
    for o in range(Y.shape[1]):
        v, g = orc.lml_grad(X, np.ascontiguousarray(Y[:, o]), kerns, ops, theta, extra_diag=diag)
        val, grad = val + v, grad + g
    return float(val), grad


def oracle_conditional(X, Y, Xnew, kernel, theta, pred_noise=True):
    """(mean [m, q], var [m]) of the oracle's conditional, column by column"""
    kerns, ops = kfold_ref.split_kernel(kernel)
    cols = [orc.predict(X, np.ascontiguousarray(Y[:, o]), Xnew, kerns, ops, theta, pred_noise=pred_noise) for o in range(Y.shape[1])]
    return np.column_stack([c[0] for c in cols]), cols[0][1]


def tail(X, Y, kernel, theta, diag=None):
    """(L_MO, dL_MO/dtheta, quads [q]) by the algebra of csrc/api_multi.hip, in float64 NumPy"""
    kerns, ops = kfold_ref.split_kernel(kernel)
    n, q = Y.shape
    L = sla.cholesky(orc.noisy_cov(X, kerns, ops, theta, "marginal", diag), lower=True)
    Kinv = sla.cho_solve((L, True), np.eye(n))
    Kinv = 0.5 * (Kinv + Kinv.T)
    V = Kinv @ Y
    quad = np.einsum("io,io->o", Y, V)
    val = -q * float(np.sum(np.log(np.diag(L)))) - 0.5 * q * n * LOG_2PI - 0.5 * float(np.sum(quad))
    # launch_grad_contract forms 1/2 sum_ij (alpha_i alpha_j - W_ij) dK_ij: with alpha = 0 and W = q K^-1 - V V^T
    G = q * Kinv - V @ V.T
    return val, loo_ref.contract(G, X, kerns, ops, theta), quad


def make_outputs(X, y, q, seed):
    """n x q outputs on the design X: column 0 is y, the others smooth functions of X plus noise, on scales from 0.3 to 3"""
    rng = np.random.default_rng(seed)
    n, d = X.shape
    cols = [y]
    for o in range(1, q):
        w = rng.normal(size=d)
        f = np.sin(X @ w + rng.uniform(0.0, 6.0)) + 0.3 * rng.normal(size=n)
        cols.append((0.3 + 2.7 * rng.random()) * f)
    return np.ascontiguousarray(np.column_stack(cols))


@functools.lru_cache(maxsize=None)
def problem(kernel, n, d, q, with_diag, gv, seed):
    """(X, Y, theta, diag or None, cond(K)) -- loo_ref.make_problem's design, theta and diagonal, q outputs on it"""
    X, y, theta, diag = loo_ref.make_problem(kernel, n, d, with_diag, gv, seed)
    Y = make_outputs(X, y, q, seed + 1)
    for a in (X, Y, theta) + ((diag,) if diag is not None else ()):
        a.setflags(write=False)
    return X, Y, theta, diag, kfold_ref.full_cond(X, kernel, theta, diag)
