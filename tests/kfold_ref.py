"""Reference for MiGP.kfold / mi_gp_kfold: the hold-out predictive of every fold of a cross-validation at fixed hyper-parameters.

    kfold_refit   the DEFINITION, no code path or algebra shared with the device: for each fold the noisy covariance of the
                  complement (oracle.noisy_cov, marginal form), its Cholesky factor, the conditional of the fold's noisy
                  observations given the complement, and that normal's log density, mean and diagonal variance.  The data
                  set has ONE covariance matrix, and every fold conditions inside it: noisy_cov is evaluated once on all points
                  and a fold takes its three blocks from it.  (Evaluated per subset, the oracle's expansion-form r2 leaves
                  rounding noise of ~1e-15 on a few diagonal entries, at other entries for every subset; sqrt(r2 + 1e-12)
                  turns that into ~1e-10 on the diagonal of an Exponential covariance, above the parity tolerance.)
    kfold_kinv    the device's algebra in NumPy: blocks of K^-1 of the full data, Sigma_I = (K^-1_II)^-1, r_I = Sigma_I alpha_I

and the cases (problems, fold layouts, tolerances) that tests/test_kfold_host.py and tests/test_gpu_kfold.py share."""
import functools

import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as orc

EPS = 2.2e-16
LOG_2PI = np.log(2.0 * np.pi)


def split_kernel(kernel):
    """'RBF*Matern32+RatQuad' -> (['RBF', 'Matern32', 'RatQuad'], ['*', '+'])"""
    return kernel.replace("*", "+").split("+"), [c for c in kernel if c in "+*"]


def kfold_refit(X, y, kernel, theta, folds, diag=None):
    """(logp [nfolds], [mean per fold], [var per fold]): one factorisation of the complement per fold."""
    kerns, ops = split_kernel(kernel)
    n = len(y)
    K = orc.noisy_cov(X, kerns, ops, theta, "marginal", diag)
    logp, means, vars_ = np.zeros(len(folds)), [], []
    for f, I in enumerate(folds):
        I = np.asarray(I, dtype=np.int64)
        J = np.setdiff1d(np.arange(n), I)
        S = K[np.ix_(I, I)]
        mu = np.zeros(len(I))
        if len(J):
            L = sla.cholesky(K[np.ix_(J, J)], lower=True)
            A = sla.solve_triangular(L, K[np.ix_(J, I)], lower=True)
            mu = A.T @ sla.solve_triangular(L, y[J], lower=True)
            S = S - A.T @ A
        S = 0.5 * (S + S.T)
        Ls = sla.cholesky(S, lower=True)
        z = sla.solve_triangular(Ls, y[I] - mu, lower=True)
        logp[f] = -0.5 * z @ z - np.sum(np.log(np.diag(Ls))) - 0.5 * len(I) * LOG_2PI
        means.append(mu)
        vars_.append(np.diag(S).copy())
    return logp, means, vars_


def kfold_kinv(X, y, kernel, theta, folds, diag=None):
    """The same three, from K^-1 and alpha = K^-1 y of the full data (what the device computes)."""
    kerns, ops = split_kernel(kernel)
    L = sla.cholesky(orc.noisy_cov(X, kerns, ops, theta, "marginal", diag), lower=True)
    Linv = sla.solve_triangular(L, np.eye(len(y)), lower=True)
    Kinv = Linv.T @ Linv
    alpha = Kinv @ y
    logp, means, vars_ = np.zeros(len(folds)), [], []
    for f, I in enumerate(folds):
        I = np.asarray(I, dtype=np.int64)
        C = sla.cholesky(Kinv[np.ix_(I, I)], lower=True)
        M = sla.solve_triangular(C, np.eye(len(I)), lower=True)
        t = M @ alpha[I]
        logp[f] = -0.5 * t @ t + np.sum(np.log(np.diag(C))) - 0.5 * len(I) * LOG_2PI
        means.append(y[I] - M.T @ t)
        vars_.append(np.sum(M * M, axis=0))
    return logp, means, vars_


def full_cond(X, kernel, theta, diag=None):
    """2-norm condition number of the noisy covariance of the full data: the scale of the parity tolerances"""
    kerns, ops = split_kernel(kernel)
    return np.linalg.cond(orc.noisy_cov(X, kerns, ops, theta, "marginal", diag))


def tolerances(cond):
    """The project's parity tolerances (tests/test_gpu_append.py, tests/test_gpu_logpdf.py): logp and mean within
    max(1e-10, 20 cond eps) of max(|ref|, 1), var within max(1e-10, 200 cond eps) of the reference variance."""
    return max(1e-10, 20.0 * cond * EPS), max(1e-10, 200.0 * cond * EPS)


def error_ratios(got, want, cond):
    """(logp, mean, var) errors of one k-fold result against a reference, each divided by its tolerance"""
    vtol, ptol = tolerances(cond)
    (lp, mu, var), (rlp, rmu, rvar) = got, want
    mu, var, rmu, rvar = (np.concatenate(a) for a in (mu, var, rmu, rvar))
    e_lp = np.max(np.abs(lp - rlp) / np.maximum(np.abs(rlp), 1.0)) / vtol
    e_mu = np.max(np.abs(mu - rmu) / np.maximum(np.abs(rmu), 1.0)) / vtol
    e_var = np.max(np.abs(var - rvar) / rvar) / ptol
    return e_lp, e_mu, e_var


# ------------------------------------------------------------------------------------------------------------------ cases
# (kernel, n, d, per-point diagonal, gv): every kernel and every size with and without a diagonal; n = 130 is two tiles with two
# rows in the second, 257 three tiles with one row in the third, 300 no multiple of anything
CASES = [
    ("RBF", 130, 2, False, 1e-2),
    ("RBF", 300, 3, True, 1e-3),
    ("Matern52", 257, 3, False, 1e-3),
    ("Matern52", 130, 2, True, 1e-2),
    ("Exponential", 300, 2, False, 1e-4),
    ("Exponential", 257, 3, True, 1e-2),
    ("RBF*Matern32+RatQuad", 300, 3, False, 1e-2),
    ("RBF*Matern32+RatQuad", 130, 2, True, 1e-3),
    ("RBF*Matern32+RatQuad", 257, 2, False, 1e-4),
]
LAYOUTS = ["loo", "3x100", "7uneven", "edges", "overlap"]


def make_theta(kernel, d, gv, jitter=1e-6):
    kerns, _ = split_kernel(kernel)
    theta = orc.synth_theta(d, nkern=len(kerns), gv=gv, jitter=jitter)
    for c, name in enumerate(kerns):
        if name == "RatQuad":
            theta[len(kerns) * d + len(kerns) + c] = 2.5  # (a shape parameter that is not the neutral 1)
    return theta


def fold_layout(name, n, seed=0):
    """The fold layouts of the parity tests, for n >= 130 points."""
    rng = np.random.default_rng(1000 + seed)
    perm = rng.permutation(n)
    if name == "loo":  # the singleton path
        return [np.array([i]) for i in range(n)]
    if name == "3x100":  # a partition at n = 300; below that the windows wrap around and overlap
        return [perm[(100 * f + np.arange(100)) % n] for f in range(3)]
    if name == "7uneven":
        sizes = np.maximum(1, np.array([3, 17, 64, 128, 1, 50, 37]) * min(n, 300) // 300)
        cuts = np.cumsum(sizes)
        return [perm[a:b] for a, b in zip(np.r_[0, cuts[:-1]], cuts)]
    if name == "edges":
        return [
            perm[:128],                                      # exactly 128 points, unsorted
            np.array([5]),                                   # a singleton among larger folds: the general path at size 1
            np.array([128, 3, 127, 126, 120, 129, 64, 121]),  # both sides of a tile boundary, several points of one diagonal tile
            np.arange(n - 1, n - 41, -1),                    # descending, up to the last point
            np.sort(perm[:127]),                             # 127 points, sorted
        ]
    if name == "overlap":
        return [np.arange(0, 60), np.arange(30, 90), np.arange(50, 130)[::-1], perm[:33]]
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def case(i):
    """(X, y, kernel, theta, diag or None, cond(K)) of CASES[i]"""
    kernel, n, d, with_diag, gv = CASES[i]
    X, y = orc.synth_problem(n, d, seed=40 + i)
    diag = np.random.default_rng(i).uniform(1e-3, 1e-1, n) if with_diag else None
    theta = make_theta(kernel, d, gv)
    return X, y, kernel, theta, diag, full_cond(X, kernel, theta, diag)


@functools.lru_cache(maxsize=None)
def case_refit(i, layout):
    """kfold_refit of CASES[i] under a layout, computed once per process; the arrays are shared: do not write to them"""
    X, y, kernel, theta, diag, _ = case(i)
    out = kfold_refit(X, y, kernel, theta, fold_layout(layout, len(y), i), diag)
    out[0].setflags(write=False)
    for a in out[1] + out[2]:
        a.setflags(write=False)
    return out
