"""Reference for MiGP.logpdf / mi_gp_logpdf: the joint log predictive density of trial points given the training data and its
gradients w.r.t. the trial inputs and outputs, from the NumPy oracle of the CONCATENATED data set -- no code path shared with
the device, and no Schur-complement algebra of its own:

    value      the trailing k entries of the joint conditional-form factorisation: -1/2 |beta[n:]|^2 - sum log diag(L)[n:]
               - k/2 log 2 pi (= LML(n + k) - LML(n) without the cancellation of that difference)
    gradients  the last k rows of oracle.lml_grad_data's dLML/dX and dLML/dy of the joint system (LML(n) does not depend on
               the trial points)
"""
import numpy as np

from oracle import gp_oracle as orc


def split_kernel(kernel):
    """'RBF*Matern32+RatQuad' -> (['RBF', 'Matern32', 'RatQuad'], ['*', '+'])"""
    return kernel.replace("*", "+").split("+"), [c for c in kernel if c in "+*"]


def joint(X, y, Xnew, ynew, diag=None, diag_new=None):
    XJ = np.vstack([X, np.atleast_2d(Xnew)])
    yJ = np.r_[y, np.asarray(ynew, dtype=np.float64).reshape(-1)]
    dJ = None if diag is None else np.r_[diag, np.asarray(diag_new, dtype=np.float64).reshape(-1)]
    return XJ, yJ, dJ


def logpdf_ref(X, y, Xnew, ynew, kernel, theta, diag=None, diag_new=None, grad=True):
    """(logp, dX [k, d], dy [k], parts) with parts = (sum log diag L22, |beta2|^2); (-inf, None, None, None) if the joint
    covariance is not positive definite."""
    kerns, ops = split_kernel(kernel)
    XJ, yJ, dJ = joint(X, y, Xnew, ynew, diag, diag_new)
    n, k = len(y), len(yJ) - len(y)
    _, L, beta = orc.lml(XJ, yJ, kerns, ops, theta, form="conditional", return_parts=True, extra_diag=dJ)
    if L is None:
        return -np.inf, None, None, None
    logdet2, quad2 = np.sum(np.log(np.diag(L)[n:])), np.sum(beta[n:] ** 2)
    val = -0.5 * quad2 - logdet2 - 0.5 * k * np.log(2.0 * np.pi)
    if not grad:
        return val, None, None, (logdet2, quad2)
    _, gy, gX = orc.lml_grad_data(XJ, yJ, kerns, ops, theta, form="conditional", extra_diag=dJ)
    return val, gX[n:], gy[n:], (logdet2, quad2)


def joint_cond(X, Xnew, kernel, theta, diag=None, diag_new=None):
    """2-norm condition number of the joint covariance (the scale of the project's parity tolerances, tests/test_gpu_append.py)"""
    kerns, ops = split_kernel(kernel)
    XJ = np.vstack([X, np.atleast_2d(Xnew)])
    dJ = None if diag is None else np.r_[diag, np.asarray(diag_new, dtype=np.float64).reshape(-1)]
    return np.linalg.cond(orc.noisy_cov(XJ, kerns, ops, theta, form="conditional", extra_diag=dJ))


def schur_density(X, y, Xnew, ynew, kernel, theta, diag=None, diag_new=None):
    """The same density the textbook way (for the host test of this file): mean and covariance of y2 | y1 from the blocks of
    oracle.noisy_cov of the joint data, through explicit solves."""
    kerns, ops = split_kernel(kernel)
    XJ, yJ, dJ = joint(X, y, Xnew, ynew, diag, diag_new)
    n = len(y)
    K = orc.noisy_cov(XJ, kerns, ops, theta, form="conditional", extra_diag=dJ)
    K11, K21, K22 = K[:n, :n], K[n:, :n], K[n:, n:]
    mean = K21 @ np.linalg.solve(K11, yJ[:n])
    cov = K22 - K21 @ np.linalg.solve(K11, K21.T)
    return mean, 0.5 * (cov + cov.T)
