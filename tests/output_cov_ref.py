"""References for the between-output covariance integrated out (option 52 of mi_gp_set_option, MiGP.set_output_cov): Y is n x q,
vec(Y) ~ N(0, Sigma (x) K_y) with Sigma q x q under the Jeffreys prior |Sigma|^-(q+1)/2 (the separable multi-output emulator of Conti
& O'Hagan 2010), Sigma integrated out:

    L_S = -q/2 log|K_y| - n/2 log|S| + log Gamma_q(n/2) - n q/2 log pi,     S = Y^T K_y^-1 Y

    forward       the DEFINITION in forward mode: solves with K_y (no K^-1 formed), slogdet of K_y and of S, and
                  g_k = -q/2 tr(K_y^-1 dK_k) + n/2 tr(S^-1 B^T dK_k B) with B = K_y^-1 Y, one dK_k at a time
    tail          the device's algebra restated in NumPy: K^-1 from the Cholesky factor, V = K^-1 Y, S = Y^T V = C_S C_S^T,
                  sum log diag, and q K^-1 - n V S^-1 V^T contracted with dK and a zero vector in the place of alpha
    predict_var   the predictive variance per output: the oracle's conditional variance times s_o = y_o^T K_c^-1 y_o / (n - q - 1)
                  (K_c the conditional form), the variance of the predictive multivariate t with n - q + 1 degrees of freedom
    quadrature_q1 q = 1 by quadrature: log of the integral of N(y; 0, s K_y) / s over s

The two gradient routes share the oracle's dK_dtheta and nothing else.  The problems are multi_output_ref.problem's; the bounds are
the project's own (loo_ref.value_ratio / grad_ratio, kfold_ref.tolerances) at cond = max(cond(K_y), cond(S)): both are inverted."""
import numpy as np
import scipy.linalg as sla
import scipy.special as sp

import kfold_ref
import loo_ref
from oracle import gp_oracle as orc

# (index into loo_ref.CASES, q), seed 70 + i as in option 51's tests; the last is n = 128, q = 126: the smallest legal n - q
CASES = [(2, 2), (3, 17), (4, 3), (8, 5), (9, 128), (10, 126)]


def log_multigamma(a, q):
    """log Gamma_q(a) = q (q - 1) / 4 log pi + sum_{j = 1 .. q} lgamma(a + (1 - j) / 2)"""
    return 0.25 * q * (q - 1) * np.log(np.pi) + float(np.sum(sp.gammaln(a + 0.5 * (1.0 - np.arange(1, q + 1)))))


def forward(X, Y, kernel, theta, diag=None):
    """(L_S, dL_S/dtheta, cond(S)) from the definition, in forward mode"""
    kerns, ops = kfold_ref.split_kernel(kernel)
    n, q = Y.shape
    K = orc.noisy_cov(X, kerns, ops, theta, "marginal", diag)
    B = np.linalg.solve(K, Y)
    S = Y.T @ B
    S = 0.5 * (S + S.T)
    val = -0.5 * q * np.linalg.slogdet(K)[1] - 0.5 * n * np.linalg.slogdet(S)[1] + sp.multigammaln(0.5 * n, q) - 0.5 * n * q * np.log(np.pi)
    dK = orc.dK_dtheta(X, kerns, ops, theta)
    fac = sla.cho_factor(K, lower=True)
    g = np.zeros(len(dK))
    for k in range(len(dK)):
        if not dK[k].any():  # (a shape parameter no component reads)
            continue
        if k > 0 and np.array_equal(dK[k], dK[k - 1]):  # (d/d jitter = d/d gv: the same matrix, the same n^3 solve)
            g[k] = g[k - 1]
            continue
        g[k] = -0.5 * q * np.trace(sla.cho_solve(fac, dK[k])) + 0.5 * n * np.trace(np.linalg.solve(S, B.T @ dK[k] @ B))
    return float(val), g, float(np.linalg.cond(S))


def tail(X, Y, kernel, theta, diag=None):
    """(L_S, dL_S/dtheta) by the algebra of csrc/api_multi.hip under option 52 = 1, in float64 NumPy"""
    kerns, ops = kfold_ref.split_kernel(kernel)
    n, q = Y.shape
    L = sla.cholesky(orc.noisy_cov(X, kerns, ops, theta, "marginal", diag), lower=True)
    Kinv = sla.cho_solve((L, True), np.eye(n))
    Kinv = 0.5 * (Kinv + Kinv.T)
    V = Kinv @ Y
    C = sla.cholesky(np.tril(Y.T @ V) + np.tril(Y.T @ V, -1).T, lower=True)  # (the leaf reads the lower triangle)
    val = -q * float(np.sum(np.log(np.diag(L)))) - n * float(np.sum(np.log(np.diag(C)))) + log_multigamma(0.5 * n, q) \
        - 0.5 * n * q * np.log(np.pi)
    Q = np.sqrt(n) * sla.solve_triangular(C, V.T, lower=True).T  # sqrt(n) V C^-T
    # launch_grad_contract forms 1/2 sum_ij (alpha_i alpha_j - W_ij) dK_ij: with alpha = 0 and W = q K^-1 - Q Q^T
    return val, loo_ref.contract(q * Kinv - Q @ Q.T, X, kerns, ops, theta)


def scales(X, Y, kernel, theta):
    """s_o = y_o^T K_c^-1 y_o / (n - q - 1) for every output, K_c the noisy covariance in the conditional form"""
    kerns, ops = kfold_ref.split_kernel(kernel)
    n, q = Y.shape
    Kc = orc.noisy_cov(X, kerns, ops, theta, "conditional")
    return np.einsum("io,io->o", Y, np.linalg.solve(Kc, Y)) / (n - q - 1)


def predict_var(X, Y, Xnew, kernel, theta, pred_noise=True):
    """[m, q]: the oracle's conditional variance (it does not depend on y) times s_o"""
    kerns, ops = kfold_ref.split_kernel(kernel)
    _, var = orc.predict(X, np.ascontiguousarray(Y[:, 0]), Xnew, kerns, ops, theta, pred_noise=pred_noise)
    return var[:, None] * scales(X, Y, kernel, theta)[None, :]


def quadrature_q1(X, y, kernel, theta, diag=None):
    """log int_0^inf N(y; 0, s K_y) / s ds by quadrature in t = log s (the Jeffreys prior is flat in t), on a grid around the
    integrand's mode t* = log(y^T K^-1 y / n); the integrand is smooth and decays like a Gaussian in t near the mode and faster
    than exp(-|t|) away from it, so the trapezoid rule converges geometrically"""
    kerns, ops = kfold_ref.split_kernel(kernel)
    n = len(y)
    K = orc.noisy_cov(X, kerns, ops, theta, "marginal", diag)
    quad = float(y @ np.linalg.solve(K, y))
    logdet = np.linalg.slogdet(K)[1]
    t = np.log(quad / n) + np.linspace(-12.0, 12.0, 4801)
    logf = -0.5 * n * (np.log(2.0 * np.pi) + t) - 0.5 * logdet - 0.5 * quad * np.exp(-t)
    top = logf.max()
    f = np.exp(logf - top)
    return float(top + np.log((t[1] - t[0]) * (f.sum() - 0.5 * (f[0] + f[-1]))))
