"""Appending points to a factorisation (mi_gp_reserve / mi_gp_append) without a GPU: the C-ABI's argument checks, and the
block-append algebra of the device code restated in NumPy against the oracle's factor of the concatenated data."""
import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as orc


def test_null_handle_is_refused_with_a_message():
    from andvaranaut_amd import _lib

    lib = _lib.load()
    assert lib.mi_gp_reserve(None, 100) == -1
    assert b"mi_gp_reserve" in lib.mi_gp_last_global_error()
    assert lib.mi_gp_append(None, None, None, None, 1, None, 256) == -1
    assert b"mi_gp_append" in lib.mi_gp_last_global_error()


def _append(L11, beta1, U11, K21, K22, y2):
    """The steps of mi_gp_append (include/mi_gp.h) on dense matrices."""
    L21 = sla.solve_triangular(L11, K21.T, lower=True).T  # K21 L11^-T
    L21_u = K21 @ U11  # the same through U = L^-T
    S = K22 - L21 @ L21.T
    L22 = np.linalg.cholesky(S)
    beta2 = sla.solve_triangular(L22, y2 - L21 @ beta1, lower=True)
    U22 = np.linalg.inv(L22).T
    U12 = -U11 @ (L21.T @ U22)
    return L21, L21_u, L22, beta2, U12, U22


def test_block_append_algebra_matches_the_oracle_factor():
    for kernel, n0, k in (("RBF", 50, 1), ("Matern52", 130, 7), ("RBF+Matern32", 100, 28)):
        kerns = kernel.replace("*", "+").split("+")
        ops = [c for c in kernel if c in "+*"]
        X, y = orc.synth_problem(n0 + k, 2, seed=n0 + k)
        theta = orc.synth_theta(2, nkern=len(kerns), gv=1e-3)
        K = orc.noisy_cov(X, kerns, ops, theta, form="conditional")
        _, L, beta = orc.lml(X, y, kerns, ops, theta, form="conditional", return_parts=True)
        _, L11, beta1 = orc.lml(X[:n0], y[:n0], kerns, ops, theta, form="conditional", return_parts=True)
        U11 = np.linalg.inv(L11).T
        L21, L21_u, L22, beta2, U12, U22 = _append(L11, beta1, U11, K[n0:, :n0], K[n0:, n0:], y[n0:])
        np.testing.assert_allclose(L21, L[n0:, :n0], rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(L21_u, L[n0:, :n0], rtol=1e-8, atol=1e-9)
        np.testing.assert_allclose(L22, L[n0:, n0:], rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(beta2, beta[n0:], rtol=1e-8, atol=1e-9)
        logdet = np.sum(np.log(np.diag(L11))) + np.sum(np.log(np.diag(L22)))
        quad = beta1 @ beta1 + beta2 @ beta2
        assert abs(logdet - np.sum(np.log(np.diag(L)))) <= 1e-10 * max(1.0, abs(logdet))
        assert abs(quad - beta @ beta) <= 1e-9 * max(1.0, quad)
        U = np.linalg.inv(L).T
        np.testing.assert_allclose(np.block([[U11, U12], [np.zeros((k, n0)), U22]]), U, rtol=1e-7, atol=1e-7 * np.abs(U).max())
        # the rebuilt diagonal-block inverse: inv([A 0; B C]) = [A^-1 0; -C^-1 B A^-1  C^-1]
        A, B, C = L11[-5:, -5:], L21[:, -5:], L22
        Ai, Ci = np.linalg.inv(A), np.linalg.inv(C)
        T = np.block([[A, np.zeros((5, k))], [B, C]])
        np.testing.assert_allclose(np.block([[Ai, np.zeros((5, k))], [-Ci @ B @ Ai, Ci]]), np.linalg.inv(T), rtol=1e-8, atol=1e-9)
