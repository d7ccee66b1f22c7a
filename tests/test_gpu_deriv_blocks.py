"""The two kernels of the gradient binding through their block-level entry points (mi_gp_deriv_assemble, mi_gp_deriv_contract)
against the NumPy reference (tests/deriv_ref.py), free of the conditioning of the joint covariance: a random symmetric W and a
random alpha stand in for K^-1 and K^-1 y."""
import ctypes

import numpy as np
import pytest
import torch

import deriv_ref as R

pytestmark = pytest.mark.gpu

KERNELS = ["RBF", "Matern52"]
# component boundaries inside tiles and a ragged last tile: N = 3, 148 (boundaries at 37, 74, 111), 258 (129) and 850 (50, 100, ..)
SHAPES = [(1, 2), (37, 3), (129, 1), (50, 16)]
KID = {"RBF": 0, "Matern52": 1}


@pytest.fixture(scope="module")
def lib():
    from andvaranaut_amd import _lib

    return _lib.load_deriv()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _pad(n):
    return (n + 63) // 64 * 64


def _blocks_close(got, ref, n1, q1, n2, q2, what):
    """every (c, c') block element-wise within 1e-13 of that block's largest magnitude"""
    worst = 0.0
    for c in range(q1):
        for cp in range(q2):
            g = got[c * n1 : (c + 1) * n1, cp * n2 : (cp + 1) * n2]
            r = ref[c * n1 : (c + 1) * n1, cp * n2 : (cp + 1) * n2]
            scale = np.abs(r).max()
            err = np.abs(g - r).max()
            if scale == 0.0:
                assert err == 0.0, (what, c, cp)
                continue
            worst = max(worst, err / scale)
            assert err <= 1e-13 * scale, (what, c, cp, err, scale)
    return worst


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_assemble_symmetric_and_rectangular(lib, kernel, n, d):
    X, _, _ = R.problem(n, d, 100 * n + d)  # one pair 1e-3 apart and one identical (n >= 4)
    X2 = np.random.default_rng(n + d).random((max(n // 2, 1) + 3, d))
    X2[0] = X[0]  # a coincident pair across the two sets
    theta = R.theta_for(d)
    th_t, X_t, X2_t = _dev(theta), _dev(X), _dev(X2)
    q = 1 + d
    N = n * q
    # symmetric: lower tiles, the diagonal, the identity in the padding
    extra = np.concatenate([np.zeros(n), np.full(n * d, 1e-2)])
    ex_t = _dev(extra)
    for noise_form in (0, 1):
        Np = _pad(N)
        ld = Np + 2
        K_t = torch.full((Np, ld), np.nan, dtype=torch.float64, device="cuda")
        r = lib.mi_gp_deriv_assemble(d, KID[kernel], th_t.data_ptr(), X_t.data_ptr(), n, q, X_t.data_ptr(), n, q, K_t.data_ptr(), ld,
                                     Np, Np, 1, noise_form, ex_t.data_ptr(), None)
        assert r == 0, lib.mi_gp_last_global_error()
        torch.cuda.synchronize()
        K = K_t.cpu().numpy()
        ref = R.train_cov(X, theta, kernel, extra)
        low = np.tril(np.ones((N, N), dtype=bool))
        got = np.where(low, K[:N, :N], ref)  # (the tiles above the diagonal are not written)
        worst = _blocks_close(got, ref, n, q, n, q, "sym")
        print(f"{kernel} ({n}, {d}) sym noise_form {noise_form}: worst block-relative error {worst:.2e}")
        # the padding of the lower tiles is exact: the identity
        for a in range(N, Np):
            row = K[a, : a + 1]
            assert row[a] == 1.0 and np.all(row[:a] == 0.0), a
        assert np.all(K[N // 64 * 64 : N, N:Np] == 0.0)  # (the last tile's padding columns beside the data rows)
    # rectangular: every pair of component counts, zeros in the padding
    n2 = X2.shape[0]
    for q1, q2 in ((q, q), (1, q), (q, 1)):
        N1, N2 = n * q1, n2 * q2
        rp, cp = _pad(N1), _pad(N2)
        ld = cp + 4
        K_t = torch.full((rp, ld), np.nan, dtype=torch.float64, device="cuda")
        r = lib.mi_gp_deriv_assemble(d, KID[kernel], th_t.data_ptr(), X_t.data_ptr(), n, q1, X2_t.data_ptr(), n2, q2, K_t.data_ptr(), ld,
                                     rp, cp, 0, 0, None, None)
        assert r == 0, lib.mi_gp_last_global_error()
        torch.cuda.synchronize()
        K = K_t.cpu().numpy()
        ref = R.cov(X, q1, X2, q2, theta, kernel)
        worst = _blocks_close(K[:N1, :N2], ref, n, q1, n2, q2, (q1, q2))
        print(f"{kernel} ({n}, {d}) rectangle ({q1}, {q2}): worst block-relative error {worst:.2e}")
        assert np.all(K[N1:, :cp] == 0.0) and np.all(K[:, N2:cp] == 0.0)
        assert np.all(np.isnan(K[:, cp:]))  # nothing is written beyond cols_pad


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_contract_random_weights(lib, kernel, n, d):
    X, _, _ = R.problem(n, d, 100 * n + d)
    theta = R.theta_for(d)
    q = 1 + d
    N = n * q
    rng = np.random.default_rng(7 * n + d)
    W = rng.standard_normal((N, N))
    W = W + W.T
    alpha = rng.standard_normal(N)
    ref, scale = R.contract(X, theta, kernel, np.outer(alpha, alpha) - W, absolute=True)
    ld = N + 3
    Wl = np.full((N, ld), np.nan)
    Wl[:, :N] = np.where(np.tril(np.ones((N, N), dtype=bool)), W, np.nan)  # the lower triangle alone is read
    T = (N + 63) // 64
    part_len = T * (T + 1) // 2 * (d + 4)
    th_t, X_t, W_t, a_t = _dev(theta), _dev(X), _dev(Wl), _dev(alpha)
    part_t = torch.zeros(part_len, dtype=torch.float64, device="cuda")
    outs = []
    for _ in range(2):
        g_t = torch.full((d + 4,), np.nan, dtype=torch.float64, device="cuda")
        r = lib.mi_gp_deriv_contract(d, KID[kernel], th_t.data_ptr(), X_t.data_ptr(), n, W_t.data_ptr(), ld, a_t.data_ptr(),
                                     part_t.data_ptr(), part_len, g_t.data_ptr(), None)
        assert r == 0, lib.mi_gp_last_global_error()
        torch.cuda.synchronize()
        outs.append(g_t.cpu().numpy())
    g = outs[0]
    assert outs[0].tobytes() == outs[1].tobytes()  # no atomics: a repeat returns the same bits
    assert g[d + 1] == 0.0
    for p in range(d + 4):
        print(f"{kernel} ({n}, {d}) p = {p}: device {g[p]:.15e} reference {ref[p]:.15e} |diff| {abs(g[p] - ref[p]):.2e} scale {scale[p]:.2e}")
    assert np.all(np.abs(g - ref) <= 1e-11 * scale), (g, ref, scale)  # (a wrong sign or factor is of the order of `scale`)


def test_block_calls_refuse_bad_arguments(lib):
    th = _dev(R.theta_for(2))
    X = _dev(np.zeros((3, 2)))
    K = torch.zeros((64, 64), dtype=torch.float64, device="cuda")
    args = [th.data_ptr(), X.data_ptr(), 3, 3, X.data_ptr(), 3, 3, K.data_ptr(), 64, 64, 64, 1, 0, None, None]
    assert lib.mi_gp_deriv_assemble(2, 2, *args) == -1 and b"kernel_id" in lib.mi_gp_last_global_error()
    assert lib.mi_gp_deriv_assemble(33, 0, *args) == -1 and b"d <= 32" in lib.mi_gp_last_global_error()
    bad = list(args)
    bad[3] = 2  # a component count that is neither 1 nor 1 + d
    assert lib.mi_gp_deriv_assemble(2, 0, *bad) == -1 and b"component" in lib.mi_gp_last_global_error()
    bad = list(args)
    bad[9] = bad[10] = 0  # padding that does not cover the rows
    assert lib.mi_gp_deriv_assemble(2, 0, *bad) == -1
    g = torch.zeros(6, dtype=torch.float64, device="cuda")
    assert lib.mi_gp_deriv_contract(2, 0, th.data_ptr(), X.data_ptr(), 3, K.data_ptr(), 64, th.data_ptr(), K.data_ptr(), 5, g.data_ptr(),
                                    None) == -1
    assert b"scratch" in lib.mi_gp_last_global_error()
