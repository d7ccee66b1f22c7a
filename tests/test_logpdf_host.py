"""Host checks for the joint log predictive density (mi_gp_logpdf): the reference of tests/logpdf_ref.py against the textbook
Schur-complement density and its central differences, and the entry's place in the C-ABI."""
import fnmatch
import os
import re

import numpy as np
import pytest
import scipy.stats as st

import logpdf_ref as ref
from conftest import ROOT
from oracle import gp_oracle as orc

D = 3
CASES = [("RBF", 1e-2, False), ("Matern52", 1e-2, True), ("RBF*Matern32+RatQuad", 1e-2, False)]


def _problem(kernel, gv, with_diag, n=60, k=5, seed=2):
    X, y = orc.synth_problem(n + k, D, seed=seed)
    theta = orc.synth_theta(D, nkern=len(ref.split_kernel(kernel)[0]), gv=gv, jitter=1e-6)
    diag = np.random.default_rng(seed).uniform(1e-3, 1e-1, n + k) if with_diag else None
    return X[:n], y[:n], X[n:], y[n:], theta, (diag[:n] if with_diag else None), (diag[n:] if with_diag else None)


def _density(X, y, Xn, yn, kernel, theta, d0, d1):
    mean, cov = ref.schur_density(X, y, Xn, yn, kernel, theta, d0, d1)
    return st.multivariate_normal.logpdf(yn, mean=mean, cov=cov)


@pytest.mark.parametrize("kernel,gv,with_diag", CASES)
def test_reference_value_is_the_schur_complement_density(kernel, gv, with_diag):
    X, y, Xn, yn, theta, d0, d1 = _problem(kernel, gv, with_diag)
    val, _, _, _ = ref.logpdf_ref(X, y, Xn, yn, kernel, theta, d0, d1, grad=False)
    want = _density(X, y, Xn, yn, kernel, theta, d0, d1)
    # both sides solve against K11 in fp64: their difference is bounded by cond(K_J) eps times the size of the quadratic form
    # (a few units here); cond <= ~kv n / gv = 1e4, so 1e-9 leaves two decades
    assert abs(val - want) <= 1e-9 * max(abs(want), 1.0), (val, want)


@pytest.mark.parametrize("kernel,gv,with_diag", CASES)
def test_reference_gradients_are_central_differences_of_that_density(kernel, gv, with_diag):
    X, y, Xn, yn, theta, d0, d1 = _problem(kernel, gv, with_diag)
    _, gX, gy, _ = ref.logpdf_ref(X, y, Xn, yn, kernel, theta, d0, d1)
    h = 1e-5  # truncation h^2 f''' ~ 1e-10 f''', rounding eps |f| / h ~ 1e-9: 1e-6 of the largest entry bounds both
    fdX, fdy = np.zeros_like(Xn), np.zeros_like(yn)
    for i in range(Xn.shape[0]):
        for m in range(D):
            P, M = Xn.copy(), Xn.copy()
            P[i, m] += h
            M[i, m] -= h
            fdX[i, m] = (_density(X, y, P, yn, kernel, theta, d0, d1) - _density(X, y, M, yn, kernel, theta, d0, d1)) / (2 * h)
        p, m_ = yn.copy(), yn.copy()
        p[i] += h
        m_[i] -= h
        fdy[i] = (_density(X, y, Xn, p, kernel, theta, d0, d1) - _density(X, y, Xn, m_, kernel, theta, d0, d1)) / (2 * h)
    assert np.max(np.abs(gX - fdX)) <= 1e-6 * np.max(np.abs(fdX)), (gX, fdX)
    assert np.max(np.abs(gy - fdy)) <= 1e-6 * np.max(np.abs(fdy)), (gy, fdy)


def test_reference_of_coincident_trial_points_is_finite():
    X, y, _, _, theta, d0, _ = _problem("Exponential", 1e-2, True)
    Xn = np.tile(X[[7]] + 0.01, (3, 1))
    val, gX, gy, _ = ref.logpdf_ref(X, y, Xn, np.array([0.1, 0.2, 0.3]), "Exponential", theta, d0, np.full(3, 1e-2))
    assert np.isfinite(val) and np.isfinite(gX).all() and np.isfinite(gy).all()


def test_logpdf_entries_are_declared_listed_bound_and_exported():
    from andvaranaut_amd import _lib

    header = open(os.path.join(ROOT, "include", "mi_gp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    mapped = re.findall(r"global:\s*([^;]+);", open(os.path.join(ROOT, "andvaranaut_amd", "csrc", "libmi_gp.map")).read())
    patterns = [p.strip() for g in mapped for p in g.split(",")]
    lib = _lib.load()
    for name in ("mi_gp_logpdf", "mi_gp_logpdf_work"):
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/mi_gp.h"
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), f"{name} is not exported by csrc/libmi_gp.map"
        assert name in _lib.EXPORTS
        assert hasattr(lib, name), f"libmi_gp.so does not export {name}"
    # the work size is append's block plus S^-1 and gamma; a bad leading dimension is refused
    assert lib.mi_gp_logpdf_work(1040) == 4 * 128 * 1040 + 65600 + 128 * 128 + 128
    assert lib.mi_gp_logpdf_work(1041) == -1 and lib.mi_gp_logpdf_work(64) == -1
    # a null handle is an argument error before any HIP call (no GPU here)
    assert lib.mi_gp_logpdf(None, None, None, None, 1, None, 128, None, None, None) == -1
    assert b"mi_gp_logpdf" in lib.mi_gp_last_global_error()
