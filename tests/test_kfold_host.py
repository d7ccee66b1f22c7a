"""Host checks for exact k-fold cross-validation (mi_gp_kfold): the refit reference of tests/kfold_ref.py against SciPy's normal
density and the oracle's conditional, the K^-1 algebra the device uses against that reference on the GPU test's own shapes,
and the entries' place in the C-ABI."""
import fnmatch
import os
import re

import numpy as np
import pytest
import scipy.stats as st

import kfold_ref as ref
from conftest import ROOT
from oracle import gp_oracle as orc


@pytest.mark.parametrize("kernel,with_diag", [("RBF", False), ("Matern52", False), ("RBF*Matern32+RatQuad", False), ("RBF", True)])
def test_refit_reference_is_the_conditional_normal_of_the_held_out_observations(kernel, with_diag):
    n, d = 60, 3
    X, y = orc.synth_problem(n, d, seed=3)
    theta = ref.make_theta(kernel, d, 1e-2)
    kerns, ops = ref.split_kernel(kernel)
    diag = np.random.default_rng(1).uniform(1e-3, 1e-1, n) if with_diag else None
    folds = [np.array([7]), np.array([3, 50, 21, 8]), np.random.default_rng(2).permutation(n)[:17]]
    logp, means, vars_ = ref.kfold_refit(X, y, kernel, theta, folds, diag)
    K = orc.noisy_cov(X, kerns, ops, theta, "marginal", diag)
    for f, I in enumerate(folds):
        J = np.setdiff1d(np.arange(n), I)
        # the textbook conditional through explicit solves, and SciPy's density of it: both sides solve against K_JJ in fp64,
        # cond(K) <= ~kv n / gv = 1e4 here, so 1e-9 leaves two decades (the bound of tests/test_logpdf_host.py)
        mean = K[np.ix_(I, J)] @ np.linalg.solve(K[np.ix_(J, J)], y[J])
        cov = K[np.ix_(I, I)] - K[np.ix_(I, J)] @ np.linalg.solve(K[np.ix_(J, J)], K[np.ix_(J, I)])
        want = st.multivariate_normal.logpdf(y[I], mean=mean, cov=0.5 * (cov + cov.T))
        assert abs(logp[f] - want) <= 1e-9 * max(abs(want), 1.0), (f, logp[f], want)
        if diag is None:
            # the oracle's conditional (diag=True, pred_noise=True) at the fold's inputs given the complement: the same mean;
            # its variance is kdiag - |A|^2 + gv, the marginal form's adds the jitter
            mu, var = orc.predict(X[J], y[J], X[I], kerns, ops, theta, pred_noise=True)
            assert np.max(np.abs(means[f] - mu)) <= 1e-9 * max(np.max(np.abs(mu)), 1.0)
            assert np.max(np.abs(vars_[f] - (var + theta[-1])) / var) <= 1e-9


@pytest.mark.parametrize("layout", ref.LAYOUTS)
@pytest.mark.parametrize("i", range(len(ref.CASES)))
def test_kinv_algebra_agrees_with_the_refit_reference_on_the_gpu_shapes(i, layout):
    """The identity the device relies on, in NumPy at the GPU test's tolerance: the reference alone stays well inside it."""
    X, y, kernel, theta, diag, cond = ref.case(i)
    folds = ref.fold_layout(layout, len(y), i)
    got = ref.kfold_kinv(X, y, kernel, theta, folds, diag)
    ratios = ref.error_ratios(got, ref.case_refit(i, layout), cond)
    print(ref.CASES[i], layout, "cond %.3g" % cond, "error / tolerance: logp %.3g mean %.3g var %.3g" % ratios)
    assert max(ratios) <= 1.0, ratios


def test_fold_layouts_are_what_the_gpu_test_needs():
    for n in (130, 257, 300):
        for name in ref.LAYOUTS:
            folds = ref.fold_layout(name, n, 1)
            for f in folds:
                assert 1 <= len(f) <= 128 and len(set(f.tolist())) == len(f) and f.min() >= 0 and f.max() < n
        edges = ref.fold_layout("edges", n, 1)
        assert len(edges[0]) == 128 and len(edges[1]) == 1 and {127, 128} <= set(edges[2].tolist())
        assert not np.array_equal(edges[0], np.sort(edges[0]))
    assert sorted(np.concatenate(ref.fold_layout("3x100", 300)).tolist()) == list(range(300))


def test_kfold_entries_are_declared_listed_bound_and_exported():
    from andvaranaut_amd import _lib

    header = open(os.path.join(ROOT, "include", "mi_gp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    mapped = re.findall(r"global:\s*([^;]+);", open(os.path.join(ROOT, "andvaranaut_amd", "csrc", "libmi_gp.map")).read())
    patterns = [p.strip() for g in mapped for p in g.split(",")]
    lib = _lib.load()
    for name in ("mi_gp_kfold", "mi_gp_kfold_work"):
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/mi_gp.h"
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), f"{name} is not exported by csrc/libmi_gp.map"
        assert name in _lib.EXPORTS
        assert hasattr(lib, name), f"libmi_gp.so does not export {name}"
    assert len(_lib.EXPORTS) == 57


def test_kfold_work_formula_and_its_refusals():
    from andvaranaut_amd import _lib

    lib = _lib.load()
    # per fold two 128 x 128 blocks and the gathered alpha_I / y_I; on top the staged index lists and bad-pivot words
    per_fold = 2 * 128 * 128 + 256
    assert lib.mi_gp_kfold_work(1, 1) == per_fold + 4
    assert lib.mi_gp_kfold_work(3, 300) == 3 * per_fold + 602
    assert lib.mi_gp_kfold_work(256, 16384) == 256 * per_fold + 2 * 16384 + 2
    assert lib.mi_gp_kfold_work(1 << 20, 1 << 30) == (1 << 20) * per_fold + (1 << 31) + 2  # (no 32-bit arithmetic)
    for p, t in ((0, 10), (-1, 10), (1, 0), (4, -5)):
        assert lib.mi_gp_kfold_work(p, t) == -1


def test_null_handle_is_an_argument_error_with_text():
    from andvaranaut_amd import _lib

    lib = _lib.load()
    # before any HIP call (no GPU here)
    assert lib.mi_gp_kfold(None, 1, None, None, None, 0, None, None, None, None) == -1
    assert b"mi_gp_kfold" in lib.mi_gp_last_global_error()
