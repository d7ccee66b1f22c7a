"""The sparse inducing-point bound on the device (include/mi_gp_sparse.h) against the long-double
reference of tests/sgpr_ref.py, at the shapes at which the tiling can go wrong: one tile of m with n no multiple of 64 and one
chunk; two ragged tiles of m and three chunks, the last one short; one past a tile in both sets with d past a block of 16.
Five kernels (one, two additive, two multiplicative components, a rational quadratic), Z once a random subset of X (coincident
pairs, r2 = 0) and once select_inducing's.

Tolerances are the project's rule with cond = cond(Kuu) (sgpr_ref.tolerances): F and the mean within max(1e-10, 20 cond eps) of
max(|ref|, 1), every gradient entry and the variance within max(1e-10, 200 cond eps), relative to max(|ref|, 1) and to the
reference variance.  tests/test_sgpr_host.py holds the CPU half: fp64 alone uses at most a quarter of each on every case here
(sgpr_ref.case_theta says which cases took other length scales for that, and why).  Every case prints its ratios."""
import ctypes

import numpy as np
import pytest

import sgpr_ref as R

pytestmark = pytest.mark.gpu


def _make(case, chunk="case"):
    from andvaranaut_amd.sparse import MiSparseGP

    X, y, Z, theta, Xnew, case_chunk = R.device_case(case)
    return MiSparseGP(X, y, Z, case[0], device=0, chunk=case_chunk if chunk == "case" else chunk), theta, Xnew


@pytest.mark.parametrize("case", R.DEVICE_CASES, ids=R.case_id)
def test_bound_gradient_and_predictive_against_long_double(case):
    import torch

    from andvaranaut_amd import MiGP

    ref = R.reference(case)
    sp, theta, Xnew = _make(case)
    try:
        F, g = sp.lml_grad(theta)
        assert sp.info == 0
        mean, var = sp.predict(theta, Xnew, pred_noise=False)
        ratios = R.error_ratios({"F": F, "grad": g, "mean": mean, "var": var}, ref, ref["cond_Kuu"])
        print(R.case_id(case), "cond(Kuu) = %.2e" % ref["cond_Kuu"], {k: "%.4f" % v for k, v in ratios.items()})
        assert max(ratios.values()) <= 1.0, ratios
        assert g[-1] == 0.0  # jitter is a constant of the fit
        _, var_n = sp.predict(theta, Xnew, pred_noise=True)
        assert np.array_equal(var_n, var + (theta[-2] + theta[-1]))

        # the same call in the same state returns the same bits; the value alone is the gradient call's value
        F2, g2 = sp.lml_grad(theta)
        assert F2 == F and np.array_equal(g2, g)
        assert sp.bound(theta) == F
        # every element a launch reads is written earlier in the same call: a work block full of NaN changes nothing
        sp.work_t.fill_(float("nan"))
        torch.cuda.synchronize()
        F3, g3 = sp.lml_grad(theta)
        assert F3 == F and np.array_equal(g3, g)
        sp.work_t.fill_(float("nan"))
        torch.cuda.synchronize()
        mean3, var3 = sp.predict(theta, Xnew, pred_noise=False)
        assert np.array_equal(mean3, mean) and np.array_equal(var3, var)
    finally:
        sp.close()
    # a lower bound of the exact log marginal likelihood at the same theta on the same data
    X, y = R.device_case(case)[:2]
    gp = MiGP(X, y, case[0], device=0, need_grad=False)
    try:
        lml = gp.lml(theta)
    finally:
        gp.close()
    assert np.isfinite(lml) and F <= lml, (F, lml)


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_three_chunks_agree_with_one_within_the_tolerances(kernel):
    case = (kernel, 700, 200, 5, 256, "subset")
    ref = R.reference(case)
    vtol, ptol = R.tolerances(ref["cond_Kuu"])
    out = []
    for chunk in (256, 768):
        sp, theta, Xnew = _make(case, chunk=chunk)
        try:
            out.append(sp.lml_grad(theta) + sp.predict(theta, Xnew, pred_noise=False))
        finally:
            sp.close()
    (Fa, ga, ma, va), (Fb, gb, mb, vb) = out
    assert abs(Fa - Fb) <= vtol * max(abs(Fb), 1.0)
    assert np.all(np.abs(ga - gb) <= ptol * np.maximum(np.abs(gb), 1.0))
    assert np.all(np.abs(ma - mb) <= vtol * np.maximum(np.abs(mb), 1.0))
    assert np.all(np.abs(va - vb) <= ptol * vb)


def test_a_repeated_inducing_point_without_jitter_is_a_bad_pivot_and_the_object_stays_usable():
    """Rows 5 and 9 of Z are one point and jitter = 0: Kuu is singular.  The two rows of Kuu are equal bit for bit, so the Schur
    complement of pivot 10 is d - d (d fl(1 / d)) with d pivot 6 -- exactly 0 whenever d fl(1 / d) rounds to 1 -- and the leaf
    reports a pivot that is not positive."""
    from andvaranaut_amd.sparse import MiSparseGP

    kernel, n, m, d = "Matern52", 300, 40, 3
    X, y = R.problem(n, d, seed=21)
    Z = X[:m].copy()
    Z[9] = Z[5]
    good = R.case_theta(kernel, d)
    bad = good.copy()
    bad[-1] = 0.0
    sp = MiSparseGP(X, y, Z, kernel, device=0)
    fresh = MiSparseGP(X, y, Z, kernel, device=0)
    try:
        F, g = sp.lml_grad(bad)
        assert sp.info == 10, sp.info
        assert F == -np.inf and not g.any()
        assert sp.bound(bad) == -np.inf and sp.info == 10
        assert sp.factor(bad) == 10
        sp._factored_theta = bad.copy()  # (the wrapper would factor again and raise on the pivot: let the library itself refuse)
        with pytest.raises(RuntimeError, match="mi_gp_sparse_factor first"):
            sp.predict(bad, X[:4])
        # with the jitter back the same object returns what a fresh one does
        F1, g1 = sp.lml_grad(good)
        F2, g2 = fresh.lml_grad(good)
        assert sp.info == 0 and np.isfinite(F1) and F1 == F2 and np.array_equal(g1, g2)
        m1 = sp.predict(good, X[:50])
        m2 = fresh.predict(good, X[:50])
        assert np.array_equal(m1[0], m2[0]) and np.array_equal(m1[1], m2[1])
    finally:
        sp.close()
        fresh.close()


def test_predict_before_factor_is_refused():
    import torch

    sp, theta, Xnew = _make(("RBF", 300, 40, 3, None, "subset"))
    try:
        xn = torch.from_numpy(Xnew).to(sp.dev)
        out = torch.empty(2 * Xnew.shape[0], dtype=torch.float64, device=sp.dev)
        torch.cuda.synchronize()
        args = (sp.h, xn.data_ptr(), Xnew.shape[0], out.data_ptr(), out.data_ptr() + 8 * Xnew.shape[0], 0)
        assert sp.lib.mi_gp_sparse_predict(*args) == -1
        assert "mi_gp_sparse_factor first" in sp.last_error()
        sp.lml_grad(theta)  # an evaluation of the bound is no factor call
        assert sp.lib.mi_gp_sparse_predict(*args) == -1
        assert sp.factor(theta) == 0
        assert sp.lib.mi_gp_sparse_predict(*args) == 0
        tp = theta.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        val = ctypes.c_double()
        assert sp.lib.mi_gp_sparse_bound_grad(sp.h, tp, ctypes.byref(val), None) == 0  # the state is the bound's again
        assert sp.lib.mi_gp_sparse_predict(*args) == -1
    finally:
        sp.close()
