"""The sparse bound's gradient by the inducing locations on the device (include/mi_gp_sparse.h, zgrad_slabs >= 1) against the
long-double dF/dZ of tests/sgpr_zgrad_ref.py, and GPMCMC.fit(optimize_inducing=True) end to end.

The tolerance is the project's gradient rule with cond = cond(Kuu) (sgpr_ref.tolerances): every entry within
max(1e-10, 200 cond eps) of max(|ref|, 1).  tests/test_sgpr_zgrad_host.py holds the CPU half: fp64 alone on the device's steps uses
at most 0.27 of it on the 30 cases of sgpr_ref.DEVICE_CASES.  Every case prints its ratio."""
import numpy as np
import pytest
import scipy.stats as st

import sgpr_ref as R
import sgpr_zgrad_ref as ZR

pytestmark = pytest.mark.gpu

# Four components with both operators, where grad_x_kernel's code-generation problem showed.  Twice sgpr_ref.case_theta's length
# scales: at the plain ones fp64 alone on the device's steps uses 0.42 of the tolerance (cond(Kuu) = 1.0e4 makes it 4.5e-10 on
# entries up to 3.7e3), at twice 0.05 (cond(Kuu) = 1.8e5) -- the reasoning of sgpr_ref.LS_FACTOR
FOUR = "RBF+Matern52*Matern32+RatQuad"


def _sparse(X, y, Z, kernel, **kw):
    from andvaranaut_amd.sparse import MiSparseGP

    return MiSparseGP(X, y, Z, kernel, device=0, **kw)


@pytest.mark.parametrize("case", R.DEVICE_CASES, ids=R.case_id)
def test_gradient_by_the_inducing_points_against_long_double(case):
    X, y, Z, theta, _, chunk = R.device_case(case)
    ref = ZR.case_reference(case)
    sp = _sparse(X, y, Z, case[0], chunk=chunk, z_grad=True)
    plain = _sparse(X, y, Z, case[0], chunk=chunk)
    try:
        F, g, gz = sp.lml_grad_z(theta)
        assert sp.info == 0 and gz.shape == Z.shape
        ratio = ZR.ratio(gz, ref)
        print(R.case_id(case), "cond(Kuu) = %.2e" % ref["cond_Kuu"], "dF/dZ ratio %.4f" % ratio)
        assert ratio <= 1.0, ratio
        # the bound and its theta gradient are bit for bit those of an object without the Z gradient, and lml_grad keeps its shape
        F0, g0 = plain.lml_grad(theta)
        assert F == F0 and np.array_equal(g, g0)
        F1, g1 = sp.lml_grad(theta)
        assert F1 == F0 and g1.shape == g0.shape and np.array_equal(g1, g0)
        assert sp.bound(theta) == F0
        with pytest.raises(ValueError, match="z_grad"):
            plain.lml_grad_z(theta)
    finally:
        sp.close()
        plain.close()


@pytest.mark.parametrize("kernel", ["RBF", "RBF+Matern32", FOUR])
def test_slab_counts_agree_within_the_tolerance_and_a_repeated_call_returns_the_same_bits(kernel):
    """(n, m, d, chunk) = (700, 200, 5, 256): chunks of 256, 256 and 188 points, so four, four and three 64-row blocks against
    four column blocks.  zgrad_slabs = 1: one slab walks every row block; 2: two row blocks per slab (two and one in the last
    chunk); the default: one row block per slab."""
    case = (kernel, 700, 200, 5, 256, "subset")
    X, y, Z, theta, _, chunk = R.device_case(case)
    if kernel == FOUR:
        theta = R.make_theta(kernel, 5, ls=2.0 * np.linspace(0.4, 1.5, 5))
    ref = ZR.reference(X, y, Z, kernel, theta, ("slabs", kernel))
    ptol = R.tolerances(ref["cond_Kuu"])[1]
    out = []
    for slabs in (1, 2, None):
        sp = _sparse(X, y, Z, kernel, chunk=chunk, z_grad=True, zgrad_slabs=slabs)
        try:
            F, g, gz = sp.lml_grad_z(theta)
            F2, g2, gz2 = sp.lml_grad_z(theta)
        finally:
            sp.close()
        assert F2 == F and np.array_equal(g2, g) and np.array_equal(gz2, gz)
        ratio = ZR.ratio(gz, ref)
        print(kernel, "zgrad_slabs =", slabs, "cond(Kuu) = %.2e" % ref["cond_Kuu"], "dF/dZ ratio %.4f" % ratio)
        assert ratio <= 1.0, (slabs, ratio)
        out.append((F, g, gz))
    for F, g, gz in out[1:]:
        assert F == out[0][0] and np.array_equal(g, out[0][1])  # the slabs regroup dF/dZ's sums alone
        assert np.all(np.abs(gz - out[0][2]) <= ptol * np.maximum(np.abs(out[0][2]), 1.0))


def test_more_than_128_dimensions_take_two_windows():
    """d = 130 (n = 200, m = 70, RBF): the kernel's passes cover dimensions [0, 128) and [128, 130).  Four times
    sgpr_ref.make_theta's length scales, which keep r2 near 2 over 130 dimensions (at the plain ones r2 is near 30, Kuu the
    identity to 1e-5 and max|dF/dZ| 1e-2: nothing to measure an error against)."""
    n, m, d = 200, 70, 130
    X, y = R.problem(n, d, seed=n + m)
    Z = X[np.sort(np.random.default_rng(1).choice(n, m, replace=False))].copy()
    theta = R.make_theta("RBF", d, ls=4.0 * np.linspace(0.4, 1.5, d))
    ref = ZR.reference(X, y, Z, "RBF", theta, "window")
    assert float(np.max(np.abs(ref["grad_z"][:, 128:]))) > 1.0  # the second window has something to get wrong
    sp = _sparse(X, y, Z, "RBF", z_grad=True)
    try:
        _, _, gz = sp.lml_grad_z(theta)
    finally:
        sp.close()
    ratio = ZR.ratio(gz, ref)
    print("d = 130: cond(Kuu) = %.2e" % ref["cond_Kuu"], "dF/dZ ratio %.4f" % ratio)
    assert ratio <= 1.0, ratio


def test_a_bad_pivot_zeroes_the_gradient_by_the_inducing_points_and_the_object_stays_usable():
    """tests/test_gpu_sparse.py's case: rows 5 and 9 of Z are one point and jitter = 0, so pivot 10 of Kuu is not positive."""
    kernel, n, m, d = "Matern52", 300, 40, 3
    X, y = R.problem(n, d, seed=21)
    Z = X[:m].copy()
    Z[9] = Z[5]
    good = R.case_theta(kernel, d)
    bad = good.copy()
    bad[-1] = 0.0
    sp = _sparse(X, y, Z, kernel, z_grad=True)
    fresh = _sparse(X, y, Z, kernel, z_grad=True)
    try:
        F1, g1, gz1 = sp.lml_grad_z(good)
        assert sp.info == 0 and gz1.any()
        F, g, gz = sp.lml_grad_z(bad)
        assert sp.info == 10, sp.info
        assert F == -np.inf and not g.any() and not gz.any() and gz.shape == (m, d)
        F2, g2, gz2 = sp.lml_grad_z(good)
        F3, g3, gz3 = fresh.lml_grad_z(good)
        assert sp.info == 0 and F2 == F3 == F1 and np.array_equal(g2, g3) and np.array_equal(gz2, gz3) and np.array_equal(gz2, gz1)
        # moving the points away from each other: set_inducing binds the new Z and the same object predicts on it
        Z2 = Z.copy()
        Z2[9] = X[m + 1]
        sp.set_inducing(Z2)
        other = _sparse(X, y, Z2, kernel, z_grad=True)
        try:
            a, b = sp.lml_grad_z(good), other.lml_grad_z(good)
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
            pa, pb = sp.predict(good, X[:50]), other.predict(good, X[:50])
            assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1])
        finally:
            other.close()
        with pytest.raises(ValueError, match="Z must be"):
            sp.set_inducing(Z2[:-1])
    finally:
        sp.close()
        fresh.close()


# ------------------------------------------------------------------------------------------------------------ the facade
N, M = 600, 20


def _fun(x):
    return np.array([x[0] ** 2 - x[0] - x[1] ** 2 * x[0] + x[1]])  # the tutorial's target


def _gp():
    from andvaranaut_amd import GPMCMC, normal, uniform

    priors = [st.uniform(loc=0, scale=2), st.uniform(loc=1, scale=0.5)]
    g = GPMCMC(kernel="Matern52", noise=True, xconrevs=[uniform(priors[0]), normal(priors[1])], yconrevs=[None], nx=2, ny=1,
               priors=priors, target=_fun, parallel=False, nproc=1, verbose=False)
    g.sample(nsamps=N, seed=1)
    return g


def test_optimising_the_inducing_points_tightens_the_bound_of_a_fixed_fit():
    g = _gp()
    try:
        # refusals come before any device call
        for kw in (dict(), dict(inducing=M, method="none"), dict(inducing=M, method="mcmc_mean")):
            with pytest.raises(ValueError, match="inducing"):
                g.fit(optimize_inducing=True, **kw)
        assert g.gp is None and g.hypers is None

        d0 = g.fit(method="map", inducing=M, inducing_seed=3, return_data=True)
        Z0, start = g.inducing.copy(), dict(g.hypers)
        theta0 = g._theta_from_hypers(g.hypers, 1e-6)
        F0 = g.gp.bound(theta0)
        # (L-BFGS-B over 40 more unknowns: the best point of at most 400 evaluations is what the test needs)
        d1 = g.fit(method="map", inducing=M, inducing_seed=3, optimize_inducing=True, start=start, maxeval=400, return_data=True)
        theta1 = g._theta_from_hypers(g.hypers, 1e-6)
        F1 = g.gp.bound(theta1)
        print("fixed Z: logp = %.6f, F = %.6f (nfev %d); optimised Z: logp = %.6f, F = %.6f (nfev %d)"
              % (d0["logp"], F0, d0["nfev"], d1["logp"], F1, d1["nfev"]))
        # the optimiser starts at the fixed fit's optimum and keeps the best point seen: not lower; the bound is variational in Z
        assert d1["logp"] > d0["logp"] + 1e-6 * abs(d0["logp"])
        assert F1 > F0 + 1e-6 * abs(F0)
        assert np.array_equal(d1["inducing_start"], Z0) and np.array_equal(g.inducing, d1["inducing"])
        assert g.inducing.shape == (M, 2) and not np.array_equal(g.inducing, Z0)
        # still a lower bound of the exact log marginal likelihood at the fitted theta
        xin, yin = g._converted(g.x, g.y - g.ym)
        lml = float(R.exact_lml(xin, yin, "Matern52", theta1))
        Kuu = R.cov(g.inducing, g.inducing, "Matern52", theta1, np.float64) + theta1[-1] * np.eye(M)
        vtol = R.tolerances(float(np.linalg.cond(Kuu)))[0]
        assert F1 <= lml + vtol * max(abs(lml), 1.0), (F1, lml)
        # predict runs on the stored, optimised points -- on this object and on one rebuilt from its state
        xt = np.random.default_rng(5).uniform([0, 1], [2, 1.5], (50, 2))
        yt = np.array([_fun(r) for r in xt])
        yp, yv = g.predict(xt, return_var=True)
        r2 = 1 - np.sum((yp - yt) ** 2) / np.sum((yt - yt.mean()) ** 2)
        print("R^2 on %d inducing points = %.7f" % (M, r2))
        assert yp.shape == (50, 1) and yv.shape == (50, 1) and np.all(np.isfinite(yp)) and np.all(yv > 0)
        fresh = _sparse(xin, yin, g.inducing, "Matern52")
        try:
            mu, var = fresh.predict(theta1, np.column_stack([g.xconrevs[i].con(xt[:, i]) for i in range(2)]), pred_noise=True)
        finally:
            fresh.close()
        yc, yvc = g.predict(xt, return_var=True, revert=False)
        assert np.array_equal(yc[:, 0], mu) and np.array_equal(yvc[:, 0], var)
    finally:
        g.change_model()
