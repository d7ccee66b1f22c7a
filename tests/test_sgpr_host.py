"""The references of the sparse inducing-point bound (tests/sgpr_ref.py) against one another on the CPU, the properties a
collapsed variational bound must have, and the CPU half of the device test's tolerance rule: the fp64 restatement of the
device's algebra alone stays within a quarter of each tolerance on every case tests/test_gpu_sparse.py relies on."""
import numpy as np
import pytest

import sgpr_ref as R

LD = np.longdouble


def _case(kernel, n=300, m=40, d=3, seed=11):
    X, y = R.problem(n, d, seed)
    Z = X[np.sort(np.random.default_rng(seed + 1).choice(n, m, replace=False))].copy()
    return X, y, Z, R.make_theta(kernel, d)


@pytest.mark.parametrize("kernel", ["RBF", "Matern52", "RBF+Matern32", "Matern52*Exponential", "RatQuad"])
def test_long_double_b_form_matches_the_dense_form(kernel):
    X, y, Z, theta = _case(kernel)
    ref = R.bound_ld(X, y, Z, kernel, theta, grad=False)
    dense = R.bound_dense(X, y, Z, kernel, theta)
    # the dense fp64 form solves with Kuu (cond up to 5e7) and the n x n Qff + s I: 1e-6 relative is what it can give
    assert abs(dense - float(ref["F"])) <= 1e-6 * abs(float(ref["F"]))


@pytest.mark.parametrize("kernel", ["RBF", "Matern52", "RBF+Matern32", "Matern52*Exponential", "RatQuad"])
def test_analytic_gradient_matches_central_differences(kernel):
    X, y, Z, theta = _case(kernel, n=120, m=25)
    g = R.bound_ld(X, y, Z, kernel, theta)["grad"]
    assert g[-1] == 0
    for k in range(theta.size - 1):  # (the jitter slot is 0 by contract: jitter is a constant of the fit)
        if abs(g[k]) == 0 and k >= theta.size - 2 - len(R.split(kernel)[0]):
            continue  # alpha of a component that is no rational quadratic
        h = 1e-6 * max(abs(theta[k]), 1e-2)
        tp, tm = theta.copy(), theta.copy()
        tp[k] += h
        tm[k] -= h
        fd = (R.bound_ld(X, y, Z, kernel, tp, grad=False)["F"] - R.bound_ld(X, y, Z, kernel, tm, grad=False)["F"]) / LD(tp[k] - tm[k])
        # central differences in long double: truncation h^2 f''' / 6 ~ 1e-12 relative steps, rounding 1e-19 |F| / h
        assert abs(fd - g[k]) <= 1e-6 * max(abs(g[k]), 1), (k, float(fd), float(g[k]))


@pytest.mark.parametrize("kernel", ["RBF", "Matern52"])
def test_nested_inducing_sets_raise_the_bound_up_to_the_exact_lml(kernel):
    n, d = 300, 3
    X, y = R.problem(n, d, seed=5)
    theta = R.make_theta(kernel, d)
    exact = float(R.exact_lml(X, y, kernel, theta, LD))
    perm = np.random.default_rng(6).permutation(n)
    last = -np.inf
    for m in (10, 20, 40, 80, 160, 300):
        F = float(R.bound_ld(X, y, X[perm[:m]].copy(), kernel, theta, grad=False)["F"])
        assert F >= last - 1e-9 * abs(F), (m, F, last)
        assert F <= exact + 1e-9 * abs(exact), (m, F, exact)
        last = F
    # Z = X: Kff - Qff = j Kff (Kff + j I)^-1 lies between 0 and j I (j = jitter).  The trace term is then at most n j / (2 s), and
    # log N(y | 0, C - E) with 0 <= E <= j I, C = Kff + s I, falls short of log N(y | 0, C) by at most n j / (2 s) + j |C^-1 y|^2 / 2
    # to first order in j / s = 1e-4
    s, j = theta[-2] + theta[-1], theta[-1]
    K = R.cov(X, X, kernel, theta, np.float64)
    alpha = np.linalg.solve(K + s * np.eye(n), y)
    assert exact - last <= 1.01 * j * (n / s + 0.5 * alpha @ alpha), (exact, last)


def test_select_inducing_picks_distinct_rows_reproducibly():
    from andvaranaut_amd.sparse import select_inducing

    X, _ = R.problem(200, 3, seed=2)
    X[17] = X[3]  # a coincident pair: at most one of the two may be chosen
    Z = select_inducing(X, 60, seed=4)
    assert Z.shape == (60, 3)
    assert len({tuple(r) for r in Z}) == 60
    assert all(any((r == x).all() for x in X) for r in Z)
    assert np.array_equal(Z, select_inducing(X, 60, seed=4))
    assert not np.array_equal(Z, select_inducing(X, 60, seed=5))
    with pytest.raises(ValueError):
        select_inducing(X, 201)
    with pytest.raises(ValueError):
        select_inducing(np.zeros((5, 2)), 2)  # one distinct row only


@pytest.mark.parametrize("case", R.DEVICE_CASES, ids=R.case_id)
def test_fp64_restatement_uses_at_most_a_quarter_of_each_tolerance(case):
    X, y, Z, theta, Xnew, chunk = R.device_case(case)
    kernel = case[0]
    ref = R.reference(case)
    got = R.device_fp64(X, y, Z, kernel, theta, chunk=chunk, Xnew=Xnew)
    ratios = R.error_ratios(got, ref, ref["cond_Kuu"])
    print(R.case_id(case), "cond(Kuu) = %.2e" % ref["cond_Kuu"], {k: "%.4f" % v for k, v in ratios.items()})
    assert max(ratios.values()) <= 0.25, ratios
