"""The leave-one-out objective of mi_gp_lml_grad (option 48 = 1; MiGP.loo_grad, GPMCMC.fit(objective="loo")) against the
references of tests/loo_ref.py -- the value against one refit per point, the gradient against Rasmussen & Williams eq. 5.13 in
forward mode -- against mi_gp_kfold's leave-one-out densities, and for what it must leave alone: the resident K^-1 and alpha, the
ordinary objective's bits, and the zeros of Z_dev that the next triangular inverse relies on.

Bounds are the project's own for the LML and its gradient, with cond = cond(K): the value within max(1e-10, 20 cond eps) of
max(|ref|, 1), the gradient per component (floored at 1e-3 of the largest) within max(1e-7, 500 cond eps).  Every parity check
prints error / bound before it asserts."""
import numpy as np
import pytest
import scipy.stats as st

import kfold_ref
import loo_ref as ref

pytestmark = pytest.mark.gpu

EPS = ref.EPS


def _gp(X, y, kernel, diag):
    from andvaranaut_amd import MiGP

    gp = MiGP(X, y, kernel, device=0)
    if diag is not None:
        gp.set_diag(diag)
    return gp


def _alpha(gp):
    import ctypes

    a = np.empty(gp.n)
    assert gp.lib.mi_gp_alpha(gp.h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 0
    return a


@pytest.mark.parametrize("i", range(len(ref.CASES)))
def test_value_and_gradient_parity_and_the_resident_state(i):
    X, y, kernel, theta, diag, cond = ref.case(i)
    v_refit, (_, g_fwd), _ = ref.case_refs(i)
    gp = _gp(X, y, kernel, diag)
    n = gp.n
    assert gp.get_option(48) == 0  # the default
    v_lml, g_lml = gp.lml_grad(theta)
    alpha_lml = _alpha(gp)
    parts = gp.lml_parts()
    val, grad = gp.loo_grad(theta)
    assert gp.info == 0 and gp.get_option(48) == 0
    rv, rg = ref.value_ratio(val, v_refit, cond), ref.grad_ratio(grad, g_fwd, cond)
    print(ref.CASES[i], "cond %.3g" % cond, "error / bound: value %.3g gradient %.3g" % (rv, rg))
    assert rv <= 1.0 and rg <= 1.0, (rv, rg, val, v_refit, grad, g_fwd)
    assert grad[-1] == grad[-2]  # d/d jitter = d/d gv
    # K^-1 and alpha stay resident with their meaning: alpha's bits, the factorisation's parts, and mi_gp_kfold's leave-one-out
    # densities, whose sum the value is (n terms of at most max|logp_i|, each within a few ulps, summed in another order)
    assert np.array_equal(_alpha(gp), alpha_lml) and gp.lml_parts() == parts
    logp, _, _, info = gp.kfold(theta, np.arange(n, dtype=np.int32).reshape(n, 1), moments=False, resident=True)
    assert not info.any()
    assert abs(val - np.sum(logp)) <= n * 4 * EPS * np.max(np.abs(logp)), (val, np.sum(logp))
    # the same call in the same state: the same bits; and the ordinary objective behind it returns what it returned before
    v2, g2 = gp.loo_grad(theta)
    assert v2 == val and np.array_equal(g2, grad)
    v3, g3 = gp.lml_grad(theta)
    assert v3 == v_lml and np.array_equal(g3, g_lml)
    gp.close()


def test_the_tail_gemm_on_128_tiles_at_46_tile_columns():
    """N = 5800: 1081 lower tiles, the GEMM's 128x128-tile path; against the float64 restatement of the reverse-mode algebra (the
    forward form and a refit per point are out of reach at this size).  cond(K) by the Gershgorin bound over the noise floor, as
    tests/test_gpu_append.py does beyond 1200 points."""
    from oracle import gp_oracle as orc

    kernel, n, d, with_diag, gv = ref.BIG
    X, y, theta, diag = ref.make_problem(kernel, n, d, with_diag, gv, 99)
    cond = np.abs(orc.noisy_cov(X, [kernel], [], theta, "marginal", diag)).sum(1).max() / (theta[-1] + theta[-2])
    v_ref, g_ref = ref.loo_reverse(X, y, kernel, theta, diag)
    gp = _gp(X, y, kernel, diag)
    val, grad = gp.loo_grad(theta)
    rv, rg = ref.value_ratio(val, v_ref, cond), ref.grad_ratio(grad, g_ref, cond)
    print(ref.BIG, "cond <= %.3g" % cond, "error / bound: value %.3g gradient %.3g" % (rv, rg))
    assert gp.info == 0 and rv <= 1.0 and rg <= 1.0, (rv, rg, val, v_ref, grad, g_ref)
    gp.close()


@pytest.mark.parametrize("i", [5, 9])
def test_switching_back_returns_a_fresh_handles_bits(i):
    """After an evaluation under option 48 = 1 the handle is as good as new: the LML + gradient, and the predictions through
    U = L^-T (mi_gp_predict_u, mi_gp_predict_grad), whose triangular inverse never writes the tiles of Z_dev below the diagonal."""
    X, y, kernel, theta, diag, _ = ref.case(i)
    Xn = np.random.default_rng(i).random((7, X.shape[1]))

    def everything(gp):
        out = [gp.lml(theta), *gp.lml_grad(theta)]
        out += list(gp.predict(theta, Xn, via_inverse=True))
        out += list(gp.predict_grad(theta, Xn))
        return out

    fresh = _gp(X, y, kernel, diag)
    want = everything(fresh)
    fresh.close()
    gp = _gp(X, y, kernel, diag)
    gp.set_objective("loo")
    assert gp.get_option(48) == 1
    assert gp.lml(theta) == want[0]  # mi_gp_lml is not affected
    val, _ = gp.lml_grad(theta)
    assert np.isfinite(val) and val != want[1]
    with pytest.raises(RuntimeError, match="batched"):
        gp.lml_grad_batch(np.stack([theta, theta]))
    assert np.array_equal(gp.lml_batch(np.stack([theta, theta])), [want[0], want[0]])
    with pytest.raises(RuntimeError, match="option 48"):
        gp.set_option(48, 2)
    assert gp.get_option(48) == 1
    gp.set_objective("lml")
    got = everything(gp)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)), [np.array_equal(a, b) for a, b in zip(got, want)]
    # ... and with the predictions straight behind the tail, no gradient evaluation in between
    gp.loo_grad(theta)
    assert all(np.array_equal(a, b) for a, b in zip(gp.predict(theta, Xn, via_inverse=True), want[3:5]))
    gp.loo_grad(theta)
    assert all(np.array_equal(a, b) for a, b in zip(gp.predict_grad(theta, Xn), want[5:]))
    gp.close()


def test_the_handles_vectors_follow_reserve_and_append():
    """The tail's vectors are sized for the capacity at the first call; mi_gp_reserve (here through an append beyond the
    capacity, which also crosses a tile boundary: 120 -> 130 points) re-sizes them."""
    from andvaranaut_amd import MiGP

    X, y, kernel, theta, _, _ = ref.case(4)
    n0 = 120
    gp = MiGP(X[:n0], y[:n0], kernel, device=0, capacity=124)
    first = gp.loo_grad(theta)
    assert np.isfinite(first[0]) and gp.info == 0
    assert gp.factor(theta) == 0 and gp.append(X[n0:122], y[n0:122]) == 0 and gp.append_refactors == 0  # inside the capacity
    inside = gp.loo_grad(theta)
    assert gp.factor(theta) == 0
    assert gp.append(X[122:], y[122:]) == 0 and gp.n == len(y) and gp.append_refactors == 1  # beyond it: reserve
    got = gp.loo_grad(theta)
    gp.close()
    for n, have in ((122, inside), (len(y), got)):
        fresh = MiGP(X[:n], y[:n], kernel, device=0)
        want = fresh.loo_grad(theta)
        fresh.close()
        assert have[0] == want[0] and np.array_equal(have[1], want[1]), (n, have, want)


def test_a_planted_bad_pivot_is_reported_as_under_the_ordinary_objective():
    import bad_pivot_cases as C

    n, p = 300, 141
    X, y = C.problem(n)
    theta = C.good_theta(0)
    gp = _gp(X, y, "RBF", None)
    good = gp.loo_grad(theta)
    assert np.isfinite(good[0]) and gp.info == 0
    gp.set_diag(C.planted_diag(n, p, theta))
    v0, g0 = gp.lml_grad(theta)
    assert v0 == -np.inf and gp.info == p + 1 and not g0.any()
    v1, g1 = gp.loo_grad(theta)
    assert v1 == -np.inf and gp.info == p + 1 and not g1.any()
    gp.set_diag(None)
    again = gp.loo_grad(theta)
    assert again[0] == good[0] and np.array_equal(again[1], good[1]) and gp.info == 0
    gp.close()


def test_map_fit_on_the_loo_objective_ends_where_the_reference_driven_fit_ends():
    from andvaranaut_amd import GPMCMC, normal, uniform
    from andvaranaut_amd.optimize import find_MAP
    from andvaranaut_amd.priors import HyperModel

    priors = [st.uniform(loc=0, scale=2), st.uniform(loc=1, scale=0.5)]
    fun = lambda x: np.array([x[0] ** 2 - x[0] - x[1] ** 2 * x[0] + x[1]])  # noqa: E731
    g = GPMCMC(kernel="RBF", noise=True, xconrevs=[uniform(priors[0]), normal(priors[1])], yconrevs=[None], nx=2, ny=1,
               priors=priors, target=fun, parallel=False, nproc=1, verbose=False)
    g.sample(nsamps=60, seed=1)
    data = g.fit(method="map", objective="loo", return_data=True)
    assert {"l", "kv", "gv"} <= set(g.hypers) and g.gp.get_option(48) == 0
    xin, yin = g._converted(g.x, g.y - g.ym)
    model = HyperModel(2, ["RBF"], noise=True, jitter=1e-6)
    f = lambda q: model.logp_dlogp(q, lambda th: ref.loo_forward(xin, yin, "RBF", th), jacobian=False)  # noqa: E731
    q, info = find_MAP(f, model.initial_point())
    print("LOO MAP: device %.12g (%d evaluations), reference %.12g (%d)" % (data["logp"], data["nfev"], info["logp"], info["nfev"]))
    assert abs(info["logp"] - data["logp"]) <= 1e-6 * abs(info["logp"])
    # ... and it is not the marginal likelihood's optimum
    lml_fit = g.fit(method="map", return_data=True)
    assert abs(lml_fit["logp"] - data["logp"]) > 1e-3 * abs(data["logp"])
