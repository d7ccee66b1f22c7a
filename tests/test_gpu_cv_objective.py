"""The k-fold cross-validation objective of mi_gp_lml_grad (option 48 = 1 with option 49 = b; MiGP.cv_grad,
GPMCMC.fit(objective="kfold")) against the references of tests/cv_objective_ref.py -- the value against one refit per fold, the
gradient against the forward-mode form -- against mi_gp_kfold's densities of the same folds, and for what it must leave alone: the
resident K^-1 and alpha, the ordinary objective's bits, the leave-one-out path's bits and the zeros of Z_dev.

Bounds are the project's own for the LML and its gradient (loo_ref.value_ratio, loo_ref.grad_ratio), with cond = cond(K).  Every
parity check prints error / bound before it asserts."""
import numpy as np
import pytest
import scipy.stats as st

import cv_objective_ref as ref
import kfold_ref
import loo_ref

pytestmark = pytest.mark.gpu

EPS = loo_ref.EPS


def _gp(X, y, kernel, diag, **kw):
    from andvaranaut_amd import MiGP

    gp = MiGP(X, y, kernel, device=0, **kw)
    if diag is not None:
        gp.set_diag(diag)
    return gp


def _alpha(gp):
    import ctypes

    a = np.empty(gp.n)
    assert gp.lib.mi_gp_alpha(gp.h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 0
    return a


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("i,b", ref.PAIRS)
def test_value_and_gradient_parity_and_the_resident_state(i, b):
    X, y, kernel, theta, diag, cond = loo_ref.case(i)
    v_refit, (_, g_fwd), _ = ref.case_refs(i, b)
    gp = _gp(X, y, kernel, diag)
    n = gp.n
    assert gp.get_option(49) == 1  # the default
    v_lml, g_lml = gp.lml_grad(theta)
    alpha_lml = _alpha(gp)
    parts = gp.lml_parts()
    val, grad = gp.cv_grad(theta, b)
    assert gp.info == 0 and gp.get_option(48) == 0 and gp.get_option(49) == 1
    rv, rg = loo_ref.value_ratio(val, v_refit, cond), loo_ref.grad_ratio(grad, g_fwd, cond)
    print(loo_ref.CASES[i], "b = %d" % b, "cond %.3g" % cond, "error / bound: value %.3g gradient %.3g" % (rv, rg))
    assert rv <= 1.0 and rg <= 1.0, (rv, rg, val, v_refit, grad, g_fwd)
    assert grad[-1] == grad[-2]  # d/d jitter = d/d gv
    # K^-1 and alpha stay resident with their meaning: alpha's bits, the factorisation's parts, and mi_gp_kfold's densities of the
    # same folds, whose sum the value is (per-fold bits are shared: only the order of the sum differs)
    assert np.array_equal(_alpha(gp), alpha_lml) and gp.lml_parts() == parts
    folds = ref.folds_of(n, b)
    logp, _, _, info = gp.kfold(theta, folds, moments=False, resident=True)
    assert not np.any(info)
    assert abs(val - np.sum(logp)) <= 4 * EPS * len(folds) * np.max(np.abs(logp)), (val, np.sum(logp))
    # the same call in the same state: the same bits; and the ordinary objective behind it returns what it returned before
    assert _same(gp.cv_grad(theta, b), (val, grad))
    assert _same(gp.lml_grad(theta), (v_lml, g_lml))
    gp.close()


@pytest.mark.parametrize("i", [4, 5])
def test_a_block_of_one_point_is_the_leave_one_out_path(i):
    X, y, kernel, theta, diag, _ = loo_ref.case(i)
    gp = _gp(X, y, kernel, diag)
    want = gp.loo_grad(theta)
    assert _same(gp.cv_grad(theta, 1), want)
    gp.cv_grad(theta, 37)
    assert _same(gp.cv_grad(theta, 1), want) and _same(gp.loo_grad(theta), want)
    gp.close()


@pytest.mark.parametrize("i,b", [(2, 128), (10, 128)])
def test_one_fold_of_all_points_is_the_marginal_likelihood(i, b):
    """n = 128 with b = 128: a single fold, L_CV is the LML and its gradient the LML's, within the bounds (another route: the
    factor of all of K^-1)."""
    X, y, kernel, theta, diag, cond = loo_ref.case(i)
    assert len(y) <= b
    gp = _gp(X, y, kernel, diag)
    v_lml, g_lml = gp.lml_grad(theta)
    val, grad = gp.cv_grad(theta, b)
    rv, rg = loo_ref.value_ratio(val, v_lml, cond), loo_ref.grad_ratio(grad, g_lml, cond)
    print(loo_ref.CASES[i], "b = %d" % b, "error / bound against the LML: value %.3g gradient %.3g" % (rv, rg))
    assert gp.info == 0 and rv <= 1.0 and rg <= 1.0, (rv, rg)
    gp.close()


def test_the_ragged_edges_have_folds_of_one_point():
    """n = 257 with b = 128 (128, 128, 1) and n = 130 with b = 43 (43, 43, 43, 1) are among the parity cases: here the layouts
    themselves, and the last fold's density against the singleton closed form of mi_gp_kfold."""
    for i, b, sizes in ((5, 128, [128, 128, 1]), (4, 43, [43, 43, 43, 1])):
        X, y, kernel, theta, diag, cond = loo_ref.case(i)
        assert (i, b) in ref.PAIRS and [len(f) for f in ref.folds_of(len(y), b)] == sizes
        gp = _gp(X, y, kernel, diag)
        val, _ = gp.cv_grad(theta, b)
        logp, _, _, _ = gp.kfold(theta, ref.folds_of(len(y), b), moments=False, resident=True)
        single, _, _, _ = gp.kfold(theta, [np.array([len(y) - 1])], moments=False, resident=True)
        assert abs(logp[-1] - single[0]) <= max(1e-10, 20 * cond * EPS) * max(abs(single[0]), 1.0)
        assert abs(val - np.sum(logp)) <= 4 * EPS * len(sizes) * np.max(np.abs(logp))
        gp.close()


def test_many_folds_in_several_passes():
    """n = 2600 with b = 3: 867 folds (seven passes of the fold kernels), the last of two points, across every tile edge; against
    the float64 restatement of the reverse-mode algebra.  cond(K) by the Gershgorin bound over the noise floor."""
    from oracle import gp_oracle as orc

    kernel, n, d, gv, b = "Matern52", 2600, 3, 1e-2, 3
    X, y, theta, diag = loo_ref.make_problem(kernel, n, d, False, gv, 98)
    cond = np.abs(orc.noisy_cov(X, [kernel], [], theta, "marginal", diag)).sum(1).max() / (theta[-1] + theta[-2])
    v_ref, g_ref = ref.cv_reverse(X, y, kernel, theta, b, diag)
    gp = _gp(X, y, kernel, diag)
    val, grad = gp.cv_grad(theta, b)
    rv, rg = loo_ref.value_ratio(val, v_ref, cond), loo_ref.grad_ratio(grad, g_ref, cond)
    print((kernel, n, d, gv), "b = %d" % b, "cond <= %.3g" % cond, "error / bound: value %.3g gradient %.3g" % (rv, rg))
    assert gp.info == 0 and rv <= 1.0 and rg <= 1.0, (rv, rg, val, v_ref, grad, g_ref)
    folds = np.arange(2598, dtype=np.int32).reshape(866, 3)
    logp, _, _, info = gp.kfold(theta, folds, moments=False, resident=True)
    last, _, _, _ = gp.kfold(theta, [np.array([2598, 2599])], moments=False, resident=True)
    total = np.sum(logp) + last[0]
    assert not np.any(info) and abs(val - total) <= 4 * EPS * 867 * np.max(np.abs(logp)), (val, total)
    gp.close()


def test_the_tail_gemm_on_128_tiles_at_46_tile_columns():
    """N = 5800 with b = 100: 1081 lower tiles, the GEMM's 128x128-tile path, against the reverse-mode restatement; cond(K) by the
    Gershgorin bound as tests/test_gpu_loo_objective.py does."""
    from oracle import gp_oracle as orc

    kernel, n, d, with_diag, gv = loo_ref.BIG
    X, y, theta, diag = loo_ref.make_problem(kernel, n, d, with_diag, gv, 99)
    cond = np.abs(orc.noisy_cov(X, [kernel], [], theta, "marginal", diag)).sum(1).max() / (theta[-1] + theta[-2])
    v_ref, g_ref = ref.cv_reverse(X, y, kernel, theta, 100, diag)
    gp = _gp(X, y, kernel, diag)
    val, grad = gp.cv_grad(theta, 100)
    rv, rg = loo_ref.value_ratio(val, v_ref, cond), loo_ref.grad_ratio(grad, g_ref, cond)
    print(loo_ref.BIG, "b = 100", "cond <= %.3g" % cond, "error / bound: value %.3g gradient %.3g" % (rv, rg))
    assert gp.info == 0 and rv <= 1.0 and rg <= 1.0, (rv, rg, val, v_ref, grad, g_ref)
    gp.close()


@pytest.mark.parametrize("i", [5, 9])
def test_switching_back_returns_a_fresh_handles_bits(i):
    """After evaluations under option 49 = 37 the handle is as good as new: the LML + gradient, and the predictions through
    U = L^-T, whose triangular inverse relies on the zeros of Z_dev below the diagonal tiles."""
    X, y, kernel, theta, diag, _ = loo_ref.case(i)
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
    gp.set_cv_block(37)
    assert gp.get_option(48) == 1 and gp.get_option(49) == 37
    assert gp.lml(theta) == want[0]  # mi_gp_lml is not affected
    val, _ = gp.lml_grad(theta)
    assert np.isfinite(val) and val != want[1]
    with pytest.raises(RuntimeError, match="batched"):
        gp.lml_grad_batch(np.stack([theta, theta]))
    assert np.array_equal(gp.lml_batch(np.stack([theta, theta])), [want[0], want[0]])
    gp.set_objective("lml")
    assert gp.get_option(49) == 37  # (the fold size stays; it has no effect now)
    got = everything(gp)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)), [np.array_equal(a, b) for a, b in zip(got, want)]
    # ... and with the predictions straight behind the tail, no gradient evaluation in between
    gp.cv_grad(theta, 37)
    assert all(np.array_equal(a, b) for a, b in zip(gp.predict(theta, Xn, via_inverse=True), want[3:5]))
    gp.cv_grad(theta, 37)
    assert all(np.array_equal(a, b) for a, b in zip(gp.predict_grad(theta, Xn), want[5:]))
    gp.close()


def test_option_49_alone_changes_no_bit_and_refuses_values_outside_1_to_128():
    X, y, kernel, theta, diag, _ = loo_ref.case(8)
    gp = _gp(X, y, kernel, diag)
    want = gp.lml_grad(theta)
    for b in (2, 37, 128):
        gp.set_option(49, b)
        assert gp.get_option(48) == 0 and gp.get_option(49) == b
        assert _same(gp.lml_grad(theta), want)
    for bad in (0, 129, -1):
        with pytest.raises(RuntimeError, match="option 49"):
            gp.set_option(49, bad)
        assert gp.get_option(49) == 128  # the option keeps its value
    gp.set_objective("loo")
    with pytest.raises(RuntimeError, match="batched"):
        gp.lml_grad_batch(np.stack([theta, theta]))
    gp.close()


def test_the_handles_scratch_follows_reserve_and_append():
    """The fold pass's scratch is sized for the capacity at the first call; mi_gp_reserve (here through an append beyond the
    capacity, which also crosses a tile boundary: 120 -> 130 points) re-sizes it."""
    from andvaranaut_amd import MiGP

    X, y, kernel, theta, _, _ = loo_ref.case(4)
    n0, b = 120, 37
    gp = MiGP(X[:n0], y[:n0], kernel, device=0, capacity=124)
    first = gp.cv_grad(theta, b)
    assert np.isfinite(first[0]) and gp.info == 0
    assert gp.factor(theta) == 0 and gp.append(X[n0:122], y[n0:122]) == 0 and gp.append_refactors == 0  # inside the capacity
    inside = gp.cv_grad(theta, b)
    assert gp.factor(theta) == 0
    assert gp.append(X[122:], y[122:]) == 0 and gp.n == len(y) and gp.append_refactors == 1  # beyond it: reserve
    got = gp.cv_grad(theta, b)
    gp.close()
    for n, have in ((122, inside), (len(y), got)):
        fresh = MiGP(X[:n], y[:n], kernel, device=0)
        want = fresh.cv_grad(theta, b)
        fresh.close()
        assert _same(have, want), (n, have, want)


def test_a_planted_bad_pivot_is_reported_as_under_the_ordinary_objective():
    import bad_pivot_cases as C

    n, p, b = 300, 141, 37
    X, y = C.problem(n)
    theta = C.good_theta(0)
    gp = _gp(X, y, "RBF", None)
    good = gp.cv_grad(theta, b)
    assert np.isfinite(good[0]) and gp.info == 0
    gp.set_diag(C.planted_diag(n, p, theta))
    v0, g0 = gp.lml_grad(theta)
    assert v0 == -np.inf and gp.info == p + 1 and not g0.any()
    v1, g1 = gp.cv_grad(theta, b)
    assert v1 == -np.inf and gp.info == p + 1 and not g1.any()
    gp.set_diag(None)
    assert _same(gp.cv_grad(theta, b), good) and gp.info == 0
    gp.close()


def test_map_fit_on_the_kfold_objective_ends_where_the_reference_driven_fit_ends():
    from andvaranaut_amd import GPMCMC, MiGP, normal, uniform
    from andvaranaut_amd.optimize import find_MAP
    from andvaranaut_amd.priors import HyperModel

    priors = [st.uniform(loc=0, scale=2), st.uniform(loc=1, scale=0.5)]
    fun = lambda x: np.array([x[0] ** 2 - x[0] - x[1] ** 2 * x[0] + x[1]])  # noqa: E731
    g = GPMCMC(kernel="RBF", noise=True, xconrevs=[uniform(priors[0]), normal(priors[1])], yconrevs=[None], nx=2, ny=1,
               priors=priors, target=fun, parallel=False, nproc=1, verbose=False)
    g.sample(nsamps=60, seed=1)
    data = g.fit(method="map", objective="kfold", nfolds=5, fold_seed=3, return_data=True)
    assert {"l", "kv", "gv"} <= set(g.hypers) and g.gp.get_option(48) == 0 and g.gp.get_option(49) == 1
    folds = data["folds"]
    assert [len(f) for f in folds] == [12] * 5 and np.array_equal(np.sort(np.concatenate(folds)), np.arange(60))
    assert np.array_equal(np.concatenate(folds), np.random.default_rng(3).permutation(60))
    perm = np.concatenate(folds)
    xin, yin = g._converted(g.x, g.y - g.ym)
    xp, yp = np.ascontiguousarray(xin[perm]), np.ascontiguousarray(yin[perm])
    model = HyperModel(2, ["RBF"], noise=True, jitter=1e-6)
    f = lambda q: model.logp_dlogp(q, lambda th: ref.cv_forward(xp, yp, "RBF", th, 12), jacobian=False)  # noqa: E731
    q, info = find_MAP(f, model.initial_point())
    print("k-fold MAP: device %.12g (%d evaluations), reference %.12g (%d)" % (data["logp"], data["nfev"], info["logp"], info["nfev"]))
    assert abs(info["logp"] - data["logp"]) <= 1e-6 * abs(info["logp"])
    # the stored handle keeps the user's row order, and cv_stats on the fitted folds scores the objective without the priors
    theta = g._theta_from_hypers(g.hypers, 1e-6)
    cond = kfold_ref.full_cond(xin, "RBF", theta)
    stats = g.cv_stats(folds=folds)
    tmp = MiGP(xp, yp, "RBF", device=0)
    val, _ = tmp.cv_grad(theta, 12)
    tmp.close()
    want = float(np.sum(kfold_ref.kfold_refit(xin, yin, "RBF", theta, folds)[0]))
    rv = max(loo_ref.value_ratio(stats["lpd"], want, cond), loo_ref.value_ratio(val, want, cond))
    print("lpd of the fitted folds: cv_stats %.12g, objective %.12g, refit %.12g, error / bound %.3g" % (stats["lpd"], val, want, rv))
    assert rv <= 1.0
    # ... and it is not the marginal likelihood's optimum
    lml_fit = g.fit(method="map", return_data=True)
    assert abs(lml_fit["logp"] - data["logp"]) > 1e-3 * abs(data["logp"])
