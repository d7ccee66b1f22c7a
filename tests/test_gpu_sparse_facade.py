"""GPMCMC.fit(inducing=...) end to end on the GPU: a MAP fit on the sparse bound of the tutorial function, the sparse
predictive through predict (variance, Gauss-Hermite reversion, EI), the refusals, and pickling."""
import pickle

import numpy as np
import pytest
import scipy.stats as st

pytestmark = pytest.mark.gpu

N, M = 400, 64


def _fun(x):
    return np.array([x[0] ** 2 - x[0] - x[1] ** 2 * x[0] + x[1]])  # the tutorial's target


def _gp(ny=1):
    from andvaranaut_amd import GPMCMC, normal, uniform

    priors = [st.uniform(loc=0, scale=2), st.uniform(loc=1, scale=0.5)]
    target = _fun if ny == 1 else (lambda x: np.array([_fun(x)[0], x[0] + x[1]]))
    g = GPMCMC(kernel="RBF", noise=True, xconrevs=[uniform(priors[0]), normal(priors[1])], yconrevs=[None] * ny, nx=2, ny=ny,
               priors=priors, target=target, parallel=False, nproc=1, verbose=False)
    g.sample(nsamps=N, seed=1)
    return g


@pytest.fixture(scope="module")
def fitted():
    g = _gp()
    data = g.fit(method="map", inducing=M, inducing_seed=3, return_data=True)
    yield g, data
    g.change_model()  # releases the device object


def test_map_fit_on_inducing_points_converges_and_predicts(fitted):
    from andvaranaut_amd.sparse import MiSparseGP

    g, data = fitted
    # L-BFGS-B stops on one of its convergence criteria, not in a failed line search (what a wrong gradient ends in) or at maxeval
    assert "CONVERGENCE" in str(data["message"]), data
    assert np.isfinite(data["logp"]) and data["nfev"] < 1000
    assert isinstance(g.gp, MiSparseGP) and g.inducing.shape == (M, 2)
    xin, _ = g._converted(g.x, g.y - g.ym)
    assert all(any((z == x).all() for x in xin) for z in g.inducing)  # rows of the converted inputs
    xt = np.random.default_rng(5).uniform([0, 1], [2, 1.5], (50, 2))
    yt = np.array([_fun(r) for r in xt])
    yp, yv = g.predict(xt, return_var=True)
    r2 = 1 - np.sum((yp - yt) ** 2) / np.sum((yt - yt.mean()) ** 2)
    print("sparse MAP fit: nfev = %d, logp = %.6f, R^2 = %.7f" % (data["nfev"], data["logp"], r2))
    assert yp.shape == (50, 1) and yv.shape == (50, 1) and np.all(yv > 0)
    assert r2 >= 0.999, r2
    # the bound the fit maximised is a lower bound of the exact log marginal likelihood at the fitted hyper-parameters
    from andvaranaut_amd import MiGP

    theta = g._theta_from_hypers(g.hypers, 1e-6)
    gp = MiGP(*g._converted(g.x, g.y - g.ym), "RBF", device=0, need_grad=False)
    try:
        assert g.gp.bound(theta) <= gp.lml(theta)
    finally:
        gp.close()
    # EI and the converted-space predictive go through the same sparse object
    g.yopt = float(g.y.min())  # (what BO sets before it asks for the expected improvement)
    ei = g.predict(xt, EI=True, EIopt="min", normvar=False)
    assert ei.shape == (50, 1) and np.all(np.isfinite(ei)) and np.all(ei >= 0.0)
    yc, yvc = g.predict(xt, return_var=True, revert=False)
    mu, var = g.gp.predict(theta, np.column_stack([g.xconrevs[i].con(xt[:, i]) for i in range(2)]), pred_noise=True)
    assert np.array_equal(yc[:, 0], mu) and np.array_equal(yvc[:, 0], var)


def test_a_pickled_object_predicts_the_same_bits(fitted):
    g, _ = fitted
    xt = np.random.default_rng(6).uniform([0, 1], [2, 1.5], (40, 2))
    yp, yv = g.predict(xt, return_var=True)
    h = pickle.loads(pickle.dumps(g))
    assert h.gp is None and np.array_equal(h.inducing, g.inducing)
    yp2, yv2 = h.predict(xt, return_var=True)
    assert np.array_equal(yp2, yp) and np.array_equal(yv2, yv)
    h.change_model()


def test_inducing_array_of_raw_inputs_and_method_none(fitted):
    g, _ = fitted
    raw = g.x[:32].copy()
    h = _gp()
    h.m, h.hypers = g.m, g.hypers
    h.fit(method="none", inducing=raw)
    assert h.inducing.shape == (32, 2)
    assert np.array_equal(h.inducing, np.column_stack([h.xconrevs[i].con(raw[:, i]) for i in range(2)]))
    yp = h.predict(g.x[:20])
    assert yp.shape == (20, 1) and np.all(np.isfinite(yp))
    h.fit(method="none")  # a dense fit drops the choice
    assert h.inducing is None
    h.change_model()


def test_what_the_sparse_bound_cannot_do_is_refused_by_name(fitted):
    g, _ = fitted
    h = _gp()
    for kw in (dict(method="mcmc_mean"), dict(method="mcmc_map"), dict(iwgp=True), dict(cwgp=True), dict(objective="loo"),
               dict(objective="kfold"), dict(trend="constant"), dict(trend="linear")):
        with pytest.raises(ValueError, match="inducing"):
            h.fit(inducing=M, **kw)
    h2 = _gp(ny=2)
    with pytest.raises(ValueError, match="inducing"):
        h2.fit(inducing=M, outputs="all")
    for bad in (0, N + 1, 5000, np.zeros((4, 3)), np.zeros(4), np.full((4, 2), np.nan)):
        with pytest.raises(ValueError, match="inducing"):
            h.fit(inducing=bad)
    assert h.gp is None and h.hypers is None  # every refusal came before any device call
    xt = g.x[:8]
    calls = [lambda: g.predict_joint(xt), lambda: g.sample_posterior(xt), lambda: g.log_predictive(xt, g.y[:8, 0]),
             lambda: g.cv_stats(nfolds=4), lambda: g.predict_mean(xt), lambda: g.sample_paths(npaths=2),
             lambda: g.predict_posterior(xt, None), lambda: g.BO(max_iter=1, refit_every=2), lambda: g.BO(max_iter=1, method="TS"),
             lambda: g._bo_potential("EI", "min", True, 1e-6), lambda: g.inverse_opt(np.array([0.1]), resident=True)]
    for call in calls:
        with pytest.raises(ValueError, match="inducing"):
            call()
