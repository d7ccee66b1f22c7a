"""CPU side of the posterior predictive: argument validation of mi_gp_factor_batch / mi_gp_predict_batch before any device
call, and GPMCMC.predict_posterior's draw selection, warp-trace refusal, failed-draw accounting and Gauss-Hermite mixture
with the device replaced by the oracle (tests are the one place allowed to do that)."""
import ctypes

import numpy as np
import pytest
import scipy.stats as st

from oracle import gp_oracle as orc


def test_batched_conditional_entry_points_validate_before_the_device():
    from andvaranaut_amd import _lib

    lib = _lib.load()
    th = (ctypes.c_double * 16)()
    info = (ctypes.c_int * 4)()
    for k in (-1, 0, 1, 4):
        assert lib.mi_gp_factor_batch(None, k, th, info) == -1
        assert lib.mi_gp_predict_batch(None, k, None, 10, None, 256, 256 * 128, None, None, 1, None, None) == -1
    assert lib.mi_gp_factor_batch(None, 1, None, None) == -1


class _OracleBatchGP:
    """predict / predict_batch of MiGP with the oracle behind them; records the thetas it was given."""

    def __init__(self, X, y, kerns, ops, bad=()):
        self.X, self.y, self.kerns, self.ops, self.bad = X, y, kerns, ops, list(bad)
        self.calls = []

    def predict(self, theta, Xnew, pred_noise=True):
        return orc.predict(self.X, self.y, Xnew, self.kerns, self.ops, theta, pred_noise=pred_noise)

    def predict_batch(self, thetas, Xnew, pred_noise=True, mixture=True):
        self.calls.append(np.array(thetas))
        k, m = len(thetas), len(Xnew)
        mu, var = np.full((k, m), np.nan), np.full((k, m), np.nan)
        self.batch_info = np.zeros(k, dtype=np.int32)
        for p, th in enumerate(thetas):
            if any(np.array_equal(th, b) for b in self.bad):
                self.batch_info[p] = 3
                continue
            mu[p], var[p] = self.predict(th, Xnew, pred_noise)
        ok = self.batch_info == 0
        mm = mu[ok].mean(axis=0) if ok.any() else np.full(m, np.nan)
        mv = (var[ok].mean(axis=0) + ((mu[ok] - mm) ** 2).mean(axis=0)) if ok.any() else np.full(m, np.nan)
        return (mu, var, mm, mv) if mixture else (mu, var)


def _fitted(bad=(), mean=0):
    from andvaranaut_amd import GPMCMC
    from andvaranaut_amd.priors import HyperModel
    from andvaranaut_amd.transform import logarithm

    rng = np.random.default_rng(2)
    priors = [st.uniform(loc=0, scale=2), st.uniform(loc=1, scale=0.5)]
    fun = lambda x: np.array([np.exp(np.sin(2 * x[0]) + x[1] ** 2)])  # noqa: E731
    x = np.column_stack([rng.uniform(0, 2, 25), rng.uniform(1, 1.5, 25)])
    y = np.array([fun(r) for r in x])
    g = GPMCMC(kernel="Matern52", noise=True, yconrevs=[logarithm()], mean=mean, nx=2, ny=1, priors=priors, target=fun,
               verbose=False)
    g.set_data(x, y)
    g.m = HyperModel(2, ["Matern52"], noise=True)
    g.hypers = {"l": np.array([0.6, 0.8]), "kv": np.array(1.3), "gv": np.array(2e-3)}
    xin, yin = g._converted(g.x, g.y - g.ym)
    g.gp = _OracleBatchGP(xin, yin, ["Matern52"], [], bad=bad)
    return g, rng


def _trace(chains, draws, seed=0, extra=None):
    from andvaranaut_amd.nuts import Trace

    rng = np.random.default_rng(seed)
    post = {"l": rng.uniform(0.4, 1.0, (chains, draws, 2)), "kv": rng.uniform(0.8, 1.6, (chains, draws)),
            "gv": rng.uniform(1e-3, 3e-3, (chains, draws))}
    post.update(extra or {})
    return Trace(post, {"lp": np.zeros((chains, draws))})


def test_draws_are_flattened_chain_major_and_evenly_spaced():
    from andvaranaut_amd import GPMCMC

    assert np.array_equal(GPMCMC._draw_indices(10, 4), [0, 2, 5, 7])
    assert np.array_equal(GPMCMC._draw_indices(10, None), np.arange(10))
    assert np.array_equal(GPMCMC._draw_indices(10, 100), np.arange(10))
    assert np.array_equal(GPMCMC._draw_indices(7, 7), np.arange(7))
    with pytest.raises(ValueError):
        GPMCMC._draw_indices(10, 0)
    g, rng = _fitted()
    tr = _trace(2, 5)
    xs = np.column_stack([rng.uniform(0, 2, 7), rng.uniform(1, 1.5, 7)])
    a = g.predict_posterior(xs, tr, ndraws=4)
    b = g.predict_posterior(xs, tr, ndraws=4)
    assert np.array_equal(a, b) and np.array_equal(g.gp.calls[0], g.gp.calls[1])
    assert np.array_equal(g.posterior_info["draws"], [0, 2, 5, 7])
    # draw 7 of the flattened trace is chain 1, draw 2
    want = g._theta_from_hypers({"l": tr.posterior["l"][1, 2], "kv": tr.posterior["kv"][1, 2], "gv": tr.posterior["gv"][1, 2]}, 1e-6)
    assert np.array_equal(g.gp.calls[0][3], want)
    g.predict_posterior(xs, tr, ndraws=None)
    assert len(g.gp.calls[-1]) == 10 and g.posterior_info["used"] == 10


def test_warp_traces_are_refused():
    g, rng = _fitted()
    xs = rng.uniform(0, 1, (3, 2)) + [0, 1]
    for key in ("iwgp", "cwgp", "cwgp_pos"):
        tr = _trace(1, 4, extra={key: np.ones((1, 4, 2))})
        with pytest.raises(ValueError, match="warp"):
            g.predict_posterior(xs, tr)
    assert not g.gp.calls


def test_failed_draws_are_dropped_and_counted():
    g, rng = _fitted()
    tr = _trace(2, 3, seed=4)
    xs = np.column_stack([rng.uniform(0, 2, 5), rng.uniform(1, 1.5, 5)])
    thetas, _ = g._posterior_thetas(tr, None, 1e-6)
    g.gp.bad = [thetas[1], thetas[4]]
    ym, yv = g.predict_posterior(xs, tr, return_var=True)
    assert g.posterior_info["failed"] == 2 and g.posterior_info["used"] == 4
    assert np.array_equal(g.posterior_info["failed_draws"], [1, 4]) and np.all(np.isfinite(ym)) and np.all(np.isfinite(yv))
    # the same as a trace without them
    keep = [0, 2, 3, 5]
    g2, _ = _fitted()
    from andvaranaut_amd.nuts import Trace

    flat = {k: v.reshape((-1,) + v.shape[2:])[keep][None] for k, v in tr.posterior.items()}
    ym2, yv2 = g2.predict_posterior(xs, Trace(flat, {}), return_var=True)
    assert np.allclose(ym, ym2, rtol=1e-14, atol=0) and np.allclose(yv, yv2, rtol=1e-13, atol=0)
    g.gp.bad = list(thetas)
    with pytest.raises(FloatingPointError):
        g.predict_posterior(xs, tr)


@pytest.mark.parametrize("mean", [0, lambda xx: np.array([0.3 * xx[0] - 0.1])])
def test_one_distinct_draw_collapses_to_predict_and_the_mixture_is_the_gh_average(mean):
    from andvaranaut_amd.nuts import Trace

    g, rng = _fitted(mean=mean)
    g.yopt = 2.0
    xs = np.column_stack([rng.uniform(0, 2, 9), rng.uniform(1, 1.5, 9)])
    one = Trace({k: np.broadcast_to(np.asarray(v), (3, 2) + np.shape(v)).copy() for k, v in g.hypers.items()}, {})
    for kw in ({}, {"normvar": True}, {"EI": True, "EIopt": "max"}, {"EI": True, "EIopt": "min"}, {"revert": False}):
        ym, yv = g.predict(xs, return_var=True, **kw)
        pm, pv = g.predict_posterior(xs, one, return_var=True, **kw)
        assert np.allclose(pm, ym, rtol=1e-14, atol=0) and np.allclose(pv, yv, rtol=1e-14, atol=0), kw
    # several draws: the average of predict() at each draw's hypers (reverted moments), variance by the second moments
    tr = _trace(2, 3, seed=7)
    flat = {k: v.reshape((-1,) + v.shape[2:]) for k, v in tr.posterior.items()}
    m1, m2 = [], []
    for i in range(6):
        g.hypers = {k: v[i] for k, v in flat.items()}
        a, b = g.predict(xs, return_var=True)
        m1.append(a[:, 0])
        m2.append(b[:, 0] + a[:, 0] ** 2)
    pm, pv = g.predict_posterior(xs, tr, return_var=True)
    rm = np.mean(m1, axis=0)
    assert np.allclose(pm[:, 0], rm, rtol=1e-13, atol=0)
    assert np.allclose(pv[:, 0], np.mean(m2, axis=0) - rm ** 2, rtol=1e-9, atol=0)
