"""Posterior predictive over hyper-parameter draws (mi_gp_factor_batch / mi_gp_predict_batch, MiGP.predict_batch,
GPMCMC.predict_posterior): every draw's rows equal mi_gp_factor + mi_gp_predict bit for bit, the oracle per draw, the
mixture NumPy's two-pass mixture of the same moments, a non-positive-definite draw is NaN and left out, the handle's other
state is untouched, and the facade collapses to predict() for a trace of one distinct draw."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _mods():
    import torch

    assert torch.cuda.is_available()
    from andvaranaut_amd import MiGP
    from oracle import gp_oracle as orc

    return MiGP, orc


def _split(kernel):
    return kernel.replace("*", "+").split("+"), [c for c in kernel if c in "+*"]


def _thetas(orc, d, nk, k, seed, ratquad=False):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        th = orc.synth_theta(d, nkern=nk, gv=10.0 ** rng.uniform(-4.5, -2.5))
        th[: nk * d] *= rng.uniform(0.7, 1.5, nk * d)
        th[nk * d: nk * d + nk] *= rng.uniform(0.8, 1.3, nk)
        if ratquad:
            th[nk * d + nk: nk * d + 2 * nk] = rng.uniform(0.5, 3.0, nk)
        out.append(th)
    return np.array(out)


def _mixture(mu, var):
    """NumPy's two-pass equal-weight mixture of the rows of mu / var."""
    mm = mu.mean(axis=0)
    return mm, var.mean(axis=0) + ((mu - mm) ** 2).mean(axis=0)


def _problem(orc, N, d, kernel, k, m, seed):
    X, y = orc.synth_problem(N, d, seed=seed)
    kerns, ops = _split(kernel)
    th = _thetas(orc, d, len(kerns), k, seed=seed + 1, ratquad="RatQuad" in kernel)
    Xs = np.random.default_rng(seed + 2).random((m, d))
    return X, y, kerns, ops, th, Xs


# N: both sides of the two-stream threshold (2100: two streams from the start); m = 1, 200, 1000; k = 1, 3, 8
BIT_CASES = [(128, 2, "RBF", 1, 1), (300, 3, "Matern52", 3, 200), (1000, 4, "RBF+Matern32", 8, 1000),
             (2100, 4, "Matern52*RBF", 3, 1000), (1000, 3, "RatQuad", 3, 200), (5000, 6, "Matern52", 3, 1000),
             (300, 2, "RBF", 8, 1), (2100, 5, "RBF", 8, 200), (128, 3, "RatQuad", 8, 1000)]


@pytest.mark.parametrize("N,d,kernel,k,m", BIT_CASES)
def test_every_draw_equals_factor_plus_predict_bit_for_bit(N, d, kernel, k, m):
    MiGP, orc = _mods()
    X, y, kerns, ops, th, Xs = _problem(orc, N, d, kernel, k, m, seed=N + k + m)
    gp = MiGP(X, y, kernel)
    mu, var, mm, mv = gp.predict_batch(th, Xs)
    assert mu.shape == (k, m) and var.shape == (k, m) and mm.shape == (m,) and mv.shape == (m,)
    assert np.all(gp.batch_info == 0)
    for p in range(k):
        assert gp.factor(th[p]) == 0
        one_mu, one_var = gp.predict(th[p], Xs, via_inverse=False)
        assert np.array_equal(mu[p], one_mu) and np.array_equal(var[p], one_var), p
    # several draw-chunks: the same rows, the chunks' mixtures combined on the host
    mu2, var2, mm2, mv2 = gp.predict_batch(th, Xs, max_batch=2)
    assert np.array_equal(mu2, mu) and np.array_equal(var2, var)
    rm, rv = _mixture(mu, var)
    assert np.allclose(mm2, rm, rtol=1e-13, atol=0) and np.allclose(mv2, rv, rtol=1e-13, atol=0)
    gp.close()


def test_the_solve_on_128x128_tiles_and_point_chunks():
    """m = 7680 at N = 5000: the single solve's GEMMs run on 128x128 tiles with a 64x64 tail, so the batched ones take that
    form too; point chunks of 3000 (the last one partial) give the same rows."""
    MiGP, orc = _mods()
    X, y, kerns, ops, th, Xs = _problem(orc, 5000, 4, "RBF", 3, 7680, seed=11)
    gp = MiGP(X, y, "RBF", need_grad=False)
    mu, var, mm, mv = gp.predict_batch(th, Xs)
    for p in range(3):
        gp.factor(th[p])
        one_mu, one_var = gp.predict(th[p], Xs)
        assert np.array_equal(mu[p], one_mu) and np.array_equal(var[p], one_var), p
    mu2, var2, mm2, mv2 = gp.predict_batch(th, Xs, chunk=3000)
    assert np.array_equal(mu2, mu) and np.array_equal(var2, var)
    assert np.array_equal(mm2, mm) and np.array_equal(mv2, mv)
    gp.close()


@pytest.mark.parametrize("N,d,kernel,k,m", [(300, 3, "Matern52", 3, 129), (1000, 4, "Matern32+RBF", 8, 1000),
                                            (700, 3, "RatQuad", 3, 300), (2048, 8, "RBF", 3, 300)])
def test_draws_and_mixture_match_the_oracle(N, d, kernel, k, m):
    MiGP, orc = _mods()
    X, y, kerns, ops, th, Xs = _problem(orc, N, d, kernel, k, m, seed=3 * N + k)
    gp = MiGP(X, y, kernel, need_grad=False)
    for pred_noise in (True, False):
        mu, var, mm, mv = gp.predict_batch(th, Xs, pred_noise=pred_noise)
        refs = [orc.predict(X, y, Xs, kerns, ops, th[p], pred_noise=pred_noise) for p in range(k)]
        rmu, rvar = np.array([r[0] for r in refs]), np.array([r[1] for r in refs])
        assert np.allclose(mu, rmu, rtol=1e-9, atol=1e-9)
        assert np.allclose(var, rvar, rtol=1e-8, atol=1e-11)
        dm, dv = _mixture(mu, var)  # the device's own per-draw moments
        assert np.allclose(mm, dm, rtol=1e-13, atol=0) and np.allclose(mv, dv, rtol=1e-13, atol=0)
        om, ov = _mixture(rmu, rvar)  # the oracle's
        assert np.allclose(mm, om, rtol=1e-9, atol=1e-9) and np.allclose(mv, ov, rtol=1e-8, atol=1e-11)
    gp.close()


def test_a_non_positive_definite_draw_is_nan_and_left_out_of_the_mixture():
    MiGP, orc = _mods()
    X, y, kerns, ops, th, Xs = _problem(orc, 900, 3, "Matern52", 5, 300, seed=5)
    th[2, -1] = -10.0  # negative jitter: not positive definite
    gp = MiGP(X, y, "Matern52")
    mu, var, mm, mv = gp.predict_batch(th, Xs)
    assert gp.batch_info[2] > 0 and np.all(np.isnan(mu[2])) and np.all(np.isnan(var[2]))
    good = [0, 1, 3, 4]
    assert np.all(gp.batch_info[good] == 0)
    dm, dv = _mixture(mu[good], var[good])
    assert np.allclose(mm, dm, rtol=1e-13, atol=0) and np.allclose(mv, dv, rtol=1e-13, atol=0)
    for p in good:
        gp.factor(th[p])
        one_mu, one_var = gp.predict(th[p], Xs, via_inverse=False)
        assert np.array_equal(mu[p], one_mu) and np.array_equal(var[p], one_var), p
    # the same across draw-chunks, one of which has the bad draw
    mu2, var2, mm2, mv2 = gp.predict_batch(th, Xs, max_batch=2)
    assert np.array_equal(mu2[good], mu[good]) and np.all(np.isnan(mu2[2]))
    assert np.allclose(mm2, dm, rtol=1e-13, atol=0) and np.allclose(mv2, dv, rtol=1e-13, atol=0)
    # every draw bad: NaN mixture
    bad = th[[2, 2]]
    mu3, var3, mm3, mv3 = gp.predict_batch(bad, Xs)
    assert np.all(gp.batch_info > 0) and np.all(np.isnan(mm3)) and np.all(np.isnan(mv3))
    gp.close()


def test_single_state_and_the_other_batch_calls_are_untouched():
    MiGP, orc = _mods()
    X, y, kerns, ops, th, Xs = _problem(orc, 1000, 3, "RBF", 4, 200, seed=21)
    theta = orc.synth_theta(3, gv=1e-3)
    gp = MiGP(X, y, "RBF")
    m0, v0 = gp.predict(theta, Xs, via_inverse=False)
    gp.predict_batch(th, Xs)
    m1, v1 = gp.predict(theta, Xs, via_inverse=False)  # refactorises: the batch call took the single factor's state
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
    mu0, vu0 = gp.predict(theta, Xs, via_inverse=True)
    gp.factor_batch(th)
    mu1, vu1 = gp.predict(theta, Xs, via_inverse=True)
    assert np.array_equal(mu0, mu1) and np.array_equal(vu0, vu1)
    l0 = gp.lml_batch(th)
    g0 = gp.lml_grad_batch(th)
    gp.factor_batch(th[::-1].copy())
    assert np.array_equal(gp.lml_batch(th), l0)
    l1, gr1 = gp.lml_grad_batch(th)
    assert np.array_equal(l1, g0[0]) and np.array_equal(gr1, g0[1])
    # the predict half needs mi_gp_factor_batch as the last batch call, with the same k
    import ctypes

    work = gp._bwork
    out = gp._bK  # (any device memory: the call is refused before it is touched)
    r = gp.lib.mi_gp_predict_batch(gp.h, 4, out.data_ptr(), 1, work.data_ptr(), gp.lda, 128 * gp.lda, out.data_ptr(),
                                   out.data_ptr(), 1, None, None)
    assert r == -1 and b"mi_gp_factor_batch" in gp.lib.mi_gp_last_error(gp.h)
    info = np.zeros(4, dtype=np.int32)
    gp.lib.mi_gp_factor_batch(gp.h, 4, th.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                              info.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    r = gp.lib.mi_gp_predict_batch(gp.h, 3, out.data_ptr(), 1, work.data_ptr(), gp.lda, 128 * gp.lda, out.data_ptr(),
                                   out.data_ptr(), 1, None, None)
    assert r == -1 and b"factorised 4" in gp.lib.mi_gp_last_error(gp.h)
    gp.close()


# ---------------------------------------------------------------- facade
def _gpmcmc(n, seed):
    import scipy.stats as st

    from andvaranaut_amd import GPMCMC

    rng = np.random.default_rng(seed)
    priors = [st.uniform(loc=0, scale=2), st.uniform(loc=1, scale=0.5)]
    fun = lambda x: np.array([np.exp(np.sin(2 * x[0]) + x[1] ** 2)])  # noqa: E731
    x = np.column_stack([rng.uniform(0, 2, n), rng.uniform(1, 1.5, n)])
    y = np.array([fun(r) for r in x])
    g = GPMCMC(kernel="Matern52", noise=True, nx=2, ny=1, priors=priors, target=fun, verbose=False)
    g.set_data(x, y)
    return g, rng


def _constant_trace(hypers, chains=2, draws=3):
    from andvaranaut_amd.nuts import Trace

    post = {k: np.broadcast_to(np.asarray(v, dtype=np.float64), (chains, draws) + np.shape(v)).copy() for k, v in hypers.items()}
    return Trace(post, {"lp": np.zeros((chains, draws))})


def test_a_trace_of_one_distinct_draw_collapses_to_predict():
    """predict() at N = 100 and 30 points takes the blocked triangular solve (MiGP.predict: U = L^-T only from 3 m >= n or the
    third sweep at one theta), the algebra of the batched path: the unreverted moments are its bits."""
    g, rng = _gpmcmc(100, seed=4)
    g.fit(method="map")
    trace = _constant_trace(g.hypers)
    xs = np.column_stack([rng.uniform(0, 2, 30), rng.uniform(1, 1.5, 30)])
    g.yopt = float(np.median(g.y))
    ym, yv = g.predict(xs, return_var=True, revert=False)
    pm, pv = g.predict_posterior(xs, trace, return_var=True, revert=False)
    assert np.array_equal(pm, ym) and np.array_equal(pv, yv)
    assert g.posterior_info["used"] == 6 and g.posterior_info["failed"] == 0
    for kw in ({}, {"normvar": True}, {"EI": True, "EIopt": "max"}, {"EI": True, "EIopt": "min"}, {"deg": 5}):
        ym, yv = g.predict(xs, return_var=True, **kw)
        pm, pv = g.predict_posterior(xs, trace, return_var=True, **kw)
        assert np.allclose(pm, ym, rtol=1e-14, atol=0) and np.allclose(pv, yv, rtol=1e-14, atol=0), kw


def test_posterior_predictive_of_a_real_mcmc_fit_matches_a_host_recomputation():
    from oracle import gp_oracle as orc

    g, rng = _gpmcmc(100, seed=8)
    trace = g.fit(method="mcmc_mean", return_data=True, draws=50, tune=50, chains=2, random_seed=3)
    xs = np.column_stack([rng.uniform(0, 2, 30), rng.uniform(1, 1.5, 30)])
    pm, pv = g.predict_posterior(xs, trace, ndraws=20, return_var=True)
    assert g.posterior_info["failed"] == 0 and g.posterior_info["used"] == 20
    idx = g.posterior_info["draws"]
    assert np.array_equal(idx, (np.arange(20) * 100) // 20)
    # host: the oracle per draw, then the Gauss-Hermite mixture
    xin, yin = g._converted(g.x, g.y - g.ym)
    xcs = np.column_stack([g.xconrevs[i].con(xs[:, i]) for i in range(g.nx)])
    flat = {k: v.reshape((-1,) + v.shape[2:]) for k, v in trace.posterior.items()}
    xi, wi = np.polynomial.hermite.hermgauss(8)
    m1, m2 = [], []
    for i in idx:
        th = g._theta_from_hypers({k: v[i] for k, v in flat.items()}, 1e-6)
        mu, var = orc.predict(xin, yin, xcs, ["Matern52"], [], th)
        yi = g.yconrevs[0].rev(np.sqrt(2.0 * var)[:, None] * xi[None, :] + mu[:, None])
        m1.append((yi @ wi) / np.sqrt(np.pi))
        m2.append(((yi ** 2) @ wi) / np.sqrt(np.pi))
    m1, m2 = np.array(m1), np.array(m2)
    rm = m1.mean(axis=0)
    rv = m2.mean(axis=0) - rm ** 2
    assert np.allclose(pm[:, 0], rm, rtol=1e-8, atol=1e-10)
    assert np.allclose(pv[:, 0], rv, rtol=1e-6, atol=1e-9)
    # the unreverted mixture against the oracle's per-draw moments
    um, uv = g.predict_posterior(xs, trace, ndraws=20, return_var=True, revert=False)
    refs = [orc.predict(xin, yin, xcs, ["Matern52"], [], g._theta_from_hypers({k: v[i] for k, v in flat.items()}, 1e-6))
            for i in idx]
    om, ov = _mixture(np.array([r[0] for r in refs]), np.array([r[1] for r in refs]))
    assert np.allclose(um[:, 0], om, rtol=1e-9, atol=1e-9) and np.allclose(uv[:, 0], ov, rtol=1e-8, atol=1e-11)
    # the selection is deterministic: the same call twice gives the same bits, all draws differ from a subset
    pm2, pv2 = g.predict_posterior(xs, trace, ndraws=20, return_var=True)
    assert np.array_equal(pm2, pm) and np.array_equal(pv2, pv)
    pa = g.predict_posterior(xs, trace, ndraws=None)
    assert g.posterior_info["used"] == 100 and np.all(np.isfinite(pa))
