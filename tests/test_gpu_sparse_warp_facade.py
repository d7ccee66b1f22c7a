"""GPMCMC.fit(method="map", inducing=..., iwgp / cwgp) on the GPU: the device posterior and its gradient through the warps against
the NumPy stand-in of tests/sgpr_data_grad_ref.py, the fit end to end, and the refusals.

The comparison uses tests/test_gpu_facade.py's rule for the dense counterpart -- the value within 1e-9 relative, the gradient
within 1e-7 max(1, max|g|) -- or, where cond(Kuu) at the point makes it looser, sgpr_ref.tolerances' pair
(sgpr_data_grad_ref.warp_tolerances); the test prints which one held.  tests/test_sgpr_data_grad_host.py holds the CPU half: fp64
alone on the device's steps uses less than 0.001 of it at this point, at the start's own length scales (factor 1)."""
import pickle

import numpy as np
import pytest

import sgpr_data_grad_ref as DR
from test_sgpr_data_grad_host import LS_FACTOR_300, warp_setup

pytestmark = pytest.mark.gpu

N, M = 300, 40
WARPS = [(False, True), (True, False), (True, True)]


def _target(x):
    return np.array([np.exp(1.5 * np.sin(2 * x[0] ** 1.5) + x[1] ** 2)])  # _warped_problem's, at module level: it pickles


def _problem():
    from test_gpu_facade import _warped_problem

    g, fun = _warped_problem(n=N)
    g.target = _target
    return g, fun


@pytest.mark.parametrize("iwgp,cwgp", WARPS)
def test_device_posterior_and_gradient_through_the_warps_against_the_stand_in(iwgp, cwgp):
    from andvaranaut_amd.sparse import MiSparseGP

    g, model, _, _, q, (x, y, xin0, yin0, zin0, zraw) = warp_setup(iwgp, cwgp, n=N, m=M, ls_factor=LS_FACTOR_300)
    _, _, exact, lik_ld, _, _ = warp_setup(iwgp, cwgp, n=N, m=M, ls_factor=LS_FACTOR_300, precise=True)
    gp = MiSparseGP(xin0, yin0, zin0, "Matern52", device=0, z_grad=iwgp, data_grad=True)
    try:
        lik_d = g._warp_likelihood(gp, x, y, xin0, iwgp, cwgp, zraw=zraw)
        vd, gd = model.logp_dlogp(q, None, jacobian=False, likelihood=lik_d)
        vd2, gd2 = model.logp_dlogp(q, None, jacobian=False, likelihood=lik_d)
    finally:
        gp.close()
    vr, gr = model.logp_dlogp(q, None, jacobian=False, likelihood=lik_ld)
    ev, eg, which = DR.warp_errors(vd, gd, vr, gr, exact.cond)
    print((iwgp, cwgp), "cond(Kuu) = %.2e" % exact.cond, "value %.3e, gradient %.3e of the tolerance" % (ev, eg), which)
    assert ev <= 1.0 and eg <= 1.0, (ev, eg)
    assert vd2 == vd and np.array_equal(gd2, gd)


@pytest.mark.parametrize("iwgp,cwgp", WARPS)
def test_warped_sparse_map_fit_installs_the_warps_and_leaves_the_reconverted_data_on_the_device(iwgp, cwgp):
    from andvaranaut_amd.priors import HyperModel
    from andvaranaut_amd.sparse import MiSparseGP
    from andvaranaut_amd.transform import wgp

    g, fun = _problem()
    try:
        # the same sparse fit without warps, and the warped one started from it
        d0 = g.fit(method="map", inducing=M, inducing_seed=3, return_data=True)
        raw0 = g.inducing_raw.copy()
        # the plain fit's optimum as a point of the warped model (the warps at their starting parameters), and its logp THERE:
        # the warped posterior is a density of the raw y and carries the priors of the warp parameters, so it differs from the
        # plain fit's logp by the warp's Jacobian sum(log y') and those priors -- constants of the plain fit.  With the output
        # warp the plain figure itself is no yardstick: on the CPU stand-in it is 1179.2 against 620.0 for the same point in
        # the warped model, which the warped fit raises to 671.7
        n_i, n_pos, n_free = g._warp_sizes(iwgp, cwgp)
        model = HyperModel(2, ["Matern52"], noise=True, n_iwgp=n_i, n_cwgp_pos=n_pos, n_cwgp=n_free)
        start = {**model.point_dict(model.initial_point()), **g.hypers}
        x, y = g.x.copy(), (g.y - g.ym).copy()
        xin0, yin0 = g._converted(x, y)
        gp0 = MiSparseGP(xin0, yin0, g.inducing, "Matern52", device=0, z_grad=iwgp, data_grad=True)
        try:
            lik0 = g._warp_likelihood(gp0, x, y, xin0, iwgp, cwgp, zraw=raw0)
            v0 = model.logp_dlogp(model.q_from_point(start), None, jacobian=False, likelihood=lik0)[0]
        finally:
            gp0.close()
        d1 = g.fit(method="map", inducing=M, inducing_seed=3, iwgp=iwgp, cwgp=cwgp, start=start, return_data=True)
        print((iwgp, cwgp), "plain: logp = %.6f (nfev %d), %.6f as a point of the warped model; warped: logp = %.6f (nfev %d), %s"
              % (d0["logp"], d0["nfev"], v0, d1["logp"], d1["nfev"], d1["message"]))
        assert "CONVERGENCE" in str(d1["message"]), d1
        assert d1["logp"] >= v0  # L-BFGS-B keeps the best point seen, and it starts at the plain fit's optimum
        if not cwgp:
            assert d1["logp"] >= d0["logp"]  # without an output warp the two are densities of the same converted y
        keys = set(g.hypers)
        assert ("iwgp" in keys) == iwgp and ("cwgp" in keys and "cwgp_pos" in keys) == cwgp
        if iwgp:
            assert isinstance(g.xconrevs[0], wgp) and np.allclose(g.xconrevs[0].params, g.hypers["iwgp"])
        if cwgp:
            assert np.allclose(np.asarray(g.yconrevs[0].params, dtype=float),
                               g._cwgp_params(np.atleast_1d(g.hypers["cwgp_pos"]), np.atleast_1d(g.hypers["cwgp"])))
        # the device holds the re-conversions, and the stored points are the raw ones under the fitted warps
        assert isinstance(g.gp, MiSparseGP)
        xin, yin = g._converted(g.x, g.y - g.ym)
        zin = np.column_stack([g.xconrevs[i].con(g.inducing_raw[:, i]) for i in range(2)])
        assert np.array_equal(g.inducing_raw, raw0) and np.array_equal(d1["inducing_raw"], raw0)
        assert all(any((z == r).all() for r in g.x) for z in g.inducing_raw)  # an int picks data rows
        assert np.array_equal(g.inducing, zin) and np.array_equal(d1["inducing"], zin)
        assert np.array_equal(g.gp.X_t.cpu().numpy(), xin) and np.array_equal(g.gp.y_t.cpu().numpy(), yin)
        assert np.array_equal(g.gp.Z_t.cpu().numpy(), zin)
        # predict works unchanged, on this object and on a pickled copy that rebuilds the device object
        xt = np.random.default_rng(5).uniform([0, 1], [2, 1.5], (60, 2))
        yt = np.array([fun(r) for r in xt])
        yp, yv = g.predict(xt, return_var=True)
        rel = np.sqrt(np.mean(((yp - yt) / yt) ** 2))
        print((iwgp, cwgp), "relative rms error of the prediction = %.4f" % rel)
        assert yp.shape == (60, 1) and np.all(np.isfinite(yp)) and np.all(yv > 0)
        h = pickle.loads(pickle.dumps(g))
        assert h.gp is None and np.array_equal(h.inducing, g.inducing) and np.array_equal(h.inducing_raw, g.inducing_raw)
        yp2, yv2 = h.predict(xt, return_var=True)
        assert np.array_equal(yp2, yp) and np.array_equal(yv2, yv)
        h.change_model()
    finally:
        g.change_model()


def test_an_array_of_raw_inducing_points_is_kept_as_passed():
    g, _ = _problem()
    try:
        raw = g.x[::7][:M].copy() + 1e-3
        d = g.fit(method="map", inducing=raw, cwgp=True, maxeval=40, return_data=True)
        assert np.array_equal(g.inducing_raw, raw) and np.array_equal(d["inducing_raw"], raw)
        assert np.array_equal(g.inducing, np.column_stack([g.xconrevs[i].con(raw[:, i]) for i in range(2)]))
    finally:
        g.change_model()


def test_refusals_come_before_any_device_call():
    import scipy.stats as st

    from andvaranaut_amd import GPMCMC, normal, uniform

    g, _ = _problem()
    for kw, why in ((dict(iwgp=True, optimize_inducing=True), "optimize_inducing"), (dict(cwgp=True, optimize_inducing=True), "optimize_inducing"),
                    (dict(iwgp=True, method="none"), "no warps"), (dict(cwgp=True, method="mcmc_mean"), "no warps"),
                    (dict(iwgp=True, cwgp=True, method="mcmc_map"), "no warps"), (dict(iwgp=True, objective="loo"), "no warps"),
                    (dict(cwgp=True, trend="constant"), "no warps"), (dict(method="mcmc_mean"), "no sampler")):
        with pytest.raises(ValueError, match="inducing") as e:
            g.fit(inducing=M, **kw)
        assert why in str(e.value), (kw, str(e.value))
    assert g.gp is None and g.hypers is None
    # warps asked of an object that has none to fit: ValueError under inducing, the dense path's plain Exception without
    priors = [st.uniform(loc=0, scale=2), st.uniform(loc=1, scale=0.5)]
    h = GPMCMC(kernel="Matern52", noise=True, xconrevs=[uniform(priors[0]), normal(priors[1])], yconrevs=[None], nx=2, ny=1,
               priors=priors, target=lambda x: np.array([x[0] + x[1]]), parallel=False, nproc=1, verbose=False)
    h.sample(nsamps=60, seed=1)
    for kw, why in ((dict(iwgp=True), "xconrevs"), (dict(cwgp=True), "yconrevs")):
        with pytest.raises(ValueError, match="inducing") as e:
            h.fit(inducing=20, **kw)
        assert why in str(e.value)
        with pytest.raises(Exception, match="wgp") as e2:
            h.fit(**kw)
        assert not isinstance(e2.value, ValueError)
    assert h.gp is None and h.hypers is None
