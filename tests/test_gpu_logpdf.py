"""MiGP.logpdf / mi_gp_logpdf: the joint log predictive density of trial points given the resident factorisation, and its
gradients w.r.t. the trial inputs and outputs, against the NumPy oracle of the concatenated data (tests/logpdf_ref.py), against
mi_gp_append (whose phase 1 it shares), and through the facade (GPMCMC.log_predictive, inverse_opt(resident=True)).

Tolerances are those of tests/test_gpu_append.py: the value within max(1e-10, 20 cond(K_J) eps) of max(|ref|, 1), gradients
within ten times max(1e-10, 200 cond eps) of the largest reference entry."""
import ctypes

import numpy as np
import pytest
import scipy.stats as st

import logpdf_ref as ref
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

EPS = 2.2e-16
KMAX = 128


def _theta(kernel, d, gv, jitter=1e-6):
    kerns, _ = ref.split_kernel(kernel)
    theta = orc.synth_theta(d, nkern=len(kerns), gv=gv, jitter=jitter)
    for c, name in enumerate(kerns):
        if name == "RatQuad":
            theta[len(kerns) * d + len(kerns) + c] = 2.5  # (a shape parameter that is not the neutral 1)
    return theta


def _tols(cond):
    return max(1e-10, 20.0 * cond * EPS), 10.0 * max(1e-10, 200.0 * cond * EPS)


def _check(got, want, cond, what):
    """value and gradients of one logpdf call against the reference; the figures go to the captured output first"""
    vtol, gtol = _tols(cond)
    (v, dX, dy), (rv, rX, ry) = got, want
    ev = abs(v - rv) / max(abs(rv), 1.0)
    print(what, "cond %.3g value err %.3g (tol %.3g)" % (cond, ev, vtol), end="")
    assert ev <= vtol, (what, v, rv, ev, vtol)
    if dX is not None:
        ex = np.max(np.abs(dX - rX)) / np.max(np.abs(rX))
        ey = np.max(np.abs(dy - ry)) / np.max(np.abs(ry))
        print(" dX err %.3g dy err %.3g (tol %.3g)" % (ex, ey, gtol), end="")
        assert ex <= gtol, (what, ex, gtol)
        assert ey <= gtol, (what, ey, gtol)
    print()


# ------------------------------------------------------------------------------------------------------------ parity grid
@pytest.mark.parametrize("d", [3, 17])
@pytest.mark.parametrize("kernel", ["RBF", "Matern52", "RBF*Matern32+RatQuad"])
@pytest.mark.parametrize("n0", [100, 128, 300])
def test_logpdf_parity_grid(n0, kernel, d):
    from andvaranaut_amd import MiGP

    Xall, yall = orc.synth_problem(n0 + KMAX, d, seed=n0 + d)
    dall = np.random.default_rng(n0).uniform(1e-3, 1e-1, n0 + KMAX)
    X, y = Xall[:n0], yall[:n0]
    for with_diag in (False, True):
        gp = MiGP(X, y, kernel, device=0)
        if with_diag:
            gp.set_diag(dall[:n0])
        for gv in (1e-2, 0.0):
            theta = _theta(kernel, d, gv)
            for k in (1, 7, KMAX):
                Xn, yn = Xall[n0 : n0 + k], yall[n0 : n0 + k]
                d0, d1 = (dall[:n0], dall[n0 : n0 + k]) if with_diag else (None, None)
                rv, rX, ry, _ = ref.logpdf_ref(X, y, Xn, yn, kernel, theta, d0, d1)
                cond = ref.joint_cond(X, Xn, kernel, theta, d0, d1)
                what = "n0=%d %s d=%d diag=%d gv=%g k=%d" % (n0, kernel, d, with_diag, gv, k)
                assert gp.factor(theta) == 0  # (drops U: the next calls run without it resident beforehand)
                _check(gp.logpdf(theta, Xn, yn, diag=d1, grad=False), (rv, None, None), cond, what + " value, no U:")
                _check(gp.logpdf(theta, Xn, yn, diag=d1), (rv, rX, ry), cond, what + " grad, no U before:")
                _check(gp.logpdf(theta, Xn, yn, diag=d1), (rv, rX, ry), cond, what + " grad, U resident:")
                _check(gp.logpdf(theta, Xn, yn, diag=d1, grad=False), (rv, None, None), cond, what + " value, U resident:")
        gp.close()


# ------------------------------------------------------------------------------------------------ consistency with append
@pytest.mark.parametrize("with_u", [False, True])
def test_logpdf_then_append_of_the_same_points(with_u):
    from andvaranaut_amd import MiGP

    n0, k, d, kernel = 300, 28, 3, "Matern52"
    X, y = orc.synth_problem(n0 + k, d, seed=17)
    theta = _theta(kernel, d, 1e-2)
    Xs = np.random.default_rng(4).random((37, d))
    cond = ref.joint_cond(X[:n0], X[n0:], kernel, theta)
    vtol, _ = _tols(cond)
    ptol = max(1e-10, 200.0 * cond * EPS)
    rv, _, _, (rlogdet, rquad) = ref.logpdf_ref(X[:n0], y[:n0], X[n0:], y[n0:], kernel, theta, grad=False)
    gp = MiGP(X[:n0], y[:n0], kernel, device=0, capacity=n0 + k)
    assert gp.factor(theta) == 0
    v, _, _ = gp.logpdf(theta, X[n0:], y[n0:], grad=with_u)  # (a gradient call leaves U resident for the append)
    ld0, q0 = gp.lml_parts()
    assert gp.append(X[n0:], y[n0:]) == 0
    ld1, q1 = gp.lml_parts()
    print("increments", ld1 - ld0, q1 - q0, "reference", rlogdet, rquad, "value", v, rv)
    assert abs((ld1 - ld0) - rlogdet) <= vtol * max(abs(ld1), 1.0)
    assert abs((q1 - q0) - rquad) <= vtol * max(abs(q1), 1.0)
    got = -0.5 * (q1 - q0) - (ld1 - ld0) - 0.5 * k * np.log(2.0 * np.pi)
    assert abs(v - got) <= vtol * max(abs(v), 1.0), (v, got)
    assert abs(v - rv) <= vtol * max(abs(rv), 1.0), (v, rv)
    fresh = MiGP(X, y, kernel, device=0)
    assert fresh.factor(theta) == 0
    for a, b in zip(gp.predict(theta, Xs, via_inverse=False), fresh.predict(theta, Xs, via_inverse=False)):
        assert np.max(np.abs(a - b)) <= ptol * max(np.max(np.abs(b)), 1.0)
    gp.close()
    fresh.close()


# ------------------------------------------------------------------------------------------------------------------ state
def _state(gp, theta, Xs):
    mu, var = gp.predict(theta, Xs, via_inverse=False)
    cmu, cov = gp.predict_cov(theta, Xs)
    return [mu, var, cmu, cov, np.array(gp.lml_parts()), gp.K_t[: gp.n, : gp.np_].cpu().numpy()]


def test_logpdf_leaves_the_handle_as_it_was_and_is_reproducible():
    import torch

    from andvaranaut_amd import MiGP

    n0, k, d, kernel = 300, 7, 17, "RBF*Matern32+RatQuad"
    X, y = orc.synth_problem(n0 + k, d, seed=23)
    theta = _theta(kernel, d, 1e-2)
    Xs = np.random.default_rng(6).random((20, d))
    Xn, yn = X[n0:], y[n0:]
    gp = MiGP(X[:n0], y[:n0], kernel, device=0)
    assert gp.factor(theta) == 0
    before = _state(gp, theta, Xs)
    v0 = gp.logpdf(theta, Xn, yn, grad=False)[0]
    for a, b in zip(before, _state(gp, theta, Xs)):
        assert np.array_equal(a, b)
    g0 = gp.logpdf(theta, Xn, yn)
    for a, b in zip(before, _state(gp, theta, Xs)):
        assert np.array_equal(a, b)
    # the same query in the same resident state: the same bits, whatever the work block held
    g1 = gp.logpdf(theta, Xn, yn)
    gp._lwork.fill_(float("nan"))
    torch.cuda.synchronize()
    g2 = gp.logpdf(theta, Xn, yn)
    gp._lwork.zero_()
    torch.cuda.synchronize()
    g3 = gp.logpdf(theta, Xn, yn)
    for g in (g1, g2, g3):
        assert g[0] == g0[0] and np.array_equal(g[1], g0[1]) and np.array_equal(g[2], g0[2])
    # either gradient alone: the same bits, the other output untouched; and the phase timers of a profiled call are filled
    r, v, dx, dy = _raw_call(gp, Xn, yn, None, k, dy=False)
    assert r == 0 and v == g0[0] and np.array_equal(dx, g0[1]) and np.all(dy == -7.25)
    r, v, dx, dy = _raw_call(gp, Xn, yn, None, k, dx=False)
    assert r == 0 and v == g0[0] and np.array_equal(dy, g0[2]) and np.all(dx == -7.25)
    gp.set_profiling(1)
    g4 = gp.logpdf(theta, Xn, yn)
    tm = gp.timers()
    assert g4[0] == g0[0] and np.array_equal(g4[1], g0[1])
    assert tm["logpdf_block_ms"] > 0.0 and tm["logpdf_weights_ms"] > 0.0 and tm["logpdf_grad_ms"] > 0.0
    assert gp.logpdf(theta, Xn, yn, grad=False)[0] == g0[0]
    tm = gp.timers()
    assert tm["logpdf_block_ms"] > 0.0 and tm["logpdf_weights_ms"] == 0.0 and tm["logpdf_grad_ms"] == 0.0
    gp.set_profiling(0)
    # ... and the value-only call without U resident
    assert gp.factor(theta) == 0
    gp._lwork.fill_(float("nan"))
    torch.cuda.synchronize()
    assert gp.logpdf(theta, Xn, yn, grad=False)[0] == v0
    # with and without U the value agrees to rounding
    cond = ref.joint_cond(X[:n0], Xn, kernel, theta)
    assert abs(v0 - g0[0]) <= _tols(cond)[0] * max(abs(v0), 1.0)
    gp.close()


# ------------------------------------------------------------------------------------------------ coincident trial points
@pytest.mark.parametrize("kernel", ["Matern52", "Exponential"])
def test_coincident_trial_points(kernel):
    from andvaranaut_amd import MiGP

    n0, d = 150, 3
    X, y = orc.synth_problem(n0, d, seed=31)
    theta = _theta(kernel, d, 1e-2)
    d0 = np.full(n0, 1e-3)
    Xn = np.tile(np.array([[0.31, 0.62, 0.47]]), (3, 1))  # three rows at one x
    yn = np.array([0.2, 0.25, 0.15])
    d1 = np.array([1e-2, 2e-2, 3e-2])
    gp = MiGP(X, y, kernel, device=0)
    gp.set_diag(d0)
    got = gp.logpdf(theta, Xn, yn, diag=d1)
    assert np.isfinite(got[0]) and np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    rv, rX, ry, _ = ref.logpdf_ref(X, y, Xn, yn, kernel, theta, d0, d1)
    _check(got, (rv, rX, ry), ref.joint_cond(X, Xn, kernel, theta, d0, d1), kernel + " coincident:")
    # a trial point on top of a training point as well
    Xn2 = np.vstack([X[[17]], X[[17]]])
    got = gp.logpdf(theta, Xn2, yn[:2], diag=d1[:2])
    rv, rX, ry, _ = ref.logpdf_ref(X, y, Xn2, yn[:2], kernel, theta, d0, d1[:2])
    _check(got, (rv, rX, ry), ref.joint_cond(X, Xn2, kernel, theta, d0, d1[:2]), kernel + " on a training point:")
    gp.close()


# ------------------------------------------------------------------------------------------------------- indefinite block
def _raw_call(gp, Xn, yn, dn, k, ldw=None, dx=True, dy=True, work=None):
    """mi_gp_logpdf on device tensors: (return value, logp, dx tensor, dy tensor), the outputs pre-filled with a sentinel"""
    import torch

    dev = gp.dev
    xn = torch.from_numpy(np.ascontiguousarray(Xn)).to(dev)
    yt = torch.from_numpy(np.ascontiguousarray(yn)).to(dev)
    dt = torch.from_numpy(np.ascontiguousarray(dn)).to(dev) if dn is not None else None
    ldw = gp.lda if ldw is None else ldw
    if work is None:
        work = torch.empty(max(int(gp.lib.mi_gp_logpdf_work(gp.lda)), 1), dtype=torch.float64, device=dev)
    dxt = torch.full((max(k, 1), gp.d), -7.25, dtype=torch.float64, device=dev)
    dyt = torch.full((max(k, 1),), -7.25, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    out = ctypes.c_double(123.0)
    r = gp.lib.mi_gp_logpdf(gp.h, xn.data_ptr(), yt.data_ptr(), dt.data_ptr() if dt is not None else None, k, work.data_ptr(), ldw,
                            ctypes.byref(out), dxt.data_ptr() if dx else None, dyt.data_ptr() if dy else None)
    torch.cuda.synchronize(dev)
    return r, out.value, dxt.cpu().numpy(), dyt.cpu().numpy()


def test_indefinite_trial_block_is_reported_and_nothing_is_written():
    from andvaranaut_amd import MiGP

    X, y = orc.synth_problem(150, 3, seed=9)
    theta = orc.synth_theta(3, gv=0.0, jitter=0.0)
    theta[0:3] = 0.05  # short length-scales: K is positive definite without any noise
    Xs = np.random.default_rng(3).random((16, 3))
    gp = MiGP(X, y, "Matern52", device=0, capacity=200)
    gp.set_diag(np.zeros(150))
    assert gp.factor(theta) == 0
    before = _state(gp, theta, Xs)
    K0 = gp.K_t.cpu().numpy().copy()
    # a duplicate of point 17 without noise: its Schur complement is 0 up to rounding; the diagonal entry of -1e-8 makes the
    # sign certain (the construction of test_non_positive_definite_append_leaves_the_handle_unchanged)
    for grad in (False, True):
        r, v, dx, dy = _raw_call(gp, X[[17]], y[[17]], np.array([-1e-8]), 1, dx=grad, dy=grad)
        assert r == 151, r
        assert v == -np.inf
        assert np.all(dx == -7.25) and np.all(dy == -7.25)
        assert b"not positive definite" in gp.lib.mi_gp_last_error(gp.h)
        assert np.array_equal(gp.K_t.cpu().numpy(), K0)
        for a, b in zip(before, _state(gp, theta, Xs)):
            assert np.array_equal(a, b)
    # the facade: -inf with zero gradients
    v, dX, dyv = gp.logpdf(theta, X[[17]], y[[17]], diag=[-1e-8])
    assert v == -np.inf and gp.info == 151 and not dX.any() and not dyv.any()
    # the handle still appends
    assert gp.append(X[[17]] + 0.01, y[[17]], diag=[1e-3]) == 0
    gp.close()


# --------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    from andvaranaut_amd import MiGP

    X, y = orc.synth_problem(140, 3, seed=4)
    theta = _theta("RBF", 3, 1e-2)
    Xn, yn = X[:KMAX] + 0.003, y[:KMAX]
    gp = MiGP(X, y, "RBF", device=0)

    def refused(text, *a, **kw):
        r, v, dx, dy = _raw_call(gp, *a, **kw)
        err = gp.lib.mi_gp_last_error(gp.h)
        assert r == -1 and b"mi_gp_logpdf" in err and text in err, (r, err)
        assert v == 123.0 and np.all(dx == -7.25) and np.all(dy == -7.25)

    refused(b"mi_gp_factor", Xn[:3], yn[:3], None, 3)  # before factor
    assert gp.factor(theta) == 0
    refused(b"1 <= k <= 128", Xn[:1], yn[:1], None, 0)
    Xbig, ybig = np.vstack([Xn, Xn[:1]]), np.r_[yn, yn[:1]]
    refused(b"1 <= k <= 128", Xbig, ybig, None, 129)
    refused(b"ldw", Xn[:3], yn[:3], None, 3, ldw=gp.np_ + 1)  # odd
    refused(b"ldw", Xn[:3], yn[:3], None, 3, ldw=gp.np_ - 2)  # short
    refused(b"diagonal", Xn[:3], yn[:3], np.full(3, 1e-3), 3)  # no diagonal is set
    gp.set_diag(np.full(140, 1e-3))
    assert gp.factor(theta) == 0
    refused(b"diagonal", Xn[:3], yn[:3], None, 3)  # one is set
    assert _raw_call(gp, Xn[:3], yn[:3], np.full(3, 1e-3), 3)[0] == 0
    with pytest.raises(ValueError):
        gp.logpdf(theta, Xn[:3], yn[:3])
    with pytest.raises(ValueError):
        gp.logpdf(theta, Xbig, ybig, diag=np.full(129, 1e-3))
    gp.close()
    # gradients need Z / W
    gp = MiGP(X, y, "RBF", device=0, need_grad=False)
    assert gp.factor(theta) == 0
    refused(b"Z_dev", Xn[:3], yn[:3], None, 3)
    refused(b"Z_dev", Xn[:3], yn[:3], None, 3, dx=False)  # dy alone is a gradient too
    r, v, _, _ = _raw_call(gp, Xn[:3], yn[:3], None, 3, dx=False, dy=False)
    assert r == 0 and np.isfinite(v)
    with pytest.raises(RuntimeError):
        gp.logpdf(theta, Xn[:3], yn[:3])
    assert np.isfinite(gp.logpdf(theta, Xn[:3], yn[:3], grad=False)[0])
    gp.close()


# ----------------------------------------------------------------------------------------------------------------- facade
def _fitted(n, ycon=None, seed=5):
    from andvaranaut_amd import GPMCMC, normal, uniform

    priors = [st.uniform(loc=0, scale=2), st.norm(loc=1.25, scale=0.08)]
    fun = lambda x: np.array([x[0] ** 2 - x[0] - x[1] ** 2 * x[0] + x[1] + 3.0])  # noqa: E731
    g = GPMCMC(kernel="RBF", noise=True, xconrevs=[uniform(priors[0]), normal(priors[1])], yconrevs=[ycon], nx=2, ny=1,
               priors=priors, target=fun, verbose=False)
    g.sample(nsamps=n, seed=seed)
    g.fit(method="map")
    return g, fun


def test_log_predictive_of_held_out_points():
    from andvaranaut_amd.transform import logarithm

    g, fun = _fitted(60, ycon=logarithm())
    rng = np.random.default_rng(12)
    x = np.column_stack([rng.uniform(0, 2, 20), rng.normal(1.25, 0.08, 20)])
    yv = np.array([fun(r)[0] for r in x]) * (1.0 + 0.01 * rng.standard_normal(20))
    got = g.log_predictive(x, yv)
    xc = np.column_stack([g.xconrevs[j].con(x[:, j]) for j in range(2)])
    theta = g._theta_from_hypers(g.hypers, 1e-6)
    rv, _, _, _ = ref.logpdf_ref(g.xc, g.yc[:, 0], xc, np.log(yv), "RBF", theta, grad=False)
    want = rv + np.sum(np.log(1.0 / yv))
    cond = ref.joint_cond(g.xc, xc, "RBF", theta)
    print("log_predictive", got, want, "cond", cond)
    assert abs(got - want) <= _tols(cond)[0] * max(abs(want), 1.0), (got, want)
    assert got == g.log_predictive(x, yv.reshape(-1, 1))
    with pytest.raises(ValueError):
        g.log_predictive(np.tile(x, (7, 1)), np.tile(yv, 7))  # 140 points


XS_FIXED = np.array([[0.4, 1.2], [0.9, 1.3], [1.3, 1.26], [1.6, 1.18], [1.05, 1.33]])


def _captured_potential(g, monkeypatch, yobs, yvarobs, resident):
    """inverse_opt's potential at XS_FIXED: _drive_input_model is replaced by an evaluation at those points"""
    from andvaranaut_amd import GPMCMC

    seen = []

    def drive(self, imodel, potential, method, **kwargs):
        seen.extend(potential(x) for x in XS_FIXED)
        return {"x0": 1.0, "x1": 1.25}, None

    monkeypatch.setattr(GPMCMC, "_drive_input_model", drive)
    g.inverse_opt(yobs, yvarobs=yvarobs, method="map", resident=resident)
    monkeypatch.undo()
    return np.array([v for v, _ in seen]), np.array([gr for _, gr in seen])


@pytest.fixture(scope="module")
def fitted150():
    return _fitted(150)


@pytest.mark.parametrize("nobs", [1, 3])
def test_inverse_opt_resident_potential_equals_the_refactorising_one(fitted150, monkeypatch, nobs):
    g, fun = fitted150
    xtrue = np.array([1.4, 1.27])
    yobs = np.array([fun(xtrue)[0] * (1.0 + 0.002 * i) for i in range(nobs)])
    yvarobs = np.full((nobs, 1), 1e-4)
    v0, g0 = _captured_potential(g, monkeypatch, yobs, yvarobs, False)
    v1, g1 = _captured_potential(g, monkeypatch, yobs, yvarobs, True)
    # the joint covariance of the potential at each x: training rows + nobs rows at x, inverse_opt's diagonal
    theta = g._theta_from_hypers(g.hypers, 0.0)
    theta[-2] = 0.0
    n = g.nsamp
    diag = np.r_[np.full(n, np.sqrt(float(np.atleast_1d(g.hypers["gv"])[0]) + 1e-6)),
                 np.full(nobs, np.sqrt(g._gh_stats_inv(yobs.reshape(-1, 1), yvarobs)))]
    cond = 0.0
    for x in XS_FIXED:
        xin = np.array([[g.xconrevs[j].con(np.array([x[j]]))[0] for j in range(2)]])
        cond = max(cond, ref.joint_cond(g.xc, np.tile(xin, (nobs, 1)), "RBF", theta, diag[:n], diag[n:]))
    vtol, gtol = _tols(cond)
    ev = np.max(np.abs(v1 - v0) / np.maximum(np.abs(v0), 1.0))
    eg = np.max(np.abs(g1 - g0), axis=1) / np.max(np.abs(g0), axis=1)
    print("nobs", nobs, "cond %.3g" % cond, "value err %.3g (tol %.3g)" % (ev, vtol), "grad err", eg, "(tol %.3g)" % gtol)
    assert np.isfinite(v0).all() and np.isfinite(v1).all()
    assert ev <= vtol
    assert np.all(eg <= gtol)


def test_inverse_opt_resident_map_reaches_the_same_optimum(fitted150, monkeypatch):
    from andvaranaut_amd.consumers import InputModel, pymc_prior

    g, fun = fitted150
    yobs = np.array([fun(np.array([1.4, 1.27]))[0]])
    yvarobs = np.array([[1e-4]])
    im0 = InputModel([pymc_prior(p, allow_truncnorm=True) for p in g.priors])
    monkeypatch.setattr(np.random, "normal", lambda size=None: im0.q_from_x([1.3, 1.26]))  # the MAP run's start
    _, x0 = g.inverse_opt(yobs, yvarobs=yvarobs, method="map")
    _, x1 = g.inverse_opt(yobs, yvarobs=yvarobs, method="map", resident=True)
    print("optimum", x0, x1, "difference", np.abs(x1 - x0))
    assert np.max(np.abs(x1 - x0)) <= 1e-6, (x0, x1)
