"""MiGP.append / mi_gp_append: conditioning a resident conditional-form factorisation on new points at fixed theta, against
the NumPy oracle of the concatenated data and against a fresh handle on all n + k points."""
import numpy as np
import pytest

from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

D = 3


def _kern(kernel):
    kerns = kernel.replace("*", "+").split("+")
    return kerns, [c for c in kernel if c in "+*"]


def _theta(kernel, noise):
    return orc.synth_theta(D, nkern=len(_kern(kernel)[0]), gv=1e-2 if noise else 0.0, jitter=1e-6)


def _cond(K, theta):
    """cond(K): exact up to 1200 points, else the Gershgorin bound over the noise floor (gv + jitter)."""
    if K.shape[0] <= 1200:
        return np.linalg.cond(K)
    return np.abs(K).sum(1).max() / (theta[-1] + theta[-2])


def _close(a, b, tol):
    return np.max(np.abs(a - b)) <= tol * max(np.max(np.abs(b)), 1.0)


@pytest.mark.parametrize("noise", [True, False])
@pytest.mark.parametrize("kernel", ["RBF", "Matern52", "RBF+Matern32"])
@pytest.mark.parametrize("n0", [100, 128, 1000, 4095, 4096])
def test_append_parity_grid(n0, kernel, noise):
    from andvaranaut_amd import MiGP

    kerns, ops = _kern(kernel)
    theta = _theta(kernel, noise)
    Xall, yall = orc.synth_problem(n0 + 128, D, seed=n0 + 3)
    Xs = np.random.default_rng(n0).random((37, D))
    for k in (1, 7, 28, 128):
        X, y = Xall[: n0 + k], yall[: n0 + k]
        fresh = MiGP(X, y, kernel, device=0)
        assert fresh.factor(theta) == 0
        ref = {"p": fresh.predict(theta, Xs, via_inverse=False), "u": fresh.predict(theta, Xs, via_inverse=True),
               "g": fresh.predict_grad(theta, Xs, refactor=False)}
        fresh.close()
        K = orc.noisy_cov(X, kerns, ops, theta, form="conditional")
        _, L, beta = orc.lml(X, y, kerns, ops, theta, form="conditional", return_parts=True)
        logdet, quad = np.sum(np.log(np.diag(L))), beta @ beta
        cond = _cond(K, theta)
        tol = max(1e-10, 20.0 * cond * 2.2e-16)
        ptol = max(1e-10, 200.0 * cond * 2.2e-16)
        for with_u in (True, False):
            gp = MiGP(X[:n0], y[:n0], kernel, device=0, capacity=n0 + k)
            assert gp.factor(theta) == 0
            if with_u:  # U = L^-T resident: the append extends it
                gp.predict(theta, Xs, via_inverse=True)
            K0 = gp.K_t[:n0, : gp.np_].cpu().numpy().copy()
            assert gp.append(X[n0:], y[n0:]) == 0
            assert gp.n == n0 + k and gp.append_refactors == 0
            assert np.array_equal(gp.K_t[:n0, : K0.shape[1]].cpu().numpy(), K0), (n0, k, kernel, noise)
            ld, q = gp.lml_parts()
            assert abs(ld - logdet) <= tol * max(abs(logdet), 1.0), (n0, k, kernel, noise, ld, logdet)
            assert abs(q - quad) <= tol * max(abs(quad), 1.0), (n0, k, kernel, noise, q, quad)
            got_p = gp.predict(theta, Xs, via_inverse=False)
            got_u = gp.predict(theta, Xs, via_inverse=True)
            got_g = gp.predict_grad(theta, Xs, refactor=False)
            assert gp.append_refactors == 0
            for a, b in zip(got_p, ref["p"]):
                assert _close(a, b, ptol), (n0, k, kernel, noise, with_u)
            for a, b in zip(got_u, ref["u"]):
                assert _close(a, b, ptol), (n0, k, kernel, noise, with_u)
            for a, b in zip(got_g, ref["g"]):
                assert _close(a, b, 10 * ptol), (n0, k, kernel, noise, with_u)
            gp.close()


def test_sequence_of_appends_matches_one_factorisation():
    from andvaranaut_amd import MiGP

    X, y = orc.synth_problem(380, D, seed=11)
    theta = _theta("Matern52", True)
    Xs = np.random.default_rng(1).random((37, D))
    gp = MiGP(X[:250], y[:250], "Matern52", device=0, capacity=380)
    assert gp.factor(theta) == 0
    gp.predict(theta, Xs, via_inverse=True)
    for i in range(10):
        assert gp.append(X[250 + 13 * i : 263 + 13 * i], y[250 + 13 * i : 263 + 13 * i]) == 0
    assert gp.n == 380 and gp.append_refactors == 0
    fresh = MiGP(X, y, "Matern52", device=0)
    assert fresh.factor(theta) == 0
    for via in (False, True):
        for a, b in zip(gp.predict(theta, Xs, via_inverse=via), fresh.predict(theta, Xs, via_inverse=via)):
            assert _close(a, b, 1e-10)
    for a, b in zip(gp.lml_parts(), fresh.lml_parts()):
        assert abs(a - b) <= 1e-10 * max(abs(b), 1.0)
    gp.close()
    fresh.close()


def test_append_at_65_tile_columns_runs_the_tail_segment():
    """n0 = 8200 pads to 65 tile columns: L21 L21^T is cut into 32 segments of two tile columns and a TAIL of one, the second
    launch of gram_segments (csrc/api_gp.hip) that no smaller size reaches.  One append of 120 points to 8320 (65 tile columns
    still), compared as test_sequence_of_appends_matches_one_factorisation compares: against a fresh factorisation of all points
    on the device, through both prediction routes and the factorisation's parts."""
    from andvaranaut_amd import MiGP

    d, n0, n1 = 4, 8200, 8320
    X, y = orc.synth_problem(n1, d, seed=17)
    theta = orc.synth_theta(d, nkern=1, gv=1e-2, jitter=1e-6)
    Xs = np.random.default_rng(3).random((37, d))
    gp = MiGP(X[:n0], y[:n0], "Matern52", device=0, capacity=n1)
    assert gp.factor(theta) == 0
    gp.predict(theta, Xs, via_inverse=True)
    assert gp.append(X[n0:], y[n0:]) == 0
    assert gp.n == n1 and gp.append_refactors == 0
    fresh = MiGP(X, y, "Matern52", device=0)
    assert fresh.factor(theta) == 0
    for via in (False, True):
        for a, b in zip(gp.predict(theta, Xs, via_inverse=via), fresh.predict(theta, Xs, via_inverse=via)):
            print("via_inverse", via, "error / bound %.3g" % (np.max(np.abs(a - b)) / (1e-10 * max(np.max(np.abs(b)), 1.0))))
            assert _close(a, b, 1e-10)
    for a, b in zip(gp.lml_parts(), fresh.lml_parts()):
        print("part error / bound %.3g" % (abs(a - b) / (1e-10 * max(abs(b), 1.0))))
        assert abs(a - b) <= 1e-10 * max(abs(b), 1.0)
    gp.close()
    fresh.close()


def test_capacity_overflow_refactorises_once_with_the_same_results():
    from andvaranaut_amd import MiGP

    X, y = orc.synth_problem(300, D, seed=5)
    theta = _theta("RBF", True)
    Xs = np.random.default_rng(2).random((20, D))
    gp = MiGP(X[:200], y[:200], "RBF", device=0)  # no capacity: the first append grows the buffers
    assert gp.factor(theta) == 0
    assert gp.append(X[200:210], y[200:210]) == 0
    assert gp.append_refactors == 1 and gp.n == 210
    cap = gp.capacity
    assert gp.append(X[210:300], y[210:300]) == 0
    assert gp.n == 300 and gp.capacity >= 300 and gp.append_refactors == (1 if cap >= 300 else 2)
    fresh = MiGP(X, y, "RBF", device=0)
    assert fresh.factor(theta) == 0
    for a, b in zip(gp.predict(theta, Xs), fresh.predict(theta, Xs)):
        assert _close(a, b, 1e-10)
    gp.close()
    fresh.close()


def test_non_positive_definite_append_leaves_the_handle_unchanged():
    from andvaranaut_amd import MiGP

    X, y = orc.synth_problem(150, D, seed=9)
    theta = orc.synth_theta(D, gv=0.0, jitter=0.0)
    theta[0:D] = 0.05  # short length-scales: K is positive definite without any noise
    Xs = np.random.default_rng(3).random((16, D))
    gp = MiGP(X, y, "Matern52", device=0, capacity=200)
    gp.set_diag(np.zeros(150))
    assert gp.factor(theta) == 0
    before = gp.predict(theta, Xs, via_inverse=False)
    K0 = gp.K_t.cpu().numpy().copy()
    parts = gp.lml_parts()
    # a duplicate of point 17 without noise: its Schur complement is 0 up to rounding of either sign; the diagonal entry of
    # -1e-8 makes the sign certain
    info = gp.append(X[[17]], y[[17]], diag=[-1e-8])
    assert info == 151, info
    assert gp.n == 150
    assert np.array_equal(gp.K_t.cpu().numpy(), K0)
    assert gp.lml_parts() == parts
    after = gp.predict(theta, Xs, via_inverse=False)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    gp.close()


def test_evaluations_at_a_new_theta_after_an_append():
    from andvaranaut_amd import MiGP

    X, y = orc.synth_problem(333, D, seed=21)
    theta = _theta("RBF+Matern32", True)
    theta2 = theta.copy()
    theta2[:D] *= 1.3
    gp = MiGP(X[:300], y[:300], "RBF+Matern32", device=0, capacity=333)
    assert gp.factor(theta) == 0
    assert gp.append(X[300:], y[300:]) == 0
    fresh = MiGP(X, y, "RBF+Matern32", device=0)
    assert abs(gp.lml(theta2) - fresh.lml(theta2)) <= 1e-12 * abs(fresh.lml(theta2))
    (v, g), (rv, rg) = gp.lml_grad(theta2), fresh.lml_grad(theta2)
    assert abs(v - rv) <= 1e-12 * abs(rv) and np.allclose(g, rg, rtol=1e-12, atol=1e-12 * np.abs(rg).max())
    th = np.stack([theta, theta2])
    assert np.allclose(gp.lml_batch(th), fresh.lml_batch(th), rtol=1e-12, atol=0)
    _, _, gy, gx = gp.lml_grad_data(theta2)
    _, _, ry, rx = fresh.lml_grad_data(theta2)
    assert gy.shape == (333,) and np.allclose(gy, ry, rtol=1e-10, atol=1e-10 * np.abs(ry).max())
    assert np.allclose(gx, rx, rtol=1e-9, atol=1e-9 * np.abs(rx).max())
    gp.close()
    fresh.close()


def test_batch_calls_are_refused_until_the_batch_is_bound_again():
    from andvaranaut_amd import MiGP
    import ctypes

    X, y = orc.synth_problem(140, D, seed=4)
    theta = _theta("RBF", True)
    gp = MiGP(X[:120], y[:120], "RBF", device=0, capacity=140)
    gp.lml_batch(np.stack([theta, theta]))
    assert gp.factor(theta) == 0
    assert gp.append(X[120:], y[120:]) == 0
    th = np.ascontiguousarray(np.stack([theta, theta]))
    out = np.empty(2)
    dpt = ctypes.POINTER(ctypes.c_double)
    # the C-ABI refuses (the caller's batch buffers are sized for 120 points) ...
    assert gp.lib.mi_gp_lml_batch(gp.h, 2, th.ctypes.data_as(dpt), out.ctypes.data_as(dpt), None) == -1
    # ... and the facade binds new ones
    ref = MiGP(X, y, "RBF", device=0)
    assert np.allclose(gp.lml_batch(th), ref.lml_batch(th), rtol=1e-12, atol=0)
    gp.close()
    ref.close()


def test_appended_diagonal_is_honoured():
    from andvaranaut_amd import MiGP

    X, y = orc.synth_problem(230, D, seed=8)
    diag = np.random.default_rng(4).uniform(1e-3, 1e-1, 230)
    theta = _theta("RBF", True)
    Xs = np.random.default_rng(5).random((12, D))
    gp = MiGP(X[:200], y[:200], "RBF", device=0, capacity=230)
    gp.set_diag(diag[:200])
    assert gp.factor(theta) == 0
    with pytest.raises(ValueError):
        gp.append(X[200:], y[200:])  # a diagonal is set: its new entries are required
    assert gp.append(X[200:], y[200:], diag=diag[200:]) == 0
    fresh = MiGP(X, y, "RBF", device=0)
    fresh.set_diag(diag)
    assert fresh.factor(theta) == 0
    for a, b in zip(gp.predict(theta, Xs), fresh.predict(theta, Xs)):
        assert _close(a, b, 1e-10)
    for a, b in zip(gp.lml_parts(), fresh.lml_parts()):
        assert abs(a - b) <= 1e-10 * max(abs(b), 1.0)
    _, L, beta = orc.lml(X, y, ["RBF"], [], theta, form="conditional", return_parts=True, extra_diag=diag)
    assert abs(gp.lml_parts()[1] - beta @ beta) <= 1e-9 * beta @ beta
    gp.close()
    fresh.close()


def test_bo_refit_every_appends_between_fits(monkeypatch):
    import scipy.stats as st

    from andvaranaut_amd import GPMCMC, MiGP, normal, uniform

    priors = [st.uniform(loc=0, scale=2), st.norm(loc=1.25, scale=0.08)]
    fun = lambda x: np.array([x[0] ** 2 - x[0] - x[1] ** 2 * x[0] + x[1] + 3.0])  # noqa: E731
    g = GPMCMC(kernel="RBF", noise=True, xconrevs=[uniform(priors[0]), normal(priors[1])], yconrevs=[None], nx=2, ny=1,
               priors=priors, target=fun, verbose=False)
    g.sample(nsamps=30, seed=3)
    g.fit(method="map")
    hypers = {k: np.copy(v) for k, v in g.hypers.items()}
    calls = []
    monkeypatch.setattr(GPMCMC, "fit", lambda self, *a, **kw: calls.append(1))
    n0 = len(g.x)
    np.random.seed(1)
    g.BO(opt_type="min", opt_method="predict", method="EI", max_iter=4, predict_samps=500, refine=False, conv=0.0,
         refit_every=4)
    assert len(calls) == 1  # the last iteration's refit only
    assert len(g.x) == n0 + 4 and g.gp.n == n0 + 3  # three points appended, the fourth waits for the (patched) refit
    for k in hypers:
        assert np.array_equal(g.hypers[k], hypers[k])
    xin, yin = g._converted(g.x[: n0 + 3], (g.y - g.ym)[: n0 + 3])
    fresh = MiGP(xin, yin, g.kernel, device=0)
    Xs = np.column_stack([np.random.default_rng(7).uniform(0, 2, 25), np.random.default_rng(8).normal(1.25, 0.08, 25)])
    mu, var = g.predict(Xs, return_var=True, revert=False)
    xs_c = np.column_stack([g.xconrevs[i].con(Xs[:, i]) for i in range(2)])
    rmu, rvar = fresh.predict(g._theta_from_hypers(g.hypers, 1e-6), xs_c, pred_noise=True)
    assert _close(mu[:, 0], rmu, 1e-10) and _close(yv := var[:, 0], rvar, 1e-10), (mu[:, 0] - rmu, yv - rvar)
    fresh.close()
    with pytest.raises(ValueError):
        g.BO(max_iter=1, refit_every=0)
    with pytest.raises(ValueError):
        g.BO(max_iter=1, refit_every=2, iwgp=True)
