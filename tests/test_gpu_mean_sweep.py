"""The matrix-free sweep of the posterior mean and its input gradient (option 53 of mi_gp_set_option, csrc/sweep_f64.hip) on
the device: every case of tests/mean_sweep_ref.py through MiGP.mean_sweep against the np.longdouble references, bound
(64 + 8 cond) eps sum |terms| (tests/test_mean_sweep_host.py validates references and bounds on the CPU); the bits of a point
do not depend on m, on its position or on a repetition; the raw C call's contract -- ignored arguments, NULL outputs, refusals;
and the facade's sensitivity methods on a small fit."""
import numpy as np
import pytest

import grad_refs as gr
import mean_sweep_ref as ms
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

IDS = [gr.case_id(c) for c in ms.CASES]


def _migp():
    import torch

    assert torch.cuda.is_available()
    from andvaranaut_amd import MiGP

    return MiGP


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("kernel,n,d", ms.CASES, ids=IDS)
def test_mean_sweep_every_case_against_longdouble(kernel, n, d):
    """mu and d mu of the 1000-point call at the reference points: error / bound <= 1 where alpha_reference vouches for the
    reference's alpha (printed otherwise); exact zeros where every term lies far below the subnormals.  The calls with the
    first m points, m = 1 .. 257, a repetition and the mean-only call return the same bits, and so does point 777 alone."""
    MiGP = _migp()
    case = ms.case_data(kernel, n, d)
    X, y, theta, Xn = case["X"], case["y"], case["theta"], case["Xn"]
    gp = MiGP(X, y, kernel)
    try:
        mu, dmu = gp.mean_sweep(theta, Xn, grad=True)
        assert gp.get_option(53) == 0
        again = gp.mean_sweep(theta, Xn, grad=True)
        only = gp.mean_sweep(theta, Xn)
        chunked = gp.mean_sweep(theta, Xn, grad=True, chunk=300)
        prefixes = {m: gp.mean_sweep(theta, Xn[:m], grad=True) for m in ms.M_VALUES[:-1]}
        alone = gp.mean_sweep(theta, Xn[777:778], grad=True)
    finally:
        gp.close()
    assert mu.shape == (1000,) and dmu.shape == (1000, d)
    assert np.isfinite(mu).all() and np.isfinite(dmu).all()
    assert _same_bits(mu, again[0]) and _same_bits(dmu, again[1]) and _same_bits(mu, only)
    assert _same_bits(mu, chunked[0]) and _same_bits(dmu, chunked[1])
    for m, (pm, pd) in prefixes.items():
        assert pm.shape == (m,) and pd.shape == (m, d)
        assert _same_bits(pm, mu[:m]) and _same_bits(pd, dmu[:m]), m
    assert _same_bits(alone[0], mu[777:778]) and _same_bits(alone[1], dmu[777:778])
    b_mu, b_dmu = ms.bounds(case)
    r_mu = gr.max_ratio(mu[ms.REF_POINTS], case["mu"], b_mu)
    r_dmu = gr.max_ratio(dmu[ms.REF_POINTS], case["dmu"], b_dmu)
    print(f"mean_sweep {kernel} n={n} d={d} cond={case['cond']:.0f}: mu error / bound {r_mu:.5f}, d mu error / bound {r_dmu:.5f} "
          f"({'asserted' if case['ok'] else 'not asserted'}: the reference alpha's own diagonal residue is {case['alpha_ratio']:.4f} "
          "of its allowance)")
    gone = ms.LD(ms.TINY) * ms.LD(2.0) ** -64
    assert (mu[ms.REF_POINTS][case["mag_mu"] < gone] == 0.0).all() and (dmu[ms.REF_POINTS][case["mag_dmu"] < gone] == 0.0).all()
    assert (r_mu <= 1.0 and r_dmu <= 1.0) or not case["ok"], (r_mu, r_dmu)


def _raw(gp, x_t, m, mean_t, dmean_t, work_t=None, var_t=None, dvar_t=None, ldw=0):
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    return gp.lib.mi_gp_predict_grad(gp.h, p(x_t), m, p(work_t), ldw, p(mean_t), p(var_t), 1, p(dmean_t), p(dvar_t))


def test_raw_call_ignores_work_and_variance_and_takes_null_outputs():
    """mi_gp_predict_grad under option 53 = 1: work_dev / var_dev / dvar_dev full of NaN change nothing and stay NaN; dmean_dev =
    NULL and mean_dev = NULL each work, both NULL is refused; behind the sweep, with the option back at 0, predict_grad returns
    the bits it returned before."""
    MiGP = _migp()
    kernel, n, d = "Matern52+RBF", 300, 5
    X, y = ms.problem(n, d, seed=11)
    theta = gr.well_conditioned_theta(kernel, d)
    Xn = np.random.default_rng(5).random((70, d))
    m = Xn.shape[0]
    gp = MiGP(X, y, kernel)
    try:
        before = gp.predict_grad(theta, Xn[:9])
        ref_mu, ref_dmu = gp.mean_sweep(theta, Xn, grad=True)
        x_t = _dev(Xn)
        work = _dev(np.full((256, gp.lda), np.nan))
        var, dvar = _dev(np.full(m, np.nan)), _dev(np.full((m, d), np.nan))
        mean, dmean = _dev(np.full(m, -77.5)), _dev(np.full((m, d), -77.5))
        gp.set_option(53, 1)
        assert gp.get_option(53) == 1
        assert _raw(gp, x_t, m, mean, dmean, work, var, dvar, gp.lda) == 0, gp.last_error()
        assert _same_bits(_host(mean), ref_mu) and _same_bits(_host(dmean), ref_dmu)
        assert np.isnan(_host(work)).all() and np.isnan(_host(var)).all() and np.isnan(_host(dvar)).all()
        mean2, dmean2 = _dev(np.full(m, -77.5)), _dev(np.full((m, d), -77.5))
        assert _raw(gp, x_t, m, mean2, None) == 0, gp.last_error()
        assert _raw(gp, x_t, m, None, dmean2) == 0, gp.last_error()
        assert _same_bits(_host(mean2), ref_mu) and _same_bits(_host(dmean2), ref_dmu)
        assert _raw(gp, x_t, m, None, None) == -1 and "option 53" in gp.last_error()
        gp.set_option(53, 0)
        after = gp.predict_grad(theta, Xn[:9], refactor=False)
        assert all(_same_bits(a, b) for a, b in zip(before, after))
        after = gp.predict_grad(theta, Xn[:9])
        assert all(_same_bits(a, b) for a, b in zip(before, after))
    finally:
        gp.close()


def test_refusals_return_minus_one_with_a_text_and_change_nothing():
    MiGP = _migp()
    kernel, n, d = "Matern32", 140, 3
    X, y = ms.problem(n, d, seed=3)
    theta = gr.well_conditioned_theta(kernel, d)
    Xn = np.random.default_rng(6).random((12, d))
    x_t = _dev(Xn)
    mean, dmean = _dev(np.full(12, -77.5)), _dev(np.full((12, d), -77.5))

    def refused(gp, m=12, words=("option 53",)):
        assert _raw(gp, x_t, m, mean, dmean) == -1
        text = gp.last_error()
        assert all(w in text for w in words), text
        assert gp.get_option(53) == 1
        assert (_host(mean) == -77.5).all() and (_host(dmean) == -77.5).all()

    gp = MiGP(X, y, kernel)
    try:
        gp.set_option(53, 1)
        refused(gp, words=("option 53", "mi_gp_factor"))  # before mi_gp_factor
        gp.set_option(53, 0)
        mu, dmu = gp.mean_sweep(theta, Xn, grad=True)
        gp.set_option(53, 1)
        refused(gp, m=0)
        assert gp.lib.mi_gp_set_option(gp.h, 53, 2) == -1 and "option 53" in gp.last_error() and gp.get_option(53) == 1
        assert gp.lib.mi_gp_set_option(gp.h, 53, -1) == -1 and gp.get_option(53) == 1
        # (none of these refusals touched the resident state: the same call, the same bits)
        assert _raw(gp, x_t, 12, mean, dmean) == 0, gp.last_error()
        assert _same_bits(_host(mean), mu) and _same_bits(_host(dmean), dmu)
        mean.fill_(-77.5)
        dmean.fill_(-77.5)
        gp.set_option(50, 1)  # (ends the resident state itself, as mi_gp_set_data does)
        refused(gp, words=("option 53", "option 50"))
        gp.set_option(50, 0)
        gp.set_option(51, 2)
        refused(gp, words=("option 53", "option 51"))
        gp.set_option(51, 1)
        gp.set_option(53, 0)
        assert gp.factor(theta) == 0  # (options 50 and 51 ended the resident state)
        mu2, dmu2 = gp.mean_sweep(theta, Xn, grad=True)
        assert _same_bits(mu2, mu) and _same_bits(dmu2, dmu)
    finally:
        gp.close()
    gp = MiGP(X, y, kernel, need_grad=False)
    try:
        assert gp.factor(theta) == 0
        gp.set_option(53, 1)
        refused(gp, words=("option 53", "Z_dev"))
        gp.set_option(53, 0)
        with pytest.raises(RuntimeError):
            gp.mean_sweep(theta, Xn)
        assert gp.get_option(53) == 0
    finally:
        gp.close()
    X9, y9 = ms.problem(6, 129, seed=4)
    gp = MiGP(X9, y9, "RBF")
    try:
        assert gp.factor(gr.well_conditioned_theta("RBF", 129)) == 0
        gp.set_option(53, 1)
        x9 = _dev(np.random.default_rng(7).random((12, 129)))
        assert gp.lib.mi_gp_predict_grad(gp.h, x9.data_ptr(), 12, None, 0, mean.data_ptr(), None, 0, None, None) == -1
        assert "option 53" in gp.last_error() and "128" in gp.last_error()
        assert (_host(mean) == -77.5).all()
    finally:
        gp.close()


def test_python_refusals_under_a_trend_and_several_outputs():
    MiGP = _migp()
    X, y = ms.problem(40, 2, seed=1)
    theta = gr.well_conditioned_theta("RBF", 2)
    gp = MiGP(X, y, "RBF")
    try:
        gp.set_trend("constant")
        with pytest.raises(ValueError, match="has no form under a trend"):
            gp.mean_sweep(theta, X)
        gp.set_trend("none")
        gp.set_outputs(np.stack([y, y * y], axis=1))
        with pytest.raises(ValueError, match="has no form under several outputs"):
            gp.mean_sweep(theta, X)
        gp.set_outputs(y)
        with pytest.raises(ValueError):
            gp.mean_sweep(theta, X[:, :1])
        assert gp.get_option(53) == 0
        assert gp.mean_sweep(theta, X).shape == (40,)
    finally:
        gp.close()


def test_sweep_sees_the_points_of_an_append_across_a_tile_boundary():
    """120 points, then 20 appended (n crosses 128): the sweep of the grown handle against a fresh handle on all 140 points -- the
    same sums over the same points, alpha from another factorisation: (64 + 8 cond) eps sum |terms|, and against the reference."""
    MiGP = _migp()
    kernel, d = "Matern52", 3
    X, y = ms.problem(140, d, seed=9)
    theta = gr.well_conditioned_theta(kernel, d)
    Xn = np.random.default_rng(8).random((33, d))
    gp = MiGP(X[:120], y[:120], kernel, capacity=200)
    try:
        short = gp.mean_sweep(theta, Xn)
        assert gp.append(X[120:], y[120:]) == 0 and gp.n == 140
        mu, dmu = gp.mean_sweep(theta, Xn, grad=True)
    finally:
        gp.close()
    alpha, cond, ok, _ = gr.alpha_reference(X, y, kernel, theta, Xn)
    assert ok
    ref_mu, mag_mu = ms.mean_reference(X, kernel, theta, Xn, alpha)
    ref_dmu, mag_dmu = gr.predict_grad_reference(X, kernel, theta, Xn, alpha)
    r_mu = gr.max_ratio(mu, ref_mu, gr.sum_bound(mag_mu, extra=8.0 * cond))
    r_dmu = gr.max_ratio(dmu, ref_dmu, gr.sum_bound(mag_dmu, extra=8.0 * cond))
    print(f"append 120 + 20: mu error / bound {r_mu:.5f}, d mu error / bound {r_dmu:.5f}")
    assert r_mu <= 1.0 and r_dmu <= 1.0
    assert not _same_bits(short, mu)  # (the 120-point conditional is another function)


# ----------------------------------------------------------------------------------------------------------------- facade
@pytest.fixture(scope="module")
def fitted():
    """The 150-point 2-D fit of tests/test_gpu_kfold.py."""
    import scipy.stats as st

    from andvaranaut_amd import GPMCMC, normal, uniform
    from andvaranaut_amd.transform import logarithm

    priors = [st.uniform(loc=0, scale=2), st.norm(loc=1.25, scale=0.08)]
    fun = lambda x: np.array([x[0] ** 2 - x[0] - x[1] ** 2 * x[0] + x[1] + 3.0])  # noqa: E731
    g = GPMCMC(kernel="RBF", noise=True, xconrevs=[uniform(priors[0]), normal(priors[1])], yconrevs=[logarithm()], nx=2, ny=1,
               priors=priors, target=fun, verbose=False)
    g.sample(nsamps=150, seed=5)
    g.fit(method="map")
    return g


def test_facade_mean_gradient_active_subspace_sobol_and_y_dist(fitted):
    """predict_mean(revert=False) and its gradient against oracle.predict / oracle.predict_grad at kfold_ref.tolerances(cond);
    active_subspace(x=Xs) is active_subspace_from_gradients of those gradients; sobol_indices is sobol_from_evaluations of the
    oracle's means on the same design within the tolerance of the means propagated through the estimators (first order in the
    means' error, doubled for the higher orders); y_dist(mean_only=True) is predict_mean on the same sample."""
    import kfold_ref as ref
    from andvaranaut_amd import sensitivity as sens
    from andvaranaut_amd.lhc import latin_sample

    g = fitted
    theta = g._theta_from_hypers(g.hypers, 1e-6)
    cond = ref.full_cond(g.xc, "RBF", theta)
    vtol, _ = ref.tolerances(cond)
    yc = g.yc[:, 0]
    Xs = latin_sample(g.priors, 40, 3)
    Xc, _ = g._converted_x(Xs, True)
    mu, grad = g.predict_mean(Xc, convert=False, revert=False, return_grad=True)
    rmu, _ = orc.predict(g.xc, yc, Xc, ["RBF"], [], theta)
    rdmu, _ = orc.predict_grad(g.xc, yc, Xc, ["RBF"], [], theta)
    e_mu = np.max(np.abs(mu[:, 0] - rmu) / np.maximum(np.abs(rmu), 1.0)) / vtol
    e_g = np.max(np.abs(grad - rdmu)) / max(np.abs(rdmu).max(), 1.0) / vtol
    print(f"facade: cond {cond:.3g}, mean error / tolerance {e_mu:.4f}, gradient error / tolerance {e_g:.4f}")
    assert mu.shape == (40, 1) and grad.shape == (40, 2)
    assert e_mu <= 1.0 and e_g <= 1.0
    # the original space: the chain rule through both conversions, against central differences of predict_mean itself
    y0, g0 = g.predict_mean(Xs, return_grad=True)
    assert _same_bits(y0, g.predict_mean(Xs)) and _same_bits(y0[:, 0], g.yconrevs[0].rev(mu[:, 0]))
    for i in range(2):
        h = 1e-5
        xp, xm = Xs.copy(), Xs.copy()
        xp[:, i] += h
        xm[:, i] -= h
        fd = (g.predict_mean(xp)[:, 0] - g.predict_mean(xm)[:, 0]) / (2 * h)
        assert np.abs(fd - g0[:, i]).max() <= 1e-5 * max(np.abs(g0[:, i]).max(), 1.0), i
    # active subspace
    out = g.active_subspace(x=Xs)
    assert _same_bits(out["grads"], grad) and _same_bits(out["x"], Xs)
    lam, V, Cm, dgsm = sens.active_subspace_from_gradients(grad)
    assert _same_bits(out["eigenvalues"], lam) and _same_bits(out["eigenvectors"], V) and _same_bits(out["C"], Cm)
    assert _same_bits(out["dgsm"], dgsm)
    assert set(out) == {"eigenvalues", "eigenvectors", "C", "dgsm", "x", "grads"}
    # Sobol indices on the design the facade draws
    M = 128
    sob = g.sobol_indices(nsamps=M, seed=11, revert=False)
    sa, sb = np.random.SeedSequence(11).spawn(2)
    A, B = latin_sample(g.priors, M, np.random.default_rng(sa)), latin_sample(g.priors, M, np.random.default_rng(sb))
    D = sens.saltelli_design(A, B)
    Dc, _ = g._converted_x(D, True)
    f, _ = orc.predict(g.xc, yc, Dc, ["RBF"], [], theta)
    fA, fB, fAB = sens.split_saltelli(f, 2)
    first, total, mean, var = sens.sobol_from_evaluations(fA, fB, fAB)
    delta = vtol * max(np.abs(f).max(), 1.0)
    dvar = 4.0 * delta * np.abs(f).max()
    t_first = 2.0 * (delta * (np.mean(np.abs(fAB - fA), axis=1) + 2.0 * np.mean(np.abs(fB))) + np.abs(first) * dvar) / var
    t_total = 2.0 * (2.0 * delta * np.mean(np.abs(fA - fAB), axis=1) + np.abs(total) * dvar) / var
    print(f"facade Sobol: first {sob['first']} (oracle {first}, tolerance {t_first}), total {sob['total']} (oracle {total}, "
          f"tolerance {t_total})")
    assert set(sob) == {"first", "total", "mean", "var"}
    assert (np.abs(sob["first"] - first) <= t_first).all() and (np.abs(sob["total"] - total) <= t_total).all()
    assert abs(sob["mean"] - mean) <= 2.0 * delta and abs(sob["var"] - var) <= 2.0 * dvar
    # y_dist
    xs, ys = g.y_dist(nsamps=50, return_data=True, seed=2, mean_only=True)
    assert _same_bits(ys, g.predict_mean(xs)) and ys.shape == (50, 1)
    xs2, ys2 = g.y_dist(nsamps=50, return_data=True, seed=2)
    assert _same_bits(xs, xs2) and not _same_bits(ys, ys2)  # (the default route is predict's Gauss-Hermite mean)


def test_facade_refusals(fitted):
    g = fitted
    x = g.x[:3]
    g.trend = "constant"
    try:
        with pytest.raises(ValueError, match="has no form under trend"):
            g.predict_mean(x)
    finally:
        g.trend = None
    g.outputs = "all"
    try:
        with pytest.raises(ValueError, match="has no form under outputs='all'"):
            g.predict_mean(x)
    finally:
        g.outputs = "first"
    mean = g.mean
    g.mean = lambda v: np.array([1.0])
    try:
        with pytest.raises(ValueError, match="non-zero mean function"):
            g.predict_mean(x, return_grad=True)
    finally:
        g.mean = mean
    with pytest.raises(ValueError):
        g.active_subspace(x=x, space="nowhere")
