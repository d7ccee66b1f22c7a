"""The GP trend with marginalised coefficients (option 50 of mi_gp_set_option; MiGP.set_trend, GPMCMC.fit(trend=...)) against the
references of tests/trend_ref.py: the value of mi_gp_lml_grad against the projected-data definition, its gradient against the
forward mode on the projected data, mi_gp_factor + mi_gp_predict against Rasmussen & Williams eqs. 2.41-2.42 through dense solves;
then what the option must leave alone and what it refuses.

Bounds are the project's own, with cond = cond(K_y): loo_ref.value_ratio and loo_ref.grad_ratio for the objective,
kfold_ref.tolerances for the conditional's mean and variance.  Every parity check prints error / bound before it asserts."""
import ctypes
import os

import numpy as np
import pytest
import scipy.stats as st

import kfold_ref
import loo_ref
import trend_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_poison_lib = None


def _poison_scratch(gp):
    """NaN into ALL of the handle's trend scratch (tools/trend_poison.hip); the scratch must exist"""
    global _poison_lib
    if _poison_lib is None:
        path = os.path.join(ROOT, "tools", "libtrendpoison.so")
        assert os.path.exists(path), "tools/libtrendpoison.so missing: run __graft_entry__.build()"
        _poison_lib = ctypes.CDLL(path)
        _poison_lib.trend_poison.argtypes = [ctypes.c_void_p]
        _poison_lib.trend_poison.restype = ctypes.c_long
    assert _poison_lib.trend_poison(gp.h) > 0


def _gp(X, y, kernel, diag, trend=None, **kw):
    from andvaranaut_amd import MiGP

    gp = MiGP(X, y, kernel, device=0, **kw)
    if diag is not None:
        gp.set_diag(diag)
    if trend is not None:
        gp.set_trend(trend)
    return gp


def _nan_upper(gp):
    """NaN into the strict upper triangle of W_dev (columns up to lda), into all of the prediction work block and into all of the
    handle's own scratch"""
    import torch

    _poison_scratch(gp)

    r = torch.arange(gp.W_t.shape[0], device=gp.W_t.device)[:, None]
    c = torch.arange(gp.W_t.shape[1], device=gp.W_t.device)[None, :]
    gp.W_t.masked_fill_(c > r, float("nan"))
    if getattr(gp, "_work", None) is not None:
        gp._work.fill_(float("nan"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("i,order", ref.CASE_IDS)
def test_value_and_gradient_parity(i, order):
    X, y, kernel, theta, diag, cond = loo_ref.case(i)
    v_ref, (_, g_ref) = ref.case_refs(i, order)
    gp = _gp(X, y, kernel, diag)
    assert gp.get_option(50) == 0  # the default
    v_lml, _ = gp.lml_grad(theta)
    parts = gp.lml_parts()
    gp.set_trend(ref.NAMES[order])
    assert gp.get_option(50) == order
    val, grad = gp.lml_grad(theta)
    assert gp.info == 0
    rv, rg = loo_ref.value_ratio(val, v_ref, cond), loo_ref.grad_ratio(grad, g_ref, cond)
    print(loo_ref.CASES[i], ref.NAMES[order], "cond %.3g" % cond, "error / bound: value %.3g gradient %.3g" % (rv, rg))
    assert rv <= 1.0 and rg <= 1.0, (rv, rg, val, v_ref, grad, g_ref)
    assert val != v_lml and abs(grad[-1] - grad[-2]) <= 1e-12 * abs(grad[-1])  # d/d jitter = d/d gv
    assert gp.lml_parts() == parts  # the factorisation's logdet and quad
    # the same call in the same state: the same bits; so with NaN in everything the call may not read
    v2, g2 = gp.lml_grad(theta)
    assert v2 == val and np.array_equal(g2, grad)
    _nan_upper(gp)
    v3, g3 = gp.lml_grad(theta)
    assert v3 == val and np.array_equal(g3, grad)
    gp.close()


def test_the_rank_128_update_on_128_tiles_at_46_tile_columns():
    """N = 5800, linear trend: 1081 lower tiles, the update W -= Q Q^T takes the GEMM's 128x128-tile path.  The value against the
    projected-data definition (the basis' two Householder reflectors applied to K: trend_ref.project_householder).  The gradient
    against the float64 restatement of the direct form, for cost: the forward mode on the projected data takes one n^3 solve per
    hyper-parameter at this size; the restatement sits within 3e-5 of the gradient's bound of the forward mode on every smaller
    case (tests/test_trend_host.py).  cond(K) by the Gershgorin bound over the noise floor, as tests/test_gpu_loo_objective.py
    does."""
    from oracle import gp_oracle as orc

    kernel, n, d, with_diag, gv = loo_ref.BIG
    X, y, theta, diag = loo_ref.make_problem(kernel, n, d, with_diag, gv, 99)
    cond = np.abs(orc.noisy_cov(X, [kernel], [], theta, "marginal", diag)).sum(1).max() / (theta[-1] + theta[-2])
    _, g_ref = ref.trend_direct(X, y, kernel, theta, 2, diag)
    v_ref = ref.trend_projected_large(X, y, kernel, theta, 2, diag)
    gp = _gp(X, y, kernel, diag, "linear")
    val, grad = gp.lml_grad(theta)
    rv, rg = loo_ref.value_ratio(val, v_ref, cond), loo_ref.grad_ratio(grad, g_ref, cond)
    print(loo_ref.BIG, "cond <= %.3g" % cond, "error / bound: value %.3g gradient %.3g" % (rv, rg))
    assert gp.info == 0 and rv <= 1.0 and rg <= 1.0, (rv, rg, val, v_ref, grad, g_ref)
    gp.close()


def test_the_gram_product_at_65_tile_columns_runs_the_tail_segment():
    """N = 8320, d = 4, constant trend: 65 tile columns, so A = H^T V is cut into 32 segments of two tile columns and a TAIL of one,
    the second launch of gram_segments (csrc/api_gp.hip) that no smaller size reaches.  The value against the projected-data
    definition (trend_ref.trend_projected_large) under test_value_and_gradient_parity's bound for the value, with cond(K) by the
    Gershgorin bound over the noise floor as in the test above.  No gradient: its references take minutes at this size."""
    from oracle import gp_oracle as orc

    kernel, n, d = "RBF", 8320, 4
    X, y, theta, diag = loo_ref.make_problem(kernel, n, d, False, 1e-2, 65)
    cond = np.abs(orc.noisy_cov(X, [kernel], [], theta, "marginal", diag)).sum(1).max() / (theta[-1] + theta[-2])
    v_ref = ref.trend_projected_large(X, y, kernel, theta, 1, diag)
    gp = _gp(X, y, kernel, diag, "constant")
    val, _ = gp.lml_grad(theta)
    rv = loo_ref.value_ratio(val, v_ref, cond)
    print((kernel, n, d), "cond <= %.3g" % cond, "error / bound: value %.3g" % rv)
    assert gp.info == 0 and rv <= 1.0, (rv, val, v_ref)
    gp.close()


@pytest.mark.parametrize("i,order", ref.CASE_IDS)
def test_predict_parity_inside_and_outside_the_design(i, order):
    """m = 9 (the pinned route, an odd count) and m = 300 (device buffers, three tile rows of work_dev, the last one ragged)"""
    X, y, kernel, theta, diag, cond = loo_ref.case(i)
    Xn, (mu_ref, var_ref, term) = ref.case_predict(i, order)
    # outside the box the trend's term carries a share of the variance that a missing or wrong term cannot hide in the tolerance
    share = float(np.min(term[5:] / var_ref[5:]))
    assert share >= ref.MIN_SHARE[order], share
    vtol, ptol = kfold_ref.tolerances(cond)
    gp = _gp(X, y, kernel, diag, ref.NAMES[order])
    for sel in (np.arange(1, 10), np.tile(np.arange(10), 30)):
        mu, var = gp.predict(theta, Xn[sel])
        e_mu = np.max(np.abs(mu - mu_ref[sel]) / np.maximum(np.abs(mu_ref[sel]), 1.0)) / vtol
        e_var = np.max(np.abs(var - var_ref[sel]) / var_ref[sel]) / ptol
        print(loo_ref.CASES[i], ref.NAMES[order], "m = %d" % len(sel), "share %.3g" % share,
              "error / bound: mean %.3g var %.3g" % (e_mu, e_var))
        assert e_mu <= 1.0 and e_var <= 1.0, (e_mu, e_var)
        _nan_upper(gp)
        assert gp.factor(theta) == 0  # (G^T, C_A^-1, beta^ and b~ are the factor's: it writes them again)
        mu2, var2 = gp.predict(theta, Xn[sel])
        assert np.array_equal(mu2, mu) and np.array_equal(var2, var)
    # without the observation noise: the same latent variance
    mu3, var3 = gp.predict(theta, Xn[:7], pred_noise=False)
    mu4, var4 = gp.predict(theta, Xn[:7])
    assert np.array_equal(mu3, mu4) and np.allclose(var4 - var3, np.sqrt(theta[-2]) ** 2, rtol=1e-9, atol=1e-14)
    gp.close()


def test_128_coefficients_every_column_block_and_every_pass_of_the_reduction():
    """d = 127, linear: p = 128 -- eight 16-column blocks in the symmetric multiply (the most LDS it asks for), a full 128 x 128
    block A, sixteen passes over a point's row in the predict reduction"""
    X, y, kernel, theta, cond, v_ref, g_ref, Xn, (mu_ref, var_ref, term) = ref.wide_case()
    gp = _gp(X, y, kernel, None, "linear")
    val, grad = gp.lml_grad(theta)
    rv, rg = loo_ref.value_ratio(val, v_ref, cond), loo_ref.grad_ratio(grad, g_ref, cond)
    vtol, ptol = kfold_ref.tolerances(cond)
    mu, var = gp.predict(theta, Xn)
    e_mu = np.max(np.abs(mu - mu_ref) / np.maximum(np.abs(mu_ref), 1.0)) / vtol
    e_var = np.max(np.abs(var - var_ref) / var_ref) / ptol
    print(ref.WIDE, "cond %.3g" % cond, "error / bound: value %.3g gradient %.3g mean %.3g var %.3g" % (rv, rg, e_mu, e_var))
    assert gp.info == 0 and rv <= 1.0 and rg <= 1.0 and e_mu <= 1.0 and e_var <= 1.0
    _nan_upper(gp)
    v2, g2 = gp.lml_grad(theta)
    mu2, var2 = gp.predict(theta, Xn)
    assert v2 == val and np.array_equal(g2, grad) and np.array_equal(mu2, mu) and np.array_equal(var2, var)
    gp.close()


def _everything(gp, theta, Xn):
    return [*gp.lml_grad(theta), *gp.predict(theta, Xn, via_inverse=False)]


@pytest.mark.parametrize("i,order", [(5, 2), (9, 1)])
def test_the_scheduling_options_change_no_bit(i, order):
    X, y, kernel, theta, diag, _ = loo_ref.case(i)
    Xn = ref.predict_points(i, X.shape[1])
    gp = _gp(X, y, kernel, diag, ref.NAMES[order])
    want = _everything(gp, theta, Xn)
    gp.close()
    for opts in ({26: 0}, {0: 0}, {0: 2}, {26: 0, 0: 2}):
        gp = _gp(X, y, kernel, diag, ref.NAMES[order])
        for k, v in opts.items():
            gp.set_option(k, v)
        got = _everything(gp, theta, Xn)
        gp.close()
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), opts


@pytest.mark.parametrize("i,order", [(5, 2), (9, 1)])
def test_switching_back_returns_a_fresh_handles_bits(i, order):
    X, y, kernel, theta, diag, _ = loo_ref.case(i)
    Xn = ref.predict_points(i, X.shape[1])
    folds = np.arange(len(y) // 10 * 10, dtype=np.int32).reshape(-1, 10)

    def ordinary(gp):
        out = _everything(gp, theta, Xn)
        lp, mu, var, info = gp.kfold(theta, folds)
        return out + [lp, np.concatenate(mu), np.concatenate(var), info]

    fresh = _gp(X, y, kernel, diag)
    want = ordinary(fresh)
    fresh.close()
    gp = _gp(X, y, kernel, diag, ref.NAMES[order])
    under = _everything(gp, theta, Xn)
    assert under[0] != want[0] and not np.array_equal(under[2], want[2])
    gp.set_trend("none")
    assert gp.get_option(50) == 0
    got = ordinary(gp)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)), [np.array_equal(a, b) for a, b in zip(got, want)]
    # ... and straight behind an evaluation and a prediction under the trend
    gp.set_trend(ref.NAMES[order])
    assert all(np.array_equal(a, b) for a, b in zip(_everything(gp, theta, Xn), under))
    gp.set_trend("none")
    assert all(np.array_equal(a, b) for a, b in zip(ordinary(gp), want))
    gp.close()


def test_every_other_entry_point_is_refused_with_its_text():
    import torch

    X, y, kernel, theta, diag, _ = loo_ref.case(4)
    gp = _gp(X, y, kernel, diag, "constant")
    lib, h, n, d = gp.lib, gp.h, gp.n, gp.d
    assert gp.factor(theta) == 0
    dpt, ipt = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    buf = torch.zeros(4 * 128 * gp.lda + 70000, dtype=torch.float64, device=gp.dev)
    torch.cuda.synchronize()
    p = buf.data_ptr()
    th = np.ascontiguousarray(theta)
    tp = th.ctypes.data_as(dpt)
    out = np.zeros(2 * len(th) + 8)
    op = out.ctypes.data_as(dpt)
    info = np.zeros(8, dtype=np.int32)
    ip = info.ctypes.data_as(ipt)
    ptr = np.array([0, 2], dtype=np.int32)
    calls = {
        "mi_gp_lml": lambda: lib.mi_gp_lml(h, tp, op),
        "mi_gp_lml_batch": lambda: lib.mi_gp_lml_batch(h, 1, tp, op, ip),
        "mi_gp_lml_grad_batch": lambda: lib.mi_gp_lml_grad_batch(h, 1, tp, op, op, ip),
        "mi_gp_factor_batch": lambda: lib.mi_gp_factor_batch(h, 1, tp, ip),
        "mi_gp_predict_batch": lambda: lib.mi_gp_predict_batch(h, 1, p, 1, p, gp.lda, 128 * gp.lda, p, p, 1, None, None),
        "mi_gp_predict_u": lambda: lib.mi_gp_predict_u(h, p, 1, p, gp.lda, p, p, 1),
        "mi_gp_predict_grad": lambda: lib.mi_gp_predict_grad(h, p, 1, p, gp.lda, p, p, 1, p, p),
        "mi_gp_predict_cov": lambda: lib.mi_gp_predict_cov(h, p, 1, p, gp.lda, p, p, 128, 1),
        "mi_gp_append": lambda: lib.mi_gp_append(h, p, p, None, 1, p, gp.lda),
        "mi_gp_logpdf": lambda: lib.mi_gp_logpdf(h, p, p, None, 1, p, gp.lda, op, None, None),
        "mi_gp_kfold": lambda: lib.mi_gp_kfold(h, 1, ptr.ctypes.data_as(ipt), ptr.ctypes.data_as(ipt), None, 0, p, None, None, ip),
        "mi_gp_alpha": lambda: lib.mi_gp_alpha(h, op),
        "mi_gp_grad_x": lambda: lib.mi_gp_grad_x(h, p),
    }
    for name, call in calls.items():
        assert call() == -1, name
        text = gp.last_error()
        assert name in text and "option 50" in text, (name, text)
    # the handle is still factored: the refusals touched nothing
    Xn = ref.predict_points(4, d)
    mu, var = gp.predict(theta, Xn)
    assert np.isfinite(mu).all() and (var > 0).all()
    # no cross-validation objective under a trend, and values outside 0 .. 2
    gp.set_option(48, 1)
    assert lib.mi_gp_lml_grad(h, tp, op, op) == -1 and "option 50" in gp.last_error() and "option 48" in gp.last_error()
    gp.set_option(48, 0)
    for bad in (-1, 3):
        assert lib.mi_gp_set_option(h, 50, bad) == -1 and "option 50" in gp.last_error()
    assert gp.get_option(50) == 1
    # the facade raises before the call
    for call in (lambda: gp.lml(theta), lambda: gp.predict(theta, Xn, via_inverse=True), lambda: gp.predict_grad(theta, Xn),
                 lambda: gp.predict_cov(theta, Xn), lambda: gp.kfold(theta, [np.arange(3)]), lambda: gp.lml_grad_data(theta),
                 lambda: gp.lml_batch(th[None]), lambda: gp.sample_posterior(theta, Xn, 1), lambda: gp.logpdf(theta, Xn[:1], y[:1]),
                 lambda: gp.set_trend("quadratic")):
        with pytest.raises(ValueError, match="trend"):
            call()
    gp.close()


def test_as_many_points_as_coefficients_are_refused():
    X, y, kernel, theta, _, _ = loo_ref.case(4)  # d = 2: three coefficients
    gp = _gp(X[:3], y[:3], kernel, None, "linear")
    with pytest.raises(RuntimeError, match="option 50"):
        gp.lml_grad(theta)
    with pytest.raises(RuntimeError, match="option 50"):
        gp.factor(theta)
    gp.set_trend("constant")
    val, _ = gp.lml_grad(theta)
    assert np.isfinite(val) and gp.info == 0
    gp.close()


def _bind_roomy(gp, cap):
    """Rebinds the handle to buffers with room for `cap` points WITHOUT reserving: the handle's capacity stays n, so a later
    mi_gp_reserve changes the layout of its scratch (the facade's own capacity path reserves at once)."""
    import torch

    from andvaranaut_amd import _lib

    cp = (cap + 127) // 128 * 128
    gp.lda = cp + 16
    Xs = torch.zeros((cap, gp.d), dtype=torch.float64, device=gp.dev)
    ys = torch.zeros(cap, dtype=torch.float64, device=gp.dev)
    Xs[: gp.n].copy_(gp.X_t)
    ys[: gp.n].copy_(gp.y_t)
    gp._roomy = (Xs, ys)
    gp.X_t, gp.y_t = Xs[: gp.n], ys[: gp.n]
    gp.K_t = torch.empty((cp + 128, gp.lda), dtype=torch.float64, device=gp.dev)
    gp.Z_t = torch.zeros((cp, gp.lda), dtype=torch.float64, device=gp.dev)
    gp.W_t = torch.zeros((cp, gp.lda), dtype=torch.float64, device=gp.dev)
    gp._work = None
    torch.cuda.synchronize()
    gp._bind()


def test_reserve_resizes_the_scratch_and_keeps_the_factored_state():
    X, y, kernel, theta, _, _ = loo_ref.case(4)
    X, y = X[:120], y[:120]  # one tile: the scratch is laid out for 128 points, behind the reserve for 384
    Xn = ref.predict_points(4, X.shape[1])
    plain = _gp(X, y, kernel, None, "linear")
    want = _everything(plain, theta, Xn)
    plain.close()
    gp = _gp(X, y, kernel, None, "linear")
    _bind_roomy(gp, 300)
    assert all(np.array_equal(u, v) for u, v in zip(_everything(gp, theta, Xn), want))  # (the leading dimension changes no bit)
    # a reserve between mi_gp_factor and mi_gp_predict: the handle stays factored and predicts the same bits
    assert gp.lib.mi_gp_reserve(gp.h, 300) == 0
    got = gp.predict(theta, Xn, via_inverse=False)  # (the facade does not factor again: same theta)
    assert np.array_equal(got[0], want[2]) and np.array_equal(got[1], want[3])
    # ... and evaluations in the re-sized scratch give the bits of a handle created at that capacity
    assert all(np.array_equal(u, v) for u, v in zip(_everything(gp, theta, Xn), want))
    gp.close()
    roomy = _gp(X, y, kernel, None, "linear", capacity=300)
    assert all(np.array_equal(u, v) for u, v in zip(_everything(roomy, theta, Xn), want))
    roomy.close()


def test_fit_with_a_linear_trend_predicts_what_the_reference_predicts_outside_the_design():
    from andvaranaut_amd import GPMCMC, uniform

    priors = [st.uniform(loc=0, scale=2), st.uniform(loc=1, scale=0.5)]
    fun = lambda x: np.array([3.0 * x[0] - 4.0 * x[1] + 0.05 * np.sin(6.0 * x[0])])  # noqa: E731  (a dominant linear part)
    g = GPMCMC(kernel="RBF", noise=True, xconrevs=[uniform(priors[0]), uniform(priors[1])], yconrevs=[None], nx=2, ny=1,
               priors=priors, target=fun, parallel=False, nproc=1, verbose=False)
    g.sample(nsamps=60, seed=1)
    g.fit(method="map", trend="linear")
    assert g.trend == "linear" and g.gp.get_option(50) == 2
    # outside the design, in the converted input space (the design fills [0, 1]^2)
    Xc = 1.0 + 0.5 * np.random.default_rng(3).random((8, 2))
    mu, var = g.predict(Xc, return_var=True, convert=False, revert=False)
    theta = g._theta_from_hypers(g.hypers, 1e-6)
    xin, yin = g._converted(g.x, g.y - g.ym)
    mu_ref, var_ref, _ = ref.predict_dense(xin, yin, Xc, "RBF", theta, 2)
    cond = kfold_ref.full_cond(xin, "RBF", theta)
    vtol, ptol = kfold_ref.tolerances(cond)
    e_mu = np.max(np.abs(mu[:, 0] - mu_ref) / np.maximum(np.abs(mu_ref), 1.0)) / vtol
    e_var = np.max(np.abs(var[:, 0] - var_ref) / var_ref) / ptol
    print("fit(trend='linear'): cond %.3g, error / bound: mean %.3g var %.3g" % (cond, e_mu, e_var))
    assert e_mu <= 1.0 and e_var <= 1.0
    for name in ("predict_joint", "sample_posterior"):
        with pytest.raises(ValueError, match="trend"):
            getattr(g, name)(Xc)
    # test_stats conditions on the training split under the same trend, at the stored hyper-parameters
    g.train, g.test = np.arange(45), np.arange(45, 60)
    stats = g.test_stats(revert=False)
    xtr, ytr = g._converted(g.x[g.train], (g.y - g.ym)[g.train])
    mu_t, var_t, _ = ref.predict_dense(xtr, ytr, stats["xtest"], "RBF", theta, 2)
    vt, pt = kfold_ref.tolerances(kfold_ref.full_cond(xtr, "RBF", theta))
    assert np.max(np.abs(stats["ypred"] - mu_t) / np.maximum(np.abs(mu_t), 1.0)) <= vt
    assert np.max(np.abs(stats["yvars"] - var_t) / var_t) <= pt
    assert g.trend == "linear" and g.predict(Xc, convert=False, revert=False).shape == (8, 1)
    with pytest.raises(ValueError, match="trend"):
        g.test_stats(method="mcmc_mean")
    # the zero-mean fit reverts to zero out there
    g.fit(method="map")
    assert g.trend is None and g.gp.get_option(50) == 0
    mu0 = g.predict(Xc, convert=False, revert=False)
    assert np.max(np.abs(mu0[:, 0] - mu[:, 0])) > 1e-6 * np.max(np.abs(mu[:, 0]))
