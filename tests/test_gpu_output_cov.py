"""The between-output covariance integrated out (option 52 of mi_gp_set_option; MiGP.set_output_cov,
GPMCMC.fit(outputs="all", output_cov="integrated")) against the references of tests/output_cov_ref.py: mi_gp_lml_grad against the
forward-mode definition (solves with K_y, slogdet), mi_gp_factor + mi_gp_predict against the oracle's conditional variance times
s_o; the invariances the model promises (re-mixing the outputs, re-scaling the covariance); then what the option must leave alone
and what it refuses.

Bounds are the project's own at cond = max(cond(K_y), cond(S)), both matrices being inverted: loo_ref.value_ratio and
loo_ref.grad_ratio for L_S and its gradient, kfold_ref.tolerances for the conditional.  Every parity check prints error / bound
before it asserts."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.stats as st

import kfold_ref
import loo_ref
import multi_output_ref as mo
import output_cov_ref as ref

pytestmark = pytest.mark.gpu


def _gp(X, Y, kernel, diag=None, cov="integrated", **kw):
    from andvaranaut_amd import MiGP

    gp = MiGP(np.array(X), np.array(Y[:, 0]), kernel, device=0, **kw)  # (copies: the cached problems are read-only)
    if diag is not None:
        gp.set_diag(np.array(diag))
    if Y.shape[1] > 1:
        gp.set_outputs(Y)
    if cov is not None:
        gp.set_output_cov(cov)
    return gp


def _nan_everything(gp):
    """NaN into the strict upper triangle of W_dev (columns up to lda) and into all of the prediction work block"""
    import torch

    r = torch.arange(gp.W_t.shape[0], device=gp.W_t.device)[:, None]
    c = torch.arange(gp.W_t.shape[1], device=gp.W_t.device)[None, :]
    gp.W_t.masked_fill_(c > r, float("nan"))
    if getattr(gp, "_work", None) is not None:
        gp._work.fill_(float("nan"))
    torch.cuda.synchronize()


def _points(d, m, seed=11):
    """m prediction points: the first half inside the design's box, the rest around it (those of tests/test_gpu_multi_output.py)"""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.vstack([rng.random((m - m // 2, d)), 1.5 * rng.random((m // 2, d)) - 0.25]))


@functools.lru_cache(maxsize=None)
def _case(i, q):
    """(X, Y, kernel, theta, diag, cond, (value, gradient) of the forward definition) of loo_ref.CASES[i] with q outputs"""
    kernel, n, d, with_diag, gv = loo_ref.CASES[i]
    X, Y, theta, diag, cond_k = mo.problem(kernel, n, d, q, with_diag, gv, 70 + i)
    v, g, cond_s = ref.forward(X, Y, kernel, theta, diag)
    g.setflags(write=False)
    return X, Y, kernel, theta, diag, max(cond_k, cond_s), (v, g)


@pytest.mark.parametrize("i,q", ref.CASES)
def test_value_and_gradient_parity(i, q):
    X, Y, kernel, theta, diag, cond, (v_ref, g_ref) = _case(i, q)
    gp = _gp(X, Y, kernel, diag, cov=None)
    assert gp.get_option(52) == 0  # the default
    v0, _ = gp.lml_grad(theta)
    parts = gp.lml_parts()
    gp.set_output_cov("integrated")
    assert gp.get_option(52) == 1 and gp.get_option(51) == q
    val, grad = gp.lml_grad(theta)
    assert gp.info == 0
    rv, rg = loo_ref.value_ratio(val, v_ref, cond), loo_ref.grad_ratio(grad, g_ref, cond)
    print(loo_ref.CASES[i], "q = %d" % q, "cond %.3g" % cond, "error / bound: value %.3g gradient %.3g" % (rv, rg))
    assert rv <= 1.0 and rg <= 1.0, (rv, rg, val, v_ref, grad, g_ref)
    assert val != v0 and abs(grad[-1] - grad[-2]) <= 1e-12 * abs(grad[-1])  # d/d jitter = d/d gv
    assert gp.lml_parts() == parts  # the factorisation's logdet and output 0's quad
    # the same call in the same state: the same bits; so with NaN in everything the call may not read
    v2, g2 = gp.lml_grad(theta)
    assert v2 == val and np.array_equal(g2, grad)
    _nan_everything(gp)
    v3, g3 = gp.lml_grad(theta)
    assert v3 == val and np.array_equal(g3, grad)
    gp.close()


def test_the_rank_update_on_128_tiles_at_46_tile_columns():
    """loo_ref.BIG's design (N = 5800: 1081 lower tiles, the update W <- q W - Q Q^T takes the GEMM's 128x128-tile path) with
    q = 3, against the forward definition.  cond(K) by the Gershgorin bound over the noise floor, as tests/test_gpu_trend.py does;
    cond(S) is that of the 3 x 3 block."""
    from oracle import gp_oracle as orc

    kernel, n, d, with_diag, gv = loo_ref.BIG
    X, y, theta, diag = loo_ref.make_problem(kernel, n, d, with_diag, gv, 99)
    Y = mo.make_outputs(X, y, 3, 100)
    cond_k = np.abs(orc.noisy_cov(X, [kernel], [], theta, "marginal", diag)).sum(1).max() / (theta[-1] + theta[-2])
    v_ref, g_ref, cond_s = ref.forward(X, Y, kernel, theta, diag)
    cond = max(cond_k, cond_s)
    gp = _gp(X, Y, kernel, diag)
    val, grad = gp.lml_grad(theta)
    rv, rg = loo_ref.value_ratio(val, v_ref, cond), loo_ref.grad_ratio(grad, g_ref, cond)
    print(loo_ref.BIG, "q = 3", "cond <= %.3g" % cond, "error / bound: value %.3g gradient %.3g" % (rv, rg))
    assert gp.info == 0 and rv <= 1.0 and rg <= 1.0, (rv, rg, val, v_ref, grad, g_ref)
    gp.close()


@pytest.mark.parametrize("i,q", [(8, 5), (3, 17)])
def test_remixing_the_outputs_moves_the_value_by_n_log_det_and_leaves_the_gradient(i, q):
    X, Y, kernel, theta, diag, cond, _ = _case(i, q)
    n = len(X)
    M = np.random.default_rng(3).normal(size=(q, q)) + 2.0 * np.eye(q)
    YM = np.ascontiguousarray(Y @ M)
    cond = max(cond, ref.forward(X, YM, kernel, theta, diag)[2])
    gp = _gp(X, Y, kernel, diag)
    val, grad = gp.lml_grad(theta)
    gp.set_outputs(YM)
    vm, gm = gp.lml_grad(theta)
    want = val - n * np.linalg.slogdet(M)[1]
    rv, rg = loo_ref.value_ratio(vm, want, cond), loo_ref.grad_ratio(gm, grad, cond)
    print(loo_ref.CASES[i], "q = %d" % q, "mixed, cond %.3g" % cond, "error / bound: value %.3g gradient %.3g" % (rv, rg))
    assert rv <= 1.0 and rg <= 1.0, (vm, want, gm, grad)
    # ... where the independent outputs of option 52 = 0 do move
    gp.set_output_cov("shared")
    _, gs_m = gp.lml_grad(theta)
    gp.set_outputs(Y)
    _, gs = gp.lml_grad(theta)
    assert loo_ref.grad_ratio(gs_m, gs, cond) > 1.0
    gp.close()


def test_rescaling_the_covariance_leaves_the_value():
    """One component without a per-point diagonal (case 4): K_y -> c K_y is kv, gv, jitter -> c kv, c gv, c jitter, and L_S does
    not move, so kv g_kv + gv g_gv + jitter g_jitter = 0 within the gradient's bound times the largest of the three terms"""
    X, Y, kernel, theta, diag, cond, _ = _case(4, 3)
    assert diag is None and "+" not in kernel and "*" not in kernel
    d = X.shape[1]
    gp = _gp(X, Y, kernel)
    _, g = gp.lml_grad(theta)
    terms = np.array([theta[d] * g[d], theta[-2] * g[-2], theta[-1] * g[-1]])
    bound = max(1e-7, 500.0 * cond * loo_ref.EPS) * np.abs(terms).max()
    print("scale invariance: sum %.3g of terms up to %.3g, error / bound %.3g" % (terms.sum(), np.abs(terms).max(), abs(terms.sum()) / bound))
    assert abs(terms.sum()) <= bound
    gp.close()


@functools.lru_cache(maxsize=None)
def _conditional_case(kernel, n, q):
    X, Y, theta, _, cond = mo.problem(kernel, n, 3, q, False, 1e-2, 7)
    Xn = _points(3, 300)
    refs = {pn: ref.predict_var(X, Y, Xn, kernel, theta, pred_noise=bool(pn)) for pn in (0, 1)}
    return X, Y, theta, cond, Xn, refs


@pytest.mark.parametrize("kernel,n,q", [("RBF", 300, 2), ("RBF+Matern52", 300, 17), ("RBF", 256, 128)])
def test_conditional_a_variance_per_output_and_the_means_of_option_51(kernel, n, q):
    """m = 1, 127 (the pinned route, one point and a ragged last block of 16) and 300 (device buffers, a ragged last block) with
    and without the observation noise; the C-ABI call into sentinel-filled buffers: q m and q m doubles are written"""
    import torch

    X, Y, theta, cond, Xn, refs = _conditional_case(kernel, n, q)
    _, ptol = kfold_ref.tolerances(cond)
    gp = _gp(X, Y, kernel)
    shared = _gp(X, Y, kernel, cov=None)
    for m in (1, 127, 300):
        got = {}
        for pn in (0, 1):
            mu, var = gp.predict(theta, Xn[:m], pred_noise=bool(pn))
            mu_s, var_s = shared.predict(theta, Xn[:m], pred_noise=bool(pn))
            assert mu.shape == (m, q) and var.shape == (m, q) and var_s.shape == (m,)
            assert np.array_equal(mu, mu_s)  # the same bits
            var_ref = refs[pn][:m]
            e_var = np.max(np.abs(var - var_ref) / var_ref) / ptol
            print((kernel, n, q), "m = %d pred_noise = %d" % (m, pn), "cond %.3g" % cond, "error / bound: var %.3g" % e_var)
            assert e_var <= 1.0
            # what one shared variance cannot show: the outputs' error bars differ, by the ratio of their scales at every point
            ratio = var / var[:, :1]
            assert ratio[:, 1:].std(axis=0).max() <= 1e-12 * ratio.max() and np.ptp(ratio[0]) > 1e-3 * ratio[0].max()
            got[pn] = (mu, var)
        # NaN in the work block and in W's upper triangle: the same bits
        _nan_everything(gp)
        mu2, var2 = gp.predict(theta, Xn[:m], pred_noise=True)
        assert np.array_equal(mu2, got[1][0]) and np.array_equal(var2, got[1][1])
        # the entry point itself, into buffers filled with a sentinel
        mp = (m + 127) // 128 * 128
        out = torch.full((2 * q * m + 64,), -7.25, dtype=torch.float64, device=gp.dev)
        xn = torch.from_numpy(Xn[:m].copy()).to(gp.dev)
        work = torch.full((mp, gp.lda), float("nan"), dtype=torch.float64, device=gp.dev)
        torch.cuda.synchronize()
        base = out.data_ptr()
        assert gp.lib.mi_gp_predict(gp.h, xn.data_ptr(), m, work.data_ptr(), gp.lda, base + 8 * 16, base + 8 * (32 + q * m), 1) == 0
        o = out.cpu().numpy()
        assert np.array_equal(o[16 : 16 + q * m].reshape(q, m).T, got[1][0])
        assert np.array_equal(o[32 + q * m : 32 + 2 * q * m].reshape(q, m).T, got[1][1])
        rest = np.r_[o[:16], o[16 + q * m : 32 + q * m], o[32 + 2 * q * m :]]
        assert (rest == -7.25).all()
    gp.close()
    shared.close()


def _everything(gp, theta, Xn):
    return [*gp.lml_grad(theta), *gp.predict(theta, Xn)]


def test_value_0_is_option_51_and_a_change_ends_the_resident_state():
    import torch

    kernel, n, q = "RBF+Matern52", 300, 5
    X, Y, theta, _, _ = mo.problem(kernel, n, 3, q, False, 1e-2, 7)
    Xn = _points(3, 50)
    plain = _gp(X, Y, kernel, cov=None)
    want = _everything(plain, theta, Xn)
    plain.close()
    gp = _gp(X, Y, kernel, cov=None)
    assert gp.lib.mi_gp_set_option(gp.h, 52, 0) == 0  # (the current value)
    assert all(np.array_equal(a, b) for a, b in zip(_everything(gp, theta, Xn), want))
    other = _gp(X, Y, kernel)
    under = _everything(other, theta, Xn)
    other.close()
    # there and back: option 51's bits again, and the integrated bits again
    gp.set_output_cov("integrated")
    got = _everything(gp, theta, Xn)
    assert all(np.array_equal(a, b) for a, b in zip(got, under)) and got[0] != want[0] and got[3].shape == (50, q)
    gp.set_output_cov("shared")
    assert gp.get_option(52) == 0
    assert all(np.array_equal(a, b) for a, b in zip(_everything(gp, theta, Xn), want))
    # the plain setter keeps the facade in step: predict sizes its variance for the option the handle has
    gp.set_option(52, 1)
    assert all(np.array_equal(a, b) for a, b in zip(_everything(gp, theta, Xn), under))
    gp.set_option(52, 0)
    assert all(np.array_equal(a, b) for a, b in zip(_everything(gp, theta, Xn), want))
    # the handle is factored; setting the current value keeps that, another value ends it (as mi_gp_set_data does)
    xn = torch.from_numpy(Xn.copy()).to(gp.dev)
    out = torch.zeros(2 * q * 50, dtype=torch.float64, device=gp.dev)
    work = torch.empty((128, gp.lda), dtype=torch.float64, device=gp.dev)
    torch.cuda.synchronize()
    call = lambda: gp.lib.mi_gp_predict(gp.h, xn.data_ptr(), 50, work.data_ptr(), gp.lda, out.data_ptr(), out.data_ptr() + 8 * q * 50, 1)  # noqa: E731
    assert gp.lib.mi_gp_set_option(gp.h, 52, 0) == 0 and call() == 0
    assert gp.lib.mi_gp_set_option(gp.h, 52, 1) == 0
    assert call() == -1 and "mi_gp_factor first" in gp.last_error()
    assert gp.lib.mi_gp_set_option(gp.h, 52, 0) == 0
    assert call() == -1 and "mi_gp_factor first" in gp.last_error()
    # one output: the option is inert
    gp.close()
    one = _gp(X, Y[:, :1], kernel, cov=None)
    w1 = _everything(one, theta, Xn)
    one.set_output_cov("integrated")
    assert all(np.array_equal(a, b) for a, b in zip(_everything(one, theta, Xn), w1))
    one.close()


def test_reserve_behind_factor_keeps_the_prediction_bits():
    import torch

    kernel = "RBF"
    X, Y, theta, _, _ = mo.problem(kernel, 300, 3, 5, False, 1e-2, 7)
    X, Y = X[:120], Y[:120]  # one tile: the scratch is laid out for 128 points, behind the reserve for 384
    Xn = _points(3, 30)
    plain = _gp(X, Y, kernel)
    want = _everything(plain, theta, Xn)
    plain.close()
    # a handle whose buffers have room for 300 points but whose capacity is still n (bound by hand: the facade reserves at once)
    gp = _gp(X, Y[:, :1], kernel)
    cp = 384
    gp.lda = cp + 16
    Xs = torch.zeros((300, gp.d), dtype=torch.float64, device=gp.dev)
    Xs[: gp.n].copy_(gp.X_t)
    gp._roomy = Xs
    gp.X_t = Xs[: gp.n]
    gp.K_t = torch.empty((cp + 128, gp.lda), dtype=torch.float64, device=gp.dev)
    gp.Z_t = torch.zeros((cp, gp.lda), dtype=torch.float64, device=gp.dev)
    gp.W_t = torch.zeros((cp, gp.lda), dtype=torch.float64, device=gp.dev)
    gp._work = None
    torch.cuda.synchronize()
    gp.set_outputs(Y)  # (allocates (q, lda) for the new lda and rebinds)
    assert all(np.array_equal(u, v) for u, v in zip(_everything(gp, theta, Xn), want))  # (the leading dimension changes no bit)
    assert gp.lib.mi_gp_reserve(gp.h, 300) == 0  # across the tile boundary: B^T and s_o move
    got = gp.predict(theta, Xn)  # (the facade does not factor again: same theta)
    assert np.array_equal(got[0], want[2]) and np.array_equal(got[1], want[3])
    assert all(np.array_equal(u, v) for u, v in zip(_everything(gp, theta, Xn), want))
    gp.close()


def test_refusals_and_a_block_that_is_not_positive_definite():
    kernel = "RBF"
    X, Y, theta, _, _ = mo.problem(kernel, 300, 3, 5, False, 1e-2, 7)
    n = len(X)
    th = np.ascontiguousarray(theta)
    tp = th.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    out = np.zeros(len(th) + 1)
    op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    gp = _gp(X, Y, kernel)
    for bad in (2, -1, 52):
        assert gp.lib.mi_gp_set_option(gp.h, 52, bad) == -1 and "option 52" in gp.last_error()
    assert gp.get_option(52) == 1
    # everything option 51 refuses stays refused; a trend and a cross-validation objective too
    assert gp.lib.mi_gp_lml(gp.h, tp, op) == -1 and "51" in gp.last_error()
    gp.set_option(48, 1)
    assert gp.lib.mi_gp_lml_grad(gp.h, tp, op, op) == -1 and "option 48" in gp.last_error()
    gp.set_option(48, 0)
    # a zero column is collinear with every other: S[1][1] = 0 and the row's off-diagonal entries are exact zeros, so the
    # factorisation of S meets the pivot 0 at (1-based) 2, whatever the rounding
    good, _ = gp.lml_grad(theta)
    Yz = np.array(Y)
    Yz[:, 1] = 0.0
    gp.set_outputs(Yz)
    val, grad = gp.lml_grad(theta)
    assert gp.info == n + 2 and val == -np.inf and not grad.any(), (gp.info, val)
    assert "option 52" in gp.last_error()
    assert gp.lib.mi_gp_alpha(gp.h, op) == -1  # (K^-1 is not resident either way)
    # columns that are collinear without a zero among them -- a copy, twice another, the sum of two others: S is singular in exact
    # arithmetic and its last pivot is of rounding size and of either sign on the device.  Either the pivot is caught where the
    # collinear column stands (n + pivot, -inf, a zero gradient) or the call succeeds on a pivot that is positive and tiny (the
    # entries it divides are of the same rounding size, so the later pivots stay what they are without that column).  For the
    # LAST column nothing follows the pivot: L_S carries -n/2 log of it, and a pivot 1e-13 of the independent column's (its share
    # of S[j][j] is above 1 / cond(S) > 1e-3) lifts the value by n/2 log 1e10 > 11 n; the test asks for n
    for j, col in ((2, Y[:, 0]), (3, 2.0 * Y[:, 1]), (5, Y[:, 0] + Y[:, 3])):
        Yc = np.array(Y)
        Yc[:, j - 1] = col
        gp.set_outputs(Yc)
        val, grad = gp.lml_grad(theta)
        print("collinear column %d: info %d value %r" % (j, gp.info, val))
        assert gp.info in (0, n + j), (j, gp.info)
        if gp.info:
            assert val == -np.inf and not grad.any() and "option 52" in gp.last_error()
        else:
            assert np.isfinite(val) and (j < Y.shape[1] or val > good + n), (j, val, good)
    # ... and the handle goes on
    gp.set_outputs(Y)
    val, grad = gp.lml_grad(theta)
    assert gp.info == 0 and np.isfinite(val) and grad.any()
    fresh = _gp(X, Y, kernel)
    v2, g2 = fresh.lml_grad(theta)
    assert v2 == val and np.array_equal(g2, grad)
    fresh.close()
    gp.close()
    # n < q + 2: mi_gp_lml_grad and mi_gp_factor return -1 with a text that names the option (the facade raises before the call)
    small = _gp(X[:6], Y[:6], kernel)  # n = 6, q = 5
    with pytest.raises(ValueError, match="q \\+ 2"):
        small.lml_grad(theta)
    assert small.lib.mi_gp_lml_grad(small.h, tp, op, op) == -1 and "option 52" in small.last_error()
    assert small.lib.mi_gp_factor(small.h, tp) == -1 and "option 52" in small.last_error()
    small.set_outputs(Y[:6, :4])  # n = q + 2
    val, _ = small.lml_grad(theta)
    assert small.info == 0 and np.isfinite(val)
    small.close()


def _target3(x):
    return np.array([3.0 * x[0] - 4.0 * x[1], 1e3 * np.sin(3.0 * x[0]) * x[1], 1e-3 * (0.2 + np.exp(x[0] - x[1]))])


def test_a_fit_of_three_outputs_on_very_different_scales():
    from andvaranaut_amd import GPMCMC, uniform

    priors = [st.uniform(loc=0, scale=2), st.uniform(loc=1, scale=0.5)]
    g = GPMCMC(kernel="RBF", noise=True, xconrevs=[uniform(priors[0]), uniform(priors[1])], yconrevs=[None] * 3, nx=2, ny=3,
               priors=priors, target=_target3, parallel=False, nproc=1, verbose=False)
    g.sample(nsamps=60, seed=1)
    g.fit(method="map", outputs="all", output_cov="integrated")
    assert g.outputs == "all" and g.output_cov == "integrated" and g.gp.get_option(51) == 3 and g.gp.get_option(52) == 1
    x = np.column_stack([2.0 * np.random.default_rng(3).random(9), 1.0 + 0.5 * np.random.default_rng(4).random(9)])
    y, yv = g.predict(x, return_var=True)
    assert y.shape == (9, 3) and yv.shape == (9, 3) and np.isfinite(y).all() and (yv > 0).all()
    # the error bars follow the outputs' scales (1 : 1e3 : 1e-3 in the targets, squared in the variances)
    # (a factor 1e6 between the scales; 1e4 of it is left to how well the one kernel fits each output)
    assert (yv[:, 1] > 1e2 * yv[:, 0]).all() and (yv[:, 2] < 1e-2 * yv[:, 0]).all()
    # converted-space variances at the fitted theta against the reference
    theta = g._theta_from_hypers(g.hypers, 1e-6)
    xin, _ = g._converted(g.x, g.y - g.ym)
    Yc = g._converted_outputs(g.y - g.ym)
    xc = np.column_stack([g.xconrevs[i].con(x[:, i]) for i in range(2)])
    _, var = g.predict(x, return_var=True, revert=False)
    var_ref = ref.predict_var(xin, Yc, xc, "RBF", theta)
    _, ptol = kfold_ref.tolerances(kfold_ref.full_cond(xin, "RBF", theta))
    e_var = np.max(np.abs(var - var_ref) / var_ref) / ptol
    print("fit(outputs='all', output_cov='integrated'): error / bound: var %.3g" % e_var)
    assert e_var <= 1.0
    # the object rebuilds its handle with the choice
    g.gp.close()
    g.gp = None
    y2, yv2 = g.predict(x, return_var=True)
    assert np.array_equal(y2, y) and np.array_equal(yv2, yv)
