"""Several outputs under one shared kernel (option 51 of mi_gp_set_option; MiGP.set_outputs, GPMCMC.fit(outputs="all")) against the
per-output oracle of tests/multi_output_ref.py: oracle.gp_oracle's LML and gradient per column at the same theta, summed, and its
conditional per column; then what the option must leave alone and what it refuses.

Bounds are the project's own, with cond = cond(K_y): loo_ref.value_ratio and loo_ref.grad_ratio for L_MO and its gradient,
kfold_ref.tolerances for the conditional's means and variance.  Every parity check prints error / bound before it asserts."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.stats as st

import bad_pivot_cases as bp
import kfold_ref
import loo_ref
import multi_output_ref as ref

pytestmark = pytest.mark.gpu

TWO = "RBF+Matern52"  # the two-component kernel


def _gp(X, Y, kernel, diag=None, **kw):
    from andvaranaut_amd import MiGP

    gp = MiGP(np.array(X), np.array(Y[:, 0]), kernel, device=0, **kw)  # (copies: the cached problems are read-only)
    if diag is not None:
        gp.set_diag(np.array(diag))
    if Y.shape[1] > 1:
        gp.set_outputs(Y)
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
    """m prediction points: the first half inside the design's box, the rest around it"""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.vstack([rng.random((m - m // 2, d)), 1.5 * rng.random((m // 2, d)) - 0.25]))


# n: an exact tile multiple, a ragged last tile, several k segments of the thin multiply and of the contraction; q: the minimum,
# one past a 16-row MFMA block, every staged row in use; every combination under both kernels, and one with a diagonal.  (The
# per-output oracle of n = 1000, q = 128 is 128 gradient evaluations: those two cases take 8 and 15 s, nearly all of it there.)
VG_CASES = [(k, n, q, False) for k in ("RBF", TWO) for n in (256, 300, 1000) for q in (2, 17, 128)] + [("RBF", 300, 17, True)]


@pytest.mark.parametrize("kernel,n,q,with_diag", VG_CASES)
def test_value_and_gradient_parity(kernel, n, q, with_diag):
    X, Y, theta, diag, cond = ref.problem(kernel, n, 3, q, with_diag, 1e-2, 7)
    v_ref, g_ref = ref.oracle_sum(X, Y, kernel, theta, diag)
    gp = _gp(X, Y[:, :1], kernel, diag)
    assert gp.get_option(51) == 1 and gp.nout == 1  # the default
    v1, _ = gp.lml_grad(theta)
    parts = gp.lml_parts()
    gp.set_outputs(Y)
    assert gp.get_option(51) == q and gp.nout == q
    val, grad = gp.lml_grad(theta)
    assert gp.info == 0
    rv, rg = loo_ref.value_ratio(val, v_ref, cond), loo_ref.grad_ratio(grad, g_ref, cond)
    print((kernel, n, q, with_diag), "cond %.3g" % cond, "error / bound: value %.3g gradient %.3g" % (rv, rg))
    assert rv <= 1.0 and rg <= 1.0, (rv, rg, val, v_ref, grad, g_ref)
    assert val != v1 and abs(grad[-1] - grad[-2]) <= 1e-12 * abs(grad[-1])  # d/d jitter = d/d gv
    assert gp.lml_parts() == parts  # the factorisation's logdet and output 0's quad
    # the same call in the same state: the same bits; so with NaN in everything the call may not read
    v2, g2 = gp.lml_grad(theta)
    assert v2 == val and np.array_equal(g2, grad)
    _nan_everything(gp)
    v3, g3 = gp.lml_grad(theta)
    assert v3 == val and np.array_equal(g3, grad)
    gp.close()


@pytest.mark.parametrize("kernel,n,q", [("RBF", 300, 17), (TWO, 256, 128)])
def test_q_copies_of_one_output(kernel, n, q):
    X, Y, theta, diag, cond = ref.problem(kernel, n, 3, 2, False, 1e-2, 7)
    y = Y[:, :1]
    gp = _gp(X, y, kernel)
    v1, g1 = gp.lml_grad(theta)
    gp.set_outputs(np.repeat(y, q, axis=1))
    val, grad = gp.lml_grad(theta)
    rv, rg = loo_ref.value_ratio(val, q * v1, cond), loo_ref.grad_ratio(grad, q * g1, cond)
    print((kernel, n, q), "copies, error / bound: value %.3g gradient %.3g" % (rv, rg))
    assert rv <= 1.0 and rg <= 1.0
    mu, var = gp.predict(theta, _points(3, 40))
    assert mu.shape == (40, q) and var.shape == (40,)
    assert all(np.array_equal(mu[:, o], mu[:, 0]) for o in range(q))
    gp.close()


@functools.lru_cache(maxsize=None)
def _conditional_case(kernel, n, q):
    X, Y, theta, _, cond = ref.problem(kernel, n, 3, q, False, 1e-2, 7)
    Xn = _points(3, 300)
    refs = {pn: ref.oracle_conditional(X, Y, Xn, kernel, theta, pred_noise=bool(pn)) for pn in (0, 1)}
    return X, Y, theta, cond, Xn, refs


@pytest.mark.parametrize("kernel,n,q", [("RBF", 300, 2), (TWO, 300, 17), ("RBF", 256, 128), (TWO, 1000, 2)])
def test_conditional_parity_and_exactly_the_outputs_are_written(kernel, n, q):
    """m = 1, 127 (the pinned route, one point and a ragged last block of 16) and 300 (device buffers, a ragged last block) with
    and without the observation noise; the C-ABI call into sentinel-filled buffers: q m and m doubles are written"""
    import torch

    X, Y, theta, cond, Xn, refs = _conditional_case(kernel, n, q)
    vtol, ptol = kfold_ref.tolerances(cond)
    gp = _gp(X, Y, kernel)
    single = _gp(X, Y[:, :1], kernel)
    for m in (1, 127, 300):
        got = {}
        for pn in (0, 1):
            mu, var = gp.predict(theta, Xn[:m], pred_noise=bool(pn))
            mu_ref, var_ref = refs[pn][0][:m], refs[pn][1][:m]
            assert mu.shape == (m, q) and var.shape == (m,)
            e_mu = np.max(np.abs(mu - mu_ref) / np.maximum(np.abs(mu_ref), 1.0)) / vtol
            e_var = np.max(np.abs(var - var_ref) / var_ref) / ptol
            mu_s, var_s = single.predict(theta, Xn[:m], pred_noise=bool(pn), via_inverse=False)
            e_one = np.max(np.abs(var - var_s) / var_s) / ptol
            e_mu0 = np.max(np.abs(mu[:, 0] - mu_s) / np.maximum(np.abs(mu_s), 1.0)) / vtol
            print((kernel, n, q), "m = %d pred_noise = %d" % (m, pn), "cond %.3g" % cond,
                  "error / bound: mean %.3g var %.3g, against the single-output predict: var %.3g mean of output 0 %.3g"
                  % (e_mu, e_var, e_one, e_mu0))
            assert e_mu <= 1.0 and e_var <= 1.0 and e_one <= 1.0 and e_mu0 <= 1.0
            got[pn] = (mu, var)
        assert np.array_equal(got[0][0], got[1][0])
        assert np.allclose(got[1][1] - got[0][1], np.sqrt(theta[-2]) ** 2, rtol=1e-9, atol=1e-14)  # the difference is gv
        # NaN in the work block and in W's upper triangle: the same bits
        _nan_everything(gp)
        mu2, var2 = gp.predict(theta, Xn[:m], pred_noise=True)
        assert np.array_equal(mu2, got[1][0]) and np.array_equal(var2, got[1][1])
        # the entry point itself, into buffers filled with a sentinel
        mp = (m + 127) // 128 * 128
        out = torch.full((q * m + m + 64,), -7.25, dtype=torch.float64, device=gp.dev)
        xn = torch.from_numpy(Xn[:m].copy()).to(gp.dev)
        work = torch.full((mp, gp.lda), float("nan"), dtype=torch.float64, device=gp.dev)
        torch.cuda.synchronize()
        base = out.data_ptr()
        assert gp.lib.mi_gp_predict(gp.h, xn.data_ptr(), m, work.data_ptr(), gp.lda, base + 8 * 16, base + 8 * (32 + q * m), 1) == 0
        o = out.cpu().numpy()
        assert np.array_equal(o[16 : 16 + q * m].reshape(q, m).T, got[1][0]) and np.array_equal(o[32 + q * m : 32 + q * m + m], got[1][1])
        rest = np.r_[o[:16], o[16 + q * m : 32 + q * m], o[32 + q * m + m :]]
        assert (rest == -7.25).all()
    gp.close()
    single.close()


def _everything(gp, theta, Xn):
    return [*gp.lml_grad(theta), *gp.predict(theta, Xn, via_inverse=False)]


def test_the_same_bits_again_under_event_edges_and_behind_a_larger_q_full_of_nan():
    import torch

    kernel, n, q = TWO, 300, 5
    X, Y, theta, _, _ = ref.problem(kernel, n, 3, 128, False, 1e-2, 7)
    Xn = _points(3, 50)
    gp = _gp(X, Y[:, :q], kernel)
    want = _everything(gp, theta, Xn)
    again = _everything(gp, theta, Xn)
    assert all(np.array_equal(a, b) for a, b in zip(again, want))
    gp.close()
    gp = _gp(X, Y[:, :q], kernel)
    gp.set_option(26, 0)
    assert all(np.array_equal(a, b) for a, b in zip(_everything(gp, theta, Xn), want))
    gp.close()
    # the scratch re-used: 128 outputs first, those from q on all NaN (planted in the device copy: set_outputs takes finite data
    # only), so that the staged rows from q on, every column of V and the partial products hold NaN when the q outputs follow
    gp = _gp(X, Y, kernel)
    gp._Y_store[q:].fill_(float("nan"))
    torch.cuda.synchronize()
    val, _ = gp.lml_grad(theta)
    mu, _ = gp.predict(theta, Xn)
    assert np.isnan(val) and np.isnan(mu[:, q:]).all() and np.array_equal(mu[:, :q], want[2])
    gp.set_outputs(Y[:, :q])
    _nan_everything(gp)
    assert all(np.array_equal(a, b) for a, b in zip(_everything(gp, theta, Xn), want))
    gp.close()


def test_switching_back_returns_a_fresh_handles_bits():
    kernel, n = "RBF", 300
    X, Y, theta, _, _ = ref.problem(kernel, n, 3, 3, False, 1e-2, 7)
    Xn = _points(3, 20)
    fresh = _gp(X, Y[:, :1], kernel)
    want = _everything(fresh, theta, Xn)
    fresh.close()
    gp = _gp(X, Y, kernel)
    under = _everything(gp, theta, Xn)
    assert under[0] != want[0] and under[2].shape == (20, 3)
    # option 51 = 1 straight behind an evaluation under q = 3: y_dev still starts with output 0
    gp.set_option(51, 1)
    gp.nout = 1
    assert all(np.array_equal(a, b) for a, b in zip(_everything(gp, theta, Xn), want))
    # ... and the facade's way back
    gp.set_outputs(Y)
    assert all(np.array_equal(a, b) for a, b in zip(_everything(gp, theta, Xn), under))
    gp.set_outputs(Y[:, :1])
    assert gp.get_option(51) == 1
    assert all(np.array_equal(a, b) for a, b in zip(_everything(gp, theta, Xn), want))
    gp.close()


def test_every_other_entry_point_is_refused_with_its_text_and_the_handle_keeps_its_state():
    import torch

    kernel, n = "RBF", 300
    X, Y, theta, _, _ = ref.problem(kernel, n, 3, 3, False, 1e-2, 7)
    Xn = _points(3, 20)
    gp = _gp(X, Y, kernel)
    lib, h = gp.lib, gp.h
    before = gp.predict(theta, Xn)
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
        assert name in text and "51" in text, (name, text)
    # no cross-validation objective under several outputs (a trend ends the resident state by its own rule: it is tried on a
    # second handle below)
    gp.set_option(48, 1)
    assert lib.mi_gp_lml_grad(h, tp, op, op) == -1 and "51" in gp.last_error() and "option 48" in gp.last_error()
    gp.set_option(48, 0)
    # the handle is still factored: the refusals touched nothing, and the prediction has the bits it had
    assert gp._factored_ok
    after = gp.predict(theta, Xn)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    # values outside 1 .. 128
    for bad in (0, 129, -1):
        assert lib.mi_gp_set_option(h, 51, bad) == -1 and "option 51" in gp.last_error()
    assert gp.get_option(51) == 3
    # behind a multi-output mi_gp_lml_grad W_dev holds q K^-1 - V V^T: mi_gp_kfold is refused under the option, with the option's
    # text, and once the option is back at 1 because K^-1 is not resident (another value ends the resident state, as
    # mi_gp_set_data does), with that text
    gp.lml_grad(theta)
    gp.set_option(51, 3)  # (the current value: changes nothing)
    assert calls["mi_gp_kfold"]() == -1 and "mi_gp_kfold" in gp.last_error() and "option 51" in gp.last_error()
    gp.set_option(51, 1)
    assert calls["mi_gp_kfold"]() == -1 and "K^-1 is not resident" in gp.last_error()
    assert calls["mi_gp_alpha"]() == -1 and "51" not in gp.last_error()
    gp.set_option(51, 3)
    # the facade raises before the call
    for call in (lambda: gp.lml(theta), lambda: gp.predict(theta, Xn, via_inverse=True), lambda: gp.predict_grad(theta, Xn),
                 lambda: gp.predict_cov(theta, Xn), lambda: gp.kfold(theta, [np.arange(3)]), lambda: gp.lml_grad_data(theta),
                 lambda: gp.lml_batch(th[None]), lambda: gp.sample_posterior(theta, Xn, 1), lambda: gp.logpdf(theta, Xn[:1], Y[:1, 0]),
                 lambda: gp.update_data(y=Y[:, 0]), lambda: gp.set_outputs(np.full((n, 2), np.nan)), lambda: gp.set_outputs(Y[:5])):
        with pytest.raises(ValueError, match="outputs"):
            call()
    gp.close()
    # a trend and several outputs: mi_gp_lml_grad and mi_gp_factor are refused
    gp = _gp(X, Y, kernel)
    gp.set_option(50, 1)
    assert gp.lib.mi_gp_lml_grad(gp.h, tp, op, op) == -1 and "51" in gp.last_error()
    assert gp.lib.mi_gp_factor(gp.h, tp) == -1 and "51" in gp.last_error()
    gp.set_option(50, 0)
    val, _ = gp.lml_grad(theta)
    assert np.isfinite(val)
    gp.close()


def test_a_bad_pivot_gives_info_minus_infinity_and_a_zero_gradient():
    X, y = bp.problem(300)
    Y = ref.make_outputs(X, y, 3, 5)
    gp = _gp(X, Y, bp.KERNEL)
    val, grad = gp.lml_grad(bp.minus_ten_theta())
    assert gp.info == 1 and val == -np.inf and not grad.any()
    val, grad = gp.lml_grad(bp.good_theta())
    assert gp.info == 0 and np.isfinite(val) and grad.any()
    gp.close()


def test_reserve_behind_factor_keeps_the_prediction_bits():
    import torch

    kernel = "RBF"
    X, Y, theta, _, _ = ref.problem(kernel, 300, 3, 5, False, 1e-2, 7)
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
    # a reserve behind an evaluation alone: nothing is factored, the scratch holds nothing to keep and the next use re-sizes it
    val, grad = gp.lml_grad(theta)
    assert gp.lib.mi_gp_reserve(gp.h, 200) == 0
    v2, g2 = gp.lml_grad(theta)
    assert v2 == val == want[0] and np.array_equal(g2, grad)
    assert all(np.array_equal(u, v) for u, v in zip(_everything(gp, theta, Xn), want))  # (the leading dimension changes no bit)
    assert gp.lib.mi_gp_reserve(gp.h, 300) == 0
    got = gp.predict(theta, Xn)  # (the facade does not factor again: same theta)
    assert np.array_equal(got[0], want[2]) and np.array_equal(got[1], want[3])
    assert all(np.array_equal(u, v) for u, v in zip(_everything(gp, theta, Xn), want))
    gp.close()
    roomy = _gp(X, Y, kernel, capacity=300)
    assert all(np.array_equal(u, v) for u, v in zip(_everything(roomy, theta, Xn), want))
    roomy.close()


def _target3(x):
    return np.array([3.0 * x[0] - 4.0 * x[1], np.sin(3.0 * x[0]) * x[1], 0.2 + np.exp(x[0] - x[1])])


def test_fit_with_every_output_and_the_default_is_the_single_output_fit():
    from andvaranaut_amd import GPMCMC, logarithm, uniform

    priors = [st.uniform(loc=0, scale=2), st.uniform(loc=1, scale=0.5)]

    def make(ny, target, ycon):
        return GPMCMC(kernel="RBF", noise=True, xconrevs=[uniform(priors[0]), uniform(priors[1])], yconrevs=ycon, nx=2, ny=ny,
                      priors=priors, target=target, parallel=False, nproc=1, verbose=False)

    g = make(3, _target3, [None, None, logarithm()])
    g.sample(nsamps=60, seed=1)
    g.fit(method="map", outputs="all")
    assert g.outputs == "all" and g.gp.get_option(51) == 3
    x = np.column_stack([2.0 * np.random.default_rng(3).random(9), 1.0 + 0.5 * np.random.default_rng(4).random(9)])
    y, yv = g.predict(x, return_var=True)
    assert y.shape == (9, 3) and yv.shape == (9, 3) and np.isfinite(y).all() and (yv > 0).all()
    mu, var = g.predict(x, return_var=True, revert=False)
    assert mu.shape == (9, 3) and var.shape == (9, 3)
    # converted-space moments at the fitted theta against the per-output oracle
    theta = g._theta_from_hypers(g.hypers, 1e-6)
    xin, _ = g._converted(g.x, g.y - g.ym)
    Yc = g._converted_outputs(g.y - g.ym)
    xc = np.column_stack([g.xconrevs[i].con(x[:, i]) for i in range(2)])
    mu_ref, var_ref = ref.oracle_conditional(xin, Yc, xc, "RBF", theta)
    cond = kfold_ref.full_cond(xin, "RBF", theta)
    vtol, ptol = kfold_ref.tolerances(cond)
    e_mu = np.max(np.abs(mu - mu_ref) / np.maximum(np.abs(mu_ref), 1.0)) / vtol
    e_var = np.max(np.abs(var - var_ref[:, None]) / var_ref[:, None]) / ptol
    print("fit(outputs='all'): cond %.3g, error / bound: mean %.3g var %.3g" % (cond, e_mu, e_var))
    assert e_mu <= 1.0 and e_var <= 1.0
    # the third column went through its own conversion (a logarithm): its reverted mean is positive
    assert (y[:, 2] > 0).all()
    for name in ("predict_joint", "sample_posterior"):
        with pytest.raises(ValueError, match="outputs"):
            getattr(g, name)(x)
    # the default models the first output alone, as a one-output object does on that column
    g.fit(method="map")
    assert g.outputs == "first" and g.gp.get_option(51) == 1
    g1 = make(1, lambda x: _target3(x)[:1], [None])
    g1.set_data(g.x, np.ascontiguousarray(g.y[:, :1]))
    g1.fit(method="map")
    for k in g1.hypers:
        assert np.array_equal(np.asarray(g.hypers[k]), np.asarray(g1.hypers[k])), k
    assert np.array_equal(g.predict(x), g1.predict(x))
