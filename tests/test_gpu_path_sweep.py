"""The path sweep (options 54 / 55 of mi_gp_set_option, csrc/paths_f64.hip, csrc/api_paths.hip) on the device: the evaluation
of random path blocks against the np.longdouble restatement of tests/paths_ref.py with its element-wise bounds, and the bits of
a path at a point against calls with other m, S, columns, outputs and chunks; the conditioning by its backward error and the
at-the-data identity; the moments of MiGP.draw_paths against the oracle's posterior; the raw call's contract and the state it
leaves; and the facade's sample_paths and per-path sensitivity estimates (tests/test_paths_host.py validates the references on
the CPU)."""
import ctypes

import numpy as np
import pytest

import grad_refs as gr
import mean_sweep_ref as ms
import paths_ref as pr
import resident_checks as rc
from andvaranaut_amd import paths
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

LD, EPS = pr.LD, pr.EPS
FIVE = "RBF+Matern52+Matern32+Exponential+RatQuad"  # (the run-time component count: gradient windows of 8)
# (kernel, n, d, F): every family and a three-component fold; n = 63, 130; d on both sides of each register window; F = 16, 48, 1040
EVAL_CASES = [("RBF", 63, 1, 16), ("Matern52", 130, 4, 48), ("Matern32", 63, 5, 1040), ("Exponential", 130, 16, 48),
              ("RatQuad", 63, 17, 16), ("RBF+Matern52*Matern32", 130, 32, 1040), ("Matern52+RBF", 130, 2, 48), (FIVE, 63, 5, 16),
              (FIVE, 130, 17, 48)]
M_ALL = 257
M_PREFIXES = (1, 63, 64, 65)
REF_POINTS = np.array([0, 1, 62, 63, 64, 65, 128, 255, 256])  # the gradient's references (the values': every point)
# c of the conditioning's backward error c n eps (|K_y||V| + |R|): V = (R^T U) U^T is two products on the GEMM, each within
# resident_checks.bound_gemm(n) / n = 2 of n eps |A||B|, against a U that resident_checks holds to U_MARGIN = 16 times the
# reference inverse's own residual -- 2 + 2 + 16
C_COND = 2 * rc.bound_gemm(1) + rc.U_MARGIN


def _migp():
    import torch

    assert torch.cuda.is_available()
    from andvaranaut_amd import MiGP

    return MiGP


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def _raw(gp, x_t, m, block_t, ldw, mean_t, dmean_t, condition, var_t=None, dvar_t=None):
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    return gp.lib.mi_gp_predict_grad(gp.h, p(x_t), m, p(block_t), ldw, p(mean_t), p(var_t), condition, p(dmean_t), p(dvar_t))


def _draw_of(gp, omega, b, W, V, ldw=None):
    """A PathDraw over a block of the test's own making (condition = 0 evaluates whatever the block holds)."""
    S, F = W.shape[1], W.shape[0]
    ldw = paths.block_ldw(S) if ldw is None else ldw
    return paths.PathDraw(gp, _dev(paths.pack_block(omega, b, W, V, ldw)), S, F, ldw, None, gp._path_serial)


def _random_block(n, d, F, S, seed):
    rng = np.random.default_rng(seed)
    omega = 3.0 * rng.standard_normal((F, d))
    omega[0] = 1e6 / np.sqrt(d) * np.where(rng.random(d) < 0.5, -1.0, 1.0)  # |om| ~ 1e6: the argument reduction
    return omega, rng.random(F) * 2.0 * np.pi, rng.standard_normal((F, S)), rng.standard_normal((n, S))


@pytest.mark.parametrize("kernel,n,d,F", EVAL_CASES, ids=[gr.case_id(c) for c in EVAL_CASES])
def test_evaluation_against_longdouble_and_bit_independence(kernel, n, d, F):
    """condition = 0 on random V, W, Omega and b (no cond(K) enters), 128 paths at 257 points -- point 0 a training point, feature 0
    with |om| ~ 1e6: |device - reference| <= bound of paths_ref.eval_reference, values at every point, gradients at REF_POINTS.
    Then the same bits from: a repetition, the value-only call, another chunk, the first S columns alone for S = 1, T - 1, T,
    T + 1, 2 T + 1 of both tiles (value-only and gradient), the first m points for m = 1, 63, 64, 65, one point alone, and one
    column alone copied into an S = 1 block."""
    MiGP = _migp()
    X, y = ms.problem(n, d, seed=11 * n + d)
    theta = gr.well_conditioned_theta(kernel, d)
    Xn = np.random.default_rng(n + d).random((M_ALL, d))
    Xn[0] = X[3]
    omega, b, W, V = _random_block(n, d, F, 128, seed=5 * n + d)
    gp = MiGP(X, y, kernel)
    try:
        assert gp.factor(theta) == 0
        full = _draw_of(gp, omega, b, W, V)
        val, dval = full.evaluate(Xn, grad=True)
        assert gp.get_option(54) == 0 and gp.get_option(55) == F
        assert val.shape == (128, M_ALL) and dval.shape == (128, M_ALL, d)
        again = full.evaluate(Xn, grad=True)
        only = full.evaluate(Xn)
        chunked = full.evaluate(Xn, grad=True, chunk=100)
        assert _same_bits(val, again[0]) and _same_bits(dval, again[1]) and _same_bits(val, only)
        assert _same_bits(val, chunked[0]) and _same_bits(dval, chunked[1])
        sizes = sorted({1, 128} | {s for T in (paths.path_tile(d, False), paths.path_tile(d, True))
                                   for s in (T - 1, T, T + 1, 2 * T + 1) if s >= 1})
        for S in sizes[:-1]:
            part = _draw_of(gp, omega, b, W[:, :S], V[:, :S])
            pv, pd = part.evaluate(Xn, grad=True)
            assert _same_bits(pv, val[:S]) and _same_bits(pd, dval[:S]), S
            assert _same_bits(part.evaluate(Xn), val[:S]), S
        three = _draw_of(gp, omega, b, W[:, :3], V[:, :3], ldw=6)
        for m in M_PREFIXES:
            pv, pd = three.evaluate(Xn[:m], grad=True)
            assert _same_bits(pv, val[:3, :m]) and _same_bits(pd, dval[:3, :m]), m
        pv, pd = three.evaluate(Xn[200:201], grad=True)
        assert _same_bits(pv, val[:3, 200:201]) and _same_bits(pd, dval[:3, 200:201])
        col = _draw_of(gp, omega, b, W[:, 77:78], V[:, 77:78])
        pv, pd = col.evaluate(Xn, grad=True)
        assert _same_bits(pv, val[77:78]) and _same_bits(pd, dval[77:78])
    finally:
        gp.close()
    ref, bound = pr.eval_reference(X, kernel, theta, omega, b, W, V, Xn, grad=False)
    Xr = np.ascontiguousarray(Xn[REF_POINTS])
    _, _, gref, gbound = pr.eval_reference(X, kernel, theta, omega, b, W, V, Xr)
    r_val = gr.max_ratio(val, ref, bound)
    r_grad = gr.max_ratio(dval[:, REF_POINTS], gref, gbound)
    print(f"path sweep {kernel} n={n} d={d} F={F}: value error / bound {r_val:.4f}, gradient error / bound {r_grad:.4f}")
    assert r_val <= 1.0 and r_grad <= 1.0, (r_val, r_grad)


def _cond_bound(Ky, V, R, R_bound, n):
    return LD(C_COND * n) * LD(EPS) * (np.abs(Ky).astype(LD) @ np.abs(V).astype(LD) + np.abs(R)) + R_bound


def _conditioning_checks(gp, X, y, kernel, theta, S, F, seed, tag):
    """condition = 1, m = 0 on a random block at the factored theta; the backward error of V and the at-the-data identity."""
    n, d = X.shape
    rng = np.random.default_rng(seed)
    omega = rng.standard_normal((F, d)) / theta[:d][None, :]
    b, W = rng.random(F) * 2.0 * np.pi, rng.standard_normal((F, S)) * np.sqrt(2.0 / F)
    _, _, _, gv, jit = orc.split_theta(theta, d, len(gr.split(kernel)[0]))
    E = np.sqrt(gv + jit) * rng.standard_normal((n, S))
    ldw = paths.block_ldw(S)
    blk = _dev(paths.pack_block(omega, b, W, E, ldw))
    gp.set_option(55, F)
    gp.set_option(54, S)
    try:
        assert _raw(gp, None, 0, blk, ldw, None, None, 1) == 0, gp.last_error()
    finally:
        gp.set_option(54, 0)
    om2, b2, W2, V = paths.unpack_block(_host(blk), F, d, ldw, n, S)
    assert _same_bits(om2, omega) and _same_bits(b2, b) and _same_bits(W2, W) and np.isfinite(V).all()
    R, R_bound = pr.residual_reference(X, y, omega, b, W, E)
    Ky = pr.noisy_cov(X, kernel, theta)
    bound = _cond_bound(Ky, V, R, R_bound, n)
    r_back = float(np.max(np.abs(Ky.astype(LD) @ V.astype(LD) - R) / bound))
    # at the data: f_s(X) = y - E - D V, D = K_y - K_f
    draw = paths.PathDraw(gp, blk, S, F, ldw, None, gp._path_serial)
    f = draw.evaluate(X)
    _, f_bound = pr.eval_reference(X, kernel, theta, omega, b, W, V, X, grad=False)
    rhs = y[:, None].astype(LD) - E.astype(LD) - pr.noise_part(X, kernel, theta) @ V.astype(LD)
    r_data = float(np.max(np.abs(f.T.astype(LD) - rhs) / (bound + f_bound.T)))
    print(f"conditioning {tag} {kernel} n={n} S={S}: backward error / bound {r_back:.4f} (c = {C_COND}), at the data {r_data:.4f}")
    assert r_back <= 1.0 and r_data <= 1.0, (r_back, r_data)


@pytest.mark.parametrize("S", (3, 128))
@pytest.mark.parametrize("kernel", ("Matern52+RBF", "Exponential"))
@pytest.mark.parametrize("n", (130, 300))
def test_conditioning_backward_error_and_the_identity_at_the_data(n, kernel, S):
    """|K_y V - R_ref| <= c n eps (|K_y||V| + |R_ref|) + R's own bound, K_y = oracle.noisy_cov (the matrix the device factorised),
    R_ref = y - Phi W - E in np.longdouble; and f_s(X) = y - E - D V within the same bound plus the evaluation's."""
    MiGP = _migp()
    X, y = ms.problem(n, 3, seed=n + 1)
    theta = gr.well_conditioned_theta(kernel, 3)
    gp = MiGP(X, y, kernel)
    try:
        assert gp.factor(theta) == 0
        _conditioning_checks(gp, X, y, kernel, theta, S, 64, seed=n + S, tag="fresh")
    finally:
        gp.close()


def test_zero_noise_draw_and_zero_prior_give_alpha():
    """E = 0, W = 0, S = 1: V = K_y^-1 y, mi_gp_alpha within (64 + 8 cond) eps of the largest |alpha|; and mi_gp_alpha returns the
    bits it returned before the path calls."""
    MiGP = _migp()
    n, d, kernel, F = 130, 3, "Matern52+RBF", 16
    X, y = ms.problem(n, d, seed=8)
    theta = gr.well_conditioned_theta(kernel, d)
    cond = float(np.linalg.cond(pr.noisy_cov(X, kernel, theta)))

    def alpha_of(gp):
        gp.lml_grad(theta)
        out = np.empty(n)
        assert gp.lib.mi_gp_alpha(gp.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 0
        return out

    gp = MiGP(X, y, kernel)
    try:
        alpha = alpha_of(gp)
        assert gp.factor(theta) == 0
        blk = _dev(paths.pack_block(np.ones((F, d)), np.zeros(F), np.zeros((F, 1)), np.zeros((n, 1)), 2))
        gp.set_option(55, F)
        gp.set_option(54, 1)
        assert _raw(gp, None, 0, blk, 2, None, None, 1) == 0, gp.last_error()
        gp.set_option(54, 0)
        V = paths.unpack_block(_host(blk), F, d, 2, n, 1)[3][:, 0]
        assert _same_bits(alpha_of(gp), alpha)
    finally:
        gp.close()
    ratio = np.abs(V - alpha).max() / ((64.0 + 8.0 * cond) * EPS * np.abs(alpha).max())
    print(f"V against mi_gp_alpha: cond {cond:.0f}, error / bound {ratio:.4f}")
    assert ratio <= 1.0


def test_moments_on_the_device_and_one_draw_against_the_reference():
    """32 draws of 128 paths through MiGP.draw_paths at n = 40, d = 2, Matern52 (the seeds for which test_paths_host.py holds the
    reference inside the caps): path means within 5 standard errors of the oracle's posterior mean at 12 points, variance
    ratios in [0.85, 1.15].  The first draw against path_reference of the same seed: the evaluation's bound plus
    |K(X*, X)| |K_y^-1| times the conditioning's bound."""
    MiGP = _migp()
    X, y, theta, Xt, mu, var = pr.moment_problem()
    kernel, S, F = pr.MOMENT_KERNEL, pr.MOMENT_S, pr.MOMENT_F
    gp = MiGP(X, y, kernel)
    try:
        vals = []
        for i, seed in enumerate(pr.MOMENT_SEEDS):
            draw = gp.draw_paths(theta, S, F, seed=seed)
            vals.append(draw.evaluate(Xt))
            if i == 0:
                first = draw.host_block()
                assert (draw.npaths, draw.nfeatures, draw.ldw, draw.seed) == (S, F, S, seed)
            draw.close()
        assert gp.get_option(54) == 0
    finally:
        gp.close()
    vals = np.vstack(vals)
    z, lo, hi = pr.moment_margins(vals, mu, var)
    print(f"device moments over {vals.shape[0]} paths: mean within {z:.2f} standard errors (cap 5), variance ratios {lo:.3f} .. "
          f"{hi:.3f} (caps 0.85, 1.15)")
    assert z <= 5.0 and 0.85 <= lo and hi <= 1.15
    ref = pr.path_reference(X, y, kernel, theta, pr.MOMENT_SEEDS[0], S, F, Xt, precise=True)
    omega, b, W, V = first
    assert _same_bits(omega, ref["omega"]) and _same_bits(b, ref["b"]) and _same_bits(W, ref["W"])
    R, R_bound = pr.residual_reference(X, y, omega, b, W, ref["E"])
    Ky = pr.noisy_cov(X, kernel, theta)
    cb = _cond_bound(Ky, V, R, R_bound, X.shape[0])
    _, eb = pr.eval_reference(X, kernel, theta, omega, b, W, V, Xt, grad=False)
    spread = np.abs(pr.kernel_ld(X, kernel, theta, Xt)) @ (np.abs(np.linalg.inv(Ky)).astype(LD) @ cb)
    ratio = float(np.max(np.abs(vals[:S].astype(LD) - ref["values"]) / (eb + spread.T)))
    print(f"one device draw against path_reference: error / bound {ratio:.4f}")
    assert ratio <= 1.0


def test_options_refusals_and_untouched_state():
    """Options 54 / 55: ranges and read-back.  Every refusal returns -1 with its text and leaves the outputs and the block as they
    were.  With option 54 back at 0, predict_grad and mean_sweep return their earlier bits; var_dev / dvar_dev stay NaN."""
    MiGP = _migp()
    kernel, n, d, S, F = "Matern32", 140, 3, 4, 32
    X, y = ms.problem(n, d, seed=3)
    theta = gr.well_conditioned_theta(kernel, d)
    Xn = np.random.default_rng(6).random((12, d))
    x_t = _dev(Xn)
    omega, b, W, V = _random_block(n, d, F, S, seed=2)
    block = paths.pack_block(omega, b, W, V, 4)
    blk = _dev(block)
    mean, dmean = _dev(np.full(S * 12, -77.5)), _dev(np.full((S * 12, d), -77.5))

    def refused(gp, words, m=12, ldw=4, condition=0, outputs=True, x=x_t):
        r = _raw(gp, x, m, blk, ldw, mean if outputs else None, dmean if outputs else None, condition)
        text = gp.last_error()
        assert r == -1 and all(w in text for w in words), (r, text)
        assert (_host(mean) == -77.5).all() and (_host(dmean) == -77.5).all() and _same_bits(_host(blk), block)

    gp = MiGP(X, y, kernel)
    try:
        assert gp.get_option(54) == 0 and gp.get_option(55) == 1024
        for bad in (-1, 129):
            assert gp.lib.mi_gp_set_option(gp.h, 54, bad) == -1 and "option 54" in gp.last_error() and gp.get_option(54) == 0
        for bad in (0, 8, 24, 65552):
            assert gp.lib.mi_gp_set_option(gp.h, 55, bad) == -1 and "option 55" in gp.last_error() and gp.get_option(55) == 1024
        gp.set_option(55, 65536)
        assert gp.get_option(55) == 65536
        gp.set_option(55, F)
        gp.set_option(54, 128)
        assert gp.get_option(54) == 128
        gp.set_option(54, S)
        refused(gp, ("option 54", "mi_gp_factor"))  # before mi_gp_factor
        gp.set_option(54, 0)
        before = gp.predict_grad(theta, Xn[:9])
        sweep = gp.mean_sweep(theta, Xn, grad=True)
        gp.set_option(54, 2)
        gp.set_option(53, 1)
        refused(gp, ("option 53", "option 54"))
        gp.set_option(53, 0)
        gp.set_option(54, S)
        refused(gp, ("option 54", "ldw"), ldw=5)
        refused(gp, ("option 54", "ldw"), ldw=2)
        refused(gp, ("option 54", "mean_dev"), outputs=False)
        refused(gp, ("option 54", "m = 0"), m=0)
        refused(gp, ("option 54",), m=-1)
        refused(gp, ("option 54", "Xnew_dev"), x=None)
        # the call itself: NaN in var_dev / dvar_dev stays NaN, the block is not written under condition = 0
        var, dvar = _dev(np.full(S * 12, np.nan)), _dev(np.full((S * 12, d), np.nan))
        assert _raw(gp, x_t, 12, blk, 4, mean, dmean, 0, var, dvar) == 0, gp.last_error()
        assert np.isnan(_host(var)).all() and np.isnan(_host(dvar)).all() and _same_bits(_host(blk), block)
        ref, bound, gref, gbound = pr.eval_reference(X, kernel, theta, omega, b, W, V, Xn)
        assert gr.max_ratio(_host(mean).reshape(S, 12), ref, bound) <= 1.0
        assert gr.max_ratio(_host(dmean).reshape(S, 12, d), gref, gbound) <= 1.0
        mean.fill_(-77.5)
        dmean.fill_(-77.5)
        gp.set_option(50, 1)  # (ends the resident state itself, as mi_gp_set_data does)
        refused(gp, ("option 54", "option 50"))
        gp.set_option(50, 0)
        gp.set_option(51, 2)
        refused(gp, ("option 54", "option 51"))
        gp.set_option(51, 1)
        gp.set_option(54, 0)
        after = gp.predict_grad(theta, Xn[:9])
        assert all(_same_bits(a, c) for a, c in zip(before, after))
        again = gp.mean_sweep(theta, Xn, grad=True)
        assert _same_bits(again[0], sweep[0]) and _same_bits(again[1], sweep[1])
    finally:
        gp.close()
    gp = MiGP(X, y, kernel, need_grad=False)
    try:
        assert gp.factor(theta) == 0
        gp.set_option(55, F)
        gp.set_option(54, S)
        refused(gp, ("option 54", "Z_dev"))
        gp.set_option(54, 0)
        with pytest.raises(RuntimeError):
            gp.draw_paths(theta, S, F)
    finally:
        gp.close()
    X9, y9 = ms.problem(6, 33, seed=4)
    gp = MiGP(X9, y9, "RBF")
    try:
        assert gp.factor(gr.well_conditioned_theta("RBF", 33)) == 0
        gp.set_option(55, F)
        gp.set_option(54, S)
        refused(gp, ("option 54", "32"), x=_dev(np.random.default_rng(7).random((12, 33))))
        gp.set_option(54, 0)
        with pytest.raises(ValueError, match="d <= 32"):
            gp.draw_paths(gr.well_conditioned_theta("RBF", 33), S, F)
    finally:
        gp.close()


def test_a_path_draw_goes_stale_and_a_fresh_draw_follows_an_append_across_a_tile():
    """A PathDraw raises after append, after factor at another theta and after close; python refusals under a trend and several
    outputs; the same seed gives the same bits; and a fresh conditioning after an append across n = 128 passes the conditioning
    checks on all 140 points."""
    MiGP = _migp()
    kernel, d = "Matern52", 3
    X, y = ms.problem(140, d, seed=9)
    theta = gr.well_conditioned_theta(kernel, d)
    theta2 = theta.copy()
    theta2[:d] *= 1.1
    Xn = np.random.default_rng(8).random((33, d))
    gp = MiGP(X[:120], y[:120], kernel, capacity=200)
    try:
        draw = gp.draw_paths(theta, 5, 64, seed=12)
        v = draw.evaluate(Xn)
        assert v.shape == (5, 33) and _same_bits(v, draw.evaluate(Xn))  # (the same factorisation: predictions do not end it)
        gp.predict(theta, Xn)
        assert _same_bits(v, draw.evaluate(Xn))
        twin = gp.draw_paths(theta, 5, 64, seed=12)
        assert _same_bits(twin.evaluate(Xn), v) and not _same_bits(gp.draw_paths(theta, 5, 64, seed=13).evaluate(Xn), v)
        assert gp.append(X[120:], y[120:]) == 0 and gp.n == 140
        with pytest.raises(RuntimeError, match="draw again"):
            draw.evaluate(Xn)
        _conditioning_checks(gp, X, y, kernel, theta, 7, 64, seed=4, tag="after an append 120 + 20")
        draw = gp.draw_paths(theta, 5, 64, seed=12)
        assert draw.n == 140 and draw.evaluate(Xn, grad=True)[1].shape == (5, 33, d)
        assert gp.factor(theta2) == 0
        with pytest.raises(RuntimeError, match="draw again"):
            draw.evaluate(Xn)
        gp.set_trend("constant")
        with pytest.raises(ValueError, match="has no form under a trend"):
            gp.draw_paths(theta, 5, 64)
        gp.set_trend("none")
        gp.set_outputs(np.stack([y, y * y], axis=1))
        with pytest.raises(ValueError, match="has no form under several outputs"):
            gp.draw_paths(theta, 5, 64)
        gp.set_outputs(y)
        draw = gp.draw_paths(theta, 5, 64, seed=12)
        assert gp.get_option(54) == 0
    finally:
        gp.close()
    with pytest.raises(RuntimeError, match="closed"):
        draw.evaluate(Xn)


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


def test_facade_sample_paths_and_per_path_sensitivity(fitted):
    """sample_paths in the original space against central differences of itself (predict_mean's test); first_paths of
    sobol_indices(npaths=4) is sobol_from_evaluations of the path object on the facade's own design, bit for bit; with npaths=0
    the three methods return what their parent code path returns, bit for bit; y_dist(npaths=3) has the stated shapes."""
    from andvaranaut_amd import sensitivity as sens
    from andvaranaut_amd.lhc import latin_sample

    g = fitted
    Xs = latin_sample(g.priors, 40, 3)
    draws = g.sample_paths(npaths=3, nfeatures=512, seed=17)
    y0, g0 = draws(Xs, return_grad=True)
    assert y0.shape == (3, 40) and g0.shape == (3, 40, 2) and _same_bits(y0, draws(Xs))
    fc, _ = draws(Xs, revert=False, return_grad=True)
    assert _same_bits(y0, np.stack([g.yconrevs[0].rev(f) for f in fc]))
    Xc, _ = g._converted_x(Xs, True)
    assert _same_bits(fc, draws(Xc, convert=False, revert=False))
    for i in range(2):
        h = 1e-5
        xp, xm = Xs.copy(), Xs.copy()
        xp[:, i] += h
        xm[:, i] -= h
        fd = (draws(xp) - draws(xm)) / (2 * h)
        assert np.abs(fd - g0[:, :, i]).max() <= 1e-5 * max(np.abs(g0[:, :, i]).max(), 1.0), i
    assert not _same_bits(y0[0], y0[1])
    # the draws scatter about the posterior mean on the scale of the predictive standard deviation
    mu = g.predict_mean(Xs, revert=False)[:, 0]
    _, yv = g.predict(Xs, revert=False, return_var=True)
    assert np.abs(fc - mu[None, :]).max() <= 8.0 * np.sqrt(np.max(yv))
    # Sobol indices: the mean-based part as before, the per-path part from the same design
    M = 128
    sob0 = g.sobol_indices(nsamps=M, seed=11, revert=False)
    sob = g.sobol_indices(nsamps=M, seed=11, revert=False, npaths=4, nfeatures=512, path_seed=23)
    sa, sb = np.random.SeedSequence(11).spawn(2)
    A, B = latin_sample(g.priors, M, np.random.default_rng(sa)), latin_sample(g.priors, M, np.random.default_rng(sb))
    D = sens.saltelli_design(A, B)
    f = g.predict_mean(D, revert=False)[:, 0]
    parent = sens.sobol_from_evaluations(*sens.split_saltelli(f, 2))
    assert set(sob0) == {"first", "total", "mean", "var"}
    for got in (sob0, sob):
        assert _same_bits(got["first"], parent[0]) and _same_bits(got["total"], parent[1])
        assert got["mean"] == parent[2] and got["var"] == parent[3]
    fp = g.sample_paths(4, 512, seed=23)(D, revert=False)
    per = [sens.sobol_from_evaluations(*sens.split_saltelli(fs, 2)) for fs in fp]
    assert sob["first_paths"].shape == (4, 2) and sob["total_paths"].shape == (4, 2)
    assert _same_bits(sob["first_paths"], np.array([r[0] for r in per]))
    assert _same_bits(sob["total_paths"], np.array([r[1] for r in per]))
    print(f"facade Sobol: first {sob['first']}, per path {sob['first_paths'].tolist()}")
    # active subspace
    _, grad = g.predict_mean(Xc, convert=False, revert=False, return_grad=True)
    out0 = g.active_subspace(x=Xs)
    out = g.active_subspace(x=Xs, npaths=3, nfeatures=512, path_seed=17)
    lam, Vv, Cm, dgsm = sens.active_subspace_from_gradients(grad)
    assert set(out0) == {"eigenvalues", "eigenvectors", "C", "dgsm", "x", "grads"}
    for got in (out0, out):
        assert _same_bits(got["eigenvalues"], lam) and _same_bits(got["eigenvectors"], Vv) and _same_bits(got["C"], Cm)
        assert _same_bits(got["dgsm"], dgsm) and _same_bits(got["grads"], grad)
    _, gc = draws(Xc, convert=False, revert=False, return_grad=True)
    assert out["eigenvalues_paths"].shape == (3, 2)
    assert _same_bits(out["eigenvalues_paths"], np.array([sens.active_subspace_from_gradients(gs)[0] for gs in gc]))
    # y_dist
    xs, ys = g.y_dist(nsamps=50, return_data=True, seed=2, mean_only=True)
    assert _same_bits(ys, g.predict_mean(xs))
    xs1, ys1 = g.y_dist(nsamps=50, return_data=True, seed=2)
    assert _same_bits(xs1, xs) and _same_bits(ys1, g.predict(xs))
    xs2, ys2 = g.y_dist(nsamps=50, return_data=True, seed=2, npaths=3, nfeatures=512, path_seed=17)
    assert _same_bits(xs2, xs) and ys2.shape == (3, 50) and _same_bits(ys2, draws(xs))


def test_facade_refusals(fitted):
    g = fitted
    g.trend = "constant"
    try:
        with pytest.raises(ValueError, match="has no form under trend"):
            g.sample_paths(2)
    finally:
        g.trend = None
    g.outputs = "all"
    try:
        with pytest.raises(ValueError, match="has no form under outputs='all'"):
            g.sample_paths(2)
    finally:
        g.outputs = "first"
    draws = g.sample_paths(2, 64, seed=1)
    mean = g.mean
    g.mean = lambda v: np.array([1.0])
    try:
        with pytest.raises(ValueError, match="non-zero mean function"):
            draws(g.x[:3], return_grad=True)
    finally:
        g.mean = mean
    with pytest.raises(ValueError):
        g.sample_paths(129)
