"""Joint conditional and posterior draws on the GPU: mi_gp_predict_cov against a NumPy/SciPy restatement of PyMC's
Marginal._build_conditional(diag=False), mi_gp_sample_cov against mean + L z with the restated Philox/Box-Muller stream
(tests/test_predict_joint_host.py), and the MiGP / GPMCMC / BO layers above them."""
import time

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.stats as st

from test_predict_joint_host import philox_normals

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def _mods():
    import torch

    assert torch.cuda.is_available()
    from andvaranaut_amd import MiGP
    from oracle import gp_oracle as orc

    return torch, MiGP, orc


def _split(kernel):
    return kernel.replace("*", "+").split("+"), [c for c in kernel if c in "+*"]


def _kd(orc, kerns, ops, theta, d):
    return float(orc.kernel_diag(kerns, ops, theta, d))


def _sigma_ref(orc, X, Xn, kerns, ops, theta, pred_noise):
    """Sigma of [3P] Marginal._build_conditional(diag=False): Kss - A^T A (+ sqrt(gv)^2 I | + jitter I), Kss in the
    full-matrix form (its diagonal is k(sqrt(1e-12)) for the Matern / Exponential kernels): oracle.sigma_joint."""
    return orc.sigma_joint(X, Xn, kerns, ops, theta, pred_noise)


def _low(gp, torch, Xn, pred_noise, ldc_extra=0):
    """mi_gp_predict_cov through the C-ABI: (mean [m], cov tensor [mp, ldc]) at the resident factor."""
    m = Xn.shape[0]
    mp = (m + 127) // 128 * 128
    ldc = mp + ldc_extra
    work = torch.empty((mp, gp.lda), dtype=torch.float64, device=gp.dev)
    xn = torch.from_numpy(np.ascontiguousarray(Xn)).to(gp.dev)
    mu = torch.empty(m, dtype=torch.float64, device=gp.dev)
    cov = torch.full((mp, ldc), float("nan"), dtype=torch.float64, device=gp.dev)
    torch.cuda.synchronize()
    r = gp.lib.mi_gp_predict_cov(gp.h, xn.data_ptr(), m, work.data_ptr(), gp.lda, mu.data_ptr(), cov.data_ptr(), ldc,
                                 1 if pred_noise else 0)
    assert r == 0, gp.last_error()
    return mu.cpu().numpy(), cov


def _predict_low(gp, torch, Xn, pred_noise, fn="mi_gp_predict"):
    m = Xn.shape[0]
    mp = (m + 127) // 128 * 128
    rows = 2 * mp if fn != "mi_gp_predict" else mp
    work = torch.empty((rows, gp.lda), dtype=torch.float64, device=gp.dev)
    xn = torch.from_numpy(np.ascontiguousarray(Xn)).to(gp.dev)
    mu = torch.empty(m, dtype=torch.float64, device=gp.dev)
    var = torch.empty(m, dtype=torch.float64, device=gp.dev)
    torch.cuda.synchronize()
    r = getattr(gp.lib, fn)(gp.h, xn.data_ptr(), m, work.data_ptr(), gp.lda, mu.data_ptr(), var.data_ptr(), 1 if pred_noise else 0)
    assert r == 0, gp.last_error()
    return mu.cpu().numpy(), var.cpu().numpy()


def _sample_low(gp, torch, cov, m, mean, s, seed, offset, extra_jitter=0.0, ldd=None, draws=None):
    """mi_gp_sample_cov through the C-ABI: (return code, draws tensor [s, ldd])."""
    ldd = m if ldd is None else ldd
    need = int(gp.lib.mi_gp_sample_cov_work(m, s))
    work = torch.empty(need, dtype=torch.float64, device=gp.dev)
    if draws is None:
        draws = torch.empty((s, ldd), dtype=torch.float64, device=gp.dev)
    mean_t = torch.from_numpy(np.ascontiguousarray(mean)).to(gp.dev)
    torch.cuda.synchronize()
    r = gp.lib.mi_gp_sample_cov(gp.h, cov.data_ptr(), cov.shape[1], m, mean_t.data_ptr(), extra_jitter, s, seed, offset,
                                draws.data_ptr(), ldd, work.data_ptr(), need)
    return r, draws


def _lower(cov, m):
    return np.tril(cov[:m, :m].cpu().numpy())


def _sym(low):
    return low + np.tril(low, -1).T


KERNELS = ["RBF", "Matern52", "Exponential", "RatQuad", "RBF+Matern32*Exponential"]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("N", [100, 384, 1000])
def test_sigma_matches_the_restated_joint_conditional(N, kernel):
    torch, MiGP, orc = _mods()
    d = 3
    X, y = orc.synth_problem(N, d, seed=N + len(kernel))
    kerns, ops = _split(kernel)
    theta = orc.synth_theta(d, nkern=len(kerns), gv=1e-3)
    if "RatQuad" in kerns:
        theta[len(kerns) * d + len(kerns) : len(kerns) * d + 2 * len(kerns)] = 1.3
    kd = _kd(orc, kerns, ops, theta, d)
    gp = MiGP(X, y, kernel)
    assert gp.factor(theta) == 0
    rng = np.random.default_rng(N)
    tol = (1e-7 if "Exponential" in kernel else 1e-9) * kd
    for m in (1, 127, 128, 129, 300):
        Xn = rng.random((m, d)) * 1.2 - 0.1
        for pred_noise in (0, 1):
            mu, cov = _low(gp, torch, Xn, pred_noise)
            mp = cov.shape[0]
            S = _sigma_ref(orc, X, Xn, kerns, ops, theta, pred_noise)
            got = _lower(cov, m)
            err = np.abs(got - np.tril(S)).max()
            assert err <= tol, (m, pred_noise, err, tol)
            # padding rows: identity in the lower triangle
            full = cov.cpu().numpy()
            pad = np.tril(full[m:, :])
            assert np.array_equal(pad, np.tril(np.eye(mp)[m:, :])), (m, pred_noise)
            # the mean is mi_gp_predict's, bit for bit; with pred_noise the diagonal is its variance (up to the full-matrix
            # form of the kernel on the diagonal, k(sqrt(1e-12)) instead of the 1 of diag=True)
            pmu, pvar = _predict_low(gp, torch, Xn, pred_noise)
            assert np.array_equal(mu.view(np.uint64), pmu.view(np.uint64)), m
            if pred_noise:
                # (the Exponential's k(sqrt(r2 + 1e-12)) moves by 2.5e5 per unit r2 at r2 = 0: a rounding-level r2 on the
                # diagonal -- the device's and the oracle's differ there -- is ~1e-10 of kv)
                kfull = np.diag(orc.kernel_matrix(Xn, None, kerns, ops, theta)) - kd
                dtol = (1e-9 if "Exponential" in kernel else 1e-11) * kd
                assert np.abs(np.diag(got) - (pvar + kfull)).max() <= dtol, (m, np.abs(np.diag(got) - (pvar + kfull)).max())
    gp.close()


def test_predict_cov_leading_dimension_beyond_mp():
    torch, MiGP, orc = _mods()
    X, y = orc.synth_problem(200, 2, seed=3)
    theta = orc.synth_theta(2, gv=1e-3)
    gp = MiGP(X, y, "Matern52")
    gp.factor(theta)
    Xn = np.random.default_rng(1).random((150, 2))
    _, c0 = _low(gp, torch, Xn, 1)
    _, c1 = _low(gp, torch, Xn, 1, ldc_extra=18)
    assert np.array_equal(_lower(c0, 150), _lower(c1, 150))
    gp.close()


@pytest.mark.parametrize("m,s,offset", [(1, 3, 0), (129, 5, 17), (300, 130, 2 ** 40)])
def test_draws_are_mean_plus_factor_times_the_restated_normals(m, s, offset):
    torch, MiGP, orc = _mods()
    d = 3
    X, y = orc.synth_problem(400, d, seed=m)
    theta = orc.synth_theta(d, gv=1e-3)
    gp = MiGP(X, y, "Matern52")
    gp.factor(theta)
    Xn = np.random.default_rng(m).random((m, d))
    mu, cov = _low(gp, torch, Xn, 1)
    S = _sym(_lower(cov, m))
    ej = 1e-9
    L = sla.cholesky(S + ej * np.eye(m), lower=True)
    seed = 0x5EED + m
    r, draws = _sample_low(gp, torch, cov, m, mu, s, seed, offset, extra_jitter=ej, ldd=m + 3)
    assert r == 0, gp.last_error()
    got = draws.cpu().numpy()[:, :m]
    z = philox_normals(seed, offset, s * m).reshape(s, m)
    ref = mu[None, :] + z @ L.T
    tol = 1e-9 * np.abs(L).max() * max(1.0, np.abs(z).max())
    assert np.abs(got - ref).max() <= tol, (np.abs(got - ref).max(), tol)
    # cov_dev now holds L_Sigma in its lower triangle, zeros above the diagonal inside the diagonal tiles
    Ld = cov.cpu().numpy()
    assert np.abs(np.tril(Ld[:m, :m]) - L).max() <= 1e-9 * np.abs(L).max()
    mp = Ld.shape[0]
    for t in range(mp // 128):
        blk = Ld[128 * t : 128 * t + 128, 128 * t : 128 * t + 128]
        assert not np.triu(blk, 1).any(), t
    gp.close()


def _mp_normals(seed, offset, count):
    """The restated stream with cos / sin / log / sqrt in 40-digit arithmetic (the device's libm differs from NumPy's by
    an ulp or two), plus rho per normal."""
    import mpmath

    from test_predict_joint_host import philox_words

    mpmath.mp.dps = 40
    nb = (count + 3) // 4
    w = philox_words(seed, [offset + q for q in range(nb)])
    z, rho = [], []
    for q in range(nb):
        for p in range(2):
            u0 = (float(int(w[q, 2 * p]) >> 11) + 0.5) * 2.0 ** -53
            u1 = (float(int(w[q, 2 * p + 1]) >> 11) + 0.5) * 2.0 ** -53
            r = mpmath.sqrt(-2 * mpmath.log(mpmath.mpf(u0)))
            z += [float(r * mpmath.cos(2 * mpmath.pi * mpmath.mpf(u1))), float(r * mpmath.sin(2 * mpmath.pi * mpmath.mpf(u1)))]
            rho += [float(r), float(r)]
    return np.array(z[:count]), np.array(rho[:count])


def test_exact_stream_on_a_diagonal_covariance():
    """RBF with the new points >= 40 length scales from the data and from each other: K(X, X*) and the off-diagonal of
    K(X*, X*) underflow, Sigma is diagonal, and (draw - mean) / sqrt(Sigma_ii) is the stream itself to a few ulp."""
    torch, MiGP, orc = _mods()
    d, m, s = 2, 130, 3
    X, y = orc.synth_problem(200, d, seed=5)
    theta = orc.synth_theta(d, gv=1e-3)  # length scales 0.4 .. 1.5
    gp = MiGP(X, y, "RBF")
    gp.factor(theta)
    Xn = 100.0 + 70.0 * np.column_stack([np.arange(m), np.arange(m) % 7])
    mu, cov = _low(gp, torch, Xn, 0)
    S = _lower(cov, m)
    assert not np.tril(S, -1).any() and (np.diag(S) > 0).all()
    c = np.diag(S).copy()
    seen = []
    for seed, offset in ((11, 0), (11, 1000), (2 ** 64 - 5, 2 ** 50 + 3)):
        runs = []
        for _ in range(2):
            _, cov = _low(gp, torch, Xn, 0)
            r, draws = _sample_low(gp, torch, cov, m, mu, s, seed, offset)
            assert r == 0, gp.last_error()
            runs.append(draws.cpu().numpy())
        assert np.array_equal(runs[0].view(np.uint64), runs[1].view(np.uint64)), "same (seed, offset), different bits"
        zd = (runs[0] - mu[None, :]) / np.sqrt(c)[None, :]
        zr, rho = _mp_normals(seed, offset, s * m)
        err = np.abs(zd.ravel() - zr)
        assert (err <= 16 * EPS * np.maximum(rho, 1.0)).all(), err.max()
        seen.append(zd.ravel())
    # disjoint offsets share no numbers (offset 0 uses blocks 0 .. 97, offset 1000 blocks 1000 ..)
    assert not np.isin(np.round(seen[0], 12), np.round(seen[1], 12)).any()
    gp.close()


def test_draw_moments_match_mean_and_sigma():
    torch, MiGP, orc = _mods()
    d, m, s = 2, 8, 20000
    X, y = orc.synth_problem(150, d, seed=8)
    theta = orc.synth_theta(d, gv=1e-3)
    gp = MiGP(X, y, "Matern52")
    gp.factor(theta)
    Xn = np.random.default_rng(3).random((m, d))
    mu, cov = _low(gp, torch, Xn, 1)
    S = _sym(_lower(cov, m))
    r, draws = _sample_low(gp, torch, cov, m, mu, s, 2024, 0)
    assert r == 0
    D = draws.cpu().numpy()
    mean_err = np.abs(D.mean(0) - mu)
    assert (mean_err <= 5 * np.sqrt(np.diag(S) / s)).all(), mean_err
    C = np.cov(D.T)
    sd = np.sqrt((np.outer(np.diag(S), np.diag(S)) + S ** 2) / s)
    assert (np.abs(C - S) <= 5 * sd).all(), np.abs(C - S) / sd
    gp.close()


def test_not_positive_definite_leaves_draws_untouched_and_the_backend_escalates():
    torch, MiGP, orc = _mods()
    d = 3
    X, y = orc.synth_problem(300, d, seed=9)
    theta = orc.synth_theta(d, gv=1e-3)
    kd = _kd(orc, ["RBF"], [], theta, d)
    theta[-1] = -1e-7 * kd  # a negative "jitter" and duplicated points: Sigma has a negative eigenvalue
    gp = MiGP(X, y, "RBF")
    assert gp.factor(theta) == 0
    Xn = np.random.default_rng(2).random((40, d)) * 3.0
    Xn[25] = Xn[3]
    Xn[31] = Xn[3]
    m = Xn.shape[0]
    mu, cov = _low(gp, torch, Xn, 0)
    sentinel = torch.full((4, m), 12345.0, dtype=torch.float64, device=gp.dev)
    r, draws = _sample_low(gp, torch, cov, m, mu, 4, 1, 0, extra_jitter=0.0, draws=sentinel)
    assert r > 0, r
    assert (draws.cpu().numpy() == 12345.0).all()
    # an explicitly indefinite matrix: the first bad pivot is reported 1-based
    bad = torch.zeros((128, 128), dtype=torch.float64, device=gp.dev)
    bad.fill_diagonal_(1.0)
    bad[1, 0] = 2.0
    r, _ = _sample_low(gp, torch, bad, 2, np.zeros(2), 1, 1, 0)
    assert r == 2, r
    out = gp.sample_posterior(theta, Xn, 3, seed=5)
    assert out.shape == (3, m) and np.isfinite(out).all()
    ej = gp.sample_info["extra_jitter"]
    assert ej > 0 and gp.sample_info["attempts"] >= 2
    assert any(np.isclose(ej, f * kd, rtol=1e-12) for f in gp.SAMPLE_JITTER_STEPS), ej
    gp.close()


def test_no_handle_state_changes_and_append():
    torch, MiGP, orc = _mods()
    d, N, n0 = 3, 500, 380
    X, y = orc.synth_problem(N, d, seed=12)
    theta = orc.synth_theta(d, gv=1e-3)
    gp = MiGP(X[:n0], y[:n0], "Matern52", capacity=N)
    gp.factor(theta)
    Xn = np.random.default_rng(4).random((200, d))
    before = _predict_low(gp, torch, Xn, 1)
    before_u = _predict_low(gp, torch, Xn, 1, fn="mi_gp_predict_u")
    mu, cov = _low(gp, torch, Xn, 0)
    assert _sample_low(gp, torch, cov, 200, mu, 7, 3, 0)[0] == 0
    after = _predict_low(gp, torch, Xn, 1)
    after_u = _predict_low(gp, torch, Xn, 1, fn="mi_gp_predict_u")
    for b, a in zip(before + before_u, after + after_u):
        assert np.array_equal(b.view(np.uint64), a.view(np.uint64))
    # append capacity untouched: the grown factor's joint conditional is a fresh factorisation's to rounding
    assert gp.append(X[n0:], y[n0:]) == 0 and gp.append_refactors == 0
    mu_a, cov_a = gp.predict_cov(theta, Xn, pred_noise=True)
    fresh = MiGP(X, y, "Matern52")
    mu_f, cov_f = fresh.predict_cov(theta, Xn, pred_noise=True)
    kd = _kd(orc, ["Matern52"], [], theta, d)
    assert np.abs(cov_a - cov_f).max() <= 1e-10 * kd and np.abs(mu_a - mu_f).max() <= 1e-9 * max(1.0, np.abs(mu_f).max())
    gp.close()
    fresh.close()


def test_backend_offsets_give_fresh_and_reproducible_draws():
    torch, MiGP, orc = _mods()
    X, y = orc.synth_problem(120, 2, seed=6)
    theta = orc.synth_theta(2, gv=1e-3)
    gp = MiGP(X, y, "RBF")
    Xn = np.random.default_rng(5).random((9, 2))
    a = gp.sample_posterior(theta, Xn, 4, seed=77)
    info_a = dict(gp.sample_info)
    b = gp.sample_posterior(theta, Xn, 4, seed=77)
    assert gp.sample_info["offset"] == info_a["offset"] + (4 * 9 + 3) // 4
    assert not np.isin(a, b).any()
    c = gp.sample_posterior(theta, Xn, 4, seed=77, offset=info_a["offset"])
    assert np.array_equal(a.view(np.uint64), c.view(np.uint64))
    mu, cov = gp.predict_cov(theta, Xn, pred_noise=False)
    assert np.array_equal(cov, cov.T) and cov.shape == (9, 9)
    gp.close()


def test_large_case_spot_check():
    torch, MiGP, orc = _mods()
    d, N, m, s = 4, 2048, 4096, 16
    X, y = orc.synth_problem(N, d, seed=21)
    theta = orc.synth_theta(d, gv=1e-3)
    gp = MiGP(X, y, "RBF")
    gp.factor(theta)
    Xn = np.random.default_rng(6).random((m, d))
    idx = np.array([0, 1, 1000, 2047, 2048, 4095])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mu, cov = _low(gp, torch, Xn, 1)
    t1 = time.perf_counter()
    got = cov.cpu().numpy()[idx, :m]  # (mi_gp_sample_cov overwrites Sigma with its factor)
    t2 = time.perf_counter()
    r, draws = _sample_low(gp, torch, cov, m, mu, s, 9, 0, extra_jitter=1e-10)
    t3 = time.perf_counter()
    assert r == 0, gp.last_error()
    print(f"N={N} m={m}: predict_cov {1e3 * (t1 - t0):.1f} ms, sample_cov s={s} {1e3 * (t3 - t2):.1f} ms")
    K = orc.noisy_cov(X, ["RBF"], [], theta, form="conditional")
    L = sla.cholesky(K, lower=True)
    A = sla.solve_triangular(L, orc.kernel_matrix(X, Xn, ["RBF"], [], theta), lower=True)
    rows = orc.kernel_matrix(Xn[idx], Xn, ["RBF"], [], theta) - A[:, idx].T @ A
    rows[np.arange(len(idx)), idx] += np.sqrt(1e-3) ** 2
    kd = 1.7
    for k, i in enumerate(idx):
        assert np.abs(got[k, : i + 1] - rows[k, : i + 1]).max() <= 1e-9 * kd, i
    assert np.isfinite(draws.cpu().numpy()).all()
    gp.close()


# ------------------------------------------------------------------------------------------------------------- facade
def _tutorial(n=40, seed=3):
    from andvaranaut_amd import GPMCMC, normal, uniform

    priors = [st.uniform(loc=0, scale=2), st.uniform(loc=1, scale=0.5)]
    fun = lambda x: np.array([x[0] ** 2 - x[0] - x[1] ** 2 * x[0] + x[1]])  # noqa: E731
    g = GPMCMC(kernel="RBF", noise=True, xconrevs=[uniform(priors[0]), normal(priors[1])], yconrevs=[None], nx=2, ny=1,
               priors=priors, target=fun, parallel=False, nproc=1, verbose=False)
    g.sample(nsamps=n, seed=seed)
    return g


def test_facade_sample_posterior_reverts_draws_pointwise():
    from andvaranaut_amd import maxmin, meanstd

    g = _tutorial()
    g.change_conrevs([maxmin(g.x[:, 0]), maxmin(g.x[:, 1])], [meanstd(g.y[:, 0])])
    g.fit(method="map")
    xt = np.random.default_rng(9).uniform([0, 1], [2, 1.5], (30, 2))
    rev = g.sample_posterior(xt, 6, seed=42)
    info = dict(g.gp.sample_info)
    xc = np.column_stack([g.xconrevs[i].con(xt[:, i]) for i in range(2)])
    conv = g.gp.sample_posterior(g._theta_from_hypers(g.hypers, 1e-6), xc, 6, seed=42, offset=info["offset"])
    means = g._mean_at(xt)
    expect = g.yconrevs[0].rev(conv) + (np.reshape(means, (1, -1)) if np.ndim(means) else means)
    assert rev.shape == (6, 30) and np.array_equal(rev, expect)
    # predict_joint: the converted-space moments of predict(revert=False) on its diagonal
    mu, cov = g.predict_joint(xt)
    pm, pv = g.predict(xt, return_var=True, revert=False)
    assert mu.shape == (30, 1) and cov.shape == (30, 30)
    assert np.allclose(mu, pm, rtol=1e-9, atol=1e-10)
    assert np.allclose(np.diag(cov), pv[:, 0], rtol=1e-9, atol=1e-12)


def test_bo_thompson_sampling_proposes_inside_the_bounds():
    g = _tutorial()
    g.fit(method="map")
    n0 = len(g.x)
    np.random.seed(4)
    g.BO(opt_type="min", opt_method="predict", method="TS", max_iter=2, predict_samps=500, conv=0.0)
    assert len(g.x) == n0 + 2
    new = g.x[n0:]
    assert (new[:, 0] >= 0).all() and (new[:, 0] <= 2).all() and (new[:, 1] >= 1).all() and (new[:, 1] <= 1.5).all(), new
