"""A GP handle under a gradient binding (mi_gp_deriv_bind, andvaranaut_amd/deriv.py) against the NumPy reference
(tests/deriv_ref.py): the log marginal likelihood, its theta gradient and the conditional of the value at new points; what the
binding refuses; an unbound handle of libmi_gp_deriv.so against libmi_gp.so; and the GPMCMC facade end to end."""
import ctypes

import numpy as np
import pytest
import torch

import deriv_ref as R

pytestmark = pytest.mark.gpu

# the block test's shapes, N = 256 (an exact tile multiple), (23, 5), 19 tile columns and 35 tile columns (the panel schedule)
SHAPES = [(1, 2), (37, 3), (129, 1), (50, 16), (128, 1), (23, 5), (300, 7), (260, 16)]
GRAD_NOISE = 1e-2


def _case(n, d, kernel):
    X, y, dY = R.problem(n, d, 1000 + 10 * n + d, close_pair=False)
    theta = R.theta_for(d)  # gv = 1e-3, l log-spaced in [0.4, 1.5], kv = 1.7
    extra = np.concatenate([np.zeros(n), np.full(n * d, GRAD_NOISE)])
    yj = np.concatenate([y, dY.T.ravel()])
    return X, y, dY, yj, theta, extra


_REF = {}


def _reference(n, d, kernel):
    """computed once per case and shared: the condition number, the LML and its gradient, the conditional at 33 points"""
    key = (n, d, kernel)
    if key not in _REF:
        X, y, dY, yj, theta, extra = _case(n, d, kernel)
        Xn = np.random.default_rng(n + d).random((33, d))
        val, g = R.lml(X, yj, theta, kernel, extra, grad=True)
        mu, var = R.predict(X, yj, Xn, theta, kernel, extra)
        _REF[key] = dict(cond=R.cond(X, theta, kernel, extra), lml=val, grad=g, Xn=Xn, mu=mu, var=var)
    return _REF[key]


@pytest.mark.parametrize("kernel", ["RBF", "Matern52"])
@pytest.mark.parametrize("n,d", SHAPES)
def test_bound_handle_against_reference(kernel, n, d):
    from andvaranaut_amd.deriv import MiDerivGP

    X, y, dY, yj, theta, extra = _case(n, d, kernel)
    ref = _reference(n, d, kernel)
    print(f"{kernel} ({n}, {d}): N = {n * (1 + d)}, cond = {ref['cond']:.3e}")
    assert ref["cond"] <= 1e7  # a condition of the case, not a measurement
    gp = MiDerivGP(X, y, dY, kernel, grad_noise=GRAD_NOISE)
    try:
        v = gp.lml(theta)
        v2, g = gp.lml_grad(theta)
        logdet, quad = gp.lml_parts()
        mu, var = gp.predict(theta, ref["Xn"])
        print(f"  lml {v:.15e} ref {ref['lml']:.15e} rel {abs(v - ref['lml']) / abs(ref['lml']):.2e}")
        print(f"  grad worst {np.abs(g - ref['grad']).max() / np.abs(ref['grad']).max():.2e} of its largest component")
        print(f"  mean worst {np.abs(mu - ref['mu']).max():.2e}, var worst {np.abs(var - ref['var']).max():.2e}")
        assert gp.info == 0
        assert abs(v - ref["lml"]) <= 1e-10 * abs(ref["lml"])
        assert v2 == v
        assert abs((-0.5 * quad - logdet - 0.5 * n * (1 + d) * R.LOG_2PI) - v) <= 1e-12 * abs(v)
        assert np.all(np.abs(g - ref["grad"]) <= 1e-8 * np.abs(ref["grad"]).max())
        assert np.allclose(mu, ref["mu"], rtol=0.0, atol=1e-9 * max(1.0, np.abs(ref["mu"]).max()))
        assert np.allclose(var, ref["var"], rtol=1e-8, atol=1e-11)
        # a repeat returns the same bits
        v3, g3 = gp.lml_grad(theta)
        assert v3 == v and g3.tobytes() == g.tobytes()
    finally:
        gp.close()


class Raw:
    """a handle of `lib` over joint-sized buffers, for the calls MiDerivGP does not make"""

    def __init__(self, lib, X, yobs, kernel_id, n_handle):
        from andvaranaut_amd import _lib

        self.lib = lib
        cfg = _lib.MiGpConfig()
        cfg.n, cfg.d, cfg.nkern = n_handle, X.shape[1], 1
        cfg.kernel_ids[0] = kernel_id
        self.h = ctypes.c_void_p()
        assert lib.mi_gp_create(ctypes.byref(cfg), ctypes.byref(self.h)) == 0
        self.np_ = int(lib.mi_gp_padded_n(self.h))
        self.ntheta = int(lib.mi_gp_num_theta(self.h))
        self.lda = self.np_ + 16
        self.X = torch.from_numpy(np.ascontiguousarray(X)).cuda()
        self.y = torch.from_numpy(np.ascontiguousarray(yobs)).cuda()
        self.K = torch.empty((self.np_ + 128, self.lda), dtype=torch.float64, device="cuda")
        self.Z = torch.zeros((self.np_, self.lda), dtype=torch.float64, device="cuda")
        self.W = torch.zeros((self.np_, self.lda), dtype=torch.float64, device="cuda")
        self.work = torch.zeros((256, self.lda), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        self.set_data()

    def set_data(self):
        from andvaranaut_amd import _lib

        b = _lib.MiGpBuffers()
        b.X_dev, b.y_dev, b.K_dev, b.lda = self.X.data_ptr(), self.y.data_ptr(), self.K.data_ptr(), self.lda
        b.Z_dev, b.W_dev = self.Z.data_ptr(), self.W.data_ptr()
        assert self.lib.mi_gp_set_data(self.h, ctypes.byref(b)) == 0

    def err(self):
        return self.lib.mi_gp_last_error(self.h).decode()

    def lml(self, theta):
        out = ctypes.c_double()
        r = self.lib.mi_gp_lml(self.h, theta.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(out))
        return r, out.value

    def lml_grad(self, theta):
        out, g = ctypes.c_double(), np.zeros(self.ntheta)
        dp = ctypes.POINTER(ctypes.c_double)
        r = self.lib.mi_gp_lml_grad(self.h, theta.ctypes.data_as(dp), ctypes.byref(out), g.ctypes.data_as(dp))
        return r, out.value, g

    def factor(self, theta):
        return self.lib.mi_gp_factor(self.h, theta.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))

    def predict(self, Xn):
        m = Xn.shape[0]
        xn = torch.from_numpy(np.ascontiguousarray(Xn)).cuda()
        mu = torch.zeros(m, dtype=torch.float64, device="cuda")
        var = torch.zeros(m, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        r = self.lib.mi_gp_predict(self.h, xn.data_ptr(), m, self.work.data_ptr(), self.lda, mu.data_ptr(), var.data_ptr(), 1)
        return r, mu.cpu().numpy(), var.cpu().numpy()

    def close(self):
        torch.cuda.synchronize()
        self.lib.mi_gp_destroy(self.h)


def test_unbound_handle_returns_the_bits_of_the_plain_library():
    from andvaranaut_amd import _lib

    rng = np.random.default_rng(5)
    N, d = 300, 3
    X = rng.random((N, d))
    y = np.sin(X.sum(1))
    theta = R.theta_for(d)
    Xn = rng.random((17, d))
    got = []
    for lib in (_lib.load(), _lib.load_deriv()):
        h = Raw(lib, X, y, 1, N)
        r0, v = h.lml(theta)
        r1, v1, g = h.lml_grad(theta)
        r2 = h.factor(theta)
        r3, mu, var = h.predict(Xn)
        assert (r0, r1, r2, r3) == (0, 0, 0, 0), h.err()
        got.append((v, v1, g.tobytes(), mu.tobytes(), var.tobytes()))
        h.close()
    assert got[0] == got[1]


def test_bind_unbind_rebind_refusals_and_bad_pivot():
    from andvaranaut_amd import _lib

    lib = _lib.load_deriv()
    n, d, kernel = 23, 5, "Matern52"
    X, y, dY, yj, theta, extra = _case(n, d, kernel)
    N = n * (1 + d)
    dp = ctypes.POINTER(ctypes.c_double)
    h = Raw(lib, X, yj, 1, N)
    try:
        # refused bindings name the entry point and what is wrong
        assert lib.mi_gp_deriv_bind(h.h, n + 1) == -1 and "mi_gp_deriv_bind" in h.err() and "npts (1 + d)" in h.err()
        assert lib.mi_gp_deriv_bind(h.h, -1) == -1 and "mi_gp_deriv_bind" in h.err()
        assert lib.mi_gp_set_option(h.h, 50, 1) == 0
        assert lib.mi_gp_deriv_bind(h.h, n) == -1 and "mode option" in h.err()
        assert lib.mi_gp_set_option(h.h, 50, 0) == 0
        assert lib.mi_gp_deriv_bind(h.h, n) == 0
        ed = torch.from_numpy(extra).cuda()
        torch.cuda.synchronize()
        assert lib.mi_gp_set_diag(h.h, ed.data_ptr()) == 0
        ref = _reference(n, d, kernel)
        assert h.factor(theta) == 0
        r, mu, var = h.predict(ref["Xn"])
        assert r == 0 and np.allclose(mu, ref["mu"], rtol=0.0, atol=1e-9)
        # every other entry point and every mode option away from its default: -1, the text names the binding, the factor stays
        buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
        p = buf.data_ptr()
        host = np.zeros(4 * N)
        hp = host.ctypes.data_as(dp)
        ip = (ctypes.c_int * 8)()
        bb = _lib.MiGpBatchBuffers()
        bb.K_dev, bb.count, bb.stride_k, bb.stride_zw = p, 1, 1 << 30, 1 << 30
        refused = {
            "mi_gp_alpha": lambda: lib.mi_gp_alpha(h.h, hp),
            "mi_gp_grad_x": lambda: lib.mi_gp_grad_x(h.h, p),
            "mi_gp_set_batch": lambda: lib.mi_gp_set_batch(h.h, ctypes.byref(bb)),
            "mi_gp_lml_batch": lambda: lib.mi_gp_lml_batch(h.h, 1, hp, hp, ip),
            "mi_gp_lml_grad_batch": lambda: lib.mi_gp_lml_grad_batch(h.h, 1, hp, hp, hp, ip),
            "mi_gp_factor_batch": lambda: lib.mi_gp_factor_batch(h.h, 1, hp, ip),
            "mi_gp_predict_batch": lambda: lib.mi_gp_predict_batch(h.h, 1, p, 1, p, h.lda, 0, p, p, 1, None, None),
            "mi_gp_predict_u": lambda: lib.mi_gp_predict_u(h.h, p, 1, p, h.lda, p, p, 1),
            "mi_gp_predict_grad": lambda: lib.mi_gp_predict_grad(h.h, p, 1, p, h.lda, p, p, 1, p, p),
            "mi_gp_predict_cov": lambda: lib.mi_gp_predict_cov(h.h, p, 1, p, h.lda, p, p, 128, 1),
            "mi_gp_sample_cov": lambda: lib.mi_gp_sample_cov(h.h, p, 128, 1, p, 0.0, 1, 1, 0, p, 1, p, lib.mi_gp_sample_cov_work(1, 1)),
            "mi_gp_reserve": lambda: lib.mi_gp_reserve(h.h, N + 1),
            "mi_gp_append": lambda: lib.mi_gp_append(h.h, p, p, None, 1, p, h.lda),
            "mi_gp_logpdf": lambda: lib.mi_gp_logpdf(h.h, p, p, None, 1, p, h.lda, hp, None, None),
            "mi_gp_kfold": lambda: lib.mi_gp_kfold(h.h, 1, ip, ip, p, 4096, p, None, None, ip),
        }
        for name, call in refused.items():
            assert call() == -1, name
            assert "mi_gp_deriv_bind" in h.err() and name in h.err(), (name, h.err())
        for opt, val in ((48, 1), (49, 4), (50, 1), (51, 2), (52, 1), (53, 1), (54, 2), (55, 32), (56, 1), (57, 3)):
            assert lib.mi_gp_set_option(h.h, opt, val) == -1, opt
            assert "mi_gp_deriv_bind" in h.err(), (opt, h.err())
            got = ctypes.c_int(-7)
            assert lib.mi_gp_get_option(h.h, opt, ctypes.byref(got)) == 0
        assert lib.mi_gp_set_option(h.h, 50, 0) == 0  # (the default itself is no change)
        r, mu2, var2 = h.predict(ref["Xn"])  # the handle is usable and its factor is still resident
        assert r == 0 and mu2.tobytes() == mu.tobytes() and var2.tobytes() == var.tobytes()
        # unbind and rebind end the resident state
        assert lib.mi_gp_deriv_bind(h.h, 0) == 0
        r, _, _ = h.predict(ref["Xn"])
        assert r == -1 and "mi_gp_factor first" in h.err()
        assert lib.mi_gp_deriv_bind(h.h, n) == 0
        assert h.factor(theta) == 0
        assert lib.mi_gp_deriv_bind(h.h, n) == 0
        r, _, _ = h.predict(ref["Xn"])
        assert r == -1 and "mi_gp_factor first" in h.err()
        a, b = ctypes.c_double(), ctypes.c_double()
        assert lib.mi_gp_lml_parts(h.h, ctypes.byref(a), ctypes.byref(b)) == -1
        # a theta that is not positive definite reports its pivot: kv + gv + jitter < 0 at the first value row
        bad = theta.copy()
        bad[d + 3] = -3.0
        r, v = h.lml(bad)
        assert r == 1 and v == -np.inf
        r, v, g = h.lml_grad(bad)
        assert r == 1 and v == -np.inf and np.all(g == 0.0)
        # ... and deeper: the jitter that turns the smallest eigenvalue negative fails at a pivot the reference's leading minors name
        K = R.train_cov(X, theta, kernel, extra)
        lam = np.linalg.eigvalsh(K)[0]
        bad = theta.copy()
        bad[d + 3] = theta[d + 3] - 2.0 * lam
        Kb = R.train_cov(X, bad, kernel, extra)
        first = next(j + 1 for j in range(N) if np.linalg.eigvalsh(Kb[: j + 1, : j + 1])[0] <= 0.0)
        lam_first = np.linalg.eigvalsh(Kb[:first, :first])[0]
        r, v = h.lml(bad)
        print(f"deep pivot: device {r}, leading minors {first} (its smallest eigenvalue {lam_first:.2e})")
        assert v == -np.inf and r >= 1
        if abs(lam_first) > 1e-9:  # (a minor this far below zero cannot pass; an earlier, nearly singular one may fail first)
            assert r <= first
        r, v = h.lml(theta)
        assert r == 0 and abs(v - ref["lml"]) <= 1e-10 * abs(ref["lml"])
    finally:
        h.close()


def test_bind_refuses_other_models():
    from andvaranaut_amd import _lib

    lib = _lib.load_deriv()
    X = np.random.default_rng(0).random((4, 2))
    h = Raw(lib, X, np.zeros(12), 2, 12)  # Matern-3/2
    try:
        assert lib.mi_gp_deriv_bind(h.h, 4) == -1 and "RBF (0) or Matern-5/2 (1)" in h.err()
    finally:
        h.close()


def _tutorial(x):
    return np.array([x[0] ** 2 - x[0] - x[1] ** 2 * x[0] + x[1]])  # tutorial.ipynb:61-63


def _tutorial_grad(x):
    return np.ascontiguousarray(np.column_stack([2.0 * x[:, 0] - 1.0 - x[:, 1] ** 2, -2.0 * x[:, 1] * x[:, 0] + 1.0]))


def test_facade_end_to_end_gradients_lower_the_holdout_rmse():
    import pickle

    import scipy.stats as st

    from andvaranaut_amd import GPMCMC, normal, uniform

    priors = [st.uniform(loc=0, scale=2), st.uniform(loc=1, scale=0.5)]
    g = GPMCMC(kernel="RBF", noise=True, xconrevs=[uniform(priors[0]), normal(priors[1])], yconrevs=[None], nx=2, ny=1,
               priors=priors, target=_tutorial, parallel=False, nproc=1, verbose=False)
    g.sample(nsamps=40, seed=1)
    assert len(g.x) == 40
    xt = np.random.default_rng(5).uniform([0, 1], [2, 1.5], (200, 2))
    yt = np.array([_tutorial(r) for r in xt])
    g.fit(method="map")
    rmse_values = float(np.sqrt(np.mean((g.predict(xt) - yt) ** 2)))
    g.set_data(g.x, g.y, _tutorial_grad(g.x))
    data = g.fit(method="map", gradients=True, return_data=True)
    yp, yv = g.predict(xt, return_var=True)
    rmse_grads = float(np.sqrt(np.mean((yp - yt) ** 2)))
    print(f"tutorial function, n = 40, 200 held-out points: RMSE {rmse_values:.3e} from the values, {rmse_grads:.3e} with the gradients "
          f"({data['nfev']} evaluations)")
    assert g.gradients and yp.shape == (200, 1) and np.all(yv > -1e-9)
    assert rmse_grads < rmse_values
    # the converted-space prediction is the reference's conditional at the fitted hyper-parameters
    xin, yin = g._converted(g.x, g.y - g.ym)
    theta = g._theta_from_hypers(g.hypers, 1e-6)
    yj = np.concatenate([yin, g.converted_gradients().T.ravel()])
    xc = np.column_stack([g.xconrevs[i].con(xt[:, i]) for i in range(2)])
    mu_r, var_r = R.predict(xin, yj, xc, theta, "RBF")
    print(f"  cond of the fitted joint covariance {R.cond(xin, theta, 'RBF'):.2e}")
    yc, yvc = g.predict(xt, return_var=True, revert=False)
    assert np.allclose(yc[:, 0], mu_r, rtol=1e-5, atol=1e-6) and np.allclose(yvc[:, 0], var_r, rtol=1e-4, atol=1e-8)
    # pickling drops the handle; the copy rebuilds it under the binding and predicts the same
    g2 = pickle.loads(pickle.dumps(g))
    assert g2.gp is None and g2.gradients
    assert np.array_equal(g2.predict(xt), yp)
    g2.gp.close()
    # test_stats refits on the training split with its rows of the gradients
    g.train_test(0.8)
    out = g.test_stats(method="none")
    assert np.isfinite(out["rmse"]) and out["ypred"].shape == (8,)
    with pytest.raises(ValueError, match="gradients=True"):
        g.predict_joint(xt)
    # without dy the object is the plain one again
    g.set_data(g.x, g.y)
    g.fit(method="map")
    assert not g.gradients and abs(float(np.sqrt(np.mean((g.predict(xt) - yt) ** 2))) - rmse_values) <= 1e-6 * rmse_values
    g.gp.close()
