"""Gradient observations without a GPU: the NumPy reference (tests/deriv_ref.py) against double automatic differentiation of
k(x, x') and of its own log marginal likelihood, the closed limits at coincident and close points, the facade's chain rule and
refusals, and the exports of libmi_gp_deriv.so."""
import os
import pickle
import subprocess

import numpy as np
import pytest
import torch

import deriv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["RBF", "Matern52"]


def _k_torch(kernel, x, xp, ls, kv):
    s = (((x - xp) / ls) ** 2).sum()
    if kernel == "RBF":
        return kv * torch.exp(-0.5 * s)
    r = torch.sqrt(s + 1e-12)
    return kv * (1.0 + R.SQ5 * r + 5.0 / 3.0 * r * r) * torch.exp(-R.SQ5 * r)


def _autograd_blocks(kernel, x, xp, theta):
    """the (1 + d) x (1 + d) covariance of [f, grad f](x) with [f, grad f](x') by torch.autograd.grad twice on k(x, x')"""
    d = len(x)
    ls, kv = torch.tensor(theta[:d]), torch.tensor(theta[d])
    xt = torch.tensor(x, requires_grad=True)
    xpt = torch.tensor(xp, requires_grad=True)
    k = _k_torch(kernel, xt, xpt, ls, kv)
    out = np.zeros((1 + d, 1 + d))
    out[0, 0] = k.item()
    gx, gxp = torch.autograd.grad(k, (xt, xpt), create_graph=True)
    out[1:, 0] = gx.detach().numpy()
    out[0, 1:] = gxp.detach().numpy()
    for c in range(d):
        (row,) = torch.autograd.grad(gx[c], xpt, retain_graph=True)
        out[1 + c, 1:] = row.numpy()
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_reference_covariance_equals_double_autograd(kernel):
    rng = np.random.default_rng(3)
    d, n = 3, 7
    X = rng.random((n, d))
    X[1] = X[0] + np.array([1e-3, 0.0, 0.0]) * 0.4  # r = 1e-3 at l_0 = 0.4
    theta = R.theta_for(d)
    K = R.cov(X, 1 + d, X, 1 + d, theta, kernel)
    scale = np.abs(K).max()
    worst = 0.0
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            assert np.sqrt((((X[i] - X[j]) / theta[:d]) ** 2).sum()) >= 1e-3 * (1 - 1e-9)
            B = _autograd_blocks(kernel, X[i], X[j], theta)
            mine = K[np.ix_(np.arange(1 + d) * n + i, np.arange(1 + d) * n + j)]
            worst = max(worst, np.abs(B - mine).max())
    print(f"{kernel}: reference against double autograd, worst {worst:.3e} of the largest entry {scale:.3e}")
    assert worst <= 1e-12 * scale


@pytest.mark.parametrize("kernel", KERNELS)
def test_reference_closed_limits(kernel):
    d = 3
    theta = R.theta_for(d)
    ls, kv = theta[:d], theta[d]
    x = np.array([[0.3, 0.5, 0.7]])
    B = R.cov(x, 1 + d, x, 1 + d, theta, kernel)
    lim = kv / ls ** 2 * (1.0 if kernel == "RBF" else 5.0 / 3.0)
    assert abs(B[0, 0] - kv) <= 1e-11 * kv
    assert np.all(B[0, 1:] == 0.0) and np.all(B[1:, 0] == 0.0)
    assert np.allclose(np.diag(B)[1:], lim, rtol=1e-5 if kernel == "Matern52" else 1e-15, atol=0.0)  # (Matern: r = 1e-6 inside)
    assert np.all(B[1:, 1:][~np.eye(d, dtype=bool)] == 0.0)
    # a pair 1e-3 apart along x_0: the leading terms of the series in dl
    x2 = x.copy()
    x2[0, 0] += 1e-3
    C = R.cov(x2, 1 + d, x, 1 + d, theta, kernel)
    u = 1e-3 / ls[0]
    c1 = 1.0 if kernel == "RBF" else 5.0 / 3.0
    # d/dx k = -kv c1 dl / l^2 (1 + O(u^2)): the series' next terms are u^2 / 2 (RBF) and 5 u^2 / 2 (Matern) of the leading one,
    # and at most 15 u^2 / 2 on the derivative diagonal (Matern, c = c' = 0)
    assert abs(C[1, 0] - (-kv * c1 * u / ls[0])) <= 3.0 * u * u * kv * c1 * u / ls[0]
    assert abs(C[0, 1] + C[1, 0]) <= 1e-16
    assert np.allclose(np.diag(C)[1:], lim, rtol=10.0 * u * u, atol=0.0)
    # the joint covariance is symmetric and positive definite with the diagonal terms
    X, _, _ = R.problem(9, d, 5)
    K = R.train_cov(X, theta, kernel, np.concatenate([np.zeros(9), np.full(27, 1e-2)]))
    assert np.abs(K - K.T).max() <= 1e-15 * np.abs(K).max()
    assert np.linalg.eigvalsh(K)[0] > 0.0


def _lml_torch(kernel, X, yj, th, extra):
    n, d = X.shape
    Xt = torch.tensor(X)
    ls, kv, gv, jit = th[:d], th[d], th[d + 2], th[d + 3]

    # the joint covariance by the closed blocks in torch (the blocks themselves are checked against double autograd above)
    a = 1.0 / ls ** 2
    D = (Xt[:, None, :] - Xt[None, :, :]).permute(2, 0, 1)
    s = (a[:, None, None] * D * D).sum(0)
    if kernel == "RBF":
        k = torch.exp(-0.5 * s)
        k1, k2 = -0.5 * k, 0.25 * k
    else:
        r = torch.sqrt(s + 1e-12)
        e = torch.exp(-R.SQ5 * r)
        k, k1, k2 = (1.0 + R.SQ5 * r + 5.0 / 3.0 * r * r) * e, -(5.0 / 6.0) * (1.0 + R.SQ5 * r) * e, (25.0 / 12.0) * e
    aD = a[:, None, None] * D
    top = torch.cat([kv * k] + [-2.0 * kv * k1 * aD[c] for c in range(d)], dim=1)
    rows = [top]
    for c in range(d):
        blk = [2.0 * kv * k1 * aD[c]]
        for cp in range(d):
            b = -4.0 * kv * k2 * aD[c] * aD[cp]
            if c == cp:
                b = b - 2.0 * kv * k1 * a[c]
            blk.append(b)
        rows.append(torch.cat(blk, dim=1))
    K = torch.cat(rows, dim=0)
    dg = torch.cat([torch.full((n,), 1.0, dtype=torch.float64) * (gv + jit), torch.full((n * d,), 1.0, dtype=torch.float64) * jit])
    K = K + torch.diag(dg + torch.tensor(extra))
    L = torch.linalg.cholesky(K)
    beta = torch.linalg.solve_triangular(L, torch.tensor(yj)[:, None], upper=False)[:, 0]
    return -0.5 * beta @ beta - torch.log(torch.diagonal(L)).sum() - 0.5 * len(yj) * R.LOG_2PI


@pytest.mark.parametrize("kernel", KERNELS)
def test_reference_theta_gradient_equals_autograd_of_the_lml(kernel):
    n, d = 11, 3
    X, y, dY = R.problem(n, d, 11, close_pair=False)
    yj = np.concatenate([y, dY.T.ravel()])
    theta = R.theta_for(d)
    extra = np.concatenate([np.zeros(n), np.full(n * d, 1e-2)])
    val, g = R.lml(X, yj, theta, kernel, extra, grad=True)
    th = torch.tensor(theta, requires_grad=True)
    vt = _lml_torch(kernel, X, yj, th, extra)
    (gt,) = torch.autograd.grad(vt, th)
    gt = gt.numpy()
    assert abs(vt.item() - val) <= 1e-12 * abs(val)
    keep = np.arange(d + 4) != d + 1  # (the alpha slot belongs to the rational quadratic: 0)
    rel = np.abs(g[keep] - gt[keep]) / np.abs(gt[keep])
    print(f"{kernel}: reference theta gradient against autograd, worst relative {rel.max():.3e}")
    assert g[d + 1] == 0.0
    assert np.all(rel <= 1e-9), (g, gt)


def test_library_exports_are_the_57_and_the_three():
    from andvaranaut_amd import _lib

    path = _lib.DERIV_LIB_PATH
    assert os.path.exists(path), "libmi_gp_deriv.so is missing: run __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    syms = sorted(line.split()[-1] for line in out.splitlines() if " T " in line)
    assert len(_lib.EXPORTS) == 57
    assert syms == sorted(_lib.EXPORTS + ["mi_gp_deriv_bind", "mi_gp_deriv_assemble", "mi_gp_deriv_contract"])
    assert sorted(_lib.DERIV_EXPORTS) == syms
    # libmi_gp.so keeps its 57
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert sorted(line.split()[-1] for line in out.splitlines() if " T " in line) == sorted(_lib.EXPORTS)
    # the header declares the three
    text = open(os.path.join(ROOT, "include", "mi_gp_deriv.h")).read()
    for name in ("mi_gp_deriv_bind", "mi_gp_deriv_assemble", "mi_gp_deriv_contract"):
        assert f"MI_GP_API int {name}(" in text


# ---------------------------------------------------------------- the facade (no device call is made below)
def _target(x):
    return np.array([x[0] ** 2 - x[0] - x[1] ** 2 * x[0] + x[1] + 3.0])  # the tutorial function + 3 (positive: logarithm applies)


def _target_grad(x):
    return np.column_stack([2.0 * x[:, 0] - 1.0 - x[:, 1] ** 2, -2.0 * x[:, 1] * x[:, 0] + 1.0])


def _facade(xconrevs=None, yconrevs=None, kernel="RBF", mean=0, n=12):
    import scipy.stats as st

    from andvaranaut_amd import GPMCMC

    priors = [st.uniform(loc=0, scale=2), st.uniform(loc=1, scale=0.5)]
    g = GPMCMC(kernel=kernel, noise=True, xconrevs=xconrevs, yconrevs=yconrevs, nx=2, ny=1, priors=priors, target=_target,
               parallel=False, nproc=1, verbose=False, mean=mean)
    x = np.random.default_rng(2).uniform([0, 1], [2, 1.5], (n, 2))
    y = np.array([_target(r) for r in x])
    return g, x, y


def test_facade_chain_rule_matches_finite_differences_of_the_converted_data():
    from andvaranaut_amd import logarithm, maxmin, meanstd

    _, x, y = _facade()
    for ycon in (meanstd(y[:, 0]), logarithm()):
        xcon = [meanstd(x[:, 0]), maxmin(x[:, 1])]
        g, _, _ = _facade(xconrevs=xcon, yconrevs=[ycon])
        g.set_data(x, y, _target_grad(x))
        got = g.converted_gradients()
        h = 1e-6
        for m in range(2):
            xp, xm = x.copy(), x.copy()
            xp[:, m] += h
            xm[:, m] -= h
            fp = np.array([_target(r)[0] for r in xp])
            fm = np.array([_target(r)[0] for r in xm])
            fd = (ycon.con(fp) - ycon.con(fm)) / (xcon[m].con(xp[:, m]) - xcon[m].con(xm[:, m]))
            # central differences: the truncation term is h^2 f''' / 6 ~ 1e-12, the rounding term eps |yc| / h ~ 1e-9
            assert np.allclose(got[:, m], fd, rtol=1e-7, atol=1e-8), (type(ycon).__name__, m)
    # without dy nothing changes, and the array is checked
    g.set_data(x, y)
    assert g.dy is None
    with pytest.raises(Exception, match="gradient data requires"):
        g.set_data(x, y, np.zeros((len(x), 3)))


def test_facade_refusals_name_what_is_missing():
    g, x, y = _facade()
    dy = _target_grad(x)
    g.set_data(x, y)
    with pytest.raises(ValueError, match=r"set_data\(x, y, dy\)"):
        g.fit(gradients=True)
    g.set_data(x, y, dy)
    for kw, text in ((dict(iwgp=True), "iwgp / cwgp"), (dict(cwgp=True), "iwgp / cwgp"), (dict(method="mcmc_mean"), "no sampler"),
                     (dict(method="mcmc_map"), "no sampler"), (dict(objective="loo"), "objective='lml'"),
                     (dict(objective="kfold"), "objective='lml'"), (dict(trend="constant"), "trend="),
                     (dict(outputs="all"), "outputs='all'"), (dict(inducing=4), "inducing points")):
        with pytest.raises(ValueError, match=text):
            g.fit(gradients=True, **kw)
    for kernel in ("RBF+Matern52", "Matern32", "RatQuad", "Exponential"):
        gk, _, _ = _facade(kernel=kernel)
        gk.set_data(x, y, dy)
        with pytest.raises(ValueError, match="needs one kernel out of"):
            gk.fit(gradients=True)
    gm, _, _ = _facade(mean=lambda r: np.array([1.0]))
    gm.set_data(x, y, dy)
    with pytest.raises(ValueError, match="zero mean function"):
        gm.fit(gradients=True)
    # the state survives pickling (the target is a module-level function)
    g.gradients, g.grad_noise = True, 1e-4
    g2 = pickle.loads(pickle.dumps(g))
    assert g2.gradients and g2.grad_noise == 1e-4 and np.array_equal(g2.dy, dy) and g2.gp is None
    with pytest.raises(ValueError, match="gradients=True"):
        g2.predict_joint(x)
