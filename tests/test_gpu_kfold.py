"""MiGP.kfold / mi_gp_kfold: exact k-fold cross-validation from the resident K^-1, against the refit reference of
tests/kfold_ref.py (one factorisation of the complement per fold, in NumPy), against a second handle on the complement, and
through the facade (GPMCMC.cv_stats).

Tolerances are the project's parity tolerances (tests/test_gpu_append.py, tests/test_gpu_logpdf.py) with cond = cond(K) of the
full data: logp and mean within max(1e-10, 20 cond eps) of max(|ref|, 1), var within max(1e-10, 200 cond eps) of the reference
variance.  Every parity check prints error / tolerance before it asserts."""
import ctypes

import numpy as np
import pytest
import scipy.stats as st

import kfold_ref as ref

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


def _csr(folds):
    sizes = [len(f) for f in folds]
    ptr = np.zeros(len(folds) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum(sizes)
    idx = np.ascontiguousarray(np.concatenate([np.asarray(f).reshape(-1) for f in folds]) if sizes else np.zeros(0), dtype=np.int32)
    return ptr, idx


def _raw(gp, folds, per_pass=None, work_len=None, work="nan", logp=True, mean=True, var=True, nfolds=None, ptr=None, idx=None):
    """mi_gp_kfold on device tensors: (return value, logp, mean, var, info), the outputs pre-filled with a sentinel.
    per_pass: folds the work block is sized for (default: all); work: 'nan' (a block full of NaN), 'none' (NULL) or a tensor"""
    import torch

    p0, i0 = _csr(folds)
    ptr = p0 if ptr is None else ptr
    idx = i0 if idx is None else idx
    nf = len(folds) if nfolds is None else nfolds
    total = max(len(i0), 1)
    dev = gp.dev
    if work_len is None:
        work_len = int(gp.lib.mi_gp_kfold_work(len(folds) if per_pass is None else per_pass, total))
    if isinstance(work, str):
        work = None if work == "none" else torch.full((max(work_len, 1),), float("nan"), dtype=torch.float64, device=dev)
    lt = torch.full((max(len(folds), 1),), SENTINEL, dtype=torch.float64, device=dev)
    mt = torch.full((total,), SENTINEL, dtype=torch.float64, device=dev)
    vt = torch.full((total,), SENTINEL, dtype=torch.float64, device=dev)
    info = np.full(max(len(folds), 1), -5, dtype=np.int32)
    torch.cuda.synchronize(dev)
    ip = ctypes.POINTER(ctypes.c_int)
    r = gp.lib.mi_gp_kfold(gp.h, nf, ptr.ctypes.data_as(ip), idx.ctypes.data_as(ip), work.data_ptr() if work is not None else None,
                           work_len, lt.data_ptr() if logp else None, mt.data_ptr() if mean else None,
                           vt.data_ptr() if var else None, info.ctypes.data_as(ip))
    torch.cuda.synchronize(dev)
    return r, lt.cpu().numpy(), mt.cpu().numpy(), vt.cpu().numpy(), info


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[1:], b[1:])) and a[0] == b[0]


def _gp(i, need_grad=True, capacity=None):
    from andvaranaut_amd import MiGP

    X, y, kernel, theta, diag, cond = ref.case(i)
    gp = MiGP(X, y, kernel, device=0, need_grad=need_grad, capacity=capacity)
    if diag is not None:
        gp.set_diag(diag)
    return gp, theta, cond


# ----------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("i", range(len(ref.CASES)))
def test_kfold_parity_with_a_refit_per_fold(i):
    gp, theta, cond = _gp(i)
    n = gp.n
    worst = 0.0
    for layout in ref.LAYOUTS:
        folds = ref.fold_layout(layout, n, i)
        logp, mu, var, info = gp.kfold(theta, folds)
        ratios = ref.error_ratios((logp, mu, var), ref.case_refit(i, layout), cond)
        print(ref.CASES[i], layout, "cond %.3g" % cond, "error / tolerance: logp %.3g mean %.3g var %.3g" % ratios)
        worst = max(worst, *ratios)
        assert not info.any()
        assert [len(a) for a in mu] == [len(f) for f in folds] == [len(a) for a in var]
        assert max(ratios) <= 1.0, (layout, ratios)
        # without the moments: the same densities
        lp2, m2, v2, _ = gp.kfold(theta, folds, moments=False, resident=True)
        assert m2 is None and v2 is None and np.array_equal(lp2, logp)
        if len({len(f) for f in folds}) == 1:  # equal folds as the rows of one array: the same call
            lp3, m3, v3, _ = gp.kfold(theta, np.stack(folds), resident=True)
            assert np.array_equal(lp3, logp) and np.array_equal(np.stack(m3), np.stack(mu)) and np.array_equal(np.stack(v3), np.stack(var))
    print(ref.CASES[i], "worst error / tolerance %.3g" % worst)
    gp.close()


# ------------------------------------------------------------------------------------------------- scratch, passes, repeats
def test_scratch_is_never_read_and_passes_do_not_change_a_bit():
    import torch

    i = 6
    gp, theta, cond = _gp(i)
    n = gp.n
    assert np.isfinite(gp.lml_grad(theta)[0])
    for layout in ("edges", "7uneven", "loo"):
        folds = ref.fold_layout(layout, n, i)
        base = _raw(gp, folds)
        assert base[0] == 0 and not base[4].any()
        assert all(np.isfinite(a).all() for a in base[1:4])
        # all folds in one pass, one and three per pass, the same call again: the same bits
        for per_pass in (1, 3, len(folds), len(folds) + 5):
            assert _same(_raw(gp, folds, per_pass=per_pass), base), (layout, per_pass)
        assert _same(_raw(gp, folds), base)
        # a zeroed work block instead of one full of NaN
        wl = int(gp.lib.mi_gp_kfold_work(len(folds), sum(len(f) for f in folds)))
        assert _same(_raw(gp, folds, work=torch.zeros(wl, dtype=torch.float64, device=gp.dev)), base)
        # the densities alone
        lone = _raw(gp, folds, mean=False, var=False)
        assert lone[0] == 0 and np.array_equal(lone[1], base[1]) and np.all(lone[2] == SENTINEL) and np.all(lone[3] == SENTINEL)
    # leave-one-out needs no work block at all
    loo = ref.fold_layout("loo", n, i)
    assert _same(_raw(gp, loo, work="none", work_len=0), _raw(gp, loo))
    # the strict upper triangle of W is scratch: full of NaN it changes nothing
    results = {layout: _raw(gp, ref.fold_layout(layout, n, i)) for layout in ref.LAYOUTS}
    rows, cols = torch.triu_indices(gp.W_t.shape[0], gp.W_t.shape[1], offset=1, device=gp.dev)
    gp.W_t[rows, cols] = float("nan")
    torch.cuda.synchronize(gp.dev)
    assert torch.isnan(gp.W_t[0, 1]) and torch.isnan(gp.W_t[127, 128]) and torch.isnan(gp.W_t[5, gp.W_t.shape[1] - 1])
    for layout in ref.LAYOUTS:
        got = _raw(gp, ref.fold_layout(layout, n, i))
        assert all(np.isfinite(a).all() for a in got[1:4]), layout
        assert _same(got, results[layout]), layout
    gp.close()


def test_singleton_path_agrees_with_the_general_path():
    i = 2
    gp, theta, cond = _gp(i)
    loo = ref.fold_layout("loo", gp.n, i)
    logp, mu, var, info = gp.kfold(theta, loo)
    # one two-point fold behind the same singletons: every fold goes through gather, leaf and moments
    lg, mg, vg, ig = gp.kfold(theta, loo + [np.array([200, 11])], resident=True)
    assert not info.any() and not ig.any()
    ratios = ref.error_ratios((lg[:-1], mg[:-1], vg[:-1]), (logp, mu, var), cond)
    print("singleton path against general path, error / tolerance: logp %.3g mean %.3g var %.3g" % ratios)
    assert max(ratios) <= 1.0, ratios
    gp.close()


# ------------------------------------------------------------------------------------------------------ device cross-check
def test_a_fold_agrees_with_a_second_handle_on_the_complement():
    from andvaranaut_amd import MiGP

    i = 0  # (RBF without a per-point diagonal: predict's prior variance kv is the full-matrix diagonal exactly)
    X, y, kernel, theta, diag, cond = ref.case(i)
    gp, _, _ = _gp(i)
    vtol, ptol = ref.tolerances(cond)
    for I in (np.array([128, 3, 127, 126, 120, 129, 64, 121]), np.array([77])):
        logp, mu, var, info = gp.kfold(theta, [I])
        J = np.setdiff1d(np.arange(len(y)), I)
        other = MiGP(X[J], y[J], kernel, device=0)
        lp2, _, _ = other.logpdf(theta, X[I], y[I], grad=False)
        mu2, var2 = other.predict(theta, X[I], pred_noise=True, via_inverse=False)
        var2 = var2 + theta[-1]  # (predict adds gv; the observations' marginal form carries the jitter as well)
        e = (abs(logp[0] - lp2) / max(abs(lp2), 1.0) / vtol, np.max(np.abs(mu[0] - mu2) / np.maximum(np.abs(mu2), 1.0)) / vtol,
             np.max(np.abs(var[0] - var2) / var2) / ptol)
        print("fold of %d against logpdf / predict on the complement, error / tolerance: logp %.3g mean %.3g var %.3g" % ((len(I),) + e))
        assert max(e) <= 1.0, e
        other.close()
    gp.close()


# ------------------------------------------------------------------------------------------------------------------ state
def test_kfold_changes_no_handle_state():
    import torch

    i = 3  # (with a per-point diagonal)
    gp, theta, cond = _gp(i)
    n = gp.n
    Xs = np.random.default_rng(8).random((20, gp.d))
    pred0 = gp.predict(theta, Xs, via_inverse=False)
    assert np.isfinite(gp.lml_grad(theta)[0])

    def state():
        alpha = np.empty(n)
        assert gp.lib.mi_gp_alpha(gp.h, alpha.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 0
        gx = torch.empty((n, gp.d), dtype=torch.float64, device=gp.dev)
        assert gp.lib.mi_gp_grad_x(gp.h, gx.data_ptr()) == 0
        return [gp.K_t.cpu().numpy(), gp.Z_t.cpu().numpy(), gp.W_t.cpu().numpy(), alpha, gx.cpu().numpy(), np.array(gp.lml_parts())]

    before = state()
    for layout in ("edges", "loo"):
        assert _raw(gp, ref.fold_layout(layout, n, i))[0] == 0
        gp.kfold(theta, ref.fold_layout(layout, n, i), resident=True)
        for a, b in zip(before, state()):
            assert np.array_equal(a, b, equal_nan=True)
    # a later factorisation predicts what it predicted before
    for a, b in zip(pred0, gp.predict(theta, Xs, via_inverse=False)):
        assert np.array_equal(a, b)
    gp.close()


# ------------------------------------------------------------------------------------------------------------ failed fold
def test_a_fold_that_is_not_positive_definite_fails_alone():
    import torch

    i = 0
    gp, theta, cond = _gp(i)
    n = gp.n
    assert np.isfinite(gp.lml_grad(theta)[0])
    folds = ref.fold_layout("7uneven", n, i)
    loo = ref.fold_layout("loo", n, i)
    good, good_loo = _raw(gp, folds), _raw(gp, loo, work="none", work_len=0)
    pos = 9
    point = int(folds[2][pos])  # planted as data: a diagonal entry of K^-1 inside fold 2 becomes -1
    assert all(point not in f for k, f in enumerate(folds) if k != 2)
    gp.W_t[point, point] = -1.0
    torch.cuda.synchronize(gp.dev)
    r, logp, mu, var, info = _raw(gp, folds)
    ptr, _ = _csr(folds)
    a, b = ptr[2], ptr[3]
    assert r == 0
    assert info[2] == pos + 1 and not np.delete(info, 2).any(), info
    assert logp[2] == -np.inf and np.isnan(mu[a:b]).all() and np.isnan(var[a:b]).all()
    keep = np.r_[0:a, b:len(mu)]
    assert np.array_equal(np.delete(logp, 2), np.delete(good[1], 2))
    assert np.array_equal(mu[keep], good[2][keep]) and np.array_equal(var[keep], good[3][keep])
    # the facade hands the same through
    lp, m, v, inf = gp.kfold(theta, folds, resident=True)
    assert inf[2] == pos + 1 and lp[2] == -np.inf and np.isnan(m[2]).all() and np.array_equal(m[3], good[2][ptr[3] : ptr[4]])
    # the singleton path
    r, logp, mu, var, info = _raw(gp, loo, work="none", work_len=0)
    assert r == 0 and info[point] == 1 and not np.delete(info, point).any()
    assert logp[point] == -np.inf and np.isnan(mu[point]) and np.isnan(var[point])
    for got, want in zip((logp, mu, var), good_loo[1:4]):
        assert np.array_equal(np.delete(got, point), np.delete(want, point))
    gp.close()


# --------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    i = 0
    gp, theta, cond = _gp(i, capacity=140)
    n = gp.n
    folds = ref.fold_layout("overlap", n, i)
    loo = [np.array([k]) for k in range(5)]

    def refused(text, fl, **kw):
        r, logp, mu, var, info = _raw(gp, fl, **kw)
        err = gp.lib.mi_gp_last_error(gp.h)
        assert r == -1 and b"mi_gp_kfold" in err and text in err, (r, err)
        assert np.all(logp == SENTINEL) and np.all(mu == SENTINEL) and np.all(var == SENTINEL) and np.all(info == -5)

    # no K^-1 resident
    for fl in (folds, loo):
        refused(b"mi_gp_lml_grad", fl)  # after set_data
    gp.lml(theta)
    refused(b"mi_gp_lml_grad", folds)  # after the value alone
    assert np.isfinite(gp.lml_grad(theta)[0])
    assert _raw(gp, folds)[0] == 0
    assert gp.factor(theta) == 0
    refused(b"mi_gp_lml_grad", folds)  # after factor
    X, y = ref.case(i)[:2]
    assert gp.append(X[:2] + 0.013, y[:2]) == 0
    refused(b"mi_gp_lml_grad", folds)  # after append
    refused(b"mi_gp_lml_grad", loo)
    n = gp.n
    assert np.isfinite(gp.lml_grad(theta)[0])
    assert _raw(gp, folds)[0] == 0
    # the folds
    refused(b"nfolds", folds, nfolds=0)
    refused(b"nfolds", folds, nfolds=-3)
    ptr, idx = _csr(folds)
    empty = ptr.copy()
    empty[2] = empty[1]  # fold 1 is empty
    refused(b"points", folds, ptr=empty)
    refused(b"points", [np.arange(129)])
    refused(b"points", loo + [np.arange(129)])
    refused(b"outside", [np.array([3, n])])
    refused(b"outside", [np.array([3, -1, 4])])
    refused(b"outside", loo + [np.array([n])])
    refused(b"repeated", [np.array([3, 9, 3])])
    refused(b"fold_ptr[0]", folds, ptr=ptr + 1)
    # the buffers
    refused(b"null", folds, logp=False)
    refused(b"null", loo, logp=False)
    refused(b"both or neither", folds, var=False)
    refused(b"both or neither", loo, mean=False)
    refused(b"null work", folds, work="none")
    total = len(idx)
    refused(b"too small", folds, work_len=int(gp.lib.mi_gp_kfold_work(1, total)) - 1)
    refused(b"too small", folds, work_len=0)
    assert _raw(gp, folds, work_len=int(gp.lib.mi_gp_kfold_work(1, total)))[0] == 0
    # the Python layer names fold sizes itself
    with pytest.raises(ValueError):
        gp.kfold(theta, [np.arange(129)])
    with pytest.raises(ValueError):
        gp.kfold(theta, [np.arange(3), np.array([], dtype=int)])
    with pytest.raises(ValueError):
        gp.kfold(theta, [])
    gp.close()
    # without the gradient buffers there is no K^-1
    gp, theta, _ = _gp(i, need_grad=False)
    gp.lml(theta)
    refused(b"mi_gp_lml_grad", folds)
    with pytest.raises(RuntimeError):
        gp.kfold(theta, folds)
    gp.close()


# ----------------------------------------------------------------------------------------------------------------- facade
@pytest.fixture(scope="module")
def fitted():
    from andvaranaut_amd import GPMCMC, normal, uniform
    from andvaranaut_amd.transform import logarithm

    priors = [st.uniform(loc=0, scale=2), st.norm(loc=1.25, scale=0.08)]
    fun = lambda x: np.array([x[0] ** 2 - x[0] - x[1] ** 2 * x[0] + x[1] + 3.0])  # noqa: E731
    g = GPMCMC(kernel="RBF", noise=True, xconrevs=[uniform(priors[0]), normal(priors[1])], yconrevs=[logarithm()], nx=2, ny=1,
               priors=priors, target=fun, verbose=False)
    g.sample(nsamps=150, seed=5)
    g.fit(method="map")
    return g


def _metrics(ypred, yt, meany):
    return {"rmse": np.sqrt(np.mean((ypred - yt) ** 2)), "mea": np.mean(np.abs(ypred - yt)),
            "mpe": np.mean(np.abs(ypred - yt) / np.abs(yt)), "r2": 1 - np.sum((ypred - yt) ** 2) / np.sum((yt - meany) ** 2)}


@pytest.mark.parametrize("nfolds", ["loo", 5])
def test_cv_stats_against_the_reference(fitted, nfolds):
    g = fitted
    n = g.nsamp
    theta = g._theta_from_hypers(g.hypers, 1e-6)
    yc = g.yc[:, 0]
    cond = ref.full_cond(g.xc, "RBF", theta)
    vtol, ptol = ref.tolerances(cond)
    # the converted space
    out = g.cv_stats(nfolds, seed=1, revert=False)
    folds = out["folds"]
    if nfolds == "loo":
        assert [f.tolist() for f in folds] == [[k] for k in range(n)]
    else:
        want = np.array_split(np.random.default_rng(1).permutation(n), 5)
        assert len(folds) == 5 and all(np.array_equal(a, b) for a, b in zip(folds, want))
    idx = np.concatenate(folds)
    rlp, rmu, rvar = ref.kfold_refit(g.xc, yc, "RBF", theta, folds)
    ratios = ref.error_ratios((out["lpd_folds"] - np.array([np.sum(np.log(1.0 / g.y[f, 0])) for f in folds]),
                               [out["ypred"]], [out["yvars"]]), (rlp, [np.concatenate(rmu)], [np.concatenate(rvar)]), cond)
    print("cv_stats", nfolds, "cond %.3g" % cond, "error / tolerance: logp %.3g mean %.3g var %.3g" % ratios)
    assert max(ratios) <= 1.0, ratios
    assert np.array_equal(out["ytest"], yc[idx]) and np.array_equal(out["xtest"], g.xc[idx]) and not out["info"].any()
    for k, v in _metrics(out["ypred"], yc[idx], np.mean(yc)).items():
        assert out[k] == pytest.approx(v, rel=1e-13), k
    # lpd: the densities of the reference plus the Jacobian of the logarithm, sum log(1 / y)
    want = np.sum(rlp) + np.sum(np.log(1.0 / g.y[idx, 0]))
    assert abs(out["lpd"] - want) <= len(folds) * vtol * max(np.max(np.abs(rlp)), 1.0) + 1e-13 * abs(want), (out["lpd"], want)
    assert out["lpd"] == pytest.approx(np.sum(out["lpd_folds"]), rel=1e-13)
    # the original units: the same Gauss-Hermite reversion applied to the reference's moments.  For the logarithm the reverted
    # mean is exp(mu + v / 2) and the variance exp(2 mu + v) (exp(v) - 1), so an error dmu of the mean and a relative error dv
    # of a variance v < 1 move them by at most dmu + dv relatively, and 2 dmu + 3 dv.
    rev = g.cv_stats(nfolds, seed=1, revert=True)
    mu_r, var_r = np.concatenate(rmu), np.concatenate(rvar)
    ymean, ym2 = g._gh_moments(0.0, mu_r.reshape(-1, 1), var_r.reshape(-1, 1))
    dmu = vtol * np.maximum(np.abs(mu_r), 1.0)
    assert np.max(var_r) < 1.0
    assert np.all(np.abs(rev["ypred"] - ymean) <= (dmu + ptol) * np.abs(ymean))
    assert np.all(np.abs(rev["yvars"] - (ym2 - ymean ** 2)) <= (2 * dmu + 3 * ptol) * (ym2 - ymean ** 2))
    assert np.array_equal(rev["ytest"], g.y[idx, 0]) and np.array_equal(rev["xtest"], g.x[idx])
    for k, v in _metrics(rev["ypred"], g.y[idx, 0], np.mean(g.y)).items():
        assert rev[k] == pytest.approx(v, rel=1e-13), k
    assert rev["lpd"] == pytest.approx(out["lpd"], rel=1e-10)  # (the density does not depend on the reversion)


def test_cv_stats_names_the_smallest_admissible_number_of_folds(fitted):
    g = fitted
    # 150 points: one fold would hold 150 > 128 of them, two folds of 75 are the fewest
    with pytest.raises(ValueError, match="smallest admissible nfolds is 2"):
        g.cv_stats(1)
    assert len(g.cv_stats(2, seed=3)["folds"]) == 2
    with pytest.raises(ValueError):
        g.cv_stats(151)
    with pytest.raises(ValueError):
        g.cv_stats("kfold")
    with pytest.raises(ValueError):
        g.cv_stats(folds=[np.arange(129)])
    # explicit folds, overlapping and not covering the data
    out = g.cv_stats(folds=[[0, 5, 9], np.arange(5, 40)], revert=False)
    assert len(out["ypred"]) == 38 and np.isfinite(out["lpd"])
