"""The CPU half of the sparse bound's gradients by the data (include/mi_gp_sparse_data.h): the long-double dF/dy and dF/dX of
tests/sgpr_data_grad_ref.py against central differences of the long-double bound, what fp64 alone costs on the device's steps at
every case of tests/test_gpu_sparse_data_grad.py, the third library's C-ABI without a GPU, and GPMCMC._warp_likelihood with raw
inducing points on a NumPy stand-in for the device object."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sgpr_data_grad_ref as DR
import sgpr_ref as R

FAKE = 4096  # an aligned address that is never dereferenced


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_long_double_gradients_agree_with_central_differences_of_the_bound(kernel):
    """Three entries of dF/dX and three of dF/dy at (n, m, d) = (300, 40, 3), h = 1e-6: the difference's truncation is what is
    left (dF/dX agreed to 3e-8 of max(|g|, 1) on entries up to 2e2, dF/dy to 4e-8); 1e-6 is asked for.  Both references are
    checked: the fp64 restatement of the device's steps is held against the same differences at its own tolerance."""
    case = (kernel, 300, 40, 3, None, "kmeanspp")
    X, y, Z, theta, _, _ = DR.device_case(case)
    ref = DR.case_reference(case)
    gy64, gx64 = DR.device_fp64_data(X, y, Z, kernel, theta)
    ptol = R.tolerances(ref["cond_Kuu"])[1]
    h = 1e-6

    def diff(Xp, yp, Xm, ym, step):
        return (R.bound_ld(Xp, yp, Z, kernel, theta, grad=False)["F"] - R.bound_ld(Xm, ym, Z, kernel, theta, grad=False)["F"]) / step

    for i, k in ((0, 0), (151, 1), (299, 2)):
        Xp, Xm = X.copy(), X.copy()
        Xp[i, k] += h
        Xm[i, k] -= h
        fd = diff(Xp, y, Xm, y, R.LD(Xp[i, k]) - R.LD(Xm[i, k]))
        g = ref["grad_x"][i, k]
        err = float(abs(fd - g) / max(abs(g), 1))
        print(kernel, "dF/dX", (i, k), "analytic %.10e, difference %.10e, error %.2e" % (float(g), float(fd), err))
        assert err <= 1e-6, (i, k, err)
        assert float(abs(fd - gx64[i, k]) / max(abs(g), 1)) <= 1e-6 + ptol, (i, k)
    for i in (3, 150, 298):
        yp, ym = y.copy(), y.copy()
        yp[i] += h
        ym[i] -= h
        fd = diff(X, yp, X, ym, R.LD(yp[i]) - R.LD(ym[i]))
        g = ref["grad_y"][i]
        err = float(abs(fd - g) / max(abs(g), 1))
        print(kernel, "dF/dy", i, "analytic %.10e, difference %.10e, error %.2e" % (float(g), float(fd), err))
        assert err <= 1e-6, (i, err)
        assert float(abs(fd - gy64[i]) / max(abs(g), 1)) <= 1e-6 + ptol, i


@pytest.mark.parametrize("case", DR.CASES, ids=R.case_id)
def test_fp64_on_the_device_steps_uses_at_most_half_the_gradient_tolerance(case):
    """(measured: at most 0.114 of the tolerance on dF/dX and 0.034 on dF/dy over the 30 cases)"""
    X, y, Z, theta, _, chunk = DR.device_case(case)
    ref = DR.case_reference(case)
    ry, rx = DR.ratios(*DR.device_fp64_data(X, y, Z, case[0], theta, chunk=chunk), ref)
    print(R.case_id(case), "cond(Kuu) = %.2e" % ref["cond_Kuu"], "max|dF/dX| = %.3e" % float(np.max(np.abs(ref["grad_x"]))),
          "dF/dy ratio %.4f, dF/dX ratio %.4f" % (ry, rx))
    assert ry <= 0.5 and rx <= 0.5, (ry, rx)


# ------------------------------------------------------------------------------------------------------------ the C-ABI
def _data_lib():
    from andvaranaut_amd import _lib as L

    return L, L.load_sparse_data()


def test_the_data_library_exports_the_nine_entry_points_and_nothing_else():
    from conftest import ROOT

    L, lib = _data_lib()
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)  # noqa: E731
    names = lambda t: sorted(set(re.findall(r"\b(mi_gp_[a-z0-9_]+)\s*\(", strip(t))))  # noqa: E731
    sparse_h = open(os.path.join(ROOT, "include", "mi_gp_sparse.h")).read()
    data_h = open(os.path.join(ROOT, "include", "mi_gp_sparse_data.h")).read()
    assert len(names(sparse_h)) == 8 and names(sparse_h) == sorted(L.SPARSE_EXPORTS)
    assert names(data_h) == ["mi_gp_sparse_bind_data_grad"] and '#include "mi_gp_sparse.h"' in data_h
    assert sorted(L.SPARSE_DATA_EXPORTS) == sorted(L.SPARSE_EXPORTS + ["mi_gp_sparse_bind_data_grad"])
    assert L.MiGpSparseConfig._fields_[-1][0] == "zgrad_slabs"
    struct = re.search(r"typedef struct \{(.*?)\} mi_gp_sparse_config;", sparse_h, flags=re.S).group(1)
    assert re.findall(r"\bint\s+([a-z_]+)\s*(?:\[[A-Z_]+\])?\s*;", strip(struct))[-1] == "zgrad_slabs"
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/lib/llvm/bin")
    if nm is not None:
        for path, want in ((L.SPARSE_DATA_LIB_PATH, L.SPARSE_DATA_EXPORTS), (L.SPARSE_LIB_PATH, L.SPARSE_EXPORTS)):
            out = subprocess.check_output([nm, "-D", "--defined-only", path], text=True)
            syms = [line.split() for line in out.splitlines() if line.strip()]
            assert sorted(s[-1] for s in syms) == sorted(want) and all(s[-2] == "T" for s in syms), syms
    # the plain sparse library does not know the new entry point
    assert not hasattr(L.load_sparse(), "mi_gp_sparse_bind_data_grad")


def test_bind_refuses_with_texts_and_makes_no_hip_call():
    L, lib = _data_lib()
    cfg = L.MiGpSparseConfig()
    cfg.n, cfg.m, cfg.d, cfg.nkern, cfg.device, cfg.chunk = 1000, 100, 3, 1, 0, 256
    cfg.kernel_ids[0] = 1
    s = ctypes.c_void_p()
    assert lib.mi_gp_sparse_create(ctypes.byref(cfg), ctypes.byref(s)) == 0  # (no HIP call: it succeeds without a GPU)
    try:
        assert lib.mi_gp_sparse_bind_data_grad(None, FAKE, FAKE, 4) == -1
        err = lib.mi_gp_sparse_last_error(None)
        assert b"mi_gp_sparse_bind_data_grad" in err and b"null object" in err, err
        assert lib.mi_gp_sparse_bind_data_grad(s, None, FAKE, 4) == -1
        err = lib.mi_gp_sparse_last_error(s)
        assert b"mi_gp_sparse_bind_data_grad" in err and b"gx_dev needs gy_dev" in err, err
        for slabs in (0, -1):
            assert lib.mi_gp_sparse_bind_data_grad(s, FAKE, FAKE, slabs) == -1
            err = lib.mi_gp_sparse_last_error(s)
            assert b"mi_gp_sparse_bind_data_grad" in err and b"xgrad_slabs" in err, err
        # binding, binding dF/dy alone and unbinding succeed on an object that has never seen a device
        for gy, gx in ((FAKE, FAKE), (FAKE, None), (None, None)):
            assert lib.mi_gp_sparse_bind_data_grad(s, gy, gx, 1) == 0
        # and the object still refuses an evaluation for the reason it had before
        th = np.array([0.5, 0.6, 0.7, 1.0, 1.0, 1e-2, 1e-6])
        out = ctypes.c_double()
        assert lib.mi_gp_sparse_bound_grad(s, th.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(out), None) == -1
        assert b"mi_gp_sparse_set_data first" in lib.mi_gp_sparse_last_error(s)
    finally:
        assert lib.mi_gp_sparse_destroy(s) == 0


# ----------------------------------------------------------------------------------------- the warps over raw inducing points
N_W, M_W = 120, 24


def warp_setup(iwgp, cwgp, n=N_W, m=M_W, ls_factor=1.0, precise=False):
    """The warped problem of tests/test_gpu_facade.py with m raw inducing points (k-means++ rows, seed 3), its HyperModel, the
    stand-in-backed posterior and a generic point q (the start's length scales times ls_factor)."""
    from andvaranaut_amd.priors import HyperModel
    from andvaranaut_amd.sparse import select_inducing
    from test_gpu_facade import _warped_problem

    g, _ = _warped_problem(n=n)
    x, y = g.x.copy(), (g.y - g.ym).copy()
    n_i, n_pos, n_free = g._warp_sizes(iwgp, cwgp)
    model = HyperModel(2, ["Matern52"], noise=True, n_iwgp=n_i, n_cwgp_pos=n_pos, n_cwgp=n_free)
    xin0, yin0 = g._converted(x, y)
    zin0, idx = select_inducing(xin0, m, seed=3, return_index=True)
    zraw = np.ascontiguousarray(x[idx])
    fake = DR.SparseStandIn(xin0, yin0, zin0, "Matern52", precise=precise)
    lik = g._warp_likelihood(fake, x, y, xin0, iwgp, cwgp, zraw=zraw)
    q = model.initial_point() + 0.1 * np.random.default_rng(0).standard_normal(model.nq)
    names = [v[0] for v in model.vars]
    assert names[:3] == ["gv", "l", "kv"]
    if ls_factor != 1.0:
        q[1:3] += np.log(ls_factor)  # (l is log-transformed)
    return g, model, fake, lik, q, (x, y, xin0, yin0, zin0, zraw)


@pytest.mark.parametrize("iwgp,cwgp", [(False, True), (True, False), (True, True)])
def test_warped_sparse_posterior_gradient_by_central_differences(iwgp, cwgp):
    """The gradient of the posterior by every variable, the warp parameters among them, against central differences: the data
    AND the inducing points move with the input warp, so dF/dZ has to join the pull-back (without it the iwgp entries miss by
    far more than the 5e-5 of test_host_logic's dense counterpart).  The output warp alone moves nothing but y: no
    set_inducing, no dF/dX, no dF/dZ."""
    g, model, fake, lik, q, _ = warp_setup(iwgp, cwgp)
    f = lambda qq: model.logp_dlogp(qq, None, jacobian=False, likelihood=lik)  # noqa: E731
    v, grad = f(q)
    assert np.isfinite(v)
    if iwgp:
        assert fake.calls == ["set_inducing", (True, True)], fake.calls
    else:
        assert fake.calls == [(False, False)], fake.calls
    for i in range(model.nq):
        h = 1e-6
        qp, qm = q.copy(), q.copy()
        qp[i] += h
        qm[i] -= h
        fd = (f(qp)[0] - f(qm)[0]) / (2 * h)
        print((iwgp, cwgp), i, "analytic %.8e, difference %.8e" % (grad[i], fd))
        assert abs(fd - grad[i]) <= 5e-5 * max(1.0, abs(fd)), (i, fd, grad[i])


def test_select_inducing_returns_the_indices_on_request():
    from andvaranaut_amd.sparse import select_inducing

    X = np.random.default_rng(0).random((50, 3))
    Z = select_inducing(X, 7, seed=2)
    Z2, idx = select_inducing(X, 7, seed=2, return_index=True)
    assert np.array_equal(Z, Z2) and np.array_equal(X[idx], Z) and len(set(idx.tolist())) == 7


LS_FACTOR_300 = 1.0  # the factor on the start's length scales that tests/test_gpu_sparse_warp_facade.py's comparison uses


@pytest.mark.parametrize("iwgp,cwgp", [(False, True), (True, False), (True, True)])
def test_fp64_alone_uses_at_most_half_the_tolerance_of_the_device_comparison(iwgp, cwgp):
    """The host half of tests/test_gpu_sparse_warp_facade.py's comparison (n = 300, 40 inducing points): the posterior and its
    gradient through the warps on the fp64 restatement against the same on the long-double references, at that test's point and
    over that test's tolerance (sgpr_data_grad_ref.warp_tolerances)."""
    _, model, _, lik, q, _ = warp_setup(iwgp, cwgp, n=300, m=40, ls_factor=LS_FACTOR_300)
    _, _, exact, lik_ld, q2, _ = warp_setup(iwgp, cwgp, n=300, m=40, ls_factor=LS_FACTOR_300, precise=True)
    assert np.array_equal(q, q2)
    v, g = model.logp_dlogp(q, None, jacobian=False, likelihood=lik)
    vr, gr = model.logp_dlogp(q, None, jacobian=False, likelihood=lik_ld)
    ev, eg, which = DR.warp_errors(v, g, vr, gr, exact.cond)
    print((iwgp, cwgp), "cond(Kuu) = %.2e" % exact.cond, "value %.3e, gradient %.3e of the tolerance" % (ev, eg), which)
    assert ev <= 0.5 and eg <= 0.5, (ev, eg)
