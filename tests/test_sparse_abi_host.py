"""The sparse inducing-point entry points (include/mi_gp_sparse.h, libmi_gp_sparse.so) without a GPU: the library exports what its
header declares and nothing else, every refusal returns -1 with a text before any HIP call, and mi_gp_sparse_work follows its
documented formula."""
import ctypes

import numpy as np
import pytest

FAKE = 4096  # an aligned address that is never dereferenced: every call below fails validation first


def _lib():
    from andvaranaut_amd import _lib as L

    return L, L.load_sparse()


def _config(L, n=1000, m=100, d=3, kernel_ids=(1,), ops=(), chunk=256):
    cfg = L.MiGpSparseConfig()
    cfg.n, cfg.m, cfg.d, cfg.nkern, cfg.device, cfg.chunk = n, m, d, len(kernel_ids), 0, chunk
    for i, k in enumerate(kernel_ids):
        cfg.kernel_ids[i] = k
    for i, o in enumerate(ops):
        cfg.ops[i] = o
    return cfg


def _create(L, lib, **kw):
    s = ctypes.c_void_p()
    r = lib.mi_gp_sparse_create(ctypes.byref(_config(L, **kw)), ctypes.byref(s))
    return r, s


def test_the_sparse_library_exports_its_header_and_nothing_else():
    import os
    import re
    import shutil
    import subprocess

    from conftest import ROOT

    L, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi_gp_sparse.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mi_gp_[a-z0-9_]+)\s*\(", text)))
    assert len(declared) == 8 and all(n.startswith("mi_gp_sparse_") for n in declared), declared
    assert sorted(L.SPARSE_EXPORTS) == declared
    assert not set(L.SPARSE_EXPORTS) & set(L.EXPORTS)  # libmi_gp.so keeps the entry points of include/mi_gp.h, no more
    for n in declared:
        assert hasattr(lib, n), f"libmi_gp_sparse.so does not export {n}"
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/lib/llvm/bin")
    if nm is not None:
        out = subprocess.check_output([nm, "-D", "--defined-only", L.SPARSE_LIB_PATH], text=True)
        syms = [line.split() for line in out.splitlines() if line.strip()]
        assert sorted(s[-1] for s in syms) == declared and all(s[-2] == "T" for s in syms), syms


@pytest.mark.parametrize("kw, why", [
    (dict(m=0), b"1 <= m"), (dict(m=-3), b"1 <= m"), (dict(m=2049, n=5000), b"1 <= m"), (dict(m=200, n=150), b"1 <= m"),
    (dict(chunk=100), b"multiple of 128"), (dict(chunk=-128), b"multiple of 128"), (dict(chunk=129), b"multiple of 128"),
    (dict(n=0, m=1), b"positive"), (dict(d=0), b"positive"),
    (dict(kernel_ids=(0, 5), ops=(0,)), b"unknown kernel id"), (dict(kernel_ids=(-1,)), b"unknown kernel id"),
    (dict(kernel_ids=(0, 1), ops=(2,)), b"ops must be"), (dict(kernel_ids=()), b"nkern"),
    (dict(kernel_ids=(0,) * 8 + (0,), ops=(0,) * 8), b"nkern"),
])
def test_create_refuses(kw, why):
    L, lib = _lib()
    if len(kw.get("kernel_ids", ())) > 8:  # nine components do not fit the config's arrays: set the count alone
        cfg = _config(L)
        cfg.nkern = 9
        s = ctypes.c_void_p()
        r = lib.mi_gp_sparse_create(ctypes.byref(cfg), ctypes.byref(s))
    else:
        r, s = _create(L, lib, **kw)
    assert r == -1
    err = lib.mi_gp_sparse_last_error(None)
    assert b"mi_gp_sparse_create" in err and why in err, err
    assert s.value is None


def test_create_refuses_null_arguments():
    L, lib = _lib()
    s = ctypes.c_void_p()
    assert lib.mi_gp_sparse_create(None, ctypes.byref(s)) == -1
    assert lib.mi_gp_sparse_create(ctypes.byref(_config(L)), None) == -1
    assert b"null" in lib.mi_gp_sparse_last_error(None)


def test_work_follows_its_formula():
    _, lib = _lib()
    for m in (1, 40, 128, 129, 200, 1000, 2048):
        for chunk in (128, 256, 8192):
            mp = (m + 127) // 128 * 128
            assert lib.mi_gp_sparse_work(m, chunk) == 9 * mp * mp + 2 * chunk * mp + 264 * mp
    for m, chunk in ((0, 128), (2049, 128), (100, 0), (100, 100), (100, -128)):
        assert lib.mi_gp_sparse_work(m, chunk) == -1
        assert b"mi_gp_sparse_work" in lib.mi_gp_sparse_last_error(None)


def test_calls_refuse_before_any_hip_call():
    L, lib = _lib()
    r, s = _create(L, lib)  # creation itself makes no HIP call: it succeeds without a GPU
    assert r == 0 and s.value is not None
    err = lambda: lib.mi_gp_sparse_last_error(s)  # noqa: E731
    need = lib.mi_gp_sparse_work(100, 256)
    try:
        # set_data: null buffers, another n, an odd or too small work length, a misaligned block
        for args in ((None, FAKE, 1000, FAKE, FAKE, need), (FAKE, None, 1000, FAKE, FAKE, need), (FAKE, FAKE, 1000, None, FAKE, need),
                     (FAKE, FAKE, 1000, FAKE, None, need)):
            assert lib.mi_gp_sparse_set_data(s, *args) == -1
            assert b"null buffer" in err()
        assert lib.mi_gp_sparse_set_data(s, FAKE, FAKE, 999, FAKE, FAKE, need) == -1
        assert b"configured" in err()
        for work_len in (need - 2, need + 1, 0, -8):
            assert lib.mi_gp_sparse_set_data(s, FAKE, FAKE, 1000, FAKE, FAKE, work_len) == -1
            assert b"work_len" in err()
        assert lib.mi_gp_sparse_set_data(s, FAKE, FAKE, 1000, FAKE, FAKE + 8, need) == -1
        assert b"aligned" in err()
        assert lib.mi_gp_sparse_set_data(None, FAKE, FAKE, 1000, FAKE, FAKE, need) == -1

        # evaluations: null theta, a noise variance s = gv + jitter <= 0, a non-finite theta, no data yet
        dp = ctypes.POINTER(ctypes.c_double)
        ntheta = 3 + 2 + 2
        out = ctypes.c_double(1.0)
        grad = np.ones(ntheta)

        def theta(gv, jitter, ls0=0.5):
            return np.array([ls0, 0.6, 0.7, 1.0, 1.0, gv, jitter])

        for th, why in ((theta(0.0, 0.0), b"must be positive"), (theta(-1e-2, 1e-6), b"must be positive"),
                        (theta(1e-6, -1e-6), b"must be positive"), (theta(1e-2, 1e-6, ls0=np.nan), b"finite"),
                        (theta(np.inf, 0.0), b"finite")):
            tp = th.ctypes.data_as(dp)
            assert lib.mi_gp_sparse_bound_grad(s, tp, ctypes.byref(out), grad.ctypes.data_as(dp)) == -1
            assert b"mi_gp_sparse_bound_grad" in err() and why in err(), err()
            assert lib.mi_gp_sparse_factor(s, tp) == -1
            assert b"mi_gp_sparse_factor" in err() and why in err(), err()
        good = theta(1e-2, 1e-6)
        tp = good.ctypes.data_as(dp)
        assert lib.mi_gp_sparse_bound_grad(s, None, ctypes.byref(out), None) == -1
        assert b"null theta" in err()
        assert lib.mi_gp_sparse_bound_grad(s, tp, ctypes.byref(out), None) == -1
        assert b"mi_gp_sparse_set_data first" in err()
        assert lib.mi_gp_sparse_factor(s, tp) == -1
        assert b"mi_gp_sparse_set_data first" in err()
        assert lib.mi_gp_sparse_bound_grad(None, tp, ctypes.byref(out), None) == -1
        assert lib.mi_gp_sparse_factor(None, tp) == -1

        # predict: before factor, null buffers, no points
        assert lib.mi_gp_sparse_predict(s, FAKE, 10, FAKE, FAKE, 0) == -1
        assert b"mi_gp_sparse_factor first" in err()
        for args in ((None, 10, FAKE, FAKE), (FAKE, 10, None, FAKE), (FAKE, 10, FAKE, None), (FAKE, 0, FAKE, FAKE)):
            assert lib.mi_gp_sparse_predict(s, *args, 1) == -1
            assert b"mi_gp_sparse_predict" in err()
        assert lib.mi_gp_sparse_predict(None, FAKE, 10, FAKE, FAKE, 0) == -1
    finally:
        assert lib.mi_gp_sparse_destroy(s) == 0
    assert lib.mi_gp_sparse_destroy(None) == 0
