"""The CPU half of the sparse bound's gradient by the inducing locations (include/mi_gp_sparse.h, zgrad_slabs): the long-double
dF/dZ of tests/sgpr_zgrad_ref.py against central differences of the long-double bound, what fp64 alone costs on the device's steps
at every case of tests/test_gpu_sparse_zgrad.py, and the configuration field without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import sgpr_ref as R
import sgpr_zgrad_ref as ZR


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_long_double_gradient_agrees_with_central_differences_of_the_bound(kernel):
    """Three entries of dF/dZ at (n, m, d) = (300, 40, 3), h = 1e-6: the difference's truncation, h^2 F''' / 6, is what is left
    (3e-8 of max(|g|, 1) at most was measured); 1e-6 is asked for."""
    case = (kernel, 300, 40, 3, None, "kmeanspp")
    X, y, Z, theta, _, _ = R.device_case(case)
    g = ZR.case_reference(case)["grad_z"]
    h = 1e-6
    for u, k in ((0, 0), (17, 1), (39, 2)):
        Zp, Zm = Z.copy(), Z.copy()
        Zp[u, k] += h
        Zm[u, k] -= h
        step = R.LD(Zp[u, k]) - R.LD(Zm[u, k])
        fd = (R.bound_ld(X, y, Zp, kernel, theta, grad=False)["F"] - R.bound_ld(X, y, Zm, kernel, theta, grad=False)["F"]) / step
        err = float(abs(fd - g[u, k]) / max(abs(g[u, k]), 1))
        print(kernel, (u, k), "analytic %.10e, difference %.10e, error %.2e" % (float(g[u, k]), float(fd), err))
        assert err <= 1e-6, (u, k, err)


@pytest.mark.parametrize("case", R.DEVICE_CASES, ids=R.case_id)
def test_fp64_on_the_device_steps_uses_at_most_half_the_gradient_tolerance(case):
    X, y, Z, theta, _, chunk = R.device_case(case)
    ref = ZR.case_reference(case)
    ratio = ZR.ratio(ZR.device_fp64_z(X, y, Z, case[0], theta, chunk=chunk), ref)
    print(R.case_id(case), "cond(Kuu) = %.2e" % ref["cond_Kuu"], "max|dF/dZ| = %.3e" % float(np.max(np.abs(ref["grad_z"]))),
          "ratio %.4f" % ratio)
    assert ratio <= 0.5, ratio


def _create(zgrad_slabs):
    from andvaranaut_amd import _lib as L

    lib = L.load_sparse()
    cfg = L.MiGpSparseConfig()
    cfg.n, cfg.m, cfg.d, cfg.nkern, cfg.device, cfg.chunk = 1000, 100, 3, 1, 0, 256
    cfg.kernel_ids[0] = 1
    cfg.zgrad_slabs = zgrad_slabs
    s = ctypes.c_void_p()
    return lib, lib.mi_gp_sparse_create(ctypes.byref(cfg), ctypes.byref(s)), s


def test_a_negative_slab_count_is_refused_by_name_and_others_create():
    lib, r, s = _create(-1)
    assert r == -1 and s.value is None
    err = lib.mi_gp_sparse_last_error(None)
    assert b"mi_gp_sparse_create" in err and b"zgrad_slabs" in err, err
    for slabs in (0, 4):
        lib, r, s = _create(slabs)  # creation makes no HIP call: it succeeds without a GPU
        assert r == 0 and s.value is not None
        assert lib.mi_gp_sparse_destroy(s) == 0


def test_the_field_is_the_last_of_the_config_and_the_header_keeps_eight_entry_points():
    from andvaranaut_amd import _lib as L
    from conftest import ROOT

    assert L.MiGpSparseConfig._fields_[-1][0] == "zgrad_slabs"
    assert L.MiGpSparseConfig.zgrad_slabs.offset == ctypes.sizeof(L.MiGpSparseConfig) - ctypes.sizeof(ctypes.c_int)
    text = open(os.path.join(ROOT, "include", "mi_gp_sparse.h")).read()
    struct = re.search(r"typedef struct \{(.*?)\} mi_gp_sparse_config;", text, flags=re.S).group(1)
    fields = re.findall(r"\bint\s+([a-z_]+)\s*(?:\[[A-Z_]+\])?\s*;", re.sub(r"/\*.*?\*/", "", struct, flags=re.S))
    assert fields[-2:] == ["chunk", "zgrad_slabs"], fields
    declared = set(re.findall(r"\b(mi_gp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert len(declared) == 8 and sorted(declared) == sorted(L.SPARSE_EXPORTS), declared
