"""The C-ABI library loads on a CPU-only box and exports every symbol include/mi_gp.h declares."""
import os
import re

from conftest import ROOT


def _declared():
    text = open(os.path.join(ROOT, "include", "mi_gp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mi_gp_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from andvaranaut_amd import _lib

    lib = _lib.load()
    names = _declared()
    assert len(names) >= 10
    for n in names:
        assert hasattr(lib, n), f"libmi_gp.so does not export {n}"
    assert sorted(_lib.EXPORTS) == names, "andvaranaut_amd/_lib.py:EXPORTS is out of sync with include/mi_gp.h"


def test_library_exports_nothing_but_the_c_abi():
    """the C-ABI is the boundary -- no internal launcher (migp::launch_gemm_f64, chol_panel_blocks, ...), kernel
    handle object or C++ runtime template instantiation is linkable from outside (-fvisibility=hidden + csrc/libmi_gp.map)."""
    import shutil
    import subprocess

    import pytest

    from andvaranaut_amd import _lib

    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/lib/llvm/bin")
    if nm is None:
        pytest.skip("no nm")
    out = subprocess.check_output([nm, "-D", "--defined-only", _lib.LIB_PATH], text=True)
    syms = [line.split() for line in out.splitlines() if line.strip()]
    assert len(syms) >= 10
    names = sorted(s[-1] for s in syms)
    assert names == _declared(), sorted(set(names) ^ set(_declared()))
    assert all(s[-2] == "T" for s in syms), [s for s in syms if s[-2] != "T"]


def test_bad_arguments_are_reported_not_crashed():
    import ctypes

    from andvaranaut_amd import _lib

    lib = _lib.load()
    # no GPU needed: argument validation happens before any HIP call
    assert lib.mi_gp_gemm_f64(0, 1, 100, 128, 16, 1.0, None, 16, None, 16, 0.0, None, 128, 0, 0, 1, 0, 0, 0, None) == -1
    assert b"multiples" in lib.mi_gp_last_global_error()
    cfg = _lib.MiGpConfig()
    cfg.n, cfg.d, cfg.nkern = 0, 1, 1
    h = ctypes.c_void_p()
    assert lib.mi_gp_create(ctypes.byref(cfg), ctypes.byref(h)) == -1
    assert b"mi_gp_create" in lib.mi_gp_last_global_error()
    # the sharded-gradient blocks validate before touching the device too
    assert lib.mi_gp_trsm_block(None, 16, None, 0, 1, None, 16, 128, None) == -1
    assert lib.mi_gp_trmv_upper(None, 16, None, 4, None, None) == -1
    assert lib.mi_gp_grad_contract_block_scratch(1000, 512, 512, 10) == (16 - 8) * 8 * 10  # 16 tile rows, slab = columns 8..15
    # batched entry points: null handle / buffers
    assert lib.mi_gp_set_batch(None, None) == -1
    assert lib.mi_gp_lml_batch(None, 1, None, None, None) == -1
    assert lib.mi_gp_lml_grad_batch(None, 1, None, None, None, None) == -1
    ids = (ctypes.c_int * 4)(0, 0, 0, 0)
    assert lib.mi_gp_grad_contract_block(2, 1, ids, ids, None, None, 100, None, 16, 64, 0, 64, None, None, 0, None, None) == -1


def test_product_package_never_imports_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "andvaranaut_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("# oracle", ""), f"{f} mentions the oracle"


def test_block_entries_reject_what_their_contract_excludes():
    """Argument validation of the block-level entries and of the compositions every entry takes: each refusal returns -1 with
    a text before any HIP call (no GPU here), instead of launching with an out-of-range k window, an unknown kernel id that
    the device would evaluate as Exponential, or a null pointer."""
    import ctypes

    from andvaranaut_amd import _lib

    lib = _lib.load()
    err = lib.mi_gp_last_global_error
    fake = 4096  # never dereferenced: every call below fails validation first

    # mi_gp_lml_partial: null buffers and n <= 0
    assert lib.mi_gp_lml_partial(None, 16, fake, 4, fake, None) == -1
    assert b"mi_gp_lml_partial" in err()
    assert lib.mi_gp_lml_partial(fake, 16, None, 4, fake, None) == -1
    assert lib.mi_gp_lml_partial(fake, 16, fake, 4, None, None) == -1
    assert lib.mi_gp_lml_partial(fake, 16, fake, 0, fake, None) == -1
    assert lib.mi_gp_lml_partial(fake, 16, fake, -3, fake, None) == -1

    # GEMM: kmode outside 0..4, k windows that would leave [0, k) or come out empty, k = 0
    def gemm(m, n, k, kmode):
        return lib.mi_gp_gemm_f64(0, 0, m, n, k, 1.0, fake, 512, fake, 512, 0.0, fake, 512, 0, kmode, 1, 0, 0, 0, None)

    def tuned(m, n, k, kmode):
        return lib.mi_gp_gemm_f64_tuned(0, 0, m, n, k, 1.0, fake, 512, fake, 512, 0.0, fake, 512, 0, kmode, 0, 0, 0, 0, None)

    for f in (gemm, tuned):
        for kmode in (-1, 5, 99):
            assert f(256, 256, 256, kmode) == -1
            assert b"kmode must be 0..4" in err()
        assert f(256, 256, 0, 0) == -1
        assert b"positive multiple of 32" in err()
        for kmode in (1, 4):
            assert f(128, 384, 256, kmode) == -1  # k < n
            assert b"k >= n" in err()
        for kmode in (2, 3):
            assert f(384, 128, 256, kmode) == -1  # k < m
            assert b"k >= m" in err()

    # compositions: unknown ids, ops outside {0, 1}, null arrays
    ids_bad = (ctypes.c_int * 8)(0, 5, 0, 0, 0, 0, 0, 0)
    ids_neg = (ctypes.c_int * 8)(-1, 0, 0, 0, 0, 0, 0, 0)
    ids_ok = (ctypes.c_int * 8)(0, 1, 0, 0, 0, 0, 0, 0)
    ops_bad = (ctypes.c_int * 8)(2, 0, 0, 0, 0, 0, 0, 0)
    ops_ok = (ctypes.c_int * 8)(1, 0, 0, 0, 0, 0, 0, 0)

    def assemble(nkern, ids, ops):
        return lib.mi_gp_assemble_block(2, nkern, ids, ops, fake, fake, 64, fake, 64, 0, 0, fake, 64, 64, 64, 0, None)

    def contract(nkern, ids, ops):
        return lib.mi_gp_grad_contract_block(2, nkern, ids, ops, fake, fake, 100, fake, 128, 0, 0, 64, fake, fake, 1 << 20,
                                             fake, None)

    for f, name in ((assemble, b"mi_gp_assemble_block"), (contract, b"mi_gp_grad_contract_block")):
        for nkern, ids, ops, why in ((2, ids_bad, ops_ok, b"unknown kernel id"), (1, ids_neg, None, b"unknown kernel id"),
                                     (2, ids_ok, ops_bad, b"ops must be"), (1, None, None, b"null kernel_ids"),
                                     (2, ids_ok, None, b"null ops")):
            assert f(nkern, ids, ops) == -1, (name, nkern, why)
            assert name in err() and why in err(), err()

    cfg = _lib.MiGpConfig()
    cfg.n, cfg.d, cfg.nkern = 100, 2, 2
    cfg.kernel_ids[0], cfg.kernel_ids[1] = 0, 1
    cfg.ops[0] = 2
    h = ctypes.c_void_p()
    assert lib.mi_gp_create(ctypes.byref(cfg), ctypes.byref(h)) == -1
    assert b"ops must be" in err()
    cfg.ops[0], cfg.kernel_ids[1] = 0, 7
    assert lib.mi_gp_create(ctypes.byref(cfg), ctypes.byref(h)) == -1
    assert b"unknown kernel id" in err()

    sc = _lib.MiGpShardConfig()
    sc.n, sc.d, sc.nkern, sc.panel_tiles, sc.world, sc.rank = 1000, 2, 2, 2, 1, 0
    sc.kernel_ids[0], sc.kernel_ids[1], sc.ops[0] = 0, 1, 3
    sc.X_dev = sc.y_dev = sc.K_dev = sc.theta_dev = sc.info_dev = sc.out_dev = fake
    sc.P_dev[0] = sc.P_dev[1] = fake
    sc.ldk, sc.ldp = 1 << 12, 1 << 20
    s = ctypes.c_void_p()
    assert lib.mi_gp_shard_create(ctypes.byref(sc), ctypes.byref(s)) == -1
    assert b"ops must be" in lib.mi_gp_shard_last_error(None)
    sc.ops[0], sc.kernel_ids[1] = 1, 9
    assert lib.mi_gp_shard_create(ctypes.byref(sc), ctypes.byref(s)) == -1
    assert b"unknown kernel id" in lib.mi_gp_shard_last_error(None)
