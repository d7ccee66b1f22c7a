"""The design call on the GPU (options 56 / 57 of mi_gp_set_option behind mi_gp_predict_cov, MiGP.design) against the long-double
greedy selection of tests/design_ref.py: the chosen sequence exactly (tests/test_design_host.py asserts the inputs' gap
condition), gains and round-0 gains within the project's fp64 rule max(1e-10, 200 cond(K_y) eps) of the largest round-0 gain;
then, without any reference, the gains as drops of the mean latent variance under append; then the contract -- after append,
coincident points, repeated and NaN-filled calls, permuted candidates, option 56 = 0 afterwards, the refusals.  Every parity
check prints error / tolerance before it asserts."""
import ctypes
import os

import numpy as np
import pytest

import design_ref as dr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [dr.case_id(c) for c in dr.CASES]
_poison_lib = None


def _poison_scratch(gp):
    """NaN into ALL of the handle's design scratch (tools/design_poison.hip); the scratch must exist"""
    global _poison_lib
    if _poison_lib is None:
        path = os.path.join(ROOT, "tools", "libdesignpoison.so")
        assert os.path.exists(path), "tools/libdesignpoison.so missing: run __graft_entry__.build()"
        _poison_lib = ctypes.CDLL(path)
        _poison_lib.design_poison.argtypes = [ctypes.c_void_p]
        _poison_lib.design_poison.restype = ctypes.c_long
    assert _poison_lib.design_poison(gp.h) > 0


def _gp(c, n=None):
    from andvaranaut_amd import MiGP

    gp = MiGP(c["X"][:n], c["y"][:n], c["kernel"], device=0)
    assert gp.factor(c["theta"]) == 0
    return gp


def _raw(gp, C, R, b, noise=1, nan=False, m=None, ldw=None, ldc=None, null=()):
    """mi_gp_predict_cov under options 56 = b / 57 = Mr on buffers of the test's own: (return code, the Mc + 2 b + 1 doubles)"""
    import torch

    Mc, Mr = len(C), len(R)
    mcp, mrp = gp._padded(Mc), gp._padded(Mr)
    dev = gp.dev
    fill = float("nan") if nan else 0.0
    xn = torch.from_numpy(np.concatenate([C, R.reshape(Mr, gp.d)])).to(dev)
    work = torch.full((mcp + mrp, gp.lda), fill, dtype=torch.float64, device=dev)
    cov = torch.full((mcp, max(mrp, 2)), fill, dtype=torch.float64, device=dev)
    out = torch.full((Mc + 2 * b + 1,), fill, dtype=torch.float64, device=dev)
    if nan:
        _poison_scratch(gp)
    torch.cuda.synchronize(dev)
    gp.set_option(57, Mr)
    gp.set_option(56, b)
    try:
        ptr = dict(x=xn.data_ptr(), work=work.data_ptr(), out=out.data_ptr(), cov=cov.data_ptr() if Mr else None)
        for k in null:
            ptr[k] = None
        r = gp.lib.mi_gp_predict_cov(gp.h, ptr["x"], Mc + Mr if m is None else m, ptr["work"], gp.lda if ldw is None else ldw, ptr["out"],
                                     ptr["cov"], mrp if ldc is None else ldc, noise)
    finally:
        gp.set_option(56, 0)
        gp.set_option(57, 0)
    return r, out.cpu().numpy()


def _check(tag, c, ref, idx, gains, gains0):
    tol = dr.tolerance(c["X"], c["kernel"], c["theta"], ref["gains0"])
    r1 = float(np.abs(gains - ref["gains"].astype(np.float64)[: len(gains)]).max() / tol) if len(gains) else 0.0
    r0 = float(np.nanmax(np.abs(gains0 - ref["gains0"].astype(np.float64))) / tol)
    print(f"{tag}: chosen {[int(i) for i in idx]}, gains error / tolerance {r1:.3e}, round-0 error / tolerance {r0:.3e} (tolerance {tol:.3e})")
    assert list(idx) == ref["idx"].tolist()
    assert r1 <= 1.0 and r0 <= 1.0
    assert np.array_equal(np.isnan(gains0), np.isnan(ref["gains0"].astype(np.float64)))


@pytest.mark.parametrize("case", dr.CASES, ids=IDS)
def test_selection_matches_the_long_double_reference(case):
    c = dr.case_data(*case)
    gp = _gp(c)
    try:
        idx, gains, gains0 = gp.design(c["theta"], c["C"], c["R"] if case[2] else None, batch=case[4])
        _check(dr.case_id(case), c, dr.reference(case), idx, gains, gains0)
        assert gp.get_option(56) == 0 and gp.get_option(57) == 0
        # the raw record: count, -1 and 0 in the unused slots
        r, o = _raw(gp, c["C"], c["R"], case[4])
        Mc, b = case[1], case[4]
        count = min(Mc, b)
        assert r == 0 and o[-1] == count and np.array_equal(o[Mc : Mc + count], idx)
        assert (o[Mc + count : Mc + b] == -1).all() and (o[Mc + b + count : Mc + 2 * b] == 0).all()
        if case == dr.CASES[0]:  # jitter only in v(c)
            i2, g2, g02 = gp.design(c["theta"], c["C"], c["R"], batch=case[4], noise=False)
            _check(dr.case_id(case) + " noise=False", c, dr.reference(case, noise=False), i2, g2, g02)
    finally:
        gp.close()


def test_gains_are_the_drops_of_the_mean_variance_under_append():
    """no reference: the chosen points appended one at a time, mean_r of predict(pred_noise=False)'s variance drops by each gain"""
    case = dr.CASES[0]
    c = dr.case_data(*case)
    gp = _gp(c)
    try:
        idx, gains, gains0 = gp.design(c["theta"], c["C"], c["R"], batch=case[4])
        tol = dr.tolerance(c["X"], c["kernel"], c["theta"], gains0)
        prev = gp.predict(c["theta"], c["R"], pred_noise=False, via_inverse=False)[1].mean()
        for k, p in enumerate(idx):
            assert gp.append(c["C"][p : p + 1], np.array([0.3 * k])) == 0
            cur = gp.predict(c["theta"], c["R"], pred_noise=False, via_inverse=False)[1].mean()
            print(f"point {k} (candidate {p}): gain {gains[k]:.6e}, drop {prev - cur:.6e}, difference / tolerance "
                  f"{abs(gains[k] - (prev - cur)) / tol:.3e}")
            assert abs(gains[k] - (prev - cur)) <= tol
            prev = cur
    finally:
        gp.close()


def test_after_an_append_across_a_tile():
    c = dr.case_data(*dr.APPEND_CASE)
    gp = _gp(c, 250)
    try:
        assert gp.append(c["X"][250:], c["y"][250:]) == 0 and gp.n == 258 and gp.np_ == 384
        idx, gains, gains0 = gp.design(c["theta"], c["C"], c["R"], batch=c["b"])
        _check("n = 250 -> 258", c, dr.reference(dr.APPEND_CASE), idx, gains, gains0)
    finally:
        gp.close()


def test_coincident_points_without_noise():
    """gv = 0: a candidate on a training point and a repeated candidate (an exact tie, the lower index of the pair stands for it)"""
    c = dr.coincident_case()
    gp = _gp(c)
    try:
        idx, gains, gains0 = gp.design(c["theta"], c["C"], c["R"], batch=c["b"])
        assert np.isfinite(gains).all() and np.isfinite(gains0).all()
        idx = [dr.DUP[0] if i == dr.DUP[1] else int(i) for i in idx]
        _check("coincident", c, c["ref"], idx, gains, gains0)
    finally:
        gp.close()


def test_same_bits_on_repeats_nan_filled_buffers_and_permuted_candidates():
    case = dr.CASES[1]
    c = dr.case_data(*case)
    gp = _gp(c)
    try:
        b = case[4]
        r0, o0 = _raw(gp, c["C"], c["R"], b)
        r1, o1 = _raw(gp, c["C"], c["R"], b)
        r2, o2 = _raw(gp, c["C"], c["R"], b, nan=True)
        assert r0 == r1 == r2 == 0
        assert np.array_equal(o0, o1) and np.array_equal(o0, o2) and np.isfinite(o0).all()
        perm = np.random.default_rng(5).permutation(case[1])
        _, op = _raw(gp, c["C"][perm], c["R"], b)
        Mc = case[1]
        assert np.array_equal(perm[op[Mc : Mc + b].astype(int)], o0[Mc : Mc + b].astype(int))
        # the variance criterion too
        q0, q1 = _raw(gp, c["C"], c["R"][:0], b), _raw(gp, c["C"], c["R"][:0], b, nan=True)
        assert q0[0] == q1[0] == 0 and np.array_equal(q0[1], q1[1]) and np.isfinite(q0[1]).all()
    finally:
        gp.close()


def test_option_56_zero_afterwards_is_predict_cov_as_before():
    case = dr.CASES[0]
    c = dr.case_data(*case)
    gp = _gp(c)
    try:
        mu0, cov0 = gp.predict_cov(c["theta"], c["R"])
        mean0, var0 = gp.predict(c["theta"], c["R"], via_inverse=False)
        gp.design(c["theta"], c["C"], c["R"], batch=case[4])
        mu1, cov1 = gp.predict_cov(c["theta"], c["R"])
        mean1, var1 = gp.predict(c["theta"], c["R"], via_inverse=False)
        assert np.array_equal(mu0, mu1) and np.array_equal(cov0, cov1) and np.array_equal(mean0, mean1) and np.array_equal(var0, var1)
    finally:
        gp.close()


def test_refusals_return_minus_one_and_name_the_option():
    from andvaranaut_amd import MiGP

    case = dr.CASES[0]
    c = dr.case_data(*case)
    C, R, b = c["C"], c["R"], case[4]
    gp = MiGP(c["X"], c["y"], c["kernel"], device=0)
    try:
        def refused(match, **kw):
            r, _ = _raw(gp, C, R, b, **kw)
            text = gp.last_error()
            assert r == -1 and "option 56" in text and match in text, (r, text)

        refused("mi_gp_factor")  # no factorisation
        assert gp.factor(c["theta"]) == 0
        gp.set_diag(np.full(gp.n, 1e-3))
        assert gp.factor(c["theta"]) == 0
        refused("per-point diagonal")
        gp.set_diag(None)
        assert gp.factor(c["theta"]) == 0
        refused("Mc >= 1", m=len(R))
        refused("Mc >= 1", m=0)
        refused("ldw", ldw=gp.lda + 1)
        refused("ldw", ldw=gp.np_ - 2)
        refused("ldc", ldc=126)
        refused("ldc", ldc=129)
        for k in ("x", "work", "out", "cov"):
            refused("null buffer", null=(k,))
        assert _raw(gp, C, R, b)[0] == 0  # nothing was broken by the refusals
        for what, value in ((56, 129), (56, -1), (57, -1)):
            with pytest.raises(RuntimeError, match=f"option {what}"):
                gp.set_option(what, value)
        assert gp.get_option(56) == 0 and gp.get_option(57) == 0
        gp.set_option(50, 1)
        refused("option 50")
        gp.set_option(50, 0)
        gp.set_option(51, 2)
        refused("option 51")
        gp.set_option(51, 1)
    finally:
        gp.close()
