"""A covariance that is not positive definite, with the first bad pivot DEEP inside the factorisation, through every schedule.

include/mi_gp.h promises for that case: the 1-based index of the first non-positive pivot (LAPACK dpotrf's info), LML = -inf, an
all +0.0 gradient, no abort, no -2, no factor / K^-1 left behind, and a handle whose next evaluation returns what it would have
returned anyway.  After a bad pivot the leaf goes on with the square root of a negative number: NaN flows through every later
strip, update and leaf on both streams, through the whole second half of a gradient evaluation, and stays in K, Z and W for the
next evaluation to overwrite.  Every failure the other modules produce is seen by the first leaf; here the failing row sits at the
leaf's block edges, in the middle and at the edges of super-panels (the second one, an extended one, one whose update rode inside
the bulk update), in the column-mode tail, and in the last tile column behind which only the padding follows.

The expected index never comes from the device: tests/bad_pivot_cases.py holds the cases and the two constructions,
tests/test_bad_pivot_host.py proves them against scipy's dpotrf.  Everything asserted here is exact -- indices, -inf, +0.0, return
codes, bit equality -- and there is no tolerance in this module.  The positions follow from the handle's option values
(mi_gp_get_option 0, 2, 4-6, 20, 21, 30, 35, 37, 46) through bad_pivot_cases.schedule; test_every_schedule_is_hit_by_a_failing_case
asserts from those values that look-ahead, an extended super-panel, the riding update, a column-mode tail behind panels and option
30's early start each see at least one failure.  Agreement of the good evaluations with the oracle is other modules' business
(test_gpu_lml.py, test_gpu_large_shapes.py).

BAD_PIVOT_REPORT=<path> appends one JSON line per case (size, position, row, entry point, reported index)."""
import ctypes
import json
import os

import numpy as np
import pytest

import bad_pivot_cases as C

pytestmark = pytest.mark.gpu

DP = ctypes.POINTER(ctypes.c_double)
NOT_FACTORED = "call mi_gp_factor first"
NO_KINV = "call mi_gp_lml_grad first"
M_NEW = 5  # prediction points of the before / after evaluations


def _mods():
    import torch

    assert torch.cuda.is_available()
    from andvaranaut_amd import MiGP

    return torch, MiGP


def _report(**kw):
    path = os.environ.get("BAD_PIVOT_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(kw) + "\n")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    """Bit equality of two results (dicts of floats / arrays): NaN payloads and the sign of zero count."""
    assert a.keys() == b.keys()
    return [k for k in a if _bits(a[k]).shape != _bits(b[k]).shape or not np.array_equal(_bits(a[k]), _bits(b[k]))]


def _options(gp):
    o = {k: gp.get_option(k) for k in C.SCHEDULE_OPTIONS}
    assert all(v is not None for v in o.values()), o
    return o


def _xnew(n):
    return np.random.default_rng(n).random((M_NEW, C.D))


def _healthy(gp):
    """No poll gave up (the failure path answers every cross-stream signal): the handle has not demoted its edges."""
    assert gp.get_option(40) == 0, gp.last_error()


def _evaluate(gp, theta, Xn):
    """Every single-handle evaluation at a good theta, by name: the bits to keep."""
    r = {"lml": gp.lml(theta)}
    assert gp.info == 0 and np.isfinite(r["lml"])
    _healthy(gp)
    r["lml_grad.v"], r["lml_grad.g"], dy, dx = gp.lml_grad_data(theta)
    assert gp.info == 0 and np.isfinite(r["lml_grad.v"]) and np.isfinite(r["lml_grad.g"]).all()
    r["dlml_dy"], r["dlml_dx"] = dy, dx
    assert np.isfinite(dy).all() and np.isfinite(dx).all()
    _healthy(gp)
    assert gp.factor(theta) == 0
    _healthy(gp)
    r["predict.mu"], r["predict.var"] = gp.predict(theta, Xn, via_inverse=False)
    r["predict_u.mu"], r["predict_u.var"] = gp.predict(theta, Xn, via_inverse=True)
    r["pgrad.mu"], r["pgrad.var"], r["pgrad.dmu"], r["pgrad.dvar"] = gp.predict_grad(theta, Xn, refactor=False)
    r["cov.mu"], r["cov.sigma"] = gp.predict_cov(theta, Xn)
    for k, v in r.items():
        assert np.isfinite(v).all(), k
    return r


class _Abi:
    """Device buffers for the C-ABI calls that must refuse a handle without a factor / without K^-1 (the facade would
    refactorise by itself and hide a stale flag)."""

    def __init__(self, torch, gp, Xn):
        self.gp, self.lib, self.h = gp, gp.lib, gp.h
        dev = gp.dev
        self.xn = torch.from_numpy(Xn).to(dev)
        self.work = torch.empty((2 * 128, gp.lda), dtype=torch.float64, device=dev)
        self.out = torch.empty(2 * M_NEW + 2 * M_NEW * C.D, dtype=torch.float64, device=dev)
        self.cov = torch.empty((128, 128), dtype=torch.float64, device=dev)
        self.gx = torch.empty((gp.n, C.D), dtype=torch.float64, device=dev)
        self.awork = torch.empty(4 * 128 * (gp.lda + 128) + 65600, dtype=torch.float64, device=dev)
        self.dnew = torch.zeros(1, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        self.alpha = np.empty(gp.n)

    def _err(self):
        return self.lib.mi_gp_last_error(self.h).decode()

    def predictors(self, has_diag):
        """(name, return value, error text) of every consumer of a resident factor."""
        lib, h, m, ldw = self.lib, self.h, M_NEW, self.gp.lda
        mu, var = self.out.data_ptr(), self.out.data_ptr() + 8 * m
        dmu, dvar = self.out.data_ptr() + 16 * m, self.out.data_ptr() + 16 * m + 8 * m * C.D
        xn, wk = self.xn.data_ptr(), self.work.data_ptr()
        res = []
        res.append(("mi_gp_predict", lib.mi_gp_predict(h, xn, m, wk, ldw, mu, var, 1), self._err()))
        res.append(("mi_gp_predict_u", lib.mi_gp_predict_u(h, xn, m, wk, ldw, mu, var, 1), self._err()))
        res.append(("mi_gp_predict_grad", lib.mi_gp_predict_grad(h, xn, m, wk, ldw, mu, var, 1, dmu, dvar), self._err()))
        res.append(("mi_gp_predict_cov", lib.mi_gp_predict_cov(h, xn, m, wk, ldw, mu, self.cov.data_ptr(), 128, 1), self._err()))
        res.append(("mi_gp_append", lib.mi_gp_append(h, xn, mu, self.dnew.data_ptr() if has_diag else None, 1,
                                                     self.awork.data_ptr(), ldw + 128), self._err()))
        return res

    def kinv_users(self):
        res = [("mi_gp_alpha", self.lib.mi_gp_alpha(self.h, self.alpha.ctypes.data_as(DP)), self._err())]
        res.append(("mi_gp_grad_x", self.lib.mi_gp_grad_x(self.h, self.gx.data_ptr()), self._err()))
        return res


def _fail_three_ways(gp, abi, theta, p, tag):
    """mi_gp_lml, mi_gp_lml_grad and mi_gp_factor on a covariance whose first bad pivot is row p (0-based): index p + 1, -inf,
    +0.0 gradient, nothing resident afterwards, no demotion.  (A return of -2 raises in the facade.)"""
    val = gp.lml(theta)
    _report(case=tag, row=p, entry="mi_gp_lml", info=gp.info)
    assert gp.info == p + 1, (tag, "mi_gp_lml", gp.info, p + 1)
    assert val == -np.inf
    _healthy(gp)
    val, grad = gp.lml_grad(theta)
    _report(case=tag, row=p, entry="mi_gp_lml_grad", info=gp.info)
    assert gp.info == p + 1, (tag, "mi_gp_lml_grad", gp.info, p + 1)
    assert val == -np.inf
    assert grad.shape == (gp.ntheta,) and np.all(grad == 0.0) and not np.signbit(grad).any(), grad
    _healthy(gp)
    for name, r, err in abi.kinv_users():
        assert r == -1 and NO_KINV in err, (tag, name, r, err)
    info = gp.factor(theta)
    _report(case=tag, row=p, entry="mi_gp_factor", info=info)
    assert info == p + 1, (tag, "mi_gp_factor", info, p + 1)
    _healthy(gp)
    for name, r, err in abi.predictors(True):
        assert r == -1 and NOT_FACTORED in err, (tag, name, r, err)


def _fail_other_schedules(gp, theta, p, tag):
    """The same index with look-ahead off (one stream) and with event edges: it must not depend on which stream saw it first."""
    la, edges = gp.get_option(0), gp.get_option(26)
    try:
        for what, value, name in ((0, 0, "one_stream"), (26, 0, "event_edges")):
            gp.set_option(what, value)
            val, grad = gp.lml_grad(theta)
            _report(case=tag, row=p, entry="mi_gp_lml_grad/" + name, info=gp.info)
            assert gp.info == p + 1, (tag, name, gp.info, p + 1)
            assert val == -np.inf and np.all(grad == 0.0) and not np.signbit(grad).any()
            _healthy(gp)  # (read before option 26 is set again: that would clear the flag)
            gp.set_option(what, la if what == 0 else edges)
    finally:
        gp.set_option(0, la)
        gp.set_option(26, edges)
    assert gp.get_option(0) == la and gp.get_option(26) == edges


@pytest.mark.parametrize("n", C.SINGLE_SIZES)
def test_first_bad_pivot_through_every_entry_point(n):
    """One handle per size: good evaluations (bits kept), then for every position a planted failure through mi_gp_lml,
    mi_gp_lml_grad and mi_gp_factor (+ the two other schedules), the refusals of everything that needs a factor or K^-1, and
    the good evaluations again -- alternately at the first theta (bits of the handle's own first evaluations) and at a
    different theta (bits of a fresh handle), straight behind the failure."""
    torch, MiGP = _mods()
    X, y = C.problem(n)
    Xn = _xnew(n)
    thetas = [C.good_theta(0), C.good_theta(1)]
    fresh = MiGP(X, y, C.KERNEL)
    try:
        before_b = _evaluate(fresh, thetas[1], Xn)
    finally:
        fresh.close()
    del fresh
    gp = MiGP(X, y, C.KERNEL)
    try:
        pos = C.positions(n, _options(gp))
        assert pos and 0 in pos.values() and n - 1 in pos.values()
        before = [_evaluate(gp, thetas[0], Xn), before_b]
        abi = _Abi(torch, gp, Xn)
        # the refusals asserted below are not refusals of the ARGUMENTS: with a factor and K^-1 resident the same calls succeed
        assert gp.factor(thetas[0]) == 0
        assert [r for _, r, _ in abi.predictors(False)[:4]] == [0, 0, 0, 0]
        gp.lml_grad(thetas[0])
        assert [r for _, r, _ in abi.kinv_users()] == [0, 0]
        for i, (name, p) in enumerate(pos.items()):
            tag = f"n={n}/{name}"
            w = i % 2  # the theta of the failure and of the evaluations behind it
            gp.set_diag(C.planted_diag(n, p, thetas[w]))
            _fail_three_ways(gp, abi, thetas[w], p, tag)
            _fail_other_schedules(gp, thetas[w], p, tag)
            # straight behind a failure that left no factor: a failed mi_gp_lml_grad as the LAST evaluation before the recovery
            val, _ = gp.lml_grad(thetas[w])
            assert val == -np.inf and gp.info == p + 1
            gp.set_diag(None)
            after = _evaluate(gp, thetas[w], Xn)
            assert _same(after, before[w]) == [], (tag, "theta", w, _same(after, before[w]))
        for w in (1, 0):
            after = _evaluate(gp, thetas[w], Xn)
            assert _same(after, before[w]) == [], (n, "end", w, _same(after, before[w]))
        _healthy(gp)
    finally:
        gp.close()


def test_set_data_ends_a_resident_factor():
    """include/mi_gp.h: mi_gp_set_data ends the resident factor, U and K^-1 -- a prediction behind it must not read the
    unfactored K of other buffers."""
    torch, MiGP = _mods()
    n = 500
    X, y = C.problem(n)
    gp = MiGP(X, y, C.KERNEL)
    try:
        Xn = _xnew(n)
        abi = _Abi(torch, gp, Xn)
        theta = C.good_theta(0)
        assert gp.factor(theta) == 0
        assert [r for _, r, _ in abi.predictors(False)[:4]] == [0, 0, 0, 0]
        gp.lml_grad(theta)
        assert gp.factor(theta) == 0
        with torch.cuda.device(gp.dev):
            gp.K_t = torch.full_like(gp.K_t, float("nan"))
            gp.Z_t = torch.zeros_like(gp.Z_t)
            gp.W_t = torch.zeros_like(gp.W_t)
            torch.cuda.synchronize(gp.dev)
        gp._bind()  # mi_gp_set_data to OTHER buffers
        for name, r, err in abi.predictors(False):
            assert r == -1 and NOT_FACTORED in err, (name, r, err)
        gp.lml_grad(theta)
        gp._bind()
        for name, r, err in abi.kinv_users():
            assert r == -1 and NO_KINV in err, (name, r, err)
        fresh = MiGP(X, y, C.KERNEL)
        try:
            want = _evaluate(fresh, theta, Xn)
        finally:
            fresh.close()
        assert _same(_evaluate(gp, theta, Xn), want) == []
    finally:
        gp.close()


def test_every_schedule_is_hit_by_a_failing_case():
    """Decided from the option values and the sizes, not assumed: each schedule of the factorisation sees a failing pivot in
    test_first_bad_pivot_through_every_entry_point -- inside it or in front of it, so that NaN flows through it."""
    torch, MiGP = _mods()
    X, y = C.problem(100)
    gp = MiGP(X, y, C.KERNEL)
    try:
        o = _options(gp)
    finally:
        gp.close()
    hit = {k: [] for k in ("one_stream", "two_streams_whole_column_mode", "look_ahead_panels", "second_panel", "extended_panel",
                           "riding_update", "column_tail_behind_panels", "early_u", "padded_last_column", "turn_at_option_46")}
    for n in C.SINGLE_SIZES:
        ntc = (n + 127) // 128
        s = C.schedule(ntc, o)
        rows = sorted(C.positions(n, o).values())
        inside = lambda c0, w: [p for p in rows if c0 * 128 <= p < (c0 + w) * 128]  # noqa: E731
        if not s["two"]:
            hit["one_stream"].append(n)
        if s["two"] and s["tail"] == 0:
            hit["two_streams_whole_column_mode"].append(n)
        if s["two"] and s["panels"]:
            hit["look_ahead_panels"].append(n)
        if s["two"] and len(s["panels"]) >= 2 and inside(*s["panels"][1][:2]):
            hit["second_panel"].append(n)
        if s["two"] and any(q[2] and inside(q[0], q[1]) for q in s["panels"]):
            hit["extended_panel"].append(n)
        if any(q[3] and inside(q[0], q[1]) for q in s["panels"]):
            hit["riding_update"].append(n)
        if s["panels"] and s["tail"] is not None and inside(s["tail"], ntc - s["tail"]):
            hit["column_tail_behind_panels"].append(n)
        if s["early"]:  # (mi_gp_lml_grad runs at every position)
            hit["early_u"].append(n)
        if n % 128 and n - 1 in rows and (ntc - 1) * 128 in rows:
            hit["padded_last_column"].append(n)
        if o[37] > 0 and ntc in (o[46], o[46] + 1):
            hit["turn_at_option_46"].append(n)
    _report(case="coverage", **{k: v for k, v in hit.items()})
    assert all(hit.values()), hit
    assert len(set(hit["turn_at_option_46"])) >= 2
    assert sum(n >= 48 * 128 - 127 for n in hit["look_ahead_panels"]) >= 1 and len(hit["look_ahead_panels"]) >= 3


# ------------------------------------------------------------------------------------------------------------- batches
K_BATCH = 5


def _batch_all(gp, th, Xn):
    """lml_batch, lml_grad_batch, factor_batch + predict_batch of one set of members: values, gradients, infos, prediction rows."""
    r = {"lml": gp.lml_batch(th)}
    r["info_lml"] = gp.batch_info.astype(np.float64)
    _healthy(gp)
    r["v"], r["g"] = gp.lml_grad_batch(th)
    r["info_grad"] = gp.batch_info.astype(np.float64)
    _healthy(gp)
    r["mu"], r["var"] = gp.predict_batch(th, Xn, mixture=False, max_batch=K_BATCH)
    r["info_factor"] = gp.batch_info.astype(np.float64)
    _healthy(gp)
    return r


def _single_all(gp, t, Xn):
    r = {"lml": gp.lml(t)}
    r["v"], r["g"] = gp.lml_grad(t)
    r["mu"], r["var"] = gp.predict(t, Xn, via_inverse=False)
    return r


@pytest.mark.parametrize("n,p,q", C.BATCH_CASES)
def test_batch_members_fail_alone(n, p, q):
    """K = 5 members on data with a repeated point: members 1 and 3 carry gv = 0, jitter = -0.05 kv (first bad pivot p + 1 by
    dpotrf, tests/test_bad_pivot_host.py), the others ordinary theta.  info_out = [0, p + 1, 0, p + 1, 0]; the good members'
    results are the bits of the same batch with good theta in places 1 and 3, and of the single entry points.  Then a batch in
    which EVERY member fails (p + 1 and pivot 1 interleaved), and a good batch behind it: the bits of a fresh handle."""
    torch, MiGP = _mods()
    X, y = C.repeated_point_problem(n, p, q)
    Xn = _xnew(n)
    g0, g1 = C.good_theta(0), C.good_theta(1)
    g2 = g0.copy()
    g2[: C.D] *= 1.07
    g2[C.D], g2[-2], g2[-1] = 1.3, 2e-4, 3e-6
    bad1, bad3, ten = C.bad_theta(n), C.bad_theta(n, kv=C.BAD_KV / 2), C.minus_ten_theta()
    good = np.array([g0, g1, g2, g0, g1])
    good[3, -2], good[4, C.D] = 5e-4, 0.9  # (no two members alike)
    mixed = good.copy()
    mixed[1], mixed[3] = bad1, bad3
    allbad = np.array([bad1, ten, bad3, ten, bad1])
    want_mixed = np.array([0, p + 1, 0, p + 1, 0], dtype=np.float64)
    want_allbad = np.array([p + 1, 1, p + 1, 1, p + 1], dtype=np.float64)

    fresh = MiGP(X, y, C.KERNEL)
    try:
        ref = _batch_all(fresh, good, Xn)
        for k in ("info_lml", "info_grad", "info_factor"):
            assert not ref[k].any(), (k, ref[k])
        for m in (0, 2, 4):  # the single entry points' bits (include/mi_gp.h: same arithmetic per element)
            one = _single_all(fresh, good[m], Xn)
            assert fresh.info == 0
            got = {"lml": ref["lml"][m], "v": ref["v"][m], "g": ref["g"][m], "mu": ref["mu"][m], "var": ref["var"][m]}
            assert _same(got, one) == [], (n, m, _same(got, one))
    finally:
        fresh.close()
    del fresh

    gp = MiGP(X, y, C.KERNEL)
    try:
        r = _batch_all(gp, mixed, Xn)
        _report(case=f"batch n={n}", row=p, entry="lml_batch / lml_grad_batch / factor_batch",
                info=[r["info_lml"].tolist(), r["info_grad"].tolist(), r["info_factor"].tolist()])
        for k in ("info_lml", "info_grad", "info_factor"):
            assert np.array_equal(r[k], want_mixed), (n, k, r[k], want_mixed)
        for m in (1, 3):
            assert r["lml"][m] == -np.inf and r["v"][m] == -np.inf
            assert np.all(r["g"][m] == 0.0) and not np.signbit(r["g"][m]).any()
            assert np.isnan(r["mu"][m]).all() and np.isnan(r["var"][m]).all()
        for m in (0, 2, 4):
            got = {k: r[k][m] for k in ("lml", "v", "g", "mu", "var")}
            want = {k: ref[k][m] for k in ("lml", "v", "g", "mu", "var")}
            assert _same(got, want) == [], (n, m, _same(got, want))
        # the single entry points report the same index for the bad members' theta
        for t in (bad1, bad3):
            assert gp.lml(t) == -np.inf and gp.info == p + 1, (n, gp.info, p + 1)
            v, g = gp.lml_grad(t)
            assert v == -np.inf and gp.info == p + 1 and np.all(g == 0.0) and not np.signbit(g).any()
            assert gp.factor(t) == p + 1
            _healthy(gp)
        # every member fails, at different indices
        r = _batch_all(gp, allbad, Xn)
        _report(case=f"batch n={n} all members bad", row=p, entry="lml_batch / lml_grad_batch / factor_batch",
                info=[r["info_lml"].tolist(), r["info_grad"].tolist(), r["info_factor"].tolist()])
        for k in ("info_lml", "info_grad", "info_factor"):
            assert np.array_equal(r[k], want_allbad), (n, k, r[k], want_allbad)
        assert np.all(r["lml"] == -np.inf) and np.all(r["v"] == -np.inf)
        assert np.all(r["g"] == 0.0) and not np.signbit(r["g"]).any()
        assert np.isnan(r["mu"]).all() and np.isnan(r["var"]).all()
        # ... and a good batch behind it returns a fresh handle's bits
        r = _batch_all(gp, good, Xn)
        assert _same(r, ref) == [], (n, _same(r, ref))
    finally:
        gp.close()


# ------------------------------------------------------------------------------------------------------ sharded driver
@pytest.mark.parametrize("n,pwt,p,q", C.DIST_CASES)
def test_sharded_driver_reports_the_first_bad_pivot(n, pwt, p, q):
    """DistGP on one rank, construction (b): lml and lml_grad return -inf / a zero gradient, info_value (the bad-pivot word,
    atomicMin(global column + 1)) is p + 1, and the next good evaluation returns the bits it returned before the failure.
    (One process playing rank r of W -- DistGP(emulate=...) -- needs a complete factor to copy the other ranks' panels from
    and has no all-reduce over the ranks' words: left out.)"""
    import torch

    assert torch.cuda.is_available()
    from andvaranaut_amd.distributed import DistGP

    X, y = C.repeated_point_problem(n, p, q)
    good, bad = C.good_theta(0), C.bad_theta(n)
    gp = DistGP(X, y, C.KERNEL, panel_width_tiles=pwt)
    try:
        assert gp.npan >= (3 if n <= 1500 else 9) and 0 <= p // (pwt * 128) < gp.npan
        v0 = gp.lml(good)
        assert np.isfinite(v0) and gp.info_value == 0x7F7F7F7F
        v1, g1 = gp.lml_grad(good)
        assert np.isfinite(v1) and np.isfinite(g1).all()
        val = gp.lml(bad)
        _report(case=f"dist n={n} pwt={pwt}", row=p, entry="DistGP.lml", info=gp.info_value)
        assert gp.info_value == p + 1, (gp.info_value, p + 1)
        assert val == -np.inf
        val, grad = gp.lml_grad(bad)
        _report(case=f"dist n={n} pwt={pwt}", row=p, entry="DistGP.lml_grad", info=gp.info_value)
        assert gp.info_value == p + 1, (gp.info_value, p + 1)
        assert val == -np.inf and grad.shape == (gp.ntheta,) and np.all(grad == 0.0) and not np.signbit(grad).any()
        v2, g2 = gp.lml_grad(good)
        assert gp.info_value == 0x7F7F7F7F
        assert _same({"v": v2, "g": g2}, {"v": v1, "g": g1}) == []
        assert _same({"v": gp.lml(good)}, {"v": v0}) == []
    finally:
        gp.close()
