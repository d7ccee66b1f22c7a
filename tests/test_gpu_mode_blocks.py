"""The modes' scratch blocks across mi_gp_reserve and mi_gp_append: every mode call gives the same bits after the handle's capacity
is raised (the blocks that hold nothing between calls are dropped and allocated again, the resident factorisation is kept), and
what test_gpu_append.py asks of appended state after an append."""
import numpy as np
import pytest

from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

N, K, D, CAP = 100, 7, 2, 300  # (the capacity goes from 100 to 300 points: over the 128- and the 256-row tile boundary)
KERNEL = "RBF"
DEFAULTS = {48: 0, 49: 1, 50: 0, 51: 1, 52: 0, 53: 0, 54: 0, 55: 1024, 56: 0, 57: 0}
NFEAT = 64


class _HoldReserve:
    """the library, with mi_gp_reserve held back"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def mi_gp_reserve(self, h, capacity):
        return 0


def _roomy(monkeypatch, X, y):
    """a MiGP on buffers for CAP points whose HANDLE still has the capacity n: the constructor's mi_gp_reserve is held back"""
    from andvaranaut_amd import MiGP, _lib

    lib = _lib.load()
    with monkeypatch.context() as m:
        m.setattr(_lib, "load", lambda: _HoldReserve(lib))
        gp = MiGP(X, y, KERNEL, device=0, capacity=CAP)
    gp.lib = lib
    return gp


def _calls(gp, theta, Xq, Xc, Xr):
    """every mode call once; the first three read the resident factorisation, the objectives evaluate anew"""
    out = {}
    out["sweep"], out["dsweep"] = gp.mean_sweep(theta, Xq, grad=True)
    draw = gp.draw_paths(theta, 3, nfeatures=NFEAT, seed=5)
    out["paths"], out["dpaths"] = draw.evaluate(Xq, grad=True)
    draw.close()
    out["picked"], out["gains"], out["gains0"] = gp.design(theta, Xc, Xr, batch=4)
    out["loo"], out["dloo"] = gp.loo_grad(theta)
    out["cv"], out["dcv"] = gp.cv_grad(theta, 5)
    return out


def test_mode_calls_across_reserve_and_append(monkeypatch):
    from andvaranaut_amd import MiGP

    X, y = orc.synth_problem(N + K, D, seed=31)
    theta = orc.synth_theta(D, gv=1e-2, jitter=1e-6)
    rng = np.random.default_rng(7)
    Xq, Xc, Xr = rng.random((12, D)), rng.random((20, D)), rng.random((8, D))
    gp = _roomy(monkeypatch, X[:N], y[:N])
    first = _calls(gp, theta, Xq, Xc, Xr)
    # one factorisation, U and alpha resident, on both sides of the reserve
    assert gp.factor(theta) == 0
    sweep = gp.mean_sweep(theta, Xq)
    assert np.array_equal(sweep, first["sweep"])
    gp._check(gp.lib.mi_gp_reserve(gp.h, CAP), "mi_gp_reserve")
    second = _calls(gp, theta, Xq, Xc, Xr)
    for key in first:
        assert np.array_equal(first[key], second[key]), key
    # appended state against a fresh handle on all points, with test_gpu_append.py's tolerances: 200 cond eps (ten times that for
    # gradients) for what reads the appended factor, 1e-12 for an evaluation from scratch
    assert gp.factor(theta) == 0
    assert gp.append(X[N:], y[N:]) == 0 and gp.n == N + K and gp.append_refactors == 0
    third = _calls(gp, theta, Xq, Xc, Xr)
    fresh = MiGP(X, y, KERNEL, device=0)
    want = _calls(fresh, theta, Xq, Xc, Xr)
    fresh.close()
    cond = np.linalg.cond(orc.noisy_cov(X, [KERNEL], [], theta, form="conditional"))
    ptol = max(1e-10, 200.0 * cond * 2.2e-16)
    tols = {"sweep": ptol, "paths": ptol, "gains": ptol, "gains0": ptol, "dsweep": 10 * ptol, "dpaths": 10 * ptol}
    for key, tol in tols.items():
        err, scale = np.max(np.abs(third[key] - want[key])), max(np.max(np.abs(want[key])), 1.0)
        print("%s: error / bound %.3g" % (key, err / (tol * scale)))
        assert err <= tol * scale, key
    assert np.array_equal(third["picked"], want["picked"])
    for v, g in (("loo", "dloo"), ("cv", "dcv")):
        assert abs(third[v] - want[v]) <= 1e-12 * abs(want[v]), v
        assert np.allclose(third[g], want[g], rtol=1e-12, atol=1e-12 * np.abs(want[g]).max()), g
    # every mode option is what it was: the defaults, and option 55 the feature count that draw_paths and evaluate leave behind
    assert {what: gp.get_option(what) for what in DEFAULTS} == {**DEFAULTS, 55: NFEAT}
    gp.close()
