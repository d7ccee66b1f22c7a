"""Every entry point of one handle against the row-blocked oracle (oracle.gp_oracle.lml_all_blocked) at 34-130 tile columns,
where the factorisation's schedule changes with the size (ntc = ceil(N / 128) tile columns; cholesky_enqueue in
andvaranaut_amd/csrc/gp_sched.hip).  The bit-identity tests compare one schedule with another: an error both share passes them.

Which shape rules each default size reaches (single evaluation, default options; the factor has ntr = ntc + 1 tile rows):

  ntc  super-panels       extended panels (35)   column-mode tail (37)  merged head (20)  split bulk (18/19)  early U (30/31)
   34  4-tile, 3          at 0, 4, 8             from column 12         -                 -                   -
   40  4-tile, 4          at 8, 12               from 16                -                 -                   -
   60  4-tile, 9          at 28, 32              from 36                -                 -                   -
   61  8-tile, 5          at 24, 32              from 40                -                 -                   -
   63  8-tile, 5          at 24, 32              from 40                -                 -                   -
   64  8-tile, 5          at 32                  from 40                -                 -                   gradient
   79  8-tile, 7          at 40, 48              from 56                -                 -                   gradient
   80  8-tile, 7          at 48                  from 56                n1 = 8            -                   gradient
   96  8-tile, 9          at 64                  from 72                n1 = 8, 16, 24    behind n1 = 8       gradient
  (extra, LARGE_SHAPES_EXTRA_NTC)
  112  8-tile, 11         at 80                  from 88                n1 = 8 .. 40      behind n1 = 8 .. 24 gradient
  130  8-tile, 14         at 96, 104             from 112               n1 = 8 .. 56      behind n1 = 8 .. 40 gradient

The rules behind the table: super-panels are 4 tiles wide up to NARROW_PANELS_MAX_TILES = 60 tile columns, 8 above.  A panel
[c0, c0 + w) is extended (option 35) when ntr - (c0 + w) <= 32 and ntc - (c0 + w) > 8.  Problems of 32 tile columns or more
start in panel mode and enter column mode once at most rl_cols = 24 columns remain.  The merged head (option 20) needs
ntc - n1 >= 72 trailing columns at a panel boundary n1 >= 8 behind a non-extended panel: it starts at 80 tile columns, not 72.
The bulk update of a merged step splits (options 18 / 19) once its tiles past the head's rounds number at least 1536 + 1024,
from 95 tile columns on; the split of a plain step (bc (bc + 3) / 2 >= 2560 trailing tiles) is never reached by a single
evaluation at these sizes.  Early U = L^-T levels (options 30 / 31) run in gradient evaluations from 64 tile columns on.  The
single-stream tail (option 21: the last 8 columns) is behind the column-mode tail at the defaults: each case also runs the
panel-mode tail (option 37 = 0) against the oracle, which reaches it.

Each grid point draws its case from a seeded RNG: 1-4 components (Exponential allowed) or RatQuad alone, d from 1 to 12 (24 to
32 at ntc = 61), kv in [0.5, 1.5], gv log-uniform from max(1e-4, N kd / 1e7) to 1e-2 (so that cond2 stays at or below about
1e7).  Tolerances are the single-path sweep's (tests/test_gpu_random_sweep.py) with cond2 from oracle.cond2_spd.
LARGE_SHAPES_SEEDS (default 1) cases per size; LARGE_SHAPES_EXTRA_NTC (comma-separated, e.g. "72,73,112,130") adds sizes.
The worst error / (cond eps) per quantity is printed at the end of the module (pytest -s) and, when LARGE_SHAPES_RATIOS names a
file, written there as JSON."""
import json
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
NAMES = ["RBF", "Matern52", "Matern32", "Exponential"]
GRID = [34, 40, 60, 61, 63, 64, 79, 80, 96]
EXTRA = [int(v) for v in os.environ.get("LARGE_SHAPES_EXTRA_NTC", "").split(",") if v.strip()]
SEEDS = int(os.environ.get("LARGE_SHAPES_SEEDS", "1"))
RATIOS = {}


def _mods():
    import torch

    assert torch.cuda.is_available()
    from andvaranaut_amd import MiGP
    from oracle import gp_oracle as orc

    return MiGP, orc


def _case(ntc, seed, orc):
    rng = np.random.default_rng(7000 + 1000 * seed + ntc)
    N = 128 * ntc - int(rng.integers(0, 127))
    if rng.random() < 0.15:
        kerns, ops = ["RatQuad"], []  # (the reference only supports RatQuad on its own, gpmcmc.py:287)
    else:
        nk = int(rng.integers(1, 5))
        kerns = [NAMES[int(rng.integers(0, 3 if i else 4))] for i in range(nk)]
        ops = [("+", "*")[int(rng.integers(0, 2))] for _ in range(nk - 1)]
    nk = len(kerns)
    d = int(rng.integers(24, 33)) if ntc == 61 else int(rng.integers(1, 13))
    X, y = orc.synth_problem(N, d, seed=ntc + 100 * seed)
    theta = orc.synth_theta(d, nkern=nk)
    theta[: nk * d] *= rng.uniform(0.7, 1.6, nk * d) * np.sqrt(max(d, 2) / 2.0)
    theta[nk * d : nk * d + nk] = rng.uniform(0.5, 1.5, nk)
    if kerns == ["RatQuad"]:
        theta[nk * d + nk] = rng.uniform(0.5, 3.0)
    kd = float(orc.kernel_diag(kerns, ops, theta, d))
    lo = min(1e-2, max(1e-4, N * kd / 1e7))  # lambda_max <= N kd
    theta[nk * d + 2 * nk] = 10.0 ** rng.uniform(np.log10(lo), -2.0)
    kernel = kerns[0] + "".join(o + k for o, k in zip(ops, kerns[1:]))
    return N, d, kerns, ops, kernel, X, y, theta, rng


def _rel(a, b):
    """max |a - b| / max(|b|, 1e-3 max|b|): per component, floored at 1e-3 of the largest component."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-3 * max(np.max(np.abs(b)), 1e-300))))


def _note(key, err, cond):
    RATIOS[key] = max(RATIOS.get(key, 0.0), err / (cond * EPS))


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    if RATIOS:
        print("worst error / (cond eps):", json.dumps(RATIOS, sort_keys=True))
        path = os.environ.get("LARGE_SHAPES_RATIOS")
        if path:
            with open(path, "w") as f:
                json.dump(RATIOS, f, indent=1, sort_keys=True)


def _lml_grad_checks(gp, orc, theta, ref, cond, expo, what):
    """LML and its parts, theta / y / X gradients of one evaluation against the blocked oracle; returns (lml, grad)."""
    tol = max(1e-8 if expo else 1e-10, 20.0 * cond * EPS)
    gtol = max(1e-5 if expo else 1e-7, 500.0 * cond * EPS)
    val = gp.lml(theta)
    logdet, quad = gp.lml_parts()
    e = abs(val - ref["lml"]) / max(abs(ref["lml"]), 1.0)
    _note("lml", e, cond)
    assert e <= tol, (what, val, ref["lml"], e, tol)
    e = abs(logdet - ref["logdet"]) / max(abs(ref["logdet"]), 1.0)
    _note("logdet", e, cond)
    assert e <= tol, (what, "logdet", logdet, ref["logdet"], e, tol)
    e = abs(quad - ref["quad"]) / max(abs(ref["quad"]), 1.0)
    _note("quad", e, cond)
    assert e <= tol, (what, "quad", quad, ref["quad"], e, tol)
    v2, g, gy, gx = gp.lml_grad_data(theta)
    assert v2 == val, (what, v2, val)  # lml(theta) is the value lml_grad(theta) returns, bit for bit
    for key, got, t in (("grad_theta", g, gtol), ("grad_y", gy, gtol), ("grad_X", gx, 10 * gtol)):
        e = _rel(got, ref[{"grad_theta": "grad", "grad_y": "gy", "grad_X": "gX"}[key]])
        _note(key, e, cond)
        assert e <= t, (what, key, e, t)
    return val, g


@pytest.mark.parametrize("ntc,seed", [(n, s) for n in GRID + EXTRA for s in range(SEEDS)])
def test_large_shape_all_entry_points_match_the_blocked_oracle(ntc, seed):
    MiGP, orc = _mods()
    N, d, kerns, ops, kernel, X, y, theta, rng = _case(ntc, seed, orc)
    expo = "Exponential" in kerns
    M, m2, mc = 500, 4, int(rng.integers(100, 201))
    Xn = rng.random((M, d))
    Xc = rng.random((mc, d)) * 1.2 - 0.1
    t0 = time.time()
    ref = orc.lml_all_blocked(X, y, kerns, ops, theta, Xnew=Xn, Xgrad=Xn[:m2], Xcov=Xc)
    cond = orc.cond2_spd(ref.pop("L"))
    print(f"ntc={ntc} N={N} d={d} {kernel} cond={cond:.3e} oracle {time.time() - t0:.1f} s")
    kd = float(orc.kernel_diag(kerns, ops, theta, d))
    gp = MiGP(X, y, kernel)
    try:
        v0, g0 = _lml_grad_checks(gp, orc, theta, ref, cond, expo, "default")
        # predictions through both routes, their point gradients, the joint covariance
        ctol = max(1e-8, 200.0 * cond * EPS)
        gtol = max(1e-5 if expo else 1e-7, 500.0 * cond * EPS)
        for via in (False, True):
            mu, var = gp.predict(theta, Xn, via_inverse=via)
            e_mu = np.max(np.abs(mu - ref["mu"]) / (1.0 + np.abs(ref["mu"])))  # (the allclose forms below, per unit of tolerance)
            e_var = np.max(np.abs(var - ref["var"]) / (np.abs(ref["var"]) + 1e-2))
            _note("mean", e_mu, cond)
            _note("variance", e_var, cond)
            assert np.allclose(mu, ref["mu"], rtol=ctol, atol=ctol), (via, e_mu, ctol)
            assert np.allclose(var, ref["var"], rtol=10 * ctol, atol=max(1e-10, ctol * 1e-2)), (via, e_var)
        pm, pv, dm, dv = gp.predict_grad(theta, Xn[:m2])
        assert np.allclose(pm, ref["mu"][:m2], rtol=ctol, atol=ctol)
        ptol = max(1e-4 if expo else 1e-6, 10 * gtol)
        for key, got, want in (("predict_grad_mean", dm, ref["dmu"]), ("predict_grad_var", dv, ref["dvar"])):
            e = np.max(np.abs(got - want)) / max(np.abs(want).max(), 1e-12)
            _note(key, e, cond)
            assert np.allclose(got, want, rtol=ptol, atol=ptol * max(np.abs(want).max(), 1e-12)), (key, e, ptol)
        _, S = gp.predict_cov(theta, Xc)
        stol = max(1e-7 if expo else 1e-9, 200.0 * cond * EPS) * kd
        e = np.abs(np.tril(S) - np.tril(ref["cov"])).max()
        _note("sigma", e / kd, cond)
        assert e <= stol, ("sigma", e, stol)
        # the same bits on every schedule: one stream with the two-stream default's panel width pinned, event edges
        width = 4 if ntc <= 60 else 8
        for opts in ([(0, 0), (2, width)], [(26, 0)]):
            for k, v in opts:
                gp.set_option(k, v)
            v1, g1 = gp.lml_grad(theta)
            assert v1 == v0 and np.array_equal(g1, g0), opts
            assert gp.lml(theta) == v0, opts
            gp.set_option(0, 1)
            gp.set_option(2, 0)
            gp.set_option(26, 2)
        # ... and a batch over [theta, perturbed theta] member by member
        th2 = theta.copy()
        th2[: len(kerns) * d] *= 1.05
        vb, gb = gp.lml_grad_batch(np.stack([theta, th2]))
        assert vb[0] == v0 and np.array_equal(gb[0], g0)
        v2, g2 = gp.lml_grad(th2)
        assert vb[1] == v2 and np.array_equal(gb[1], g2)
        # the panel-mode tail (no column mode): the last super-panels, the single-stream tail (option 21), other arithmetic
        gp.set_option(37, 0)
        _lml_grad_checks(gp, orc, theta, ref, cond, expo, "option 37 = 0")
        gp.set_option(37, 24)
    finally:
        gp.close()


def test_config3_lml_grad_n16384_per_component():
    """BASELINE config 3 (Matern52, N = 16384, d = 16): every theta component and every component of the X gradient within
    1e-8 of the largest one, against the blocked oracle (test_config3_lml_grad_n16384 checks a central difference along the
    gradient's own direction, which a wrong small component passes)."""
    MiGP, orc = _mods()
    N, d = 16384, 16
    X, y = orc.synth_problem(N, d, seed=0)
    theta = orc.synth_theta(d)
    t0 = time.time()
    ref = orc.lml_all_blocked(X, y, ["Matern52"], [], theta)
    del ref["L"]
    print(f"config 3 blocked oracle: {time.time() - t0:.1f} s")
    gp = MiGP(X, y, "Matern52")
    val, g, gy, gx = gp.lml_grad_data(theta)
    gp.close()
    assert abs(val - ref["lml"]) <= 1e-10 * abs(ref["lml"]), (val, ref["lml"])
    err = np.abs(g - ref["grad"]).max() / np.abs(ref["grad"]).max()
    errx = np.abs(gx - ref["gX"]).max() / np.abs(ref["gX"]).max()
    erry = np.abs(gy - ref["gy"]).max() / np.abs(ref["gy"]).max()
    print(f"config 3: theta {err:.3e}, X {errx:.3e}, y {erry:.3e} of the largest component")
    assert err <= 1e-8, (g, ref["grad"])
    assert errx <= 1e-8, errx
    assert erry <= 1e-8, erry
