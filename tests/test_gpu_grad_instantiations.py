"""Every instantiation of the three kernels that differentiate through the composite covariance (csrc/grad_predict.hip:
GRAD_CONTRACT_KERNELS[5][2], GRAD_X_KERNELS[5][3], PREDICT_GRAD_KERNELS[5], component counts 5 to 8 through <8>) against a
reference of the same sum that does not depend on cond(K): the kernels' own inputs (random weights, or the device's K^-1,
alpha and w rows) contracted on the host in extended precision, bound 64 eps sum |terms|.  And the derivative math of
base_kernel_val_der entry by entry against 40-digit mpmath.  tests/grad_refs.py holds the case lists and the references
(tests/test_grad_refs_host.py: the lists cover the tables).  The worst error-to-bound ratio per table entry goes to
grad_instantiations.json in the directory $MIGP_TEST_RECORD_DIR names (default: test_records/ in the repository root)."""
import json
import os

import numpy as np
import pytest

import grad_refs as gr
from grad_refs import EPS, LD, TINY
from oracle import gp_oracle as orc
from test_gpu_blocks import ULP_CASES, _dev, _grid, _host, _ids, _lib, _same_bits

pytestmark = pytest.mark.gpu

RECORD = {}


def _record(section, key, ratio, **more):
    """Keep the worst ratio per key and rewrite the record (the tests run in any order and selection)."""
    sec = RECORD.setdefault(section, {})
    old = sec.get(key)
    if old is None or ratio >= old["ratio"]:
        sec[key] = dict(ratio=ratio, **more)
    out = os.environ.get("MIGP_TEST_RECORD_DIR") or os.path.join(gr.ROOT, "test_records")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "grad_instantiations.json"), "w") as f:
        json.dump(RECORD, f, indent=1, sort_keys=True)


def _migp():
    import torch

    assert torch.cuda.is_available()
    from andvaranaut_amd import MiGP

    return MiGP


def _problem(n, d, seed):
    X, y = orc.synth_problem(max(n, 3), d, seed=seed)
    return np.ascontiguousarray(X[:n]), np.ascontiguousarray(y[:n])


# ------------------------------------------------------------------ grad_contract_kernel: mi_gp_grad_contract_block
@pytest.mark.parametrize("kernel,d", gr.CONTRACT_CASES, ids=[gr.case_id(c) for c in gr.CONTRACT_CASES])
def test_grad_contract_every_instantiation_against_numpy(kernel, d):
    """test_gpu_blocks.test_grad_contract_block_slabs_against_numpy's method, one whole-matrix call per case: dyadic X and
    power-of-two length scales (r2 exact), a random symmetric W and a random alpha, reference 1/2 sum_lower (alpha_i alpha_j -
    W_ij) dK_ij/dtheta from oracle.dK_dtheta, bound 64 eps sum |terms| + TINY per parameter.  n = 130: three 64-row tiles, the
    last of 2 rows.  The length scales are powers of two near sqrt(d), so that r2 stays of order 1 at every d."""
    lib = _lib()
    kerns, ops = gr.split(kernel)
    nk, n = len(kerns), gr.CONTRACT_N
    rng = np.random.default_rng(1000 * d + nk)
    X = rng.integers(0, 64, (n, d)) / 64.0
    e0 = int(round(np.log2(np.sqrt(d))))
    theta = orc.pack_theta(2.0 ** rng.integers(e0 - 1, e0 + 1, (nk, d)), rng.uniform(0.5, 2.0, nk), 0.2, 1e-6,
                           alpha=rng.uniform(0.5, 3.0, nk))
    ntheta = nk * d + 2 * nk + 2
    Wm = rng.uniform(-1.0, 1.0, (n, n))
    Wm = 0.5 * (Wm + Wm.T)
    al = rng.uniform(-1.0, 1.0, n)
    M = np.outer(al, al) - Wm
    i, j = np.arange(n)[:, None], np.arange(n)[None, :]
    omega = np.where(i > j, 1.0, np.where(i == j, 0.5, 0.0))
    terms = (omega * M)[None] * orc.dK_dtheta(X, kerns, ops, theta)
    ref = terms.sum(axis=(1, 2))
    bound = 64 * EPS * np.abs(terms).sum(axis=(1, 2)) + TINY
    del terms
    ids, opv = _ids(kerns, ops)
    ldw = n + 6
    Wbuf = np.zeros((n, ldw))
    Wbuf[:, :n] = Wm
    npad = (n + 63) // 64 * 64
    tX, tth, tW, tal = _dev(X), _dev(theta), _dev(Wbuf), _dev(al)
    tg = _dev(np.full(ntheta, -77.5))
    tpart = _dev(np.zeros(max(lib.mi_gp_grad_contract_block_scratch(n, 0, npad, ntheta), 1)))
    r = lib.mi_gp_grad_contract_block(d, nk, ids, opv, tth.data_ptr(), tX.data_ptr(), n, tW.data_ptr(), ldw, 0, 0, npad,
                                      tal.data_ptr(), tpart.data_ptr(), tpart.numel(), tg.data_ptr(), None)
    assert r == 0, lib.mi_gp_last_global_error()
    got = _host(tg).copy()
    assert np.isfinite(got).all()
    ratio = np.abs(got - ref) / bound
    groups = {"ls": ratio[: nk * d], "kv": ratio[nk * d: nk * d + nk], "gv": ratio[-2:-1], "jitter": ratio[-1:]}
    rq = [c for c, k in enumerate(kerns) if k == "RatQuad"]
    if rq:
        groups["alpha"] = ratio[nk * d + nk + np.array(rq)]
    worst = {g: float(v.max()) for g, v in groups.items()}
    slot, col = gr.contract_entry(kernel)
    entry = f"<{gr.NK_SLOTS[slot]}, {'true' if col else 'false'}>"
    print(f"grad_contract_kernel{entry} {kernel} d={d}: worst error / bound per group {worst}")
    _record("grad_contract_kernel", entry, max(worst.values()), case=gr.case_id((kernel, d)), groups=worst)
    if nk >= 5:
        _record("grad_contract_kernel_counts", str(nk), max(worst.values()), case=gr.case_id((kernel, d)))
    for c, k in enumerate(kerns):
        if k != "RatQuad":
            assert got[nk * d + nk + c] == 0.0, (c, got[nk * d + nk + c])
    for g, v in groups.items():  # every parameter group by itself: length scales per component and dimension, kv, alpha, gv, jitter
        assert (v <= 1.0).all(), (g, int(np.argmax(v)), float(v.max()))
    assert got[-1] == got[-2]


# --------------------------------------------------------------------------------------- grad_x_kernel: the handle
@pytest.mark.parametrize("kernel,n,d", gr.GRAD_X_CASES, ids=[gr.case_id(c) for c in gr.GRAD_X_CASES])
def test_grad_x_every_instantiation_against_its_own_inverse(kernel, n, d):
    """dLML/dX of MiGP.lml_grad_data against sum_j (alpha_i alpha_j - Kinv_ij) dK_ij/dx_im formed on the host in np.longdouble
    from the DEVICE's K^-1 (the lower triangle of W_t; the strict upper triangle is scratch) and alpha = -gy: what the kernel
    itself read.  Per entry 64 eps sum |terms| + TINY, whatever cond(K).  K^-1 and alpha themselves are guarded end to end
    against the oracle at 1e-9 of the largest entry (cond < ~1e3 here); a second evaluation returns the same bits."""
    MiGP = _migp()
    kerns, ops = gr.split(kernel)
    X, y = _problem(n, d, seed=n + d)
    theta = gr.well_conditioned_theta(kernel, d)
    gp = MiGP(X, y, kernel)
    try:
        val, g, gy, gx = gp.lml_grad_data(theta)
        assert np.isfinite(val)
        low = gp.W_t[:n, :n].cpu().numpy()
        val2, g2, gy2, gx2 = gp.lml_grad_data(theta)
    finally:
        gp.close()
    assert _same_bits(gx, gx2) and _same_bits(gy, gy2) and _same_bits(g, g2) and val == val2
    assert np.isfinite(gx).all()
    Kinv = np.tril(low) + np.tril(low, -1).T
    ref, mag = gr.grad_x_reference(X, kernel, theta, Kinv, -gy)
    ratio = gr.max_ratio(gx, ref, gr.sum_bound(mag))
    slot, col = gr.grad_x_entry(kernel, d)
    entry = f"<{gr.NK_SLOTS[slot]}, {gr.GX_WINDOWS[col]}>"
    print(f"grad_x_kernel{entry} {kernel} n={n} d={d}: worst error / bound {ratio:.4f}")
    _record("grad_x_kernel", entry, ratio, case=gr.case_id((kernel, n, d)))
    if len(kerns) >= 5:
        _record("grad_x_kernel_counts", str(len(kerns)), ratio, case=gr.case_id((kernel, n, d)))
    assert ratio <= 1.0, ratio
    # K^-1 and alpha themselves, and the whole path, against the oracle
    _, gyo, gXo = orc.lml_grad_data(X, y, kerns, ops, theta)
    Ko = np.linalg.inv(orc.noisy_cov(X, kerns, ops, theta))
    assert np.abs(Kinv - Ko).max() <= 1e-9 * np.abs(Ko).max()
    assert np.abs(gy - gyo).max() <= 1e-9 * np.abs(gyo).max()
    assert np.abs(gx - gXo).max() <= 1e-9 * np.abs(gXo).max(), (np.abs(gx - gXo).max(), np.abs(gXo).max())


# -------------------------------------------------------------------------------------------- predict_grad_kernel
@pytest.mark.parametrize("kernel,n,d", gr.PREDICT_CASES, ids=[gr.case_id(c) for c in gr.PREDICT_CASES])
def test_predict_grad_every_instantiation_against_its_own_rows(kernel, n, d):
    """d var = -2 sum_i w_i dk_i/dx* from the DEVICE's w rows (rows mp + p of the work block, mp = ceil(m / 128) 128), and d mu
    = sum_i alpha_i dk_i/dx* with alpha from a host solve of the oracle's conditional-form covariance, both in np.longdouble:
    64 eps sum |terms| (+ 8 cond eps sum |terms| for alpha's own forward error, cond computed here) + TINY.  d var is asserted
    in every case; d mu where grad_refs.alpha_reference finds the oracle's alpha inside that allowance -- everywhere but where an
    Exponential component meets d > 1 -- and is printed and recorded otherwise.  Five queries: a
    training point (r2 = 0 exactly), a point 40 length scales away -- finite gradients, exactly 0 where every term is far
    below the subnormals -- and three in the cube."""
    MiGP = _migp()
    kerns, ops = gr.split(kernel)
    X, y = _problem(n, d, seed=7 * n + d)
    theta = gr.well_conditioned_theta(kernel, d)
    Xn = gr.predict_queries(X, theta, d, seed=n + d)
    m, mp_ = Xn.shape[0], 128
    gp = MiGP(X, y, kernel)
    try:
        mu, var, dmu, dvar = gp.predict_grad(theta, Xn)
        w = gp._work2[mp_: mp_ + m, :n].cpu().numpy()
        again = gp.predict_grad(theta, Xn)
    finally:
        gp.close()
    assert all(_same_bits(a, b) for a, b in zip((mu, var, dmu, dvar), again))
    assert np.isfinite(dmu).all() and np.isfinite(dvar).all() and np.isfinite(w).all()
    alpha, cond, alpha_ok, alpha_dev = gr.alpha_reference(X, y, kernel, theta, Xn)
    rv, magv = gr.predict_grad_reference(X, kernel, theta, Xn, -2.0 * w)
    rm, magm = gr.predict_grad_reference(X, kernel, theta, Xn, alpha)
    ratio_v = gr.max_ratio(dvar, rv, gr.sum_bound(magv))
    ratio_m = gr.max_ratio(dmu, rm, gr.sum_bound(magm, extra=8.0 * cond))
    per_point = [float(np.max(np.abs(dvar[p].astype(LD) - rv[p]) / gr.sum_bound(magv[p]))) for p in range(m)]
    slot = gr.predict_entry(kernel)[0]
    entry = f"<{gr.NK_SLOTS[slot]}>"
    print(f"predict_grad_kernel{entry} {kernel} n={n} d={d} cond={cond:.0f}: d var error / bound {ratio_v:.4f} "
          f"(per query {['%.3f' % v for v in per_point]}), d mu error / bound {ratio_m:.5f} "
          f"({'asserted' if alpha_ok else 'not asserted'}: the reference alpha's own diagonal residue is {alpha_dev:.4f} of its allowance)")
    worst = max(ratio_v, ratio_m) if alpha_ok else ratio_v
    _record("predict_grad_kernel", entry, worst, case=gr.case_id((kernel, n, d)), dvar=ratio_v, dmu=ratio_m, dmu_asserted=bool(alpha_ok),
            cond=cond)
    if len(kerns) >= 5:
        _record("predict_grad_kernel_counts", str(len(kerns)), worst, case=gr.case_id((kernel, n, d)))
    gone = LD(TINY) * LD(2.0) ** -64
    assert (dvar[magv < gone] == 0.0).all() and (dmu[magm < gone] == 0.0).all()
    assert ratio_v <= 1.0, (ratio_v, per_point)
    assert ratio_m <= 1.0 or not alpha_ok, ratio_m


# ------------------------------------------------------------------------------ derivative entries against mpmath
@pytest.mark.parametrize("name,kv,alpha,ls,xmax,c0,c1", ULP_CASES)
def test_kernel_derivative_entries_against_mpmath(name, kv, alpha, ls, xmax, c0, c1):
    """dk/dr2 of base_kernel_val_der element by element: one training point at 0 (y = 2), d = 1, a power-of-two length scale
    and the r2 grid of test_covariance_entries_against_mpmath as the query points (225 to ~1800) of ONE predict_grad call (r2 =
    x^2 / l^2 exactly).  Then d mu_p = alpha_0 kv k'(r2_p) 2 x_p / l^2 with alpha_0 = y / (kv k(0) + gv + jitter), and d var_p = -2 w_p
    (the same factor) with the device's own w_p: both in 40-digit mpmath, so that only k' is under test.  Bound: that test's
    (c0 + c1 |exp argument|) ulp with c0 + 4 for the seven further roundings between k' and the output (the noisy diagonal,
    its root, the two divisions behind alpha_0, kv k', the product with 2 (x* - x) / l^2 and with alpha_0: about half an ulp
    each), and its absolute floor of 4 subnormal ulps times everything that multiplies exp(-argument)."""
    import mpmath as mp

    mp.mp.dps = 40
    MiGP = _migp()
    x = _grid(xmax)
    m = x.size
    yv, gv, jit = 2.0, 0.1, 1e-6
    theta = orc.pack_theta([[ls]], [kv], gv, jit, alpha=[alpha])
    gp = MiGP(np.zeros((1, 1)), np.array([yv]), name)
    try:
        mu, var, dmu, dvar = gp.predict_grad(theta, x[:, None])
        mp_ = (m + 127) // 128 * 128
        w = gp._work2[mp_: mp_ + m, 0].cpu().numpy()
    finally:
        gp.close()
    assert np.isfinite(dmu).all() and np.isfinite(dvar).all()
    # (the prior diagonal is kv k(r2 = 0): 1 - O(1e-6) times kv for the families with the 1e-12 under the root)
    a0 = mp.mpf(yv) / (mp.mpf(float(kv)) * gr.k_truth(name, 0.0, alpha) + mp.mpf(gv) + mp.mpf(jit))
    worst = {}
    for what, got in (("dmu", dmu[:, 0]), ("dvar", dvar[:, 0])):
        ratio = np.empty(m)
        for p in range(m):
            dk, arg, pre = gr.dk_truth(name, (x[p] / ls) ** 2, alpha)
            f = mp.mpf(float(kv)) * 2 * mp.mpf(float(x[p])) / (mp.mpf(float(ls)) ** 2)
            f *= a0 if what == "dmu" else -2 * mp.mpf(float(w[p]))
            truth = float(f * dk)
            ulp = np.spacing(abs(truth))
            bound = max((c0 + 4.0 + c1 * float(arg)) * ulp, 4 * TINY * float(abs(f) * pre))
            ratio[p] = abs(got[p] - truth) / bound
        k = int(np.argmax(ratio))
        worst[what] = float(ratio[k])
        print(f"k' {name} kv={kv} alpha={alpha} ls={ls} {what}: worst error / bound {ratio[k]:.4f} at r2 = {(x[k] / ls) ** 2!r} "
              f"(got {got[k]!r})")
    _record("dk_dr2", f"{name} kv={kv} alpha={alpha} ls={ls}", max(worst.values()), **worst)
    assert worst["dmu"] <= 1.0 and worst["dvar"] <= 1.0, worst


@pytest.mark.parametrize("kv,alpha", [(1.0, 0.5), (1.7, 2.0), (1.0, 8.0)])
def test_ratquad_dalpha_against_mpmath(kv, alpha):
    """RatQuad's dk/dalpha = k (-log1p(u) + u / (1 + u)) through mi_gp_grad_contract_block: n = 2, X = [0, x], W = 0 and alpha_v
    = (1, 1), so the alpha slot is kv dk/dalpha(r2) alone (the diagonal's r2 = 0 term is exactly 0).  41 values of r2 = x^2
    from 2^-20 to 2^20, each exact.  Bound (8 + alpha) ulp of the truth plus 4 eps k (log1p(u) + u / (1 + u)) for the
    cancellation of the two terms at small u."""
    lib = _lib()
    xs = np.sort(np.concatenate([2.0 ** np.arange(-10, 11), 1.5 * 2.0 ** np.arange(-10, 10)]))
    assert xs.size == 41 and xs[0] ** 2 == 2.0 ** -20 and xs[-1] ** 2 == 2.0 ** 20
    ids, opv = _ids(["RatQuad"], [])
    theta = orc.pack_theta([[1.0]], [kv], 0.1, 1e-6, alpha=[alpha])
    tth, tW, tal = _dev(theta), _dev(np.zeros((2, 8))), _dev(np.ones(2))
    tpart = _dev(np.zeros(max(lib.mi_gp_grad_contract_block_scratch(2, 0, 64, 5), 1)))
    worst, at = 0.0, None
    for xv in xs:
        tX, tg = _dev(np.array([[0.0], [xv]])), _dev(np.full(5, -77.5))
        r = lib.mi_gp_grad_contract_block(1, 1, ids, opv, tth.data_ptr(), tX.data_ptr(), 2, tW.data_ptr(), 8, 0, 0, 64,
                                          tal.data_ptr(), tpart.data_ptr(), tpart.numel(), tg.data_ptr(), None)
        assert r == 0, lib.mi_gp_last_global_error()
        got = _host(tg)[2]
        t, big = gr.ratquad_dalpha_truth(xv * xv, alpha)
        truth = kv * float(t)
        bound = (8.0 + alpha) * np.spacing(abs(truth)) + 4 * EPS * kv * float(big)
        ratio = abs(got - truth) / bound
        if ratio >= worst:
            worst, at = float(ratio), (float(xv * xv), float(got), truth)
    print(f"RatQuad dk/dalpha kv={kv} alpha={alpha}: worst error / bound {worst:.4f} at (r2, got, truth) = {at}")
    _record("ratquad_dk_dalpha", f"kv={kv} alpha={alpha}", worst, r2=at[0])
    assert worst <= 1.0, (worst, at)
