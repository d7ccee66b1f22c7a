"""Batched evaluation member by member: every kernel of mi_gp_lml_batch / mi_gp_lml_grad_batch / mi_gp_factor_batch /
mi_gp_predict_batch finds its problem as blockIdx.z times a stride, so a launch that read problem 0's theta, or used a wrong
stride, would still be right for problem 0 -- and for every member that shares the affected parameter.  Here every member
differs from every other one in EVERY field of theta (each ls, kv, RatQuad alpha, gv, jitter), each member is checked against
the oracle and against the single entry points' bits (include/mi_gp.h: same arithmetic per element), and the batch is
evaluated again permuted.  Then: k changing across calls on one handle, non-positive-definite members at every position, the
per-point diagonal, caller strides with sentinels through the C-ABI, and one large batched gradient.

BATCH_SWEEP_RATIOS=<path> appends one JSON line per sweep case with the measured error / (cond eps) per quantity."""
import ctypes
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ["RBF", "Matern52", "Matern32", "Exponential"]
EPS = 2.2e-16
DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)


def _mods():
    import torch

    assert torch.cuda.is_available()
    from andvaranaut_amd import MiGP
    from oracle import gp_oracle as orc

    return MiGP, orc


def _kernel(kerns, ops):
    return kerns[0] + "".join(o + k for o, k in zip(ops, kerns[1:]))


def _split(kernel):
    return kernel.replace("*", "+").split("+"), [c for c in kernel if c in "+*"]


def _close_ratio(a, b):
    """max |a - b| / max(|b|, 1e-3 max |b|): per component, with the floor of test_gpu_random_sweep.py."""
    scale = np.maximum(np.abs(b), 1e-3 * max(np.max(np.abs(b)), 1e-300))
    return float(np.max(np.abs(a - b) / scale))


def _cond(orc, X, kerns, ops, theta, extra_diag=None):
    """2-norm condition number of the (symmetric positive-definite) noisy covariance."""
    w = np.linalg.eigvalsh(orc.noisy_cov(X, kerns, ops, theta, extra_diag=extra_diag))
    return float(w[-1] / w[0]) if w[0] > 0 else np.inf


def _draw_thetas(orc, rng, d, kerns, K, gv_jitter=True):
    """K thetas that differ from one another in every field: each ls, kv, alpha, gv and jitter drawn per member."""
    nk = len(kerns)
    out = []
    for _ in range(K):
        th = orc.synth_theta(d, nkern=nk)
        th[: nk * d] *= rng.uniform(0.7, 1.6, nk * d) * (np.sqrt(d / 2.0) if d > 32 else 1.0)
        th[nk * d: nk * d + nk] = rng.uniform(0.5, 2.0, nk)
        th[nk * d + nk: nk * d + 2 * nk] = rng.uniform(0.5, 3.0, nk)  # (alpha: read by RatQuad only)
        th[-2] = 10.0 ** rng.uniform(-5, -2) if gv_jitter else 0.0
        th[-1] = 10.0 ** rng.uniform(-7, -5) if gv_jitter else 0.0
        out.append(th)
    th = np.array(out)
    if K > 1:  # no two members share any entry that the kernels read
        for j in range(th.shape[1]):
            assert len(np.unique(th[:, j])) == K or not gv_jitter and j >= th.shape[1] - 2
    return th


def _random_case(rng):
    if rng.random() < 0.15:
        kerns, ops = ["RatQuad"], []  # the reference supports RatQuad only on its own (gpmcmc.py:287)
    else:
        nk = int(rng.integers(1, 9))
        kerns = [NAMES[int(rng.integers(0, 4))] for _ in range(nk)]
        ops = [("+", "*")[int(rng.integers(0, 2))] for _ in range(nk - 1)]
    if rng.random() < 0.25:  # one off a 128-row tile boundary
        N = 128 * int(rng.integers(1, 11)) + int(rng.choice([-1, 1]))
    else:
        N = int(rng.choice([int(rng.integers(1, 128)), int(rng.integers(128, 401)), int(rng.integers(400, 1301))]))
    if rng.random() < 0.1:
        d = int(rng.integers(129, 201))
    else:
        d = int(rng.choice([int(rng.integers(1, 4)), int(rng.integers(4, 33)), int(rng.integers(33, 71))]))
    K = int(rng.integers(1, 13))
    # keep the oracle gradients cheap (their cost is ~ nk d N^2 per member): fewer components, then fewer dimensions
    while len(kerns) * d * N * N > 1.5e8 and len(kerns) > 1:
        kerns, ops = kerns[:-1], ops[:-1]
    while d * N * N > 1.5e8 and d > 1:
        d = max(1, d // 2)
    return N, d, kerns, ops, K, int(rng.integers(1, 300))


def _singles(gp, th, Xn=None):
    """The single entry points' results per member: lml, (lml, grad) of lml_grad, and factor + predict (blocked solve) with
    and without the predictive noise."""
    out = []
    for t in th:
        r = {"lml": gp.lml(t), "info": gp.info}
        r["v"], r["g"] = gp.lml_grad(t)
        if Xn is not None:
            r["pred"] = gp.predict(t, Xn, pred_noise=True, via_inverse=False)
            r["pred0"] = gp.predict(t, Xn, pred_noise=False, via_inverse=False)
        out.append(r)
    return out


def _batch_all(gp, th, Xn):
    vals = gp.lml_batch(th)
    info = gp.batch_info.copy()
    v2, grads = gp.lml_grad_batch(th)
    assert np.array_equal(vals, v2), (vals, v2)  # lml_batch == lml_grad_batch's values, bit for bit
    assert np.array_equal(gp.batch_info, info)
    mu, var = gp.predict_batch(th, Xn, pred_noise=True, mixture=False)
    mu0, var0 = gp.predict_batch(th, Xn, pred_noise=False, mixture=False)
    return vals, grads, mu, var, mu0, var0


# ---------------------------------------------------------------------------------------------------------- (a) sweep
@pytest.mark.parametrize("seed", range(int(os.environ.get("SWEEP_SEEDS_BATCH", "16"))))
def test_batch_sweep_every_member(seed):
    MiGP, orc = _mods()
    rng = np.random.default_rng(7000 + seed)
    N, d, kerns, ops, K, M = _random_case(rng)
    kernel = _kernel(kerns, ops)
    X, y = orc.synth_problem(max(N, 3), d, seed=100 + seed)
    X, y = X[:N], y[:N]
    th = _draw_thetas(orc, rng, d, kerns, K)
    Xn = rng.random((M, d))
    expo = "Exponential" in kerns
    gp = MiGP(X, y, kernel)
    vals, grads, mu, var, mu0, var0 = _batch_all(gp, th, Xn)
    assert np.all(gp.batch_info == 0), gp.batch_info
    case = (kernel, N, d, K, M)
    rec = {"seed": seed, "kernel": kernel, "N": N, "d": d, "K": K, "M": M, "lml": 0.0, "grad": 0.0, "mean": 0.0, "var": 0.0}
    for p, s in enumerate(_singles(gp, th, Xn)):
        # the single entry points' bits
        assert s["info"] == 0 and s["lml"] == vals[p] and s["v"] == vals[p], (case, p, s["lml"], vals[p])
        assert np.array_equal(s["g"], grads[p]), (case, p, s["g"], grads[p])
        assert np.array_equal(s["pred"][0], mu[p]) and np.array_equal(s["pred"][1], var[p]), (case, p)
        assert np.array_equal(s["pred0"][0], mu0[p]) and np.array_equal(s["pred0"][1], var0[p]), (case, p)
        # the oracle, with the cond-scaled tolerances of test_gpu_random_sweep.py (reasoning there)
        cond = _cond(orc, X, kerns, ops, th[p])
        ref, gref = orc.lml_grad(X, y, kerns, ops, th[p])
        tol = max(1e-8 if expo else 1e-10, 20.0 * cond * EPS)
        gtol = max(1e-5 if expo else 1e-7, 500.0 * cond * EPS)
        e_l = abs(vals[p] - ref) / max(abs(ref), 1.0)
        e_g = _close_ratio(grads[p], gref)
        assert e_l <= tol, (case, p, vals[p], ref, cond)
        assert e_g <= gtol, (case, p, grads[p], gref, cond)
        rmu, rvar = orc.predict(X, y, Xn, kerns, ops, th[p])
        ctol = max(1e-8, 200.0 * cond * EPS)  # (the conditional form has the same diagonal: jitter + sqrt(gv)^2)
        assert np.allclose(mu[p], rmu, rtol=ctol, atol=ctol), (case, p)
        assert np.allclose(var[p], rvar, rtol=10 * ctol, atol=max(1e-10, ctol * 1e-2)), (case, p)
        rec["lml"] = max(rec["lml"], e_l / (cond * EPS))
        rec["grad"] = max(rec["grad"], e_g / (cond * EPS))
        rec["mean"] = max(rec["mean"], float(np.max(np.abs(mu[p] - rmu) / np.maximum(np.abs(rmu), 1.0))) / (cond * EPS))
        rec["var"] = max(rec["var"], float(np.max(np.abs(var[p] - rvar) / np.maximum(np.abs(rvar), 1e-2))) / (cond * EPS))
    # permuted batches: every output is the original's, permuted, bit for bit (nothing depends on the problem index)
    for perm in (np.arange(K)[::-1], np.roll(np.arange(K), 1)):
        pv, pg, pmu, pvar, pmu0, pvar0 = _batch_all(gp, th[perm], Xn)
        assert np.array_equal(pv, vals[perm]) and np.array_equal(pg, grads[perm]), (case, perm)
        assert np.array_equal(pmu, mu[perm]) and np.array_equal(pvar, var[perm]), (case, perm)
        assert np.array_equal(pmu0, mu0[perm]) and np.array_equal(pvar0, var0[perm]), (case, perm)
    gp.close()
    if os.environ.get("BATCH_SWEEP_RATIOS"):
        with open(os.environ["BATCH_SWEEP_RATIOS"], "a") as f:
            f.write(json.dumps(rec) + "\n")


# ------------------------------------------------------------------------------------------------- (b) shape across calls
def test_batch_size_changes_across_calls_on_one_handle():
    """The BatchedEvaluator pattern: chains leave and k drops below the buffers' count, the buffers grow at 12 -- each call
    of lml_batch / lml_grad_batch / factor_batch (+ predict_batch) returns the single entry points' bits."""
    MiGP, orc = _mods()
    N, d, kernel = 333, 4, "Matern32*RBF+Exponential"
    kerns, ops = _split(kernel)
    X, y = orc.synth_problem(N, d, seed=21)
    rng = np.random.default_rng(21)
    th = _draw_thetas(orc, rng, d, kerns, 12)
    Xn = rng.random((37, d))
    gp = MiGP(X, y, kernel)
    ref = _singles(gp, th, Xn)
    calls = ["lml", "grad", "factor"]
    for i, k in enumerate([8, 3, 8, 1, 5, 12, 2]):
        sel = np.roll(np.arange(12), -i)[:k]  # (a different subset of the members each time)
        what = calls[i % 3]
        if what == "lml":
            vals = gp.lml_batch(th[sel])
            assert all(vals[j] == ref[p]["lml"] for j, p in enumerate(sel)), (k, what)
        elif what == "grad":
            vals, grads = gp.lml_grad_batch(th[sel])
            assert all(vals[j] == ref[p]["v"] and np.array_equal(grads[j], ref[p]["g"]) for j, p in enumerate(sel)), (k, what)
        else:
            mu, var = gp.predict_batch(th[sel], Xn, mixture=False)
            assert all(np.array_equal(mu[j], ref[p]["pred"][0]) and np.array_equal(var[j], ref[p]["pred"][1])
                       for j, p in enumerate(sel)), (k, what)
        assert np.all(gp.batch_info == 0)
    gp.close()


def test_batch_of_many_problems_at_small_n():
    MiGP, orc = _mods()
    N, d, kernel = 45, 3, "RBF+Matern52"
    kerns, ops = _split(kernel)
    X, y = orc.synth_problem(N, d, seed=45)
    rng = np.random.default_rng(45)
    th = _draw_thetas(orc, rng, d, kerns, 21)
    Xn = rng.random((19, d))
    gp = MiGP(X, y, kernel)
    vals, grads, mu, var, _, _ = _batch_all(gp, th, Xn)
    for p, s in enumerate(_singles(gp, th, Xn)):
        assert s["v"] == vals[p] and np.array_equal(s["g"], grads[p]), p
        assert np.array_equal(s["pred"][0], mu[p]) and np.array_equal(s["pred"][1], var[p]), p
        cond = _cond(orc, X, kerns, ops, th[p])
        ref, gref = orc.lml_grad(X, y, kerns, ops, th[p])
        assert abs(vals[p] - ref) <= max(1e-10, 20.0 * cond * EPS) * max(abs(ref), 1.0), (p, vals[p], ref)
        assert _close_ratio(grads[p], gref) <= max(1e-7, 500.0 * cond * EPS), (p, grads[p], gref)
    gp.close()


# ---------------------------------------------------------------------------------------- (c) non-positive-definite members
@pytest.mark.parametrize("bad", [[0], [2], [4], [0, 1, 2, 3, 4]])
def test_non_positive_definite_member_at_every_position(bad):
    MiGP, orc = _mods()
    N, d, kernel = 260, 3, "Matern52"
    X, y = orc.synth_problem(N, d, seed=3)
    rng = np.random.default_rng(len(bad) * 10 + bad[0])
    th = _draw_thetas(orc, rng, d, ["Matern52"], 5)
    Xn = rng.random((50, d))
    gp = MiGP(X, y, kernel)
    good_v, good_g = gp.lml_grad_batch(th)
    _, _, good_mix_m, good_mix_v = gp.predict_batch(th, Xn)
    tb = th.copy()
    for j, p in enumerate(bad):
        # negative jitter: fails at the first pivot, or (-0.3 kv) only further down the factorisation
        tb[p, -1] = -10.0 if j % 2 == 0 else -0.3 * tb[p, d]
    single_info = []
    for p in bad:
        assert gp.lml(tb[p]) == -np.inf
        single_info.append(gp.info)
        assert gp.factor(tb[p]) == single_info[-1]
    assert all(i > 0 for i in single_info)
    ok = [p for p in range(5) if p not in bad]
    vals = gp.lml_batch(tb)
    assert [gp.batch_info[p] for p in bad] == single_info and all(gp.batch_info[p] == 0 for p in ok)
    v2, grads = gp.lml_grad_batch(tb)
    assert np.array_equal(vals, v2)
    assert [gp.batch_info[p] for p in bad] == single_info
    for p in bad:
        assert vals[p] == -np.inf and np.all(grads[p] == 0.0) and not np.any(np.signbit(grads[p])), (p, grads[p])
    # the other members: the bits of the same batch without the bad ones
    assert np.array_equal(vals[ok], good_v[ok]) and np.array_equal(grads[ok], good_g[ok])
    mu, var, mix_m, mix_v = gp.predict_batch(tb, Xn)
    assert [gp.batch_info[p] for p in bad] == single_info
    assert np.all(np.isnan(mu[bad])) and np.all(np.isnan(var[bad]))
    if ok:
        gmu, gvar, ref_m, ref_v = gp.predict_batch(th[ok], Xn)
        assert np.array_equal(mu[ok], gmu) and np.array_equal(var[ok], gvar)
        assert np.array_equal(mix_m, ref_m) and np.array_equal(mix_v, ref_v)  # the mixture leaves the bad members out
        assert not np.array_equal(mix_m, good_mix_m) or not np.array_equal(mix_v, good_mix_v)
    else:
        assert np.all(np.isnan(mix_m)) and np.all(np.isnan(mix_v))
    gp.close()


# --------------------------------------------------------------------------------------------------- (d) per-point diagonal
@pytest.mark.parametrize("N,d,kernel,noise", [(300, 3, "Matern52", False), (300, 3, "Matern52", True),
                                              (201, 2, "RBF*Matern32", True), (129, 4, "RatQuad", False)])
def test_batch_with_a_per_point_diagonal(N, d, kernel, noise):
    MiGP, orc = _mods()
    kerns, ops = _split(kernel)
    X, y = orc.synth_problem(N, d, seed=N + d)
    rng = np.random.default_rng(N)
    th = _draw_thetas(orc, rng, d, kerns, 4, gv_jitter=noise)
    v = 10.0 ** rng.uniform(-4, -2, N)
    Xn = rng.random((20, d))
    gp = MiGP(X, y, kernel)
    th_plain = th.copy()
    if not noise:  # (gv = jitter = 0 without the diagonal leaves K numerically singular: that pass gets some noise)
        th_plain[:, -2] = 1e-3
    plain_v, plain_g = gp.lml_grad_batch(th_plain)
    gp.set_diag(v)
    vals = gp.lml_batch(th)
    v2, grads = gp.lml_grad_batch(th)
    assert np.array_equal(vals, v2) and np.all(gp.batch_info == 0)
    mu, var = gp.predict_batch(th, Xn, mixture=False)
    for p, s in enumerate(_singles(gp, th, Xn)):
        assert s["lml"] == vals[p] and s["v"] == vals[p] and np.array_equal(s["g"], grads[p]), p
        assert np.array_equal(s["pred"][0], mu[p]) and np.array_equal(s["pred"][1], var[p]), p
        cond = _cond(orc, X, kerns, ops, th[p], extra_diag=v)
        ref, gref = orc.lml_grad(X, y, kerns, ops, th[p], extra_diag=v)
        assert abs(vals[p] - ref) <= max(1e-10, 20.0 * cond * EPS) * max(abs(ref), 1.0), (p, vals[p], ref)
        assert _close_ratio(grads[p], gref) <= max(1e-7, 500.0 * cond * EPS), (p, grads[p], gref)
    gp.set_diag(None)
    pv, pg = gp.lml_grad_batch(th_plain)
    assert np.array_equal(pv, plain_v) and np.array_equal(pg, plain_g)
    gp.close()


# ---------------------------------------------------------------------------------------- (e) caller strides, C-ABI errors
SENTINEL = 0x7FF8DEAD0000BEEF  # a NaN with a payload


def _sentinel_buffer(torch, dev, n):
    return torch.full((n,), SENTINEL, dtype=torch.int64, device=dev)


def _outside(total, stride, used, count):
    """Mask of the elements of a strided buffer outside every problem's slice (the gaps and the tail)."""
    m = np.ones(total, dtype=bool)
    for p in range(count):
        m[p * stride: p * stride + used] = False
    return m


@pytest.mark.parametrize("N,d,kernel,K", [(301, 5, "Matern32+RBF", 3), (129, 2, "Exponential", 4), (77, 3, "RatQuad", 2)])
def test_caller_strides_through_the_c_abi(N, d, kernel, K):
    import torch

    from andvaranaut_amd import _lib

    MiGP, orc = _mods()
    kerns, ops = _split(kernel)
    X, y = orc.synth_problem(N, d, seed=N)
    rng = np.random.default_rng(N + 1)
    th = np.ascontiguousarray(_draw_thetas(orc, rng, d, kerns, K))
    m = 45
    Xn = rng.random((m, d))
    ref = MiGP(X, y, kernel)  # the facade's packed buffers
    rv, rg = ref.lml_grad_batch(th)
    rmu, rvar, rmm, rmv = ref.predict_batch(th, Xn)
    ref.close()

    gp = MiGP(X, y, kernel)
    lib, h, lda, np_, dev = gp.lib, gp.h, gp.lda, gp.np_, gp.dev
    need_k, need_z = (np_ + 128) * lda, np_ * lda
    sk, sz = need_k + 4 * lda, need_z + 2 * lda  # even gaps of a few rows
    Kb = _sentinel_buffer(torch, dev, K * sk)
    Zb = _sentinel_buffer(torch, dev, K * sz)
    Wb = _sentinel_buffer(torch, dev, K * sz)
    mp = (m + 127) // 128 * 128
    sw = mp * lda + 6 * lda
    work = _sentinel_buffer(torch, dev, K * sw)
    outs = _sentinel_buffer(torch, dev, 2 * K * m + 2 * m + 64)
    torch.cuda.synchronize(dev)
    b = _lib.MiGpBatchBuffers()
    b.K_dev, b.Z_dev, b.W_dev, b.stride_k, b.stride_zw, b.count = Kb.data_ptr(), Zb.data_ptr(), Wb.data_ptr(), sk, sz, K
    assert lib.mi_gp_set_batch(h, ctypes.byref(b)) == 0
    out, grads, info = np.empty(K), np.empty((K, gp.ntheta)), np.zeros(K, dtype=np.int32)
    assert lib.mi_gp_lml_grad_batch(h, K, th.ctypes.data_as(DP), out.ctypes.data_as(DP), grads.ctypes.data_as(DP),
                                    info.ctypes.data_as(IP)) == 0
    assert np.all(info == 0) and np.array_equal(out, rv) and np.array_equal(grads, rg)
    out2 = np.empty(K)
    assert lib.mi_gp_lml_batch(h, K, th.ctypes.data_as(DP), out2.ctypes.data_as(DP), None) == 0
    assert np.array_equal(out2, rv)
    assert lib.mi_gp_factor_batch(h, K, th.ctypes.data_as(DP), info.ctypes.data_as(IP)) == 0 and np.all(info == 0)
    xn = torch.from_numpy(Xn).to(dev)
    o = outs.view(torch.float64)
    base = o.data_ptr()
    torch.cuda.synchronize(dev)
    assert lib.mi_gp_predict_batch(h, K, xn.data_ptr(), m, work.data_ptr(), lda, sw, base, base + 8 * K * m, 1,
                                   base + 8 * 2 * K * m, base + 8 * (2 * K * m + m)) == 0, lib.mi_gp_last_error(h)
    oh = o.cpu().numpy()
    assert np.array_equal(oh[: K * m].reshape(K, m), rmu) and np.array_equal(oh[K * m: 2 * K * m].reshape(K, m), rvar)
    assert np.array_equal(oh[2 * K * m: 2 * K * m + m], rmm) and np.array_equal(oh[2 * K * m + m: 2 * K * m + 2 * m], rmv)
    # every sentinel outside the problems' slices is untouched
    for buf, stride, used in ((Kb, sk, need_k), (Zb, sz, need_z), (Wb, sz, need_z), (work, sw, mp * lda)):
        host = buf.cpu().numpy()
        assert np.all(host[_outside(host.size, stride, used, K)] == SENTINEL)
    assert np.all(outs.cpu().numpy()[2 * K * m + 2 * m:] == SENTINEL)

    def err():
        return lib.mi_gp_last_error(h).decode()

    # the -1 returns of mi_gp_set_batch / batch_internal / mi_gp_predict_batch, each with its text
    for bad_sk, bad_sz in ((need_k + 1, sz), (need_k - 2, sz), (sk, need_z + 1), (sk, need_z - 2)):
        bb = _lib.MiGpBatchBuffers()
        bb.K_dev, bb.Z_dev, bb.W_dev, bb.stride_k, bb.stride_zw, bb.count = Kb.data_ptr(), Zb.data_ptr(), Wb.data_ptr(), bad_sk, bad_sz, K
        assert lib.mi_gp_set_batch(h, ctypes.byref(bb)) == -1
        assert "strides must be even" in err() and str(need_k) in err()
    bb = _lib.MiGpBatchBuffers()
    bb.K_dev, bb.Z_dev, bb.W_dev, bb.stride_k, bb.stride_zw, bb.count = Kb.data_ptr(), Zb.data_ptr(), Wb.data_ptr(), sk, sz, 0
    assert lib.mi_gp_set_batch(h, ctypes.byref(bb)) == -1 and "count >= 1" in err()
    # (the refused calls left the good binding in place)
    assert lib.mi_gp_lml_batch(h, K, th.ctypes.data_as(DP), out2.ctypes.data_as(DP), None) == 0 and np.array_equal(out2, rv)
    big = np.ascontiguousarray(np.concatenate([th, th[:1]]))
    assert lib.mi_gp_lml_batch(h, K + 1, big.ctypes.data_as(DP), np.empty(K + 1).ctypes.data_as(DP), None) == -1
    assert err() == f"batch of {K + 1} problems, buffers for {K}"
    assert lib.mi_gp_lml_batch(h, 0, th.ctypes.data_as(DP), out2.ctypes.data_as(DP), None) == -1
    assert err() == f"batch of 0 problems, buffers for {K}"
    nan_th = th.copy()
    nan_th[K - 1, 1] = np.inf
    assert lib.mi_gp_lml_batch(h, K, nan_th.ctypes.data_as(DP), out2.ctypes.data_as(DP), None) == -1
    assert err() == f"theta[1] of problem {K - 1} is not finite"
    nan_th[K - 1, 1], nan_th[0, gp.ntheta - 1] = th[K - 1, 1], np.nan
    assert lib.mi_gp_lml_grad_batch(h, K, nan_th.ctypes.data_as(DP), out2.ctypes.data_as(DP), grads.ctypes.data_as(DP), None) == -1
    assert err() == f"theta[{gp.ntheta - 1}] of problem 0 is not finite"
    # predict_batch needs mi_gp_factor_batch with the same k as the last batch call
    assert lib.mi_gp_predict_batch(h, K, xn.data_ptr(), m, work.data_ptr(), lda, sw, base, base + 8 * K * m, 1, None, None) == -1
    assert err() == "mi_gp_predict_batch: mi_gp_factor_batch must be the last batch call"
    if K > 1:
        assert lib.mi_gp_factor_batch(h, K - 1, th.ctypes.data_as(DP), None) == 0
        assert lib.mi_gp_predict_batch(h, K, xn.data_ptr(), m, work.data_ptr(), lda, sw, base, base + 8 * K * m, 1, None, None) == -1
        assert err() == f"mi_gp_predict_batch: {K} problems, the last mi_gp_factor_batch factorised {K - 1}"
    # without Z / W: the LML batch runs (same bits), the gradient batch is refused
    bb.count, bb.Z_dev, bb.W_dev = K, None, None
    assert lib.mi_gp_set_batch(h, ctypes.byref(bb)) == 0
    assert lib.mi_gp_lml_batch(h, K, th.ctypes.data_as(DP), out2.ctypes.data_as(DP), None) == 0 and np.array_equal(out2, rv)
    assert lib.mi_gp_lml_grad_batch(h, K, th.ctypes.data_as(DP), out2.ctypes.data_as(DP), grads.ctypes.data_as(DP), None) == -1
    assert err() == "mi_gp_lml_grad_batch needs Z_dev and W_dev in mi_gp_set_batch"
    torch.cuda.synchronize(dev)
    host = Kb.cpu().numpy()
    assert np.all(host[_outside(host.size, sk, need_k, K)] == SENTINEL)
    gp.close()


# ------------------------------------------------------------------------------------------- (f) one large batched gradient
def test_large_batched_gradient_matches_the_singles():
    """N = 8320: 65 tile columns (a ragged last one past 64) in lockstep for two members that differ in every field."""
    MiGP, orc = _mods()
    N, d, kernel = 8320, 4, "Matern52+RBF"
    kerns, ops = _split(kernel)
    X, y = orc.synth_problem(N, d, seed=83)
    th = _draw_thetas(orc, np.random.default_rng(83), d, kerns, 2)
    th[:, -2] = [3e-3, 1.1e-2]  # (moderate noise: the 1e-10 bound is well inside cond eps at this size)
    gp = MiGP(X, y, kernel)
    vals, grads = gp.lml_grad_batch(th)
    assert np.all(gp.batch_info == 0)
    for p in range(2):
        v, g = gp.lml_grad(th[p])
        assert v == vals[p] and np.array_equal(g, grads[p]), p
        ref = orc.lml(X, y, kerns, ops, th[p])
        assert abs(vals[p] - ref) <= 1e-10 * abs(ref), (p, vals[p], ref)
    gp.close()
