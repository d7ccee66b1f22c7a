"""Every stage of the conditional, read out of the caller's work_dev / cov_dev after a C-ABI call and judged by the element-wise
backward-error statistics of tests/conditional_checks.py against exactly what the stage read: the K* rows (the upper half of
work after mi_gp_predict_u; mi_gp_assemble_block must return the same bits), L and beta from K_t, U from Z_t.  No bound depends
on cond(K); the forward-error tests (test_gpu_grad_predict.py, test_gpu_predict_joint.py, test_gpu_predict_posterior.py,
test_gpu_random_sweep.py) see the same stages only through their final numbers.  work_dev, cov_dev and the moment outputs are
filled with NaN before every call: a result that depends on unwritten scratch gives inf.

Entry points: mi_gp_predict (rho_A, rho_mean, rho_var), mi_gp_predict_u (rho_AU, rho_mean, rho_var), mi_gp_predict_grad (per-point
route at m = 1 and 16: rho_AU row-wise; blocked solve at m = 17 and 129: rho_A and the bits of mi_gp_predict; rho_w either way),
mi_gp_predict_cov + mi_gp_sample_cov (rho_A, rho_Sigma, the identity in the padding, rho_LSigma), mi_gp_predict_batch and
mi_gp_predict / _predict_u after mi_gp_append across a tile boundary.  Query counts m = 1, 16, 17, 127, 128, 129, 300, with and
without pred_noise; a row below is the worst over those (the statistic with the largest value / bound and its bound).

Bounds (conditional_checks): rho_A <= 2 np + 1; rho_AU, rho_w, rho_mean <= 2 np; rho_var, rho_Sigma <= 4; rho_LSigma <= 2 mp + 1.
test_conditional_checks_host.py shows that the algorithm itself, in plain fp64, stays a factor 4 under each of them on these
problems (N = 2600 aside), and that planted faults of one tile, one chunk or one term exceed them.

Measured on an MI355X (the -s output of this module; n is the padded size):

case                                         n | statistic worst value / bound (query count m, pred_noise pn) ...
------------------------------------------------------------------------------------------------------------------------
conditional-100 predict                    128 | rho_A 18.70 / 257 (m 300 pn 0) | rho_mean 0.92 / 256 (m 300 pn 0) | rho_var 0.01 / 4 (m 300 pn 1)
conditional-100 predict_u                  128 | rho_AU 1.04 / 256 (m 129 pn 0) | rho_mean 0.85 / 256 (m 128 pn 0) | rho_var 0.02 / 4 (m 129 pn 0)
conditional-100 predict_grad               128 | rho_AU 1.93 / 256 (m 16 pn 0) | rho_mean 0.74 / 256 (m 129 pn 0) | rho_var 0.01 / 4 (m 129 pn 0) | rho_w 7.37 / 256 (m 129 pn 0) | rho_A 18.70 / 257 (m 129 pn 0)
conditional-100 predict_cov + sample_cov   128 | rho_A 18.70 / 257 (m 300 pn 0) | rho_Sigma 0.02 / 4 (m 127 pn 0) | rho_LSigma 38.72 / 769 (m 300 pn 0)
conditional-300 predict                    384 | rho_A 18.74 / 769 (m 300 pn 0) | rho_mean 1.03 / 768 (m 128 pn 0) | rho_var 0.01 / 4 (m 300 pn 1)
conditional-300 predict_u                  384 | rho_AU 1.39 / 768 (m 129 pn 0) | rho_mean 0.74 / 768 (m 128 pn 0) | rho_var 0.01 / 4 (m 128 pn 0)
conditional-300 predict_grad               384 | rho_AU 3.07 / 768 (m 16 pn 0) | rho_mean 0.66 / 768 (m 129 pn 0) | rho_var 0.00 / 4 (m 129 pn 0) | rho_w 5.77 / 768 (m 17 pn 0) | rho_A 16.50 / 769 (m 129 pn 0)
conditional-300 predict_cov + sample_cov   384 | rho_A 18.74 / 769 (m 300 pn 0) | rho_Sigma 0.01 / 4 (m 300 pn 0) | rho_LSigma 7.02 / 257 (m 128 pn 0)
conditional-800 predict                    896 | rho_A 23.79 / 1793 (m 300 pn 0) | rho_mean 1.08 / 1792 (m 300 pn 0) | rho_var 0.00 / 4 (m 127 pn 0)
conditional-800 predict_u                  896 | rho_AU 0.00 / 1792 (m 1 pn 0) | rho_mean 1.04 / 1792 (m 129 pn 0) | rho_var 0.00 / 4 (m 128 pn 0)
conditional-800 predict_grad               896 | rho_AU 4.72 / 1792 (m 1 pn 0) | rho_mean 0.67 / 1792 (m 17 pn 0) | rho_var 0.00 / 4 (m 129 pn 1) | rho_w 11.37 / 1792 (m 129 pn 0) | rho_A 21.66 / 1793 (m 129 pn 0)
conditional-800 predict_cov + sample_cov   896 | rho_A 23.79 / 1793 (m 300 pn 0) | rho_Sigma 0.00 / 4 (m 16 pn 0) | rho_LSigma 5.40 / 257 (m 128 pn 1)
conditional-2600 predict                  2688 | rho_A 34.68 / 5377 (m 128 pn 0) | rho_mean 1.03 / 5376 (m 300 pn 0) | rho_var 0.00 / 4 (m 300 pn 0)
conditional-2600 predict_u                2688 | rho_AU 6.53 / 5376 (m 128 pn 0) | rho_mean 1.18 / 5376 (m 129 pn 0) | rho_var 0.00 / 4 (m 300 pn 1)
conditional-2600 predict_grad             2688 | rho_AU 5.95 / 5376 (m 16 pn 0) | rho_mean 0.92 / 5376 (m 129 pn 0) | rho_var 0.00 / 4 (m 129 pn 1) | rho_w 16.70 / 5376 (m 16 pn 0) | rho_A 29.94 / 5377 (m 129 pn 0)
conditional-2600 predict_cov + sample_cov  2688 | rho_A 34.68 / 5377 (m 128 pn 0) | rho_Sigma 0.01 / 4 (m 300 pn 0) | rho_LSigma 6.33 / 257 (m 127 pn 1)
ill-800 predict                            896 | rho_A 432.54 / 1793 (m 127 pn 0) | rho_mean 1.12 / 1792 (m 300 pn 0) | rho_var 0.00 / 4 (m 300 pn 0)
ill-800 predict_u                          896 | rho_AU 0.00 / 1792 (m 1 pn 0) | rho_mean 1.09 / 1792 (m 300 pn 0) | rho_var 0.00 / 4 (m 128 pn 0)
ill-800 predict_grad                       896 | rho_AU 4.66 / 1792 (m 16 pn 0) | rho_mean 0.92 / 1792 (m 17 pn 0) | rho_var 0.00 / 4 (m 129 pn 1) | rho_w 8.45 / 1792 (m 129 pn 0) | rho_A 404.77 / 1793 (m 129 pn 0)
ill-800 predict_cov + sample_cov           896 | rho_A 432.54 / 1793 (m 127 pn 0) | rho_Sigma 0.00 / 4 (m 1 pn 0) | rho_LSigma 4.85 / 257 (m 127 pn 0)
conditional-2600 m 12100                  2688 | rho_AU 0.00 / 5376 (predict_u) | rho_A 42.59 / 5377 (predict)
append-258 U extended                      384 | rho_A 41.68 / 769 (p m 17 pn 0) | rho_mean 0.78 / 768 (p m 129 pn 1) | rho_var 0.01 / 4 (u m 300 pn 0) | rho_AU 1.37 / 768 (u m 300 pn 0)
append-258 U formed after                  384 | rho_A 41.68 / 769 (p m 17 pn 0) | rho_mean 0.67 / 768 (u m 129 pn 1) | rho_var 0.01 / 4 (u m 129 pn 1) | rho_AU 1.37 / 768 (u m 300 pn 0)
factor-batch-800-0 predict_batch           896 | rho_A 20.72 / 1793 (m 300 pn 1) | rho_mean 1.04 / 1792 (m 300 pn 1) | rho_var 0.00 / 4 (m 300 pn 1)
factor-batch-800-1 predict_batch           896 | rho_A 25.09 / 1793 (m 128 pn 0) | rho_mean 1.67 / 1792 (m 300 pn 1) | rho_var 0.00 / 4 (m 300 pn 1)
factor-batch-800-2 predict_batch           896 | rho_A 21.57 / 1793 (m 300 pn 1) | rho_mean 1.02 / 1792 (m 17 pn 1) | rho_var 0.00 / 4 (m 128 pn 0)

(rho_AU = 0.00: the device's kmode-4 product and rocBLAS's K* triu(U) agree bit for bit there -- checked entry by entry on the
12100-point case, 32.5e6 entries; at m = 128 rocBLAS rounds differently and the statistic reads 1 to 7.  ill-800: rho_A 433 is the
product with the explicit leaf inverses at cond(K) 6e9, 224 in the host emulation, LAPACK's solve 3.)
"""
import functools

import numpy as np
import pytest

import conditional_checks as cc
import resident_checks as rc
from oracle import gp_oracle as orc
from test_gpu_blocks import EPS, _fold_sensitivity, _ids
from test_gpu_resident_matrices import DEV, _t, handle

pytestmark = pytest.mark.gpu

T = rc.TILE
FAR = 1 << 24   # column offset of mi_gp_assemble_block: no entry of the block is on the global diagonal
NAN = float("nan")
PROBLEMS = cc.WELL + [cc.ILL]


def _nan(*shape):
    import torch

    return torch.full(shape, NAN, dtype=torch.float64, device=DEV)


def _same_bits(a, b):
    import torch

    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)))


def assemble(p, theta_t, Xr_t, Xc_t, rows_pad, cols_pad):
    """K(Xr, Xc) of p's kernel at theta_t through mi_gp_assemble_block, zeros in the padding, no diagonal term."""
    import torch

    from andvaranaut_amd import _lib

    lib = _lib.load()
    kerns, ops = rc._kern(p.kernel)
    ids, opv = _ids(kerns, ops)
    out = _nan(rows_pad, cols_pad)
    torch.cuda.synchronize()
    r = lib.mi_gp_assemble_block(p.d, len(kerns), ids, opv, theta_t.data_ptr(), Xr_t.data_ptr(), Xr_t.shape[0], Xc_t.data_ptr(),
                                 Xc_t.shape[0], 0, FAR, out.data_ptr(), cols_pad, rows_pad, cols_pad, 0, None)
    assert r == 0, lib.mi_gp_last_global_error()
    torch.cuda.synchronize()
    return out


def call(gp, fn, Xn, pred_noise, halves, grad=False):
    """One conditional through the C-ABI on NaN-filled buffers: (work [halves * mp, lda], mean [m], var [m]) on the device."""
    import torch

    m = Xn.shape[0]
    mp = rc.padded(m)
    work, mu, var = _nan(halves * mp, gp.lda), _nan(m), _nan(m)
    xn = _t(Xn)
    args = [gp.h, xn.data_ptr(), m, work.data_ptr(), gp.lda, mu.data_ptr(), var.data_ptr(), 1 if pred_noise else 0]
    if grad:
        dmu, dvar = _nan(m, gp.d), _nan(m, gp.d)
        args += [dmu.data_ptr(), dvar.data_ptr()]
    torch.cuda.synchronize()
    r = getattr(gp.lib, fn)(*args)
    assert r == 0, (fn, r, gp.last_error())
    torch.cuda.synchronize()
    if grad:
        assert bool(torch.isfinite(dmu).all()) and bool(torch.isfinite(dvar).all()), (fn, m)
    return work, mu, var


class Resident:
    """What the conditional reads from one factorisation: L and beta out of a K buffer, U out of Z_t once it is resident."""

    def __init__(self, gp, p, Kbuf=None, points_of=None):
        self.gp, self.p, self.points_of = gp, p, points_of or p
        self.n, self.npad = gp.n, gp.np_
        self.nt = self.npad // T
        K = gp.K_t if Kbuf is None else Kbuf
        self.L = K[: self.npad, : self.npad].tril()
        self.beta = K[self.npad, : self.npad].clone()
        self.ops = rc._kern(p.kernel)[1]
        self.theta_t = _t(p.theta)
        self._ks = {}

    @property
    def U(self):
        return self.gp.Z_t[: self.npad, : self.npad]

    def points(self, m):
        return cc.query_points(self.points_of, m)

    def kstar(self, m):
        """The K* bits of the m query points (mp x np): mi_gp_assemble_block's, which the upper half of mi_gp_predict_u's work
        must repeat bit for bit (handles with U buffers)."""
        if m not in self._ks:
            Xn = self.points(m)
            mp = rc.padded(m)
            ks = assemble(self.p, self.theta_t, _t(Xn), self.gp.X_t, mp, self.npad)
            assert not bool(ks[m:].any()) and not bool(ks[:, self.n:].any()), "K* padding is not zero"
            if self.gp.Z_t is not None:
                work, _, _ = call(self.gp, "mi_gp_predict_u", Xn, 0, 2)
                assert _same_bits(work[mp:, : self.npad], ks), (self.p.name, m, "K* rows of mi_gp_predict_u != mi_gp_assemble_block")
            self._ks[m] = ks
        return self._ks[m]

    def moments(self, pred_noise):
        return cc.prior_diag_noise(self.p.theta, self.p.d, self.ops, pred_noise)


class Row:
    """The measured statistics of one case: per statistic the entry with the largest value / bound."""

    def __init__(self, label, res):
        self.label, self.res, self.got, self.bad = label, res, {}, []

    def add(self, key, value, bound, where, explain=None):
        if key not in self.got or not value / bound <= self.got[key][0] / self.got[key][1]:
            self.got[key] = (value, bound, where)
        if not value <= bound:
            self.bad.append((key, where, value, bound, explain() if explain else ""))

    def work_rows(self, key, stat, bound, where, *args):
        """A statistic over work rows: a failure names the worst tile and the branch of the solve's recursion behind it."""
        self.add(key, stat(*args), bound, where, lambda: cc.describe_solve(rc.worst_tile(stat, *args), self.res.nt))

    def moments(self, A, mu, var, m, pred_noise, where):
        r = self.res
        kd, noise = r.moments(pred_noise)
        beta = r.beta
        self.add("rho_mean", cc.rho_mean(A[:m], beta, mu, r.n), rc.bound_gemm(r.npad), where,
                 lambda: rc.describe(rc.worst_tile(cc.rho_mean, A[:m], beta, mu, r.n)))
        self.add("rho_var", cc.rho_var(A[:m], var, r.n, kd, noise), cc.BOUND_VAR, where,
                 lambda: rc.describe(rc.worst_tile(cc.rho_var, A[:m], var, r.n, kd, noise)))

    def close(self):
        text = f"CONDITIONAL {self.label:36s} n {self.res.npad:5d}"
        for key, (value, bound, where) in self.got.items():
            text += f" | {key} {value:8.2f} <= {bound} ({where})"
        print(text)
        assert not self.bad, (self.label, self.bad)


@pytest.fixture(scope="module", params=PROBLEMS, ids=[p.name for p in PROBLEMS])
def res(request):
    """One handle per problem, factored once, U resident (formed by mi_gp_predict_u)."""
    p = request.param
    gp, _ = handle(p)
    try:
        assert gp.factor(p.theta) == 0
        r = Resident(gp, p)
        r.kstar(1)
        yield r
    finally:
        gp.close()


CASES = [(m, pn) for m in cc.QUERY_COUNTS for pn in (0, 1)]


def check_predict(row, r, m, pn, where):
    mp = rc.padded(m)
    ks = r.kstar(m)
    work, mu, var = call(r.gp, "mi_gp_predict", r.points(m), pn, 1)
    A = work[:mp, : r.npad]
    row.work_rows("rho_A", cc.rho_A, rc.bound_L(r.npad), where, ks[:m], A[:m], r.L)
    row.moments(A, mu, var, m, pn, where)
    return A, mu, var


def check_predict_u(row, r, m, pn, where):
    mp = rc.padded(m)
    ks = r.kstar(m)
    work, mu, var = call(r.gp, "mi_gp_predict_u", r.points(m), pn, 2)
    A = work[:mp, : r.npad]
    assert _same_bits(work[mp:, : r.npad], ks), (where, "the K* rows changed between two calls")
    row.work_rows("rho_AU", cc.rho_AU, rc.bound_gemm(r.npad), where, ks[:m], A[:m], r.U)
    row.moments(A, mu, var, m, pn, where)
    return A, mu, var


# ------------------------------------------------------------------------------------------ the four single entry points
def test_predict_leaves_solved_rows_and_their_moments(res):
    row = Row(res.p.name + " predict", res)
    for m, pn in CASES:
        check_predict(row, res, m, pn, f"m {m} noise {pn}")
    row.close()


def test_predict_u_leaves_the_product_with_U_and_its_moments(res):
    row = Row(res.p.name + " predict_u", res)
    for m, pn in CASES:
        check_predict_u(row, res, m, pn, f"m {m} noise {pn}")
    row.close()


def test_predict_grad_rows_by_either_route_and_the_w_rows(res):
    """m <= 16: A_p = U^T k*_p row by row (columns < n: the kernel writes no others, the NaN beyond them stays) and the same bits
    from a second call; m > 16: the blocked solve, with the bits of mi_gp_predict in rows and moments.  w_p = U A_p in the upper
    half of work either way."""
    r = res
    row = Row(r.p.name + " predict_grad", r)
    for m in (1, 16, 17, 129):
        mp = rc.padded(m)
        ks = r.kstar(m)
        for pn in (0, 1):
            where = f"m {m} noise {pn}"
            work, mu, var = call(r.gp, "mi_gp_predict_grad", r.points(m), pn, 2, grad=True)
            A, w = work[:mp, : r.npad], work[mp:, : r.npad]
            if m <= 16:
                row.work_rows("rho_AU", cc.rho_AU, rc.bound_gemm(r.npad), where, ks[:m], A[:m], r.U, r.n)
                again = call(r.gp, "mi_gp_predict_grad", r.points(m), pn, 2, grad=True)
                assert _same_bits(again[0][:m, : r.n], A[:m, : r.n]) and _same_bits(again[1], mu) and _same_bits(again[2], var), where
            else:
                row.work_rows("rho_A", cc.rho_A, rc.bound_L(r.npad), where, ks[:m], A[:m], r.L)
                pwork, pmu, pvar = call(r.gp, "mi_gp_predict", r.points(m), pn, 1)
                assert _same_bits(pwork[:mp, : r.npad], A) and _same_bits(pmu, mu) and _same_bits(pvar, var), where
            row.moments(A, mu, var, m, pn, where)
            row.add("rho_w", cc.rho_w(r.U, A[:m], w[:m], r.n), rc.bound_gemm(r.npad), where,
                    lambda: rc.describe(rc.worst_tile(cc.rho_w, r.U, A[:m], w[:m], r.n)))
    row.close()


@functools.lru_cache(maxsize=4)
def _kss_reference(name, m):
    """(oracle K(X*, X*) in the full-matrix form, the element-wise tolerance of the assembly test)."""
    p = next(q for q in PROBLEMS if q.name == name)
    Xn = cc.query_points(p, m)
    kerns, ops = rc._kern(p.kernel)
    ref = orc.kernel_matrix(Xn, Xn, kerns, ops, p.theta)
    s_r2, s_val = _fold_sensitivity(kerns, ops, p.theta, Xn, Xn)
    return ref, 8.0 * EPS * (p.d + 4) * s_r2 + 8.0 * EPS * s_val + 4.0 * EPS * np.abs(ref)


def kss(r, m):
    """K** (mp x mp, no diagonal term) from mi_gp_assemble_block, held against the oracle."""
    xn = _t(r.points(m))
    K = assemble(r.p, r.theta_t, xn, xn, rc.padded(m), rc.padded(m))
    ref, bound = _kss_reference(r.p.name, m)
    err = np.abs(K[:m, :m].cpu().numpy() - ref)
    assert (err <= bound).all(), (r.p.name, m, "assembled K** against the oracle", float(np.max(err / bound)))
    return K


def test_predict_cov_leaves_rows_sigma_and_sample_cov_its_factor(res):
    import torch

    r = res
    gp = r.gp
    row = Row(r.p.name + " predict_cov + sample_cov", r)
    for m in cc.QUERY_COUNTS:
        mp = rc.padded(m)
        ks, Kss, Xn = r.kstar(m), kss(r, m), r.points(m)
        for pn in (0, 1):
            where = f"m {m} noise {pn}"
            work, mu, cov = _nan(mp, gp.lda), _nan(m), _nan(mp, mp)
            xn = _t(Xn)
            torch.cuda.synchronize()
            ret = gp.lib.mi_gp_predict_cov(gp.h, xn.data_ptr(), m, work.data_ptr(), gp.lda, mu.data_ptr(), cov.data_ptr(), mp, pn)
            assert ret == 0, gp.last_error()
            torch.cuda.synchronize()
            A = work[:, : r.npad]
            row.work_rows("rho_A", cc.rho_A, rc.bound_L(r.npad), where, ks[:m], A[:m], r.L)
            assert not bool(A[m:].any()), (where, "padding rows of A are not zero")
            shift = cc.shift_of(r.p, pn)
            row.add("rho_Sigma", cc.rho_Sigma(Kss, shift, A, cov, m), cc.BOUND_SIGMA, where,
                    lambda: rc.describe(rc.worst_tile(cc.rho_Sigma, Kss, shift, A, cov, m)))
            assert cc.sigma_padding_is_identity(cov, m), (where, "padding of Sigma is not the identity")
            sigma = cov.tril()   # (mi_gp_sample_cov overwrites Sigma with its factor)
            s = 3
            need = int(gp.lib.mi_gp_sample_cov_work(m, s))
            scratch, draws = _nan(need), _nan(s, m)
            torch.cuda.synchronize()
            ret = gp.lib.mi_gp_sample_cov(gp.h, cov.data_ptr(), mp, m, mu.data_ptr(), 0.0, s, 7, 0, draws.data_ptr(), m,
                                          scratch.data_ptr(), need)
            assert ret == 0, (where, ret, gp.last_error())
            torch.cuda.synchronize()
            assert bool(torch.isfinite(draws).all()), where
            row.add("rho_LSigma", cc.rho_LSigma(sigma, cov), rc.bound_L(mp), where,
                    lambda: rc.describe(rc.worst_tile(cc.rho_LSigma, sigma, cov)))
    row.close()


# ------------------------------------------------------------------------------------------ the 128x128-tile GEMM kernel
def test_many_points_put_the_updates_on_the_128_tile_kernel():
    """N = 2600, m = 12100: 95 row tiles x 21 tile columns.  The solve's first update (95 x 11 tiles) and the K* U product
    (95 x 21) have at least 1024 tiles and run on the 128x128-tile kernel; every case above stays on 64x64 tiles."""
    p = rc.CONDITIONAL[1]
    m = 12100
    gp, _ = handle(p)
    try:
        assert gp.factor(p.theta) == 0
        r = Resident(gp, p)
        assert rc.padded(m) // T * (r.nt - r.nt // 2) >= 1024
        row = Row(p.name + " m 12100", r)
        mp = rc.padded(m)
        ks = r.kstar(m)
        work, _, _ = call(gp, "mi_gp_predict_u", r.points(m), 1, 2)
        row.work_rows("rho_AU", cc.rho_AU, rc.bound_gemm(r.npad), "predict_u", ks[:m], work[:m, : r.npad], r.U)
        del work
        work, _, _ = call(gp, "mi_gp_predict", r.points(m), 1, 1)
        row.work_rows("rho_A", cc.rho_A, rc.bound_L(r.npad), "predict", ks[:m], work[:m, : r.npad], r.L)
        assert not bool(work[m:mp, : r.npad].any())
        row.close()
    finally:
        gp.close()


# ------------------------------------------------------------------------------------------ after an append
@pytest.mark.parametrize("with_u", [True, False], ids=["U-resident", "U-formed-after"])
def test_after_an_append_across_a_tile_boundary(with_u):
    """250 -> 258 points (np 256 -> 384): the conditional against the grown L, beta and U -- U extended in place by the append,
    or formed from the grown factor by the first mi_gp_predict_u behind it."""
    from andvaranaut_amd import MiGP

    stages = rc.APPEND
    p = stages[-1]
    X, y, _ = rc.problem_data(p)
    n0 = stages[0].N
    gp = MiGP(X[:n0], y[:n0], p.kernel, device=0, capacity=rc.APPEND_CAPACITY)
    try:
        assert gp.factor(p.theta) == 0
        if with_u:
            call(gp, "mi_gp_predict_u", cc.query_points(p, 3), 0, 2)
        assert gp.append(X[n0:], y[n0:]) == 0
        assert gp.n == p.N and gp.np_ == 384 and gp.append_refactors == 0
        r = Resident(gp, p)
        r.kstar(1)
        row = Row(p.name + (" U extended" if with_u else " U formed after"), r)
        for m, pn in ((1, 1), (17, 0), (129, 1), (300, 0)):
            check_predict(row, r, m, pn, f"predict m {m} noise {pn}")
            check_predict_u(row, r, m, pn, f"predict_u m {m} noise {pn}")
        row.close()
    finally:
        gp.close()


# ------------------------------------------------------------------------------------------ batch
def test_predict_batch_leaves_every_member_its_rows_and_moments():
    import torch

    ps = rc.BATCH_FACTOR
    gp, _ = handle(ps[0], need_grad=False)
    try:
        assert not gp.factor_batch(np.stack([p.theta for p in ps])).any()
        members = [Resident(gp, p, gp._bK[k], points_of=ps[0]) for k, p in enumerate(ps)]   # (one set of points per call)
        rows = [Row(p.name + " predict_batch", r) for p, r in zip(ps, members)]
        k = len(ps)
        for m, pn in ((1, 0), (17, 1), (128, 0), (129, 1), (300, 1)):
            mp = rc.padded(m)
            Xn = members[0].points(m)
            work, mu, var = _nan(k, mp, gp.lda), _nan(k, m), _nan(k, m)
            xn = _t(Xn)
            torch.cuda.synchronize()
            ret = gp.lib.mi_gp_predict_batch(gp.h, k, xn.data_ptr(), m, work.data_ptr(), gp.lda, mp * gp.lda, mu.data_ptr(),
                                             var.data_ptr(), pn, None, None)
            assert ret == 0, gp.last_error()
            torch.cuda.synchronize()
            for q, (r, row) in enumerate(zip(members, rows)):
                where = f"m {m} noise {pn}"
                A = work[q, :, : r.npad]
                row.work_rows("rho_A", cc.rho_A, rc.bound_L(r.npad), where, r.kstar(m)[:m], A[:m], r.L)
                row.moments(A, mu[q], var[q], m, pn, where)
        for row in rows:
            row.close()
    finally:
        gp.close()


# ------------------------------------------------------------------------------------------ the statistics' own eyes on the device
def test_the_statistics_see_a_planted_fault_on_the_device():
    """The torch products that pass a clean work block fail a copy with one 128 x 128 tile scaled by 1 + 1e-9, and name it."""
    p = cc.WELL[1]
    m = 300
    gp, _ = handle(p)
    try:
        assert gp.factor(p.theta) == 0
        r = Resident(gp, p)
        ks = r.kstar(m)[:m]
        A = call(gp, "mi_gp_predict", r.points(m), 1, 1)[0][:m, : r.npad]
        AU = call(gp, "mi_gp_predict_u", r.points(m), 1, 2)[0][:m, : r.npad]
        assert cc.rho_A(ks, A, r.L) <= rc.bound_L(r.npad) and cc.rho_AU(ks, AU, r.U) <= rc.bound_gemm(r.npad)
        for stat, rows, other, bound in ((cc.rho_A, A, r.L, rc.bound_L(r.npad)), (cc.rho_AU, AU, r.U, rc.bound_gemm(r.npad))):
            F = rows.clone()
            F[T:2 * T, :T] *= 1.0 + 1e-9
            w = rc.worst_tile(stat, ks, F, other)
            assert w.value >= 10 * bound and w.tile[0] == 1, (stat.__name__, cc.describe_solve(w, r.nt))
    finally:
        gp.close()
