"""The cases of tests/test_gpu_bad_pivot.py against LAPACK, without the device: the index the device has to report is what
scipy.linalg.lapack.dpotrf reports for the oracle's covariance of the same inputs (tests/bad_pivot_cases.py holds the cases).

Construction (a), the planted per-point diagonal -- checked NUMERICALLY for every position (at the library's default options) of
every size up to bad_pivot_cases.HOST_NUMERIC_MAX_N = 2400 points (1 .. 19 tile columns), and for the good problem (v = 0:
info 0) at those sizes; for the sizes above (3072 .. 10300) by the ARGUMENT in bad_pivot_cases's docstring: the leading p x p block
is the good problem's, pivot p + 1 is at most -(kd + gv + jitter) in real arithmetic.  That argument does not depend on the size,
and the device asserts info = 0 for the good problem at every size itself.
Construction (b), the repeated point under negative noise -- checked numerically for EVERY case (batch and sharded driver):
dpotrf reports p + 1, every earlier pivot >= 1e-3 kv, the failing Schur complement <= -1e-3 kv."""
import numpy as np
import pytest
from scipy.linalg import lapack, solve_triangular

import bad_pivot_cases as C
from oracle import gp_oracle as orc


def _info(K):
    _, info = lapack.dpotrf(K, lower=1, clean=0, overwrite_a=0)
    return int(info)


@pytest.mark.parametrize("n", [n for n in C.SINGLE_SIZES if n <= C.HOST_NUMERIC_MAX_N])
def test_planted_diagonal_fails_at_its_row(n):
    X, _ = C.problem(n)
    for which in (0, 1):
        theta = C.good_theta(which)
        K = orc.noisy_cov(X, C.KERNS, C.OPS, theta)
        assert _info(K) == 0
        pos = C.positions(n, C.DEFAULT_OPTIONS)
        assert pos and max(pos.values()) == n - 1
        for name, p in pos.items():
            v = C.planted_diag(n, p, theta)
            Kv = orc.noisy_cov(X, C.KERNS, C.OPS, theta, extra_diag=v)
            assert np.array_equal(Kv[:p, :p], K[:p, :p])  # the leading block is the good problem's
            assert Kv[p, p] <= -(C.prior_variance(theta)) < 0
            assert _info(Kv) == p + 1, (n, name, p)


def test_planted_diagonal_form():
    """v[p] = -2 (kd + gv + jitter) and nothing else, for any theta: the diagonal entry becomes -(kd + gv + jitter)."""
    for which in (0, 1):
        th = C.good_theta(which)
        v = C.planted_diag(300, 17, th)
        assert np.count_nonzero(v) == 1 and v[17] == -2.0 * (th[C.D] + th[-2] + th[-1])
    assert not np.array_equal(C.good_theta(0), C.good_theta(1))
    differs = C.good_theta(0) != C.good_theta(1)
    assert differs[: C.D + 1].all() and differs[-2:].all()  # (every field Matern52 reads: ls, kv, gv, jitter)


@pytest.mark.parametrize("n,p,q", C.repeated_point_cases())
def test_repeated_point_fails_at_its_row(n, p, q):
    X, _ = C.repeated_point_problem(n, p, q)
    theta = C.bad_theta(n)
    kv = C.BAD_KV
    K = orc.noisy_cov(X[: p + 1], C.KERNS, C.OPS, theta)  # (the index is a matter of the leading (p + 1) x (p + 1) block alone)
    assert _info(K) == p + 1
    c, info = lapack.dpotrf(K[:p, :p], lower=1, clean=1)
    assert info == 0
    piv = np.diag(c) ** 2
    assert piv.min() >= 1e-3 * kv, piv.min()
    w = solve_triangular(c, K[:p, p], lower=True)
    schur = K[p, p] - w @ w
    assert schur <= -1e-3 * kv, schur
    # room: the conditions hold with a factor of 30 and more
    assert piv.min() >= 0.03 * kv and schur <= -0.03 * kv, (piv.min(), schur)


def test_kv_scales_the_pivots_exactly():
    """The batch's second bad member uses kv / 2: K + jitter I scales by a power of two, bit for bit, and with it every pivot."""
    n, p, q = C.BATCH_CASES[0]
    X, _ = C.repeated_point_problem(n, p, q)
    K1 = orc.noisy_cov(X, C.KERNS, C.OPS, C.bad_theta(n))
    K2 = orc.noisy_cov(X, C.KERNS, C.OPS, C.bad_theta(n, kv=C.BAD_KV / 2))
    assert np.array_equal(K1, 2.0 * K2)
    assert _info(K1) == _info(K2) == p + 1


def test_minus_ten_fails_at_the_first_pivot():
    th = C.minus_ten_theta()
    assert C.prior_variance(th) + th[-2] + th[-1] < 0
    n, p, q = C.BATCH_CASES[0]
    X, _ = C.repeated_point_problem(n, p, q)
    assert _info(orc.noisy_cov(X, C.KERNS, C.OPS, th)) == 1


def test_good_members_factorise_on_repeated_point_data():
    """The batch's good members see the repeated point too: K + (gv + jitter) I stays positive definite (checked where cheap)."""
    for n, p, q in C.BATCH_CASES[:2]:
        X, _ = C.repeated_point_problem(n, p, q)
        for which in (0, 1):
            assert _info(orc.noisy_cov(X, C.KERNS, C.OPS, C.good_theta(which))) == 0


def test_schedule_model_at_the_defaults():
    """The model of the schedule at the library's default options: what include/mi_gp.h says about options 0, 20, 30, 35, 37, 46."""
    o = C.DEFAULT_OPTIONS
    for ntc in (1, 3):
        s = C.schedule(ntc, o)
        assert not s["two"] and s["tail"] == 0 and not s["panels"]
    for ntc in (4, 7, 8, 19, 24, 31):
        s = C.schedule(ntc, o)
        assert s["two"] and s["tail"] == 0 and not s["panels"]
    for ntc in (32, 33, 40, 52):
        s = C.schedule(ntc, o)
        assert s["two"] and s["panels"] and all(w <= 4 for _, w, _, _ in s["panels"])
        assert ntc - s["tail"] <= o[37] and any(e for _, _, e, _ in s["panels"])
    s = C.schedule(81, o)
    assert s["early"] and [q[0] for q in s["panels"] if q[3]] == [8] and s["tail"] == 64
    assert sum(w for _, w, _, _ in s["panels"]) == s["tail"]
    assert not C.schedule(79, o)["panels"][1][3]
    # every size of the device module covers row 0, its last row, and only rows inside the problem
    for n in C.SINGLE_SIZES:
        pos = C.positions(n, o)
        assert all(0 <= p < n for p in pos.values()) and len(set(pos.values())) == len(pos)
    assert sum(n % 128 != 0 for n in C.SINGLE_SIZES) * 2 >= len(C.SINGLE_SIZES)
