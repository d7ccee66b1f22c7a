"""The statistics of tests/conditional_checks.py on the host, before they judge the device (test_gpu_conditional_checks.py).

Problems: the conditional form at N = 100, 300 and 800 (conditional_checks.WELL without its N = 2600) and the ill-conditioned
ill-800 (RBF, d = 2, length scales 1.5, kv 1.7, gv = jitter = 1e-7; cond(K) 6e9, predictive variances ~1e-7), m = 300 query points.

(a) room: the emulation of the device's algorithm in plain fp64 -- resident_checks.emulate_factor and emulate_U, then
    emulate_solve / emulate_AU / wave_reduce / emulate_Sigma here -- stays a factor 4 under every bound, and so does a LAPACK
    solve from the same L.
(b) planted faults, each at least 10 x over its bound with worst_tile naming the tile: a tile of A scaled by 1 + 1e-9, a tile
    column of the kmode-4 k range left out of A = K* U, a 16-entry chunk left out of a mean, the noise left out of a variance, a
    tile of A A^T left out of Sigma, a non-zero in a padding column of A, a 16-deep chunk left out of one update of the solve.

Measured (printed by the tests with -s):
conditional-100  n  128 cond 1.2e+06 | rho_A 25.92 (LAPACK 3.06) <= 257 / 4 | rho_AU 0.00, rho_w 2.38, rho_mean 0.86 <= 256 / 4 | rho_var 0.01, rho_Sigma 0.08 <= 4 / 4 | rho_LSigma 91.46 <= 769 / 4
conditional-300  n  384 cond 2.5e+06 | rho_A 22.15 (LAPACK 3.55) <= 769 / 4 | rho_AU 0.00, rho_w 3.30, rho_mean 0.75 <= 768 / 4 | rho_var 0.00, rho_Sigma 0.03 <= 4 / 4 | rho_LSigma 16.26 <= 769 / 4
conditional-800  n  896 cond 4.0e+06 | rho_A 28.47 (LAPACK 3.28) <= 1793 / 4 | rho_AU 4.77, rho_w 8.20, rho_mean 1.40 <= 1792 / 4 | rho_var 0.00, rho_Sigma 0.02 <= 4 / 4 | rho_LSigma 31.12 <= 769 / 4
ill-800          n  896 cond 6.3e+09 | rho_A 224.06 (LAPACK 2.69) <= 1793 / 4 | rho_AU 3.23, rho_w 7.82, rho_mean 1.63 <= 1792 / 4 | rho_var 0.00, rho_Sigma 0.01 <= 4 / 4 | rho_LSigma 9.97 <= 769 / 4
(rho_mean, rho_var and rho_Sigma: the largest over the rows of the emulated solve, of LAPACK's solve and of K* U.)
conditional-300 fault A tile (1, 0) x (1 + 1e-9): rho_A 4.5e+06
conditional-300 fault A tile (2, 0) x (1 + 1e-9): rho_A 4.5e+06
conditional-300 fault A tile (0, 1) x (1 + 1e-9): rho_A 1.06e+05
conditional-100 fault noise left out: rho_var 1.31e+09
ill-800 fault A tile (1, 0) x (1 + 1e-9): rho_A 4.5e+06; tile (1, 6): 224 (clean 224, bound 1793); smallest fault seen in tile column 0: 1e-12
conditional-800 fault A tile (1, 0) x (1 + 1e-9): rho_A 4.5e+06
conditional-800 fault A tile (2, 0) x (1 + 1e-9): rho_A 4.5e+06
conditional-800 fault A tile (0, 5) x (1 + 1e-9): rho_A 3.51e+04
conditional-300 fault noise left out: rho_var 8.81e+08
conditional-800 fault noise left out: rho_var 3.31e+08
ill-800 fault noise left out: rho_var 3.31e+05

What the statistics cannot see, measured and not asserted: on ill-800 the entries of A grow along the row (|A| |L|^T is
dominated by the late columns), so a (1 + 1e-9) scaling of a tile in a LATE tile column stays under eps |A||L|^T.  There the
fault is planted in tile column 0, and test_smallest_visible_fault_on_the_ill_conditioned_problem records the smallest relative
fault rho_A still sees there."""
import numpy as np
import pytest
import scipy.linalg as sla

import conditional_checks as cc
import resident_checks as rc

T = rc.TILE
M = 300
HOST = cc.WELL[:3] + [cc.ILL]
BY_NAME = {p.name: p for p in HOST}
WELL_NAMES = [p.name for p in cc.WELL[:3]]
MULTI_TILE = WELL_NAMES[1:]


class Emulation:
    def __init__(self, p):
        self.p = p
        K, y = rc.problem_cov(p)
        self.Kaug = rc.pad_problem(K, y)
        self.N, self.n = p.N, self.Kaug.shape[1]
        self.nt = self.n // T
        self.Laug, self.invs = rc.emulate_factor(self.Kaug)
        self.L, self.beta = self.Laug[: self.n], self.Laug[self.n]
        self.U = rc.emulate_U(self.L, self.invs)
        self.Xn = cc.query_points(p, M)
        self.Ks, self.Kss = cc.problem_cross(p, self.Xn)
        self.A = cc.emulate_solve(self.L, self.invs, self.Ks)
        self.A_lapack = sla.solve_triangular(self.L, self.Ks.T, lower=True, check_finite=False).T
        self.AU = cc.emulate_AU(self.Ks, self.U)
        self.W = self.A @ np.triu(self.U).T
        self.ops = rc._kern(p.kernel)[1]
        self.cond = np.linalg.cond(K) if p.N <= 800 else float("nan")

    def moments(self, A, pred_noise, skip=None):
        kd, noise = cc.prior_diag_noise(self.p.theta, self.p.d, self.ops, pred_noise)
        mean, var = cc.wave_reduce(A, self.beta, self.N, kd, noise, skip)
        return mean, var, kd, noise


@pytest.fixture(scope="module")
def emu(request):
    return Emulation(BY_NAME[request.param])


def on(names):
    return pytest.mark.parametrize("emu", list(names), indirect=True)


# ------------------------------------------------------------------------------------------ the helpers themselves
def test_torch_and_numpy_agree():
    import torch

    e = Emulation(cc.WELL[1])
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))  # noqa: E731
    mean, var, kd, noise = e.moments(e.A, 1)
    S = cc.emulate_Sigma(e.Kss, 1e-4, e.A, M)
    Ls = np.linalg.cholesky(S + np.tril(S, -1).T)
    cases = ((cc.rho_A, (e.Ks, e.A, e.L)), (cc.rho_AU, (e.Ks, e.AU, e.U)), (cc.rho_AU, (e.Ks, e.AU, e.U, e.N)),
             (cc.rho_w, (e.U, e.A, e.W, e.N)), (cc.rho_mean, (e.A, e.beta, mean, e.N)), (cc.rho_LSigma, (S, Ls)))
    for stat, args in cases:
        a, b = stat(*args), stat(*[t(x) if isinstance(x, np.ndarray) else x for x in args])
        assert np.isfinite(a) and abs(a - b) <= 4.0, (stat.__name__, a, b)
    a = cc.rho_Sigma(e.Kss, 1e-4, e.A, S, M)
    b = cc.rho_Sigma(t(e.Kss), 1e-4, t(e.A), t(S), M)
    assert np.isfinite(a) and abs(a - b) <= 1.0
    assert cc.rho_var(e.A, var, e.N, kd, noise) == cc.rho_var(t(e.A), t(var), e.N, kd, noise)


def test_prior_diag_noise_follows_the_fold():
    th = np.array([1.0] * 6 + [1.2, 0.5, 3.0] + [1.0] * 3 + [0.3, 1e-6])
    assert cc.prior_diag_noise(th, 2, ["+", "*"], 1) == ((1.2 + 0.5) * 3.0, np.sqrt(0.3) * np.sqrt(0.3))
    assert cc.prior_diag_noise(th, 2, ["*", "+"], 0) == (1.2 * 0.5 + 3.0, 0.0)


def test_solve_branch_and_uneven_halving():
    assert cc.solve_branch(7, 4) == [(0, 7), (3, 4), (3, 2), (4, 1)]
    assert cc.solve_branch(21, 20) == [(0, 21), (10, 11), (15, 6), (18, 3), (19, 2), (20, 1)]
    assert cc.solve_branch(1, 0) == [(0, 1)]


def test_sigma_padding_rule():
    S = np.tril(np.eye(256))
    S[:130, :130] = 0.5
    assert cc.sigma_padding_is_identity(S, 130)
    for i, j, v in ((200, 3, 1e-300), (255, 255, 1.0 + rc.EPS), (131, 130, -0.0), (140, 140, np.nan)):
        F = S.copy()
        F[i, j] = v
        assert not cc.sigma_padding_is_identity(F, 130), (i, j)


# ------------------------------------------------------------------------------------------ (a) room under every bound
@on(BY_NAME)
def test_clean_emulation_has_room(emu):
    e = emu
    n = e.n
    got = {"rho_A": cc.rho_A(e.Ks, e.A, e.L), "rho_A LAPACK": cc.rho_A(e.Ks, e.A_lapack, e.L),
           "rho_AU": cc.rho_AU(e.Ks, e.AU, e.U), "rho_w": cc.rho_w(e.U, e.A, e.W, e.N)}
    bounds = {"rho_A": rc.bound_L(n), "rho_A LAPACK": rc.bound_L(n), "rho_AU": rc.bound_gemm(n), "rho_w": rc.bound_gemm(n)}
    for name, A in (("", e.A), (" LAPACK", e.A_lapack), (" via U", e.AU)):
        for pn in (0, 1):
            mean, var, kd, noise = e.moments(A, pn)
            got["rho_mean" + name] = max(got.get("rho_mean" + name, 0.0), cc.rho_mean(A, e.beta, mean, e.N))
            got["rho_var" + name] = max(got.get("rho_var" + name, 0.0), cc.rho_var(A, var, e.N, kd, noise))
            bounds["rho_mean" + name], bounds["rho_var" + name] = rc.bound_gemm(n), cc.BOUND_VAR
            shift = cc.shift_of(e.p, pn)
            S = cc.emulate_Sigma(e.Kss, shift, A, M)
            got["rho_Sigma" + name] = max(got.get("rho_Sigma" + name, 0.0), cc.rho_Sigma(e.Kss, shift, A, S, M))
            bounds["rho_Sigma" + name] = cc.BOUND_SIGMA
            assert cc.sigma_padding_is_identity(S, M)
            if not name:
                Laug, _ = rc.emulate_factor(np.vstack([S + np.tril(S, -1).T, np.zeros((1, S.shape[0]))]))
                got["rho_LSigma"] = max(got.get("rho_LSigma", 0.0), cc.rho_LSigma(S, Laug[:-1]))
                bounds["rho_LSigma"] = rc.bound_L(S.shape[0])
    print(f"HOST {e.p.name} n {n} cond {e.cond:.1e} | " + " | ".join(f"{k} {got[k]:.2f} <= {bounds[k]} / 4" for k in got))
    over = {k: (got[k], bounds[k] / 4) for k in got if not got[k] <= bounds[k] / 4}
    assert not over, over


# ------------------------------------------------------------------------------------------ (b) planted faults
@on(MULTI_TILE)
def test_fault_A_tile_scaled(emu):
    """One 128 x 128 tile of A times (1 + 1e-9), in tile column 0 and in the last row tile of the last column but one."""
    e = emu
    for ti, tj in ((1, 0), (M // T, 0), (0, e.nt - 2)):
        F = e.A.copy()
        F[ti * T:(ti + 1) * T, tj * T:(tj + 1) * T] *= 1.0 + 1e-9
        w = rc.worst_tile(cc.rho_A, e.Ks, F, e.L)
        assert w.value >= 10 * rc.bound_L(e.n), (ti, tj, w.value)
        assert w.tile[0] == ti and w.tile[1] >= tj, (ti, tj, cc.describe_solve(w, e.nt))  # (column tj of A enters columns >= tj of A L^T)
        print(f"HOST {e.p.name} fault A tile ({ti}, {tj}) x (1 + 1e-9): rho_A {w.value:.3g}")


@on(MULTI_TILE)
def test_fault_solve_update_drops_a_chunk(emu):
    """One update of the recursion leaves out 16 values of k: the node that joins the two halves, and the last uneven one."""
    e = emu
    nodes = [(c0, w) for c0, w in cc.solve_branch(e.nt, e.nt - 1) if w > 1]
    for c0, w in (nodes[0], nodes[-1]):
        F = cc.emulate_solve(e.L, e.invs, e.Ks, skip_update=(c0, w, 32, 48))
        wt = rc.worst_tile(cc.rho_A, e.Ks, F, e.L)
        assert wt.value >= 10 * rc.bound_L(e.n), (c0, w, wt.value)
        assert c0 + w // 2 <= wt.tile[1] < c0 + w, (c0, w, cc.describe_solve(wt, e.nt))  # (the columns the update writes)


@on(MULTI_TILE)
def test_fault_AU_tile_column_of_the_k_range_left_out(emu):
    e = emu
    for tj, tk in ((e.nt - 1, 0), (e.nt - 1, e.nt - 1), (1, 1)):
        F = cc.emulate_AU(e.Ks, e.U, skip=(tj, tk))
        w = rc.worst_tile(cc.rho_AU, e.Ks, F, e.U)
        assert w.value >= 10 * rc.bound_gemm(e.n) and w.tile[1] == tj, (tj, tk, rc.describe(w))
        assert rc.worst_tile(cc.rho_AU, e.Ks, F, e.U, e.N).tile[1] == tj


@on(WELL_NAMES)
def test_fault_mean_chunk_left_out(emu):
    """The 16 entries of A_p . beta that carry most, left out of one row's mean."""
    e = emu
    row = 129
    mean, _, _, _ = e.moments(e.A, 1)
    assert cc.rho_mean(e.A, e.beta, mean, e.N) <= rc.bound_gemm(e.n) / 4
    terms = np.abs(e.A[row, : e.N] * e.beta[: e.N])
    k0 = 16 * int(np.argmax(terms[: e.N // 16 * 16].reshape(-1, 16).sum(axis=1)))
    mean, _, _, _ = e.moments(e.A, 1, skip=(row, k0, k0 + 16))
    w = rc.worst_tile(cc.rho_mean, e.A, e.beta, mean, e.N)
    assert w.value >= 10 * rc.bound_gemm(e.n) and w.tile == (row // T, 0), rc.describe(w)


@on(WELL_NAMES + ["ill-800"])
def test_fault_noise_left_out_of_a_variance(emu):
    e = emu
    mean, var, kd, noise = e.moments(e.A, 1)
    _, var0, _, _ = e.moments(e.A, 0)
    assert noise > 0
    F = var.copy()
    F[257] = var0[257]
    w = rc.worst_tile(cc.rho_var, e.A, F, e.N, kd, noise)
    assert w.value >= 10 * cc.BOUND_VAR and w.tile == (2, 0), rc.describe(w)
    print(f"HOST {e.p.name} fault noise left out: rho_var {w.value:.3g}")


@on(WELL_NAMES + ["ill-800"])
def test_fault_Sigma_tile_of_AAT_left_out(emu):
    e = emu
    shift = cc.shift_of(e.p, 0)
    for ti, tj, tk in ((2, 1, e.nt - 1), (1, 1, 0), (2, 0, e.nt // 2)):
        S = cc.emulate_Sigma(e.Kss, shift, e.A, M, skip=(ti, tj, tk))
        w = rc.worst_tile(cc.rho_Sigma, e.Kss, shift, e.A, S, M)
        assert w.value >= 10 * cc.BOUND_SIGMA and w.tile == (ti, tj), (ti, tj, tk, rc.describe(w))


@on(["conditional-300"])
def test_fault_in_a_padding_column_of_A(emu):
    """1e-300 where an exact zero belongs: the entry is its own denominator (L is the identity there), ratio 1 / eps."""
    e = emu
    assert e.N < e.n - 2 and not e.A[:, e.N:].any()
    for i, j in ((0, e.N), (M - 1, e.n - 1)):
        F = e.A.copy()
        F[i, j] = 1e-300
        w = rc.worst_tile(cc.rho_A, e.Ks, F, e.L)
        assert w.value >= 0.25 / rc.EPS and w.tile == (i // T, j // T)
        assert cc.rho_AU(e.Ks, F, e.U) == np.inf  # (|K*| |U| is 0 there)
    F = e.A.copy()
    F[5, 7] = np.nan
    assert cc.rho_A(e.Ks, F, e.L) == np.inf


@on(["ill-800"])
def test_smallest_visible_fault_on_the_ill_conditioned_problem(emu):
    """Tile (1, 0) of A times (1 + f): the late tile column moves nothing at 1e-9 (recorded), tile column 0 is seen at 1e-9;
    the smallest f of 1e-9, 1e-10, ... that still exceeds the bound is printed."""
    e = emu
    bound = rc.bound_L(e.n)

    def faulty(tj, f):
        F = e.A.copy()
        F[T:2 * T, tj * T:(tj + 1) * T] *= 1.0 + f
        return rc.worst_tile(cc.rho_A, e.Ks, F, e.L)

    w = faulty(0, 1e-9)
    assert w.value >= 10 * bound and w.tile[0] == 1, rc.describe(w)
    late = faulty(e.nt - 1, 1e-9).value
    seen = [f for f in 10.0 ** -np.arange(9, 17) if faulty(0, f).value > bound]
    print(f"HOST ill-800 fault A tile (1, 0) x (1 + 1e-9): rho_A {w.value:.3g}; tile (1, {e.nt - 1}): {late:.3g} (clean "
          f"{cc.rho_A(e.Ks, e.A, e.L):.3g}, bound {bound}); smallest fault seen in tile column 0: {min(seen):.0e}")
