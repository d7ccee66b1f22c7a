"""The backward-error statistics of tests/resident_checks.py on the host, before they judge the device (test_gpu_resident_matrices.py):

(a) room: the NumPy emulation of the device's algorithm, in plain fp64, stays a factor 4 under every bound on each problem the
    GPU module evaluates -- rho_L <= (2n + 1) / 4, both U statistics <= 4 max(1, rho_ref) -- so that a bound the device misses
    is the device's doing and not the algorithm's.  Measured: rho_L 4 to 98 (LAPACK 3 to 11) against (2n + 1) / 4 = 64 to 2112;
    the U statistics 0.5 to 5.0 against LAPACK's 0.5 to 5.6; the ill-conditioned inputs are N = 1600 RBF gv 1e-8 (cond 1.2e9,
    rho_L 98) and N = 800 RatQuad gv 1e-6 (cond 4.0e8, rho_L 32).
(b) planted faults: each one, planted into the emulation's output, pushes its statistic over the bound the GPU module uses.

What the statistics cannot see, measured here and not asserted: a fault that is small against eps |A||B| of its element.  A
(1 + 1e-9) scaling of a tile of L in a LATE tile column moves L L^T by little of |L||L^T| (the early columns carry K): rho_L
171 at N = 4100, tile (32, 31), under the bound of 8449 -- in tile column 0 the same fault gives 9e6 at every size, and that
is the one asserted.  1e-12 under the diagonal of U sits below eps |U||U^T| where U is large: rho_W 122 to 1170 at the
ill-conditioned N = 800 and 1600 (bounds 1792, 3328), 1e3 to 5e11 at N = 300 and 2600, where it is asserted."""
import numpy as np
import pytest

import resident_checks as rc

T = rc.TILE
BY_NAME = {p.name: p for p in rc.all_problems()}


class Emulation:
    """One problem through the emulation; U, K^-1 and the LAPACK inverse are formed on first use."""

    def __init__(self, p):
        self.p = p
        K, y = rc.problem_cov(p)
        self.Kaug = rc.pad_problem(K, y)
        self.n = self.Kaug.shape[1]
        self.nt = self.n // T
        self.Laug, self.invs = rc.emulate_factor(self.Kaug)
        self.L = self.Laug[: self.n]
        self._U = self._W = self._ref = None

    @property
    def U(self):
        if self._U is None:
            self._U = rc.emulate_U(self.L, self.invs)
        return self._U

    @property
    def W(self):
        if self._W is None:
            self._W = rc.emulate_W(self.U)
        return self._W

    @property
    def ref(self):
        """(rho_ref left, rho_ref right) of X_ref = LAPACK's inverse of the emulated L."""
        if self._ref is None:
            Ur = rc.reference_inverse(self.L).T
            self._ref = rc.rho_U_left(self.L, Ur), rc.rho_U_right(self.L, Ur)
        return self._ref

    def tile(self, A, i, j):
        return A[i * T:(i + 1) * T, j * T:(j + 1) * T]


@pytest.fixture(scope="module")
def emu(request):
    return Emulation(BY_NAME[request.param])


def on(names):
    """The module-scoped emulation of each named problem (pytest builds each once and runs its tests together)."""
    return pytest.mark.parametrize("emu", list(names), indirect=True)


ALL = [p.name for p in rc.all_problems()]
MULTI_TILE = [p.name for p in rc.SINGLE[1:]]              # every single-evaluation size with an off-diagonal tile
FAULT_SIZES = [p.name for p in rc.SINGLE[1:5]]            # N = 300, 800, 1600, 2600
WELL_CONDITIONED = ["single-300", "single-2600"]          # gv = 1e-4


# ------------------------------------------------------------------------------------------ the statistics themselves
def test_ratio_rule():
    import torch

    num = np.array([0.0, 0.0, 1e-300, 3.0 * rc.EPS, np.nan, 1.0, -0.0])
    den = np.array([0.0, 2.0, 0.0, 1.5, 1.0, np.nan, 0.0])
    want = np.array([0.0, 0.0, np.inf, 2.0, np.inf, np.inf, 0.0])
    assert np.array_equal(rc.ratio(num, den), want)
    assert np.array_equal(rc.ratio(torch.from_numpy(num), torch.from_numpy(den)).numpy(), want)


def test_torch_and_numpy_agree():
    """The same statistics through torch (what the GPU module runs) and NumPy, on a problem with padding."""
    import torch

    e = Emulation(rc.SINGLE[1])
    t = torch.from_numpy
    beta = e.Laug[e.n]
    alpha = e.U @ beta
    for stat, args in ((rc.rho_L, (e.Kaug, e.Laug)), (rc.rho_U_left, (e.L, e.U)), (rc.rho_U_right, (e.L, e.U)),
                       (rc.rho_W, (e.U, e.W)), (rc.rho_alpha, (e.U, beta, alpha))):
        a, b = stat(*args), stat(*[t(np.ascontiguousarray(x)) for x in args])
        # (two BLAS calls of one product may round differently: the statistics agree to a few units, not to the bit)
        assert np.isfinite(a) and abs(a - b) <= 4.0, (stat.__name__, a, b)
        wa, wb = rc.worst_tile(stat, *args), rc.worst_tile(stat, *[t(np.ascontiguousarray(x)) for x in args])
        assert wa.tiles.shape == wb.tiles.shape and abs(wa.value - a) == 0.0 and abs(wb.value - b) == 0.0


def test_worst_tile_names_the_tile():
    e = Emulation(rc.SINGLE[1])
    F = e.W.copy()
    e.tile(F, 2, 1)[5, 7] *= 1.0 + 1e-6
    w = rc.worst_tile(rc.rho_W, e.U, F)
    assert w.tile == (2, 1) and w.value == rc.rho_W(e.U, F) and w.tiles.shape == (e.nt, e.nt)
    assert rc.worst_tile(rc.rho_L, e.Kaug, e.Laug).tiles.shape == (e.nt + 1, e.nt)  # (the beta row is a tile row of its own)
    assert "row 2, column 1" in rc.describe(w)


def test_doubling_nodes_cover_every_off_diagonal_tile_once():
    for nt in (1, 2, 3, 7, 13, 21, 27, 33):
        full, partial = rc.doubling_nodes(nt)
        seen = np.zeros((nt, nt), dtype=int)
        for _, t0, s, s2 in full + partial:
            seen[t0:t0 + s, t0 + s:t0 + s + s2] += 1
        assert np.array_equal(seen, np.triu(np.ones((nt, nt), dtype=int), 1)), nt
        assert bool(partial) == (nt & (nt - 1) != 0)  # partial nodes exactly when nt is no power of two


# ------------------------------------------------------------------------------------------ (a) room under every bound
@on(ALL)
def test_clean_emulation_has_room(emu):
    n = emu.n
    r_l = rc.rho_L(emu.Kaug, emu.Laug)
    left, right = rc.rho_U_left(emu.L, emu.U), rc.rho_U_right(emu.L, emu.U)
    ref_l, ref_r = emu.ref
    print(f"{emu.p.name}: n {n} rho_L {r_l:.1f} (room {(2 * n + 1) / 4:.0f}) rho_U_left {left:.2f} (ref {ref_l:.2f}) "
          f"rho_U_right {right:.2f} (ref {ref_r:.2f})")
    assert r_l <= rc.bound_L(n) / 4, rc.describe(rc.worst_tile(rc.rho_L, emu.Kaug, emu.Laug))
    assert left <= rc.bound_U(ref_l) / 4, rc.describe(rc.worst_tile(rc.rho_U_left, emu.L, emu.U))
    assert right <= rc.bound_U(ref_r) / 4, rc.describe(rc.worst_tile(rc.rho_U_right, emu.L, emu.U))


@on(FAULT_SIZES)
def test_clean_emulation_meets_the_product_bounds(emu):
    beta = emu.Laug[emu.n]
    assert rc.rho_W(emu.U, emu.W) <= rc.bound_gemm(emu.n)
    assert rc.rho_alpha(emu.U, beta, emu.U @ beta) <= rc.bound_gemm(emu.n)


# ------------------------------------------------------------------------------------------ (b) planted faults
@on(MULTI_TILE)
def test_fault_L_tile_scaled(emu):
    """One off-diagonal tile of L times (1 + 1e-9): rho_L at least 10 x its bound, at every size (tile column 0: first and last
    tile row; see the module docstring for late tile columns)."""
    for ti in (1, emu.nt - 1):
        F = emu.Laug.copy()
        emu.tile(F, ti, 0)[:] *= 1.0 + 1e-9
        w = rc.worst_tile(rc.rho_L, emu.Kaug, F)
        assert w.value >= 10 * rc.bound_L(emu.n), (ti, w.value)
        assert ti in w.tile  # (row ti of L enters the rows and the columns ti of L L^T)


@on(FAULT_SIZES[1:])
def test_fault_L_tile_in_fp32(emu):
    for ti, tj in ((emu.nt // 2 + 1, emu.nt // 2), (emu.nt - 1, emu.nt - 2)):
        F = emu.Laug.copy()
        blk = emu.tile(F, ti, tj)
        blk[:] = blk.astype(np.float32)
        assert rc.rho_L(emu.Kaug, F) > rc.bound_L(emu.n), (ti, tj)


@on(MULTI_TILE)
def test_fault_beta_entry(emu):
    """The largest entry of beta off by 1e-9 relative."""
    F = emu.Laug.copy()
    k = int(np.argmax(np.abs(F[emu.n])))
    F[emu.n, k] *= 1.0 + 1e-9
    w = rc.worst_tile(rc.rho_L, emu.Kaug, F)
    assert w.value > rc.bound_L(emu.n) and w.tile[0] == emu.nt  # (the beta row is the last tile row)


@on(FAULT_SIZES)
def test_fault_U_tile_scaled(emu):
    b_left, b_right = (rc.bound_U(r) for r in emu.ref)
    for (ti, tj), also_w in (((0, 1), True), ((emu.nt - 2, emu.nt - 1), True), ((0, emu.nt - 1), False)):
        F = emu.U.copy()
        emu.tile(F, ti, tj)[:] *= 1.0 + 1e-9
        wl, wr = rc.worst_tile(rc.rho_U_left, emu.L, F), rc.worst_tile(rc.rho_U_right, emu.L, F)
        assert wl.value > 10 * b_left and wr.value > 10 * b_right, (ti, tj, wl.value, wr.value)
        if also_w:  # K^-1 left as it was: it no longer belongs to this U
            assert rc.rho_W(F, emu.W) > 10 * rc.bound_gemm(emu.n), (ti, tj)


@on(FAULT_SIZES)
def test_fault_U_stale_partial_node(emu):
    """Every size here has a tile-column count that is no power of two: each trailing partial node in turn keeps a zero U12."""
    _, partial = rc.doubling_nodes(emu.nt)
    assert partial
    b_left, b_right = (rc.bound_U(r) for r in emu.ref)
    for node in partial:
        F = rc.emulate_U(emu.L, emu.invs, skip=(node,))
        w = rc.worst_tile(rc.rho_U_left, emu.L, F)
        assert w.value > 10 * b_left and rc.rho_U_right(emu.L, F) > 10 * b_right, node
        _, t0, s, s2 = node
        assert t0 + s <= w.tile[0] < t0 + s + s2 and w.tile[1] < t0 + s  # (X = U^T: the rows of the node's second half)


@on(WELL_CONDITIONED)
def test_fault_U_garbage_under_the_diagonal(emu):
    """1e-12 under the diagonal inside a diagonal tile of U, K^-1 recomputed from the full tile as the device would: rho_U does
    not look there (triu), rho_W does."""
    t = emu.nt // 2
    for r, c in ((5, 2), (127, 0), (64, 63)):
        F = emu.U.copy()
        F[t * T + r, t * T + c] = 1e-12
        W = emu.W.copy()
        for j in range(t + 1):
            emu.tile(W, t, j)[:] = rc.w_tile(F, t, j)
        w = rc.worst_tile(rc.rho_W, F, W)
        assert w.value > rc.bound_gemm(emu.n) and w.tile[0] == t, (r, c, w.value)
        assert rc.rho_U_left(emu.L, F) == rc.rho_U_left(emu.L, emu.U)


@on(FAULT_SIZES)
def test_fault_W_tile_with_a_late_k_range(emu):
    for i, j in ((emu.nt - 2, 1), (emu.nt - 2, emu.nt - 2)):
        F = emu.W.copy()
        emu.tile(F, i, j)[:] = rc.w_tile(emu.U, i, j, k_first=i + 1)
        w = rc.worst_tile(rc.rho_W, emu.U, F)
        assert w.value > 10 * rc.bound_gemm(emu.n) and w.tile == (i, j)


@on(["single-300"])
def test_fault_in_the_padding(emu):
    """1e-300 where an exact zero belongs.  In K^-1 the denominator |U||U^T| is 0 there: ratio inf.  In L and U the entry is
    part of its own denominator, so it has a relative error of 1 with nothing else to be relative to: ratio 1 / eps = 4.5e15
    (half of it for the U statistics, whose denominator (|X||L|)^2 holds the entry twice)."""
    n, N = emu.n, emu.p.N
    assert N < n - 2
    for i, j in ((N + 1, 3), (n - 1, N), (n - 1, n - 2)):   # padding row x real column, padding x padding
        F = emu.Laug.copy()
        F[i, j] = 1e-300
        assert rc.rho_L(emu.Kaug, F) >= 0.25 / rc.EPS
        F = emu.U.copy()
        F[j, i] = 1e-300
        assert min(rc.rho_U_left(emu.L, F), rc.rho_U_right(emu.L, F), rc.rho_W(F, emu.W)) >= 0.25 / rc.EPS
        F = emu.W.copy()
        F[i, j] = 1e-300
        w = rc.worst_tile(rc.rho_W, emu.U, F)
        assert w.value == np.inf and w.tile == (i // T, j // T)
    F = emu.Laug.copy()
    F[n, N] = 1e-300   # beta's padding
    assert rc.rho_L(emu.Kaug, F) >= 0.25 / rc.EPS
    F = emu.Kaug.copy()
    F[n - 1, N] = 1e-300   # the covariance itself: the factor's padding no longer belongs to it
    assert rc.rho_L(F, emu.Laug) == np.inf
    # the clean matrices: finite, i.e. identity in the padding and exact zeros around it
    assert np.isfinite([rc.rho_L(emu.Kaug, emu.Laug), rc.rho_U_left(emu.L, emu.U), rc.rho_W(emu.U, emu.W)]).all()
