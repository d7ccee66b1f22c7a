"""Element-wise backward-error statistics for the three matrices every result of the library passes through -- the factor L
(with beta = L^-1 y as its last row) in K_dev, U = L^-T in Z_dev and the lower triangle of K^-1 = U U^T in W_dev -- and a
NumPy emulation of the device's algorithm (blocked Cholesky with explicit leaf inverses, block doubling of U with trailing
partial nodes, K^-1 tile by tile), written from the comments of csrc/gp_sched.hip.

Every statistic is max over j <= i of |residual|_ij / (eps * (product of absolute values)_ij) and works on NumPy arrays and on
torch fp64 tensors alike (on the GPU every product here is a torch matmul, i.e. rocBLAS, independent of the project's GEMM).
Ratio rule: where the denominator is 0 the numerator must be exactly 0 (ratio 0), else the ratio is inf -- in the identity
padding every off-diagonal denominator is 0, so this rule is what pins "identity in the padding, exact zeros around it":
a non-zero there gives inf where the denominator does not hold the entry itself (K^-1 against |U||U^T|) and 1 / eps = 4.5e15
where it does (an entry of L or U is its own and only term).  A NaN anywhere gives inf.

n below is the PADDED size (a multiple of 128)."""
import collections

import numpy as np
import scipy.linalg as sla

EPS = 2.0 ** -52
TILE = 128


# ------------------------------------------------------------------------------------------ NumPy / torch dispatch
def _np(a):
    return isinstance(a, np.ndarray)


def _abs(a):
    return np.abs(a) if _np(a) else a.abs()


def _tril(a, k=0):
    return np.tril(a, k) if _np(a) else a.tril(k)


def _triu(a, k=0):
    return np.triu(a, k) if _np(a) else a.triu(k)


def _sub_eye(a):
    """a - I (a square), out of place."""
    if _np(a):
        r = a.copy()
        idx = np.arange(a.shape[0])
        r[idx, idx] -= 1.0
        return r
    r = a.clone()
    r.diagonal().sub_(1.0)
    return r


def ratio(num, den):
    """|num| / (eps den) element-wise under the ratio rule of the module docstring (den >= 0)."""
    if _np(num):
        num = np.abs(num)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            r = num / (EPS * den)
        r = np.where(den == 0, np.where(num == 0, 0.0, np.inf), r)
        return np.where(np.isnan(r), np.inf, r)
    import torch

    num = num.abs()
    r = num / (EPS * den)
    zero, inf = torch.zeros((), dtype=r.dtype, device=r.device), torch.full((), float("inf"), dtype=r.dtype, device=r.device)
    r = torch.where(den == 0, torch.where(num == 0, zero, inf), r)
    return torch.where(torch.isnan(r), inf, r)


# ------------------------------------------------------------------------------------------ ratio matrices
def ratios_L(Kaug, Laug):
    """Kaug: (n + 1) x n, K with y^T appended (zero-padded).  Laug: (n + 1) x n, the factor with beta^T appended: beta is
    checked as the last row of the same trapezoid factorisation, which is how the device computes it."""
    n = Laug.shape[1]
    L = _tril(Laug[:n])
    Laug = _tril(Laug)  # (row n is kept whole: j <= n for every column)
    return _tril(ratio(Kaug - Laug @ L.T, _abs(Laug) @ _abs(L).T))


def ratios_U_left(L, U):
    """X L - I with X = triu(U)^T against the condition-aware (|X||L|)^2: every triangular inversion satisfies
    |X - L^-1| <= c eps |L^-1||L||L^-1| (Higham, Accuracy and Stability, section 14), the doubling recursion included."""
    L = _tril(L)
    X = _triu(U).T
    M = _abs(X) @ _abs(L)
    return _tril(ratio(_sub_eye(X @ L), M @ M))


def ratios_U_right(L, U):
    L = _tril(L)
    X = _triu(U).T
    M = _abs(L) @ _abs(X)
    return _tril(ratio(_sub_eye(L @ X), M @ M))


def ratios_W(U, W):
    """Lower triangle of W against triu(U) triu(U)^T: the device's product reads the whole diagonal tile of U, so a non-zero
    under the diagonal inside a diagonal tile shows here.  W's strict upper triangle is scratch and not compared."""
    T = _triu(U)
    return _tril(ratio(W - T @ T.T, _abs(T) @ _abs(T).T))


def ratios_alpha(U, beta, alpha):
    """alpha = U beta as an n x 1 column."""
    T = _triu(U)
    b = beta.reshape(-1, 1)
    return ratio(alpha.reshape(-1, 1) - T @ b, _abs(T) @ _abs(b))


def _max(r):
    return float(r.max())


def rho_L(Kaug, Laug):
    return _max(ratios_L(Kaug, Laug))


def rho_U_left(L, U):
    return _max(ratios_U_left(L, U))


def rho_U_right(L, U):
    return _max(ratios_U_right(L, U))


def rho_W(U, W):
    return _max(ratios_W(U, W))


def rho_alpha(U, beta, alpha):
    return _max(ratios_alpha(U, beta, alpha))


RATIOS = {rho_L: ratios_L, rho_U_left: ratios_U_left, rho_U_right: ratios_U_right, rho_W: ratios_W, rho_alpha: ratios_alpha}

Worst = collections.namedtuple("Worst", "value tile tiles")


def tile_maxima(r):
    """Per-128x128-tile maxima of a ratio matrix (ragged edges -- the beta row, the alpha column -- are tiles of their own)."""
    rows, cols = r.shape
    tr, tc = -(-rows // TILE), -(-cols // TILE)
    if _np(r):
        p = np.zeros((tr * TILE, tc * TILE))
        p[:rows, :cols] = r
        return p.reshape(tr, TILE, tc, TILE).max(axis=(1, 3))
    import torch

    p = torch.zeros((tr * TILE, tc * TILE), dtype=r.dtype, device=r.device)
    p[:rows, :cols] = r
    return p.reshape(tr, TILE, tc, TILE).amax(dim=(1, 3)).cpu().numpy()


def worst_tile(stat, *inputs):
    """Same inputs as the statistic `stat` (one of the rho_* functions): Worst(value, (tile row, tile column), tile maxima)."""
    t = tile_maxima(RATIOS[stat](*inputs))
    arg = np.unravel_index(int(np.argmax(t)), t.shape)
    return Worst(float(t[arg]), (int(arg[0]), int(arg[1])), t)


def describe(w):
    """Text for an assertion message: the arg-max tile and how far it stands out from the median of the tiles that hold anything."""
    held = w.tiles[w.tiles > 0]
    med = float(np.median(held)) if held.size else 0.0
    return f"worst tile (row {w.tile[0]}, column {w.tile[1]}) = {w.value:.4g}, median over non-empty tiles {med:.4g}"


# ------------------------------------------------------------------------------------------ bounds
def bound_L(n):
    """(n + 1) + n: gamma_{n+1} of Higham Thm 10.3 (any summation order) plus the checking product's own rounding."""
    return (n + 1) + n


def bound_gemm(n):
    """2 n: the project's GEMM contract bound 2 k eps |A||B| (k = n), the check's product included."""
    return 2 * n


U_MARGIN = 16  # up to 8 doubling levels (256 tile columns), two products each, each adding a residual of the reference's size


def bound_U(rho_ref):
    return U_MARGIN * max(1.0, rho_ref)


def reference_inverse(L):
    """X_ref = L^-1 by LAPACK (host), the yardstick of the U statistics: rho_ref is the same statistic for X_ref."""
    L = np.tril(L)
    return sla.solve_triangular(L, np.eye(L.shape[0]), lower=True, check_finite=False)


# ------------------------------------------------------------------------------------------ emulation of the device's algorithm
def padded(n):
    return -(-int(n) // TILE) * TILE


def pad_problem(K, y):
    """Kaug ((np + 1) x np) of an n x n covariance and its outputs: identity in the padding, y^T zero-padded as row np."""
    n = K.shape[0]
    npad = padded(n)
    Kaug = np.zeros((npad + 1, npad))
    Kaug[:n, :n] = K
    idx = np.arange(n, npad)
    Kaug[idx, idx] = 1.0
    Kaug[npad, :n] = y
    return Kaug


def emulate_factor(Kaug):
    """Blocked Cholesky of the trapezoid [K; y^T] on 128-column tiles (left-looking): leaf = Cholesky of the diagonal block,
    strip = the rows below times the EXPLICIT inverse of the leaf (transposed).  Returns (Laug, leaf inverses)."""
    A = np.array(Kaug, dtype=np.float64)
    n = A.shape[1]
    eye = np.eye(TILE)
    invs = []
    for c0 in range(0, n, TILE):
        c1 = c0 + TILE
        if c0:
            A[c0:, c0:c1] -= A[c0:, :c0] @ A[c0:c1, :c0].T
        Lcc = np.linalg.cholesky(A[c0:c1, c0:c1])
        inv = sla.solve_triangular(Lcc, eye, lower=True, check_finite=False)
        A[c0:c1, c0:c1] = Lcc
        A[c1:, c0:c1] = A[c1:, c0:c1] @ inv.T
        invs.append(inv)
    return np.tril(A), invs


def doubling_nodes(nt):
    """(level s, first tile, tiles of the first half, tiles of the second half) in the device's order: every full node level by
    level, then the trailing partial nodes level by level (a partial node's first half is a full node of the level below, its
    second half was built by the partial nodes of the levels below).  Returns (full nodes, partial nodes)."""
    full, partial = [], []
    s = 1
    while s < nt:
        full += [(s, q * 2 * s, s, s) for q in range(nt // (2 * s))]
        s *= 2
    s = 1
    while s < nt:
        nfull = nt // (2 * s)
        rem = nt - nfull * 2 * s
        if rem > s:
            partial.append((s, nfull * 2 * s, s, rem - s))
        s *= 2
    return full, partial


def doubling_node(L, U, node):
    """[[L11, 0], [L21, L22]]^-T = [[U11, -U11 L21^T U22], [0, U22]]: writes U12 of one node (P = U11 L21^T, U12 = -P U22)."""
    _, t0, s, s2 = node
    a0, a1, a2 = t0 * TILE, (t0 + s) * TILE, (t0 + s + s2) * TILE
    P = U[a0:a1, a0:a1] @ L[a1:a2, a0:a1].T
    U[a0:a1, a1:a2] = -(P @ U[a1:a2, a1:a2])


def emulate_U(L, invs, skip=()):
    """U = L^-T: leaves from the leaf inverses, then block doubling.  Nodes listed in `skip` are left at zero (a stale node)."""
    n = L.shape[0]
    U = np.zeros((n, n))
    for c, inv in enumerate(invs):
        U[c * TILE:(c + 1) * TILE, c * TILE:(c + 1) * TILE] = inv.T
    full, partial = doubling_nodes(n // TILE)
    for node in full + partial:
        if node not in skip:
            doubling_node(L, U, node)
    return U


def w_tile(U, i, j, k_first=None):
    """Tile (i, j), j <= i, of K^-1 = U U^T: the k range starts at tile i (U is upper triangular) unless k_first says otherwise.
    Reads the WHOLE diagonal tile of U, as the device's launch does."""
    k0 = (i if k_first is None else k_first) * TILE
    return U[i * TILE:(i + 1) * TILE, k0:] @ U[j * TILE:(j + 1) * TILE, k0:].T


def emulate_W(U):
    """Lower tiles of K^-1 = U U^T, tile by tile; the strict upper tiles stay zero."""
    n = U.shape[0]
    W = np.zeros((n, n))
    for i in range(n // TILE):
        for j in range(i + 1):
            W[i * TILE:(i + 1) * TILE, j * TILE:(j + 1) * TILE] = w_tile(U, i, j)
    return W


# ------------------------------------------------------------------------------------------ the problems both test modules use
Problem = collections.namedtuple("Problem", "name N kernel d theta form diag_seed seed")


def _kern(kernel):
    return kernel.replace("*", "+").split("+"), [c for c in kernel if c in "+*"]


def _theta(kernel, d, gv=1e-4, ls_scale=1.0, kv=1.7):
    from oracle import gp_oracle as orc

    th = orc.synth_theta(d, nkern=len(_kern(kernel)[0]), kv=kv, gv=gv)
    nk = len(_kern(kernel)[0])
    th[: nk * d] *= ls_scale
    return th


# single lml_grad evaluations (marginal form): the smallest size of each regime of the schedule, none a multiple of 128; the
# kernels rotate, N = 1600 / RBF / gv 1e-8 and N = 800 / RatQuad / gv 1e-6 are the ill-conditioned inputs (cond(K) ~ 1e9)
_SINGLE = [
    (100, "RBF", 2, 1e-4),               # 1 tile column
    (300, "Matern52", 3, 1e-4),          # 3: first partial doubling node
    (800, "RatQuad", 4, 1e-6),           # 7: partial nodes on two levels
    (1600, "RBF", 5, 1e-8),              # 13
    (2600, "Matern32+RBF", 2, 1e-4),     # 21: look-ahead and extended panels from 20 on
    (3400, "Exponential*RBF", 3, 1e-4),  # 27: column mode from the start
    (4100, "Matern52", 4, 1e-4),         # 33: panels in front of a column-mode tail, 128x128 GEMM launches
]
SINGLE = [Problem(f"single-{N}", N, k, d, _theta(k, d, gv), "marginal", None, N) for N, k, d, gv in _SINGLE]
REGROUP_SIZES = (2600, 4100)   # once more with options 37, 35 and 32 at 0: no column mode, no extended panels, no thin kernel
REGROUP_OPTIONS = (37, 35, 32)
# factor + predict(via_inverse=True): conditional form, a per-point diagonal set, U by the stand-alone inverse_transpose
CONDITIONAL = [Problem("conditional-800", 800, "Matern52", 3, _theta("Matern52", 3), "conditional", 801, 800),
               Problem("conditional-2600", 2600, "RBF", 4, _theta("RBF", 4), "conditional", 2601, 2600)]
# batches of three thetas on the same data
_BATCH_VARIANTS = ((0.8, 1.7, 1e-4), (1.0, 1.2, 3e-4), (1.25, 2.3, 1e-3))  # (length-scale factor, kv, gv)


def batch_problems(N, kernel, d, form, tag):
    return [Problem(f"{tag}-{N}-{p}", N, kernel, d, _theta(kernel, d, gv, s, kv), form, None, N + 7)
            for p, (s, kv, gv) in enumerate(_BATCH_VARIANTS)]


BATCH_GRAD = {800: batch_problems(800, "Matern32+RBF", 3, "marginal", "batch"),
              2600: batch_problems(2600, "Matern52", 2, "marginal", "batch")}   # (column mode of a batch: option 38's launches)
BATCH_FACTOR = batch_problems(800, "Matern32+RBF", 3, "conditional", "factor-batch")
BAD_MEMBER_JITTER = -10.0  # kd + gv + jitter < 0: the member's first pivot fails (info = 1)
# append: reserve(400), factor at 250, + 5 -> 255, + 3 -> 258 (np 256 -> 384, the beta row moves)
APPEND_CAPACITY, APPEND_STAGES = 400, (250, 255, 258)
APPEND = [Problem(f"append-{n}", n, "Matern52", 3, _theta("Matern52", 3), "conditional", None, 258) for n in APPEND_STAGES]


def all_problems():
    """Every (N, kernel, theta, form) the GPU module evaluates (the bad batch member aside: nothing is asserted about it)."""
    return SINGLE + CONDITIONAL + BATCH_GRAD[800] + BATCH_GRAD[2600] + BATCH_FACTOR + APPEND


def problem_data(p):
    """(X, y, per-point diagonal or None) of a problem.  The append stages share one data set (its first N points)."""
    from oracle import gp_oracle as orc

    total = APPEND_STAGES[-1] if p.name.startswith("append") else p.N
    X, y = orc.synth_problem(total, p.d, seed=p.seed)
    diag = None if p.diag_seed is None else np.random.default_rng(p.diag_seed).uniform(0.0, 1e-3, p.N)
    return X[: p.N], y[: p.N], diag


def problem_cov(p):
    """The oracle's covariance of a problem in its noise form, the per-point diagonal added."""
    from oracle import gp_oracle as orc

    X, y, diag = problem_data(p)
    kerns, ops = _kern(p.kernel)
    return orc.noisy_cov(X, kerns, ops, p.theta, form=p.form, extra_diag=diag), y
