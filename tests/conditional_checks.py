"""Element-wise backward-error statistics for every stage of the conditional -- the work rows A = K* L^-T of the blocked solve
(trsm_rec, api_gp.hip), the same rows through U (A = K* U: one GEMM with kmode 4, or one trmv_upper_t pass per point), the rows
w_p = U A_p, the reduction to mean and variance (predict_reduce_kernel), the Schur complement Sigma = K** + shift I - A A^T and
its factor -- in the style of tests/resident_checks.py, whose ratio rule, tile helpers, bounds and factor emulation are used
here and not repeated.  Each stage is judged against exactly what it read (K*, L, beta and U as they sit in the caller's and the
handle's buffers), so no bound depends on cond(K).

Every statistic is max over entries of |residual| / (eps * denominator) under resident_checks.ratio: a zero denominator requires
an exactly zero numerator (this is what pins the exact zeros of the padding columns n .. np of A: there K* is 0, L is the
identity, and a non-zero A_pj is its own denominator: ratio 1 / eps), NaN gives inf (work and cov buffers are NaN-filled before
every call, so a result that depends on unwritten scratch fails).  On the GPU the products are torch matmuls (rocBLAS),
independent of the project's GEMM; the two reductions are checked in np.longdouble on the host.

statistic   residual / denominator                                                    bound
rho_A       K* - A L^T / |A| |L|^T, all m x np entries                                bound_L(np): the A rows are further rows of
                                                                                      the trapezoid factorisation that gives beta
rho_AU      A - K* triu(U) / |K*| |triu(U)|  (columns < n only for the per-point      bound_gemm(np)
            route, which writes no others)
rho_w       w - triu(U) A_p / |triu(U)| |A_p|, columns < n                            bound_gemm(np)
rho_mean    mean_p - A_p . beta / |A_p| . |beta|                                      bound_gemm(np)
rho_var     var_p - (kd - sum A_pi^2 + noise) / n sum A_pi^2 + |kd| + noise           4: the sum of n squares in any order is off
                                                                                      by less than n eps sum A^2 (1), then two
                                                                                      roundings of partial results no larger than
                                                                                      |kd| + sum A^2 + noise (1 each), one spare
rho_Sigma   Sigma - (K** + shift I - A A^T) / |K**| + shift I + np |A| |A|^T,         4: the GEMM contract 2 k eps |A||B| at k = np
            j <= i < m                                                                (2 / np of the last term), the checking
                                                                                      product (1 / np of it), the update's and the
                                                                                      shift's roundings (1 each of the first two)
rho_LSigma  resident_checks.rho_L of the Sigma bits and the factor mi_gp_sample_cov   bound_L(mp)
            leaves in their place

n is the number of points, np = padded(n), m the number of query points, mp = padded(m)."""
import numpy as np

import resident_checks as rc
from resident_checks import EPS, TILE, bound_gemm, bound_L, describe, emulate_factor, padded, ratio, tile_maxima, worst_tile  # noqa: F401

BOUND_VAR = 4
BOUND_SIGMA = 4


# ------------------------------------------------------------------------------------------ NumPy / torch dispatch
def _host(a):
    return a if isinstance(a, np.ndarray) else a.detach().cpu().numpy()


def _long(a):
    return _host(a).astype(np.longdouble)


def _eye_like(a, scale):
    """scale * I of a's (square) shape, type and device."""
    if rc._np(a):
        return scale * np.eye(a.shape[0])
    import torch

    return scale * torch.eye(a.shape[0], dtype=a.dtype, device=a.device)


# ------------------------------------------------------------------------------------------ ratio matrices
def ratios_A(Kstar, A, L):
    """Kstar, A: m x np (the right-hand side the solve read, the rows it left); L: np x np, the resident factor."""
    L = rc._tril(L)
    return ratio(Kstar - A @ L.T, rc._abs(A) @ rc._abs(L).T)


def ratios_AU(Kstar, A, U, cols=None):
    """A = K* triu(U).  cols = n restricts the check to columns < n (U is upper triangular: they depend on rows < n of U and
    entries < n of K* alone) -- the per-point route writes nothing else."""
    c = A.shape[1] if cols is None else cols
    T = rc._triu(U)[:c, :c]
    Kstar, A = Kstar[:, :c], A[:, :c]
    return ratio(A - Kstar @ T, rc._abs(Kstar) @ rc._abs(T))


def ratios_w(U, A, w, n):
    """The rows w_p = U A_p (w = A triu(U)^T) over columns < n; reads entries < n of A only, as trmv_upper_kernel does."""
    T = rc._triu(U)[:n, :n]
    A, w = A[:, :n], w[:, :n]
    return ratio(w - A @ T.T, rc._abs(A) @ rc._abs(T).T)


def ratios_mean(A, beta, mean, n):
    """m x 1.  The reference dot products run in np.longdouble on the host."""
    a, b = _long(A)[:, :n], _long(beta).reshape(-1)[:n]
    num = _long(mean).reshape(-1) - a @ b
    den = np.abs(a) @ np.abs(b)
    return ratio(num.astype(np.float64), den.astype(np.float64)).reshape(-1, 1)


def prior_diag_noise(theta, d, ops, pred_noise):
    """(kd, noise) in fp64 exactly as predict_reduce (api_gp.hip) forms them: kd the left-to-right +/* fold of the kv,
    noise = sqrt(gv)^2 with pred_noise, else 0.  ops: the '+' / '*' between the components."""
    nk = len(ops) + 1
    th = np.asarray(theta, dtype=np.float64)
    kd = th[nk * d]
    for c in range(1, nk):
        kd = kd + th[nk * d + c] if ops[c - 1] == "+" else kd * th[nk * d + c]
    sg = np.sqrt(th[nk * d + 2 * nk])
    return float(kd), float(sg * sg) if pred_noise else 0.0


def ratios_var(A, var, n, kd, noise):
    """m x 1.  Says nothing about the sign of var: kd - sum A^2 cancels, and the reference does not promise a positive result."""
    s2 = (_long(A)[:, :n] ** 2).sum(axis=1)
    num = _long(var).reshape(-1) - (np.longdouble(kd) - s2 + np.longdouble(noise))
    den = n * s2 + abs(kd) + noise
    return ratio(num.astype(np.float64), den.astype(np.float64)).reshape(-1, 1)


def ratios_Sigma(Kss, shift, A, Sigma, m):
    """Lower triangle j <= i < m.  Kss: K(X*, X*) without the diagonal term (m x m at least), A: the work rows (np columns),
    Sigma: what mi_gp_predict_cov left in cov_dev."""
    npad = A.shape[1]
    A, Kss, Sigma = A[:m], Kss[:m, :m], Sigma[:m, :m]
    I = _eye_like(Kss, shift)
    return rc._tril(ratio(Sigma - (Kss + I - A @ A.T), rc._abs(Kss) + I + npad * (rc._abs(A) @ rc._abs(A).T)))


def sigma_padding_is_identity(Sigma, m):
    """Rows m .. mp - 1 of the lower triangle hold the identity, bit for bit (-0.0 and NaN fail)."""
    S = np.tril(_host(Sigma))[m:, : Sigma.shape[0]]
    want = np.tril(np.eye(Sigma.shape[0]))[m:]
    return bool(np.array_equal(S.view(np.int64), want.view(np.int64)))


def ratios_LSigma(Sigma, Lsig):
    """resident_checks.ratios_L on the mp x mp lower triangles: the Sigma bits mi_gp_sample_cov read (padding included: the
    identity) and the factor it wrote over them.  A zero row stands where that function expects y^T and beta^T."""
    if rc._np(Sigma):
        z = np.zeros((1, Sigma.shape[1]))
        return rc.ratios_L(np.vstack([np.tril(Sigma), z]), np.vstack([np.tril(Lsig), z]))
    import torch

    z = torch.zeros((1, Sigma.shape[1]), dtype=Sigma.dtype, device=Sigma.device)
    return rc.ratios_L(torch.cat([Sigma.tril(), z]), torch.cat([Lsig.tril(), z]))


def _rho(fn):
    def stat(*args, **kw):
        return float(fn(*args, **kw).max())

    stat.__name__ = fn.__name__.replace("ratios_", "rho_")
    rc.RATIOS[stat] = fn  # (resident_checks.worst_tile finds the ratio matrix of a statistic there)
    return stat


rho_A, rho_AU, rho_w, rho_mean = _rho(ratios_A), _rho(ratios_AU), _rho(ratios_w), _rho(ratios_mean)
rho_var, rho_Sigma, rho_LSigma = _rho(ratios_var), _rho(ratios_Sigma), _rho(ratios_LSigma)


# ------------------------------------------------------------------------------------------ emulation of the device's algorithm
def emulate_solve(L, invs, Kstar, skip_update=None):
    """X L^T = K* in place, as trsm_rec does it: tile columns [c0, c0 + w) are halved as w / 2 and w - w / 2; a single tile
    column is a product with the explicit inverse of its leaf (transposed); between the halves one GEMM update
    B[:, second] -= X[:, first] L[second, first]^T.  skip_update = (c0, w, k0, k1): the update of that node leaves out columns
    k0 .. k1 - 1 of its k range (a planted fault)."""
    B = np.array(Kstar, dtype=np.float64)
    T = TILE

    def rec(c0, w):
        if w == 1:
            B[:, c0 * T:(c0 + 1) * T] = B[:, c0 * T:(c0 + 1) * T] @ invs[c0].T
            return
        w1 = w // 2
        rec(c0, w1)
        a, b, c = c0 * T, (c0 + w1) * T, (c0 + w) * T
        Lb = L[b:c, a:b]
        if skip_update is not None and skip_update[:2] == (c0, w):
            Lb = Lb.copy()
            Lb[:, skip_update[2]:skip_update[3]] = 0.0
        B[:, b:c] -= B[:, a:b] @ Lb.T
        rec(c0 + w1, w - w1)

    rec(0, L.shape[0] // T)
    return B


def solve_branch(nt, tc):
    """The nodes (c0, w) of trsm_rec's recursion over nt tile columns that contain tile column tc, root first."""
    path, c0, w = [], 0, nt
    while True:
        path.append((c0, w))
        if w == 1:
            return path
        w1 = w // 2
        c0, w = (c0, w1) if tc < c0 + w1 else (c0 + w1, w - w1)


def describe_solve(w, nt):
    """describe() of a work-row statistic plus the branch of the recursion that produced the worst tile column."""
    return describe(w) + "; solve nodes (first tile column, width) " + " > ".join(f"({c0}, {ww})" for c0, ww in solve_branch(nt, w.tile[1]))


def emulate_AU(Kstar, U, skip=None):
    """A = K* U tile column by tile column with the k range of kmode 4, k < (tj + 1) * 128.  skip = (tj, tk): tile column tj
    leaves out the 128 values k of tile tk (a planted fault)."""
    T = TILE
    A = np.zeros_like(Kstar)
    for tj in range(U.shape[0] // T):
        k1 = (tj + 1) * T
        Ub = U[:k1, tj * T:k1]
        if skip is not None and skip[0] == tj:
            Ub = Ub.copy()
            Ub[skip[1] * T:(skip[1] + 1) * T] = 0.0
        A[:, tj * T:k1] = Kstar[:, :k1] @ Ub
    return A


def wave_reduce(A, beta, n, kd, noise, skip=None):
    """mean and var of every row as predict_row_sums orders them: 64 lane-strided partial sums, then the wave64 tree.
    skip = (row, k0, k1): that row's mean leaves out entries k0 .. k1 - 1 (a planted fault)."""
    m = A.shape[0]
    k = np.arange(padded(n))
    lanes = np.zeros((2, m, 64))
    a = np.where(k[None, :] < n, A[:, : k.size], 0.0)
    b = np.zeros(k.size)
    b[:n] = beta[:n]
    ab = a * b[None, :]
    if skip is not None:
        ab[skip[0], skip[1]:skip[2]] = 0.0
    for j in range(0, k.size, 64):
        lanes[0] += ab[:, j:j + 64]
        lanes[1] += a[:, j:j + 64] ** 2
    width = 32
    while width:
        lanes[:, :, :width] += lanes[:, :, width:2 * width]
        width //= 2
    return lanes[0, :, 0], kd - lanes[1, :, 0] + noise


def emulate_Sigma(Kss, shift, A, m, skip=None):
    """The lower tiles of (K** + shift I) - A A^T over the padded square, identity in the padding.  skip = (ti, tj, tk): tile
    (ti, tj) leaves out the 128 values k of tile tk (a planted fault)."""
    T = TILE
    mp = padded(m)
    S = np.eye(mp)
    S[:m, :m] = Kss[:m, :m] + shift * np.eye(m)
    Ap = np.zeros((mp, A.shape[1]))
    Ap[:m] = A[:m]
    for ti in range(mp // T):
        for tj in range(ti + 1):
            a, b = Ap[ti * T:(ti + 1) * T], Ap[tj * T:(tj + 1) * T]
            if skip is not None and skip[:2] == (ti, tj):
                a = a.copy()
                a[:, skip[2] * T:(skip[2] + 1) * T] = 0.0
            S[ti * T:(ti + 1) * T, tj * T:(tj + 1) * T] -= a @ b.T
    return S


# ------------------------------------------------------------------------------------------ the problems both test modules use
# conditional form: 1, 3, 7 and 21 tile columns (3, 7 and 21 halve unevenly).  N = 100 is a sum kernel (kd is a fold of two kv);
# with one tile column the product with the explicit leaf inverse is the whole solve and (2 np + 1) / 4 = 64 is the narrowest
# room: the host emulation measures rho_A 26 here (plain RBF, d = 2, at the same size: 44 to 60, too close to 64 to choose)
SMALL = [rc.Problem("conditional-100", 100, "Matern32+RBF", 2, rc._theta("Matern32+RBF", 2), "conditional", None, 100),
         rc.Problem("conditional-300", 300, "Matern52", 3, rc._theta("Matern52", 3), "conditional", None, 300)]
WELL = SMALL + rc.CONDITIONAL   # N = 100, 300, 800, 2600


def _ill_theta():
    from oracle import gp_oracle as orc

    return orc.pack_theta([[1.5, 1.5]], [1.7], 1e-7, 1e-7)


# the regime Bayesian optimisation runs in: long length scales, gv 1e-7, predictive variances ~1e-8; cond(K) ~ 6e9
ILL = rc.Problem("ill-800", 800, "RBF", 2, _ill_theta(), "conditional", None, 800)
QUERY_COUNTS = (1, 16, 17, 127, 128, 129, 300)


def query_points(p, m, salt=0):
    """m query points in [-0.1, 1.1]^d (the data fill the unit cube)."""
    return np.random.default_rng(1000 * p.seed + m + salt).random((m, p.d)) * 1.2 - 0.1


def problem_cross(p, Xn):
    """(K* zero-padded to m x np, K** m x m in the full-matrix form, no diagonal term) of the oracle."""
    from oracle import gp_oracle as orc

    X, _, _ = rc.problem_data(p)
    kerns, ops = rc._kern(p.kernel)
    Ks = np.zeros((Xn.shape[0], padded(p.N)))
    Ks[:, : p.N] = orc.kernel_matrix(Xn, X, kerns, ops, p.theta)
    return Ks, orc.kernel_matrix(Xn, Xn, kerns, ops, p.theta)


def shift_of(p, pred_noise):
    """The diagonal term of Sigma (include/mi_gp.h): sqrt(gv)^2 with pred_noise, else the jitter."""
    nk = len(rc._kern(p.kernel)[0])
    gv, jitter = p.theta[nk * p.d + 2 * nk], p.theta[nk * p.d + 2 * nk + 1]
    sg = np.sqrt(gv)
    return float(sg * sg) if pred_noise else float(jitter)
