"""Each block-level entry of the C-ABI (include/mi_gp.h, "block-level operations") against a direct reference of the same
operation, on well-conditioned or exactly representable operands, so that the bounds are a few eps (times the length of
the sums) and not the cond(K)-scaled tolerances of the end-to-end tests: mi_gp_assemble_block (and the device exp / sqrt /
pow behind every covariance entry, against 40-digit mpmath), mi_gp_chol_panel, mi_gp_trsm_block, mi_gp_trmv_upper,
mi_gp_lml_partial and mi_gp_grad_contract_block.  These are the launches the single-GPU evaluation makes, too."""
import ctypes
import math

import numpy as np
import pytest

from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
TINY = 5e-324
SENTINEL = -77.5
INFO_NONE = 0x7F7F7F7F


def _lib():
    from andvaranaut_amd import _lib

    return _lib.load()


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def _ids(kerns, ops):
    ids = (ctypes.c_int * 8)(*([orc.KERNEL_IDS[k] for k in kerns] + [0] * (8 - len(kerns))))
    opv = (ctypes.c_int * 8)(*([{"+": 0, "*": 1}[o] for o in ops] + [0] * (8 - len(ops))))
    return ids, opv


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


# --------------------------------------------------------------------------------------------------- mi_gp_assemble_block
def _assemble(kerns, ops, theta, Xr, Xc, row0, col0, rows_pad, cols_pad, ldk, noise_form):
    lib = _lib()
    d = Xr.shape[1]
    ids, opv = _ids(kerns, ops)
    K0 = np.full((rows_pad, ldk), SENTINEL)
    tK, tth, tXr, tXc = _dev(K0), _dev(np.asarray(theta, dtype=np.float64)), _dev(Xr), _dev(Xc)
    r = lib.mi_gp_assemble_block(d, len(kerns), ids, opv, tth.data_ptr(), tXr.data_ptr(), Xr.shape[0], tXc.data_ptr(),
                                 Xc.shape[0], row0, col0, tK.data_ptr(), ldk, rows_pad, cols_pad, noise_form, None)
    assert r == 0, lib.mi_gp_last_global_error()
    K = _host(tK)
    assert _same_bits(K[:, cols_pad:], K0[:, cols_pad:]), "columns past cols_pad were written"
    return K


def _noise(form, theta, d, nk):
    _, _, _, gv, jitter = orc.split_theta(theta, d, nk)
    return gv, jitter


def _expected_diag(kdiag, form, gv, jitter):
    """The noisy diagonal in the order each noise form adds its terms (oracle.noisy_cov)."""
    s = np.sqrt(gv)
    if form == 0:
        return (kdiag + s * s) + jitter
    if form == 1:
        return (kdiag + jitter) + s * s
    return kdiag + (jitter + gv)


def _fold_sensitivity(kerns, ops, theta, Xr, Xc):
    """Per element: sum over components of |dK/dK_c| (|kv_c dk_c/dr2| |Xs_i|^2 + |Xs_j|^2 scale, |K_c|) -- the first-order
    effect of an r2 error relative to the norms and of a relative error in each component's value."""
    d = Xr.shape[1]
    nk = len(kerns)
    ls, kv, alpha, _, _ = orc.split_theta(theta, d, nk)
    comps, dks, norms = [], [], []
    for c in range(nk):
        r2 = orc.square_dist(Xr, Xc, ls[c])
        comps.append(kv[c] * orc.base_kernel(kerns[c], r2, alpha[c]))
        dks.append(np.abs(kv[c] * orc.base_kernel_dr2(kerns[c], r2, alpha[c])))
        a, b = Xr * (1.0 / ls[c]), Xc * (1.0 / ls[c])
        norms.append(np.sum(a * a, 1)[:, None] + np.sum(b * b, 1)[None, :])
    s_r2 = np.zeros_like(comps[0])
    s_val = np.zeros_like(comps[0])
    for c in range(nk):
        coef = np.ones_like(comps[0])
        T = comps[0]
        for i in range(1, nk):
            if i == c:
                coef = np.ones_like(T) if ops[i - 1] == "+" else np.abs(T)
            elif i > c and ops[i - 1] == "*":
                coef = coef * np.abs(comps[i])
            T = T + comps[i] if ops[i - 1] == "+" else T * comps[i]
        s_r2 += coef * dks[c] * norms[c]
        s_val += coef * np.abs(comps[c])
    return s_r2, s_val


ASSEMBLE_CASES = [
    # kerns, ops, d
    (["RBF"], [], 1),
    (["Matern52"], [], 31),
    (["Matern32"], [], 32),
    (["Exponential"], [], 33),
    (["RatQuad"], [], 129),
    (["RBF", "Matern52"], ["*"], 32),
    (["Matern32", "RatQuad", "Exponential"], ["+", "*"], 33),
    (["RBF", "Matern52", "Matern32", "Exponential", "RatQuad", "RBF", "Matern52", "Matern32"],
     ["+", "*", "+", "*", "+", "*", "+"], 3),
]
# (row0, col0, nrows, ncols, rows_pad, cols_pad): blocks crossing the global diagonal, missing it, ragged under their pads
GEOMETRIES = [
    (0, 0, 100, 100, 128, 128),
    (128, 64, 70, 150, 128, 192),    # diagonal crosses the block and runs on into the column padding
    (0, 256, 128, 90, 128, 128),     # above the diagonal: none of it inside
    (320, 0, 33, 200, 64, 256),      # below the diagonal, ragged rows
    (60, 0, 40, 59, 64, 128),        # the diagonal enters only in the padding (global row 60 + i = column i -> columns 60..123)
]


@pytest.mark.parametrize("geom", GEOMETRIES)
@pytest.mark.parametrize("case", ASSEMBLE_CASES)
def test_assemble_block_matches_the_oracle(case, geom):
    kerns, ops, d = case
    row0, col0, nrows, ncols, rows_pad, cols_pad = geom
    nk = len(kerns)
    rng = np.random.default_rng(d * 1000 + nk * 10 + row0 + col0)
    N = max(row0 + nrows, col0 + ncols)
    X = rng.random((N, d))
    ls = rng.uniform(0.4, 1.5, (nk, d)) * math.sqrt(d)
    theta = orc.pack_theta(ls, rng.uniform(0.5, 2.0, nk), 0.3, 1e-6, alpha=rng.uniform(0.5, 3.0, nk))
    Xr, Xc = X[row0: row0 + nrows], X[col0: col0 + ncols]
    for form in (0, 2):
        K = _assemble(kerns, ops, theta, Xr, Xc, row0, col0, rows_pad, cols_pad, cols_pad + 6, form)
        ref = orc.kernel_matrix(Xr, Xc, kerns, ops, theta)
        s_r2, s_val = _fold_sensitivity(kerns, ops, theta, Xr, Xc)
        gi = np.arange(rows_pad)[:, None] + row0
        gj = np.arange(cols_pad)[None, :] + col0
        on_diag = gi == gj
        inside = (np.arange(rows_pad)[:, None] < nrows) & (np.arange(cols_pad)[None, :] < ncols)
        # padding: the identity exactly where the GLOBAL diagonal runs through it, zeros elsewhere
        pad_ref = np.where(on_diag, 1.0, 0.0)
        assert _same_bits(K[:rows_pad, :cols_pad][~inside], pad_ref[~inside]), "padding is not the global identity"
        got = K[:nrows, :ncols]
        dmask = on_diag[:nrows, :ncols]
        gv, jitter = _noise(form, theta, d, nk)
        bound = 8.0 * EPS * (d + 4) * s_r2 + 8.0 * EPS * s_val + 4.0 * EPS * np.abs(ref)
        ref = ref.copy()
        ref[dmask] = _expected_diag(ref[dmask], form, gv, jitter)
        bound[dmask] += 4.0 * EPS * np.abs(ref[dmask])
        err = np.abs(got - ref)
        assert (err <= bound).all(), (kerns, geom, form, float(np.max(err / np.maximum(bound, TINY))))


@pytest.mark.parametrize("noise_form", [0, 1, 2])
@pytest.mark.parametrize("kerns,ops,d", [(["RBF"], [], 2), (["RBF"], [], 40), (["RBF", "RBF", "RBF"], ["+", "*"], 5)])
def test_assemble_block_diagonal_is_bit_exact(kerns, ops, d, noise_form):
    """Dyadic X and power-of-two length scales: r2 = 0 exactly on the diagonal, every RBF term is exactly kv, and the noise
    terms are plain fp64 adds in the order of the noise form -- the diagonal must equal the oracle's bit for bit.  The chosen
    kv / gv / jitter round differently when jitter goes in before or after sg^2, so a swapped order cannot pass."""
    nk = len(kerns)
    kv = np.array([1.7]) if nk == 1 else np.array([1.2, 0.5, 1.0])  # the diagonal kernel value is 1.7 either way
    theta = orc.pack_theta(np.full((nk, d), 0.5), kv, 0.3, 1e-6)
    kd = orc.kernel_diag(kerns, ops, theta, d)
    orders = {f: _expected_diag(kd, f, 0.3, 1e-6) for f in (0, 1, 2)}
    assert orders[0] != orders[1] and orders[1] != orders[2], "test values do not tell the noise orders apart"
    rng = np.random.default_rng(d + noise_form)
    X = rng.integers(-16, 16, (200, d)) / 8.0
    for row0, col0, nrows, ncols in ((0, 0, 200, 200), (64, 0, 136, 200), (0, 128, 200, 72)):
        rows_pad, cols_pad = (nrows + 63) // 64 * 64, (ncols + 63) // 64 * 64
        K = _assemble(kerns, ops, theta, X[row0: row0 + nrows], X[col0: col0 + ncols], row0, col0, rows_pad, cols_pad,
                      cols_pad + 2, noise_form)
        full = orc.noisy_cov(X, kerns, ops, theta, form={0: "marginal", 1: "conditional", 2: "explicit"}[noise_form])
        i = np.arange(max(row0, col0), min(row0 + nrows, col0 + ncols))
        got = K[i - row0, i - col0]
        assert got.size > 0
        assert _same_bits(got, full[i, i]), (noise_form, got[:3], full[i[:3], i[:3]])
        assert _same_bits(got, np.full(got.size, orders[noise_form]))


# ------------------------------------------------------------------------------- covariance entries against 40-digit mpmath
def _truth(name, r2, alpha, kv):
    import mpmath as mp

    mp.mp.dps = 40
    r2 = mp.mpf(float(r2))
    if name == "RBF":
        v, arg = mp.exp(-r2 / 2), r2 / 2
    elif name == "RatQuad":
        a = mp.mpf(float(alpha))
        v, arg = mp.power(1 + r2 / 2 / a, -a), a
    else:
        r = mp.sqrt(r2 + mp.mpf(1e-12))
        if name == "Matern52":
            s5 = mp.mpf(2.23606797749979)
            poly = 1 + s5 * r + mp.mpf(5.0 / 3.0) * r * r
            v, arg = poly * mp.exp(-s5 * r), s5 * r
        elif name == "Matern32":
            s3 = mp.mpf(1.7320508075688772)
            poly = 1 + s3 * r
            v, arg = poly * mp.exp(-s3 * r), s3 * r
        else:
            v, arg = mp.exp(-r / 2), r / 2
    kv = mp.mpf(float(kv))
    return float(kv * v), float(arg), float(kv * poly) if name in ("Matern52", "Matern32") else float(kv)


# r2 grid: dense near 0 (where the 1e-12 under the root matters), then out past the RBF underflow (r2 ~ 1490) and into the
# Matern / Exponential tails (r ~ 330 / 1490, r2 ~ 1.1e5 / 2.2e6).  X = integers / 8 on one axis, the column point at 0,
# length scale a power of two: r2 = x^2 / l^2 exactly (X * (1/ls), the MFMA dot product and the norms are exact).
def _grid(xmax):
    x = np.unique(np.concatenate([np.arange(0, 64), np.round(np.geomspace(64, xmax * 8, 1800))]).astype(np.int64))
    return x / 8.0


ULP_CASES = [
    # name, kv, alpha, ls, xmax, c0 (ulp), c1 (ulp per unit of the exp argument / of alpha)
    ("RBF", 1.0, 1.0, 1.0, 56.0, 2.0, 0.0),
    ("RBF", 1.7, 1.0, 0.5, 28.0, 3.0, 0.0),
    ("Matern52", 1.0, 1.0, 1.0, 340.0, 6.0, 6.0),
    ("Matern32", 1.7, 1.0, 2.0, 900.0, 6.0, 6.0),
    ("Exponential", 1.0, 1.0, 1.0, 1500.0, 6.0, 6.0),
    ("RatQuad", 1.0, 0.5, 1.0, 1500.0, 4.0, 1.0),
    ("RatQuad", 1.7, 2.0, 1.0, 1500.0, 4.0, 1.0),
    ("RatQuad", 1.0, 8.0, 0.5, 600.0, 4.0, 1.0),
]


@pytest.mark.parametrize("name,kv,alpha,ls,xmax,c0,c1", ULP_CASES)
def test_covariance_entries_against_mpmath(name, kv, alpha, ls, xmax, c0, c1):
    """Device exp_nonpos / sqrt_pos / pow and the Matern polynomials: error <= (c0 + c1 |exp argument|) ulp of the truth (for
    RatQuad c1 multiplies alpha), with an absolute floor of 4 subnormal ulps.  RBF's c0 follows migp_math.h's claim
    (exp_nonpos <= 1 ulp against libm); the Matern / Exponential c1 is the conditioning of exp(-c r) in r, whose own error is
    sqrt_pos's plus the rounding of r2 + 1e-12.  The absolute floor is 4 subnormal ulps of exp(-c r) times the factor that
    multiplies it (kv and the Matern polynomial): where exp(-c r) is subnormal (Matern52 beyond r ~ 317) it carries only a few
    bits, and the formula as PyMC writes it -- polynomial times exp, the oracle's order too -- scales that quantum by the
    polynomial (~2e5 at r = 332: measured 9e4 ulps of a 4.1e-318 truth, an absolute error of 4.5e-319)."""
    x = _grid(xmax)
    n = x.size
    X = x[:, None]
    theta = orc.pack_theta([[ls]], [kv], 0.1, 1e-6, alpha=[alpha])
    rows_pad = (n + 63) // 64 * 64
    K = _assemble([name], [], theta, X, np.zeros((1, 1)), 0, 1 << 24, rows_pad, 64, 66, 0)
    got = K[:n, 0]
    assert (K[:, 1:64] == 0.0).all() and (K[n:, 0] == 0.0).all()
    r2 = (x / ls) ** 2
    truth = np.empty(n)
    arg = np.empty(n)
    pre = np.empty(n)
    for i in range(n):
        truth[i], arg[i], pre[i] = _truth(name, r2[i], alpha, kv)
    ulp = np.spacing(np.abs(truth))
    bound = np.maximum((c0 + c1 * arg) * ulp, 4 * TINY * pre)
    err = np.abs(got - truth)
    worst = int(np.argmax(err / bound))
    assert (err <= bound).all(), (name, kv, alpha, f"r2={r2[worst]!r} got={got[worst]!r} truth={truth[worst]!r} "
                                  f"ulps={err[worst] / ulp[worst]:.2f} allowed={bound[worst] / ulp[worst]:.2f}")
    assert truth[-1] < 1e-300 or name == "RatQuad", "the sweep should reach the underflow"


# ---------------------------------------------------------------------------------------- mi_gp_chol_panel / mi_gp_trsm_block
def _exact_factor(rng, R, W):
    """An R x W lower trapezoid L (dyadic entries, diagonal in [1, 2), off-diagonal multiples of 1/256 up to 3/256 in
    magnitude: well conditioned) and A = L L11^T, whose every entry is exact in fp64: L is A's exact Cholesky factor."""
    L = rng.integers(-3, 4, (R, W)) / 256.0
    L[np.triu_indices(W, 1)] = 0.0
    L[np.arange(W), np.arange(W)] = 1.0 + rng.integers(0, 16, W) / 16.0
    return L


def _panel(A, W, row_tiles, w_tiles, col_base, lda_extra=64):
    lib = _lib()
    R = A.shape[0]
    buf = np.full((R, W + lda_extra), SENTINEL)
    buf[:, :W] = A
    tA, tdinv = _dev(buf), _dev(np.zeros(w_tiles * 16384))
    tinfo = _dev(np.array([INFO_NONE], dtype=np.int32))
    r = lib.mi_gp_chol_panel(tA.data_ptr(), buf.shape[1], row_tiles, w_tiles, tdinv.data_ptr(), tinfo.data_ptr(), col_base,
                             None)
    assert r == 0, lib.mi_gp_last_global_error()
    out = _host(tA)
    assert _same_bits(out[:, W:], buf[:, W:]), "columns right of the panel were written"
    return out, tA, tdinv, int(_host(tinfo)[0])


@pytest.mark.parametrize("w_tiles,row_tiles", [(1, 3), (2, 3), (3, 5), (5, 7), (8, 9)])
def test_chol_panel_against_the_exact_factor(w_tiles, row_tiles):
    rng = np.random.default_rng(w_tiles * 10 + row_tiles)
    W, R = 128 * w_tiles, 128 * row_tiles
    L = _exact_factor(rng, R, W)
    A = L @ L[:W].T
    out, _, _, info = _panel(A, W, row_tiles, w_tiles, col_base=384)
    assert info == INFO_NONE
    low = np.tril(np.ones((W, W), dtype=bool))
    err_top = np.abs(out[:W, :W] - L[:W])[low]
    err_below = np.abs(out[W:, :W] - L[W:])
    tol = W * EPS * np.abs(L).max()
    assert err_top.max() <= tol and err_below.max() <= tol, (err_top.max(), err_below.max(), tol)


@pytest.mark.parametrize("p", [37, 127, 128, 129, 383])
def test_chol_panel_reports_the_first_bad_pivot(p):
    """A = L D L^T with D = I except D_pp = -1: the first p pivots are those of L L^T and pivot p is -L_pp^2 exactly in
    real arithmetic, far from zero -- info = col_base + p + 1 (finite input, as in the library's own non-PD tests)."""
    rng = np.random.default_rng(p)
    W, R = 384, 512
    L = _exact_factor(rng, R, W)
    D = np.ones(W)
    D[p] = -1.0
    A = (L * D) @ L[:W].T
    _, _, _, info = _panel(A, W, 4, 3, col_base=1000)
    assert info == 1000 + p + 1, info


@pytest.mark.parametrize("m", [128, 384])
@pytest.mark.parametrize("c0_tiles,w_tiles", [(1, 1), (2, 3), (1, 4)])
def test_trsm_block_against_exact_solutions(c0_tiles, w_tiles, m):
    """X L^T = B over tile columns [c0, c0 + w) with the leaf inverses chol_panel wrote: B = X L^T exactly for a dyadic X,
    and B = identity rows gives rows of L^-T (fp64 reference); B is padded on both sides and the padding stays."""
    lib = _lib()
    rng = np.random.default_rng(100 * c0_tiles + 10 * w_tiles + m)
    ntc = c0_tiles + w_tiles + 1
    N = 128 * ntc
    L = _exact_factor(rng, N, N)
    F, tF, tdinv, info = _panel(L @ L.T, N, ntc, ntc, col_base=0, lda_extra=2)
    assert info == INFO_NONE
    c0, W = 128 * c0_tiles, 128 * w_tiles
    Lb = L[c0: c0 + W, c0: c0 + W]
    ldf = N + 2
    for kind in ("exact", "identity"):
        if kind == "exact":
            X = rng.integers(-8, 9, (m, W)) / 16.0
            B = X @ Lb.T  # exact
        else:
            rows = rng.choice(W, m, replace=W < m) if m <= W else np.arange(m) % W
            B = np.eye(W)[rows]
            X = np.linalg.solve(Lb, B.T).T  # rows of Lb^-T
        lead, ldb = 4, W + 10
        buf = np.full((m, ldb), SENTINEL)
        buf[:, lead: lead + W] = B
        tB = _dev(buf)
        r = lib.mi_gp_trsm_block(tF.data_ptr(), ldf, tdinv.data_ptr(), c0_tiles, w_tiles, tB.data_ptr() + 8 * lead, ldb, m,
                                 None)
        assert r == 0, lib.mi_gp_last_global_error()
        got = _host(tB)
        assert _same_bits(got[:, :lead], buf[:, :lead]) and _same_bits(got[:, lead + W:], buf[:, lead + W:])
        err = np.abs(got[:, lead: lead + W] - X)
        tol = 4 * W * EPS * np.abs(X).max()
        assert err.max() <= tol, (kind, err.max(), tol)


# -------------------------------------------------------------------------------------------------------- mi_gp_trmv_upper
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 257, 1000])
def test_trmv_upper_against_long_double(n):
    lib = _lib()
    rng = np.random.default_rng(n)
    ld = n + 3
    U = rng.uniform(-1.0, 1.0, (n, ld))
    U[np.tril_indices(n, -1)] = np.nan  # the strictly lower part must not be read into the result
    x = rng.uniform(-1.0, 1.0, n)
    tU, tx, to = _dev(U), _dev(x), _dev(np.full(n + 4, SENTINEL))
    r = lib.mi_gp_trmv_upper(tU.data_ptr(), ld, tx.data_ptr(), n, to.data_ptr(), None)
    assert r == 0, lib.mi_gp_last_global_error()
    out = _host(to)
    assert (out[n:] == SENTINEL).all()
    Ut = np.triu(np.nan_to_num(U[:, :n]))
    ref = (Ut.astype(np.longdouble) @ x.astype(np.longdouble)).astype(np.float64)
    bound = n * EPS * (np.abs(Ut) @ np.abs(x)) + TINY
    assert np.isfinite(out[:n]).all()
    assert (np.abs(out[:n] - ref) <= bound).all(), float(np.max(np.abs(out[:n] - ref) / bound))


# ------------------------------------------------------------------------------------------------------- mi_gp_lml_partial
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1024, 1025, 4097])
def test_lml_partial_against_fsum(n):
    lib = _lib()
    rng = np.random.default_rng(n)
    ld = n + 2
    import torch

    tL = torch.full((n, ld), float("nan"), dtype=torch.float64, device="cuda:0")  # only the diagonal may be read
    diag = rng.uniform(0.3, 3.0, n)
    tL.diagonal().copy_(torch.from_numpy(diag))
    beta = rng.uniform(-2.0, 2.0, n)
    tb = _dev(beta)
    out0 = np.full(6, SENTINEL)
    to = _dev(out0)
    r = lib.mi_gp_lml_partial(tL.data_ptr(), ld, tb.data_ptr(), n, to.data_ptr(), None)
    assert r == 0, lib.mi_gp_last_global_error()
    out = _host(to)
    assert (out[3:] == SENTINEL).all(), "out[3..] must stay untouched"
    logs = [math.log(v) for v in diag]
    s1, s2 = math.fsum(logs), math.fsum(b * b for b in beta)
    c = (n / 128 + 16) * EPS
    assert abs(out[1] - s1) <= c * math.fsum(abs(v) for v in logs) + 2 * EPS * abs(s1), (out[1], s1)
    assert abs(out[2] - s2) <= c * s2, (out[2], s2)
    lml = -0.5 * n * 1.8378770664093453 - 0.5 * out[2] - out[1]
    assert abs(out[0] - lml) <= 4 * EPS * (0.5 * n * 1.8378770664093453 + 0.5 * out[2] + abs(out[1])), (out[0], lml)


# ----------------------------------------------------------------------------------------------- mi_gp_grad_contract_block
CONTRACT_CASES = [
    (["Matern52"], [], 3, 300),
    (["RBF", "RatQuad"], ["*"], 2, 200),
    (["Exponential", "Matern32", "RBF"], ["+", "*"], 3, 257),
]


@pytest.mark.parametrize("kerns,ops,d,n", CONTRACT_CASES)
def test_grad_contract_block_slabs_against_numpy(kerns, ops, d, n):
    """A random symmetric W and a random alpha (not K^-1: the bound does not depend on cond(K)); dyadic X and power-of-two
    length scales make r2 exact, so the only error is the kernels' function evaluation and the summation.  Every slab of
    several tilings of [0, n) -- global rows (row0 = 0 < col0), a row0 between, and the slab alone in its own buffer
    (row0 = col0) -- equals 1/2 sum_lower (alpha_i alpha_j - W_ij) dK_ij/dtheta over its columns, diagonal once; the slabs
    of a tiling add up to the whole."""
    lib = _lib()
    nk = len(kerns)
    rng = np.random.default_rng(n + d)
    X = rng.integers(0, 64, (n, d)) / 8.0
    theta = orc.pack_theta(2.0 ** rng.integers(0, 3, (nk, d)), rng.uniform(0.5, 2.0, nk), 0.2, 1e-6,
                           alpha=rng.uniform(0.5, 3.0, nk))
    ntheta = nk * d + 2 * nk + 2
    Wm = rng.uniform(-1.0, 1.0, (n, n))
    Wm = 0.5 * (Wm + Wm.T)
    al = rng.uniform(-1.0, 1.0, n)
    M = np.outer(al, al) - Wm
    dK = orc.dK_dtheta(X, kerns, ops, theta)
    i = np.arange(n)[:, None]
    j = np.arange(n)[None, :]
    omega = np.where(i > j, 1.0, np.where(i == j, 0.5, 0.0))
    ids, opv = _ids(kerns, ops)
    ldw = n + 6
    Wbuf = np.zeros((n, ldw))
    Wbuf[:, :n] = Wm
    tX, tth, tW, tal = _dev(X), _dev(theta), _dev(Wbuf), _dev(al)
    tg = _dev(np.zeros(ntheta))
    npad = (n + 63) // 64 * 64

    def slab(col0, cols, mode):
        jm = (j >= col0) & (j < col0 + cols)
        terms = (omega * jm * M)[None] * dK
        ref = terms.sum(axis=(1, 2))
        bound = 64 * EPS * np.abs(terms).sum(axis=(1, 2)) + TINY
        nsc = lib.mi_gp_grad_contract_block_scratch(n, col0, cols, ntheta)
        tpart = _dev(np.zeros(max(nsc, 1)))
        if mode == "own":  # the slab alone: rows col0.., columns col0 .. col0 + cols, its own leading dimension
            row0 = col0
            own = np.full((n - col0, cols + 2), np.nan)
            w = min(cols, n - col0)
            own[:, :w] = Wm[col0:, col0: col0 + w]
            tbuf, ptr, ld = _dev(own), None, cols + 2
            ptr = tbuf.data_ptr()
        else:
            row0 = 0 if mode == "global" else max(col0 - 64, 0)
            tbuf, ld = tW, ldw
            ptr = tW.data_ptr() + 8 * (row0 * ldw + col0)
        r = lib.mi_gp_grad_contract_block(d, nk, ids, opv, tth.data_ptr(), tX.data_ptr(), n, ptr, ld, row0, col0, cols,
                                          tal.data_ptr(), tpart.data_ptr(), tpart.numel(), tg.data_ptr(), None)
        assert r == 0, lib.mi_gp_last_global_error()
        got = _host(tg).copy()
        assert (np.abs(got - ref) <= bound).all(), (mode, col0, cols, np.max(np.abs(got - ref) / bound))
        return got, bound

    whole = (M[None] * dK).sum(axis=(1, 2)) * 0.5
    tilings = [[(0, npad)], [(0, 64), (64, 128), (192, npad - 192)], [(c, 64) for c in range(0, npad, 64)]]
    for t, tiling in enumerate(tilings):
        for mode in ("global", "between", "own"):
            parts = [slab(c0, cols, mode) for c0, cols in tiling if c0 < n]
            total = np.sum([g for g, _ in parts], axis=0)
            tb = np.sum([b for _, b in parts], axis=0) + 64 * EPS * np.abs(0.5 * M[None] * dK).sum(axis=(1, 2))
            assert (np.abs(total - whole) <= tb).all(), (t, mode, np.max(np.abs(total - whole) / tb))
