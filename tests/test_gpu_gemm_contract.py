"""The whole public contract of mi_gp_gemm_f64 / mi_gp_gemm_f64_tuned (include/mi_gp.h): all four transpose forms, tri, the
triangular k ranges of kmode 1-4, both tile kernels and the 128x128 launch that finishes its tail on 64x64 tiles, k values
whose 16-deep chunk counts cover every residue of the 64x64-tile kernel's unroll by three, general alpha / beta (beta = 0 over
a NaN-filled C), batches with strides, and padded leading dimensions.

Every element is checked against the fp64 product with the componentwise bound of a k-term dot product,
    |C - ref| <= 2 k eps (|alpha| |op(A)| |op(B)| + |beta| |C0|),
which both the kernel's and NumPy's summation orders satisfy; a dropped chunk, a misplaced tile or a scalar rounded to float
is many orders of magnitude outside it.  Everything the call may not write (padding columns, the gaps between batch items,
tiles above the block diagonal of a tri launch) must come back bit for bit.  The operands' padding holds NaN: a read past
the k range the tile needs would poison the result."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SENTINEL = -123.25
BIG, SMALL = "128x128", "64x64"


def _lib():
    from andvaranaut_amd import _lib

    return _lib.load()


def _operands(rng, m, n, k, kmode):
    """op(A) (m x k) and op(B) (k x n), with zeros where kmode skips k (the triangular shape the mode presumes)."""
    A = rng.uniform(-1.0, 1.0, (m, k))
    B = rng.uniform(-1.0, 1.0, (k, n))
    i = np.arange(m)[:, None]
    j = np.arange(n)[None, :]
    ka = np.arange(k)[None, :]
    kb = np.arange(k)[:, None]
    if kmode == 1:    # op(B) lower triangular: k >= j
        B[kb < j] = 0.0
    elif kmode == 2:  # op(A) lower triangular: k <= i
        A[ka > i] = 0.0
    elif kmode == 3:  # op(A) upper triangular: k >= i
        A[ka < i] = 0.0
    elif kmode == 4:  # op(B) upper triangular: k <= j
        B[kb > j] = 0.0
    return A, B


def _padded(M, pad, fill):
    """M in a row-major buffer with `pad` extra columns of `fill`: (buffer, leading dimension)."""
    buf = np.full((M.shape[0], M.shape[1] + pad), fill)
    buf[:, : M.shape[1]] = M
    return buf, M.shape[1] + pad


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _check(got, C0, A, B, alpha, beta, tri, what):
    """got / C0: m x ldc (C0 may hold NaN when beta == 0); A, B: op(A), op(B)."""
    m, k = A.shape
    n = B.shape[1]
    c0 = np.nan_to_num(C0[:, :n]) if beta == 0.0 else C0[:, :n]
    ref = alpha * (A @ B) + beta * c0
    bound = 2.0 * k * EPS * (abs(alpha) * (np.abs(A) @ np.abs(B)) + abs(beta) * np.abs(c0))
    win = got[:, :n]
    assert _same_bits(got[:, n:], C0[:, n:]), f"{what}: columns past n were written"
    if tri:
        i = np.arange(m)[:, None]
        j = np.arange(n)[None, :]
        lower = j <= i
        above = j >= (i // 128 + 1) * 128  # tiles above the block diagonal
        assert _same_bits(win[above], C0[:, :n][above]), f"{what}: a tile above the block diagonal was written"
        win, ref, bound = win[lower], ref[lower], bound[lower]
    assert np.isfinite(win).all(), f"{what}: non-finite result (NaN from C with beta = 0, or from operand padding)"
    err = np.abs(win - ref)
    bad = err > bound
    assert not bad.any(), f"{what}: {bad.sum()} elements outside 2 k eps |.|: max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3g}"


def _call(transa, transb, m, n, k, alpha, beta, tri, kmode, kernel, seed, tail_small=0, pad=6):
    import torch

    lib = _lib()
    rng = np.random.default_rng(seed)
    A, B = _operands(rng, m, n, k, kmode)
    As, lda = _padded(A.T if transa else A, pad, np.nan)
    Bs, ldb = _padded(B.T if transb else B, pad, np.nan)
    C0 = rng.uniform(-1.0, 1.0, (m, n + pad + 4))
    C0[:, n:] = SENTINEL
    if beta == 0.0:
        C0[:, :n] = np.nan  # beta = 0 must not read C
    dev = torch.device("cuda:0")
    tA, tB, tC = (torch.from_numpy(x.copy()).to(dev) for x in (As, Bs, C0))
    sb = {BIG: 0, SMALL: 1 << 30}[kernel]
    r = lib.mi_gp_gemm_f64_tuned(transa, transb, m, n, k, alpha, tA.data_ptr(), lda, tB.data_ptr(), ldb, beta, tC.data_ptr(),
                                 C0.shape[1], tri, kmode, sb, tail_small, 8, 0, None)
    assert r == 0, lib.mi_gp_last_global_error()
    torch.cuda.synchronize()
    assert _same_bits(tA.cpu().numpy(), As) and _same_bits(tB.cpu().numpy(), Bs)
    _check(tC.cpu().numpy(), C0, A, B, alpha, beta, tri,
           f"transa={transa} transb={transb} m={m} n={n} k={k} tri={tri} kmode={kmode} {kernel} alpha={alpha} beta={beta}")


def _shape(kmode):
    """(m, n, k) for a kmode: the triangular operand square and as long in k as the product (k = n for 1 / 4, k = m for 2 / 3)."""
    return {0: (384, 256, 160), 1: (384, 256, 256), 2: (384, 256, 384), 3: (384, 256, 384), 4: (384, 256, 256)}[kmode]


@pytest.mark.parametrize("kernel", [BIG, SMALL])
@pytest.mark.parametrize("kmode", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("tri", [0, 1])
@pytest.mark.parametrize("transa,transb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_every_form_and_kmode_gives_the_full_product(transa, transb, tri, kmode, kernel):
    """Each kmode with zeros where it skips k equals the full product, in every transpose form, triangular or not, on both
    tile kernels (kmode 2 always runs on 128x128 tiles)."""
    m, n, k = _shape(kmode)
    _call(transa, transb, m, n, k, 0.37, -2.5, tri, kmode, kernel, seed=100 * kmode + 10 * tri + 2 * transa + transb)


@pytest.mark.parametrize("kernel", [BIG, SMALL])
@pytest.mark.parametrize("kmode", [1, 2, 3, 4])
def test_kmode_with_k_longer_than_the_triangle(kmode, kernel):
    """k beyond the triangular square: the rows / columns past it are ordinary dense k."""
    m, n, k = _shape(kmode)
    _call(0, 1, m, n, k + 256, -1.0, 1.0, 0, kmode, kernel, seed=7 + kmode)


@pytest.mark.parametrize("kernel", [BIG, SMALL])
@pytest.mark.parametrize("k", [32, 96, 160, 384, 4224])
def test_k_values_cover_every_chunk_residue(k, kernel):
    """k / 16 = 2, 6, 10, 24, 264: residues 2, 0, 1, 0, 0 (mod 3) of the 64x64-tile kernel's three-chunk loop and its tail."""
    _call(0, 1, 256, 128, k, 0.37, 1.0, 0, 0, kernel, seed=k)
    _call(1, 0, 256, 256, k, -1.0, -2.5, 1, 0, kernel, seed=k + 1)


@pytest.mark.parametrize("kernel", [BIG, SMALL])
@pytest.mark.parametrize("beta", [1.0, -2.5, 0.0])
@pytest.mark.parametrize("alpha", [1.0, -1.0, 0.37])
def test_scalars(alpha, beta, kernel):
    """General alpha and beta on both epilogues; beta = 0 over a NaN-filled C returns alpha op(A) op(B) exactly as finite."""
    _call(0, 0, 256, 384, 96, alpha, beta, 0, 0, kernel, seed=abs(int(alpha * 100) + int(beta * 10)) + 3)
    _call(1, 1, 384, 384, 160, alpha, beta, 1, 0, kernel, seed=abs(int(alpha * 100) + int(beta * 10)) + 4)


def test_alpha_zero_returns_beta_c():
    _call(0, 1, 256, 256, 128, 0.0, -2.5, 0, 0, SMALL, seed=11)
    _call(0, 1, 256, 256, 128, 0.0, -2.5, 0, 0, BIG, seed=12)


@pytest.mark.parametrize("tri", [0, 1])
@pytest.mark.parametrize("transa,transb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_128_tile_launch_with_its_tail_on_64_tiles(transa, transb, tri):
    """More than one round of 512 128x128 tiles with a remainder of at most 384: the remainder runs on 64x64 tiles
    (tail_small; small_below = 0 keeps the whole launch off the 64x64 kernel).  3072 x 2816 = 528 tiles (tail 16); the 3072 x 3072 trapezoid = 300 tiles is under a round, so tri uses
    4608 x 2560 = 210 + 16 x 20 = 530 tiles (tail 18)."""
    m, n = (4608, 2560) if tri else (3072, 2816)
    _call(transa, transb, m, n, 96, 0.37, -2.5, tri, 0, BIG, seed=31 + tri + 2 * transa + transb, tail_small=1)


@pytest.mark.parametrize("m,n,k,kmode,tri", [
    (256, 256, 96, 0, 0),      # 4 tiles x 3 < 1024: the 64x64-tile kernel
    (2560, 2560, 32, 0, 1),    # 210 tiles x 3 = 630 < 1024: still 64x64 tiles
    (2560, 2560, 64, 0, 0),    # 400 tiles, alone below 1024 -- x 3 = 1200: the 128x128-tile kernel
    (384, 384, 384, 3, 1),     # the K^-1 = U U^T form, batched
    (256, 384, 384, 4, 0),     # the U12 = -P U22 form, batched
])
def test_batched_with_distinct_strides(m, n, k, kmode, tri):
    """batch = 3 through mi_gp_gemm_f64 with strides larger than the matrices (NaN / sentinel in the gaps): each item is its
    own product and the gaps stay as they were.  The tile form is chosen from tiles x batch."""
    import torch

    lib = _lib()
    rng = np.random.default_rng(m + n + k + kmode)
    transa, transb = (0, 1) if kmode != 4 else (0, 0)
    batch, pad = 3, 4
    ops = [_operands(rng, m, n, k, kmode) for _ in range(batch)]
    As = [_padded(A.T if transa else A, pad, np.nan) for A, _ in ops]
    Bs = [_padded(B.T if transb else B, pad, np.nan) for _, B in ops]
    lda, ldb, ldc = As[0][1], Bs[0][1], n + 2
    sA, sB, sC = As[0][0].size + 6 * lda, Bs[0][0].size + 2 * ldb + 2, m * ldc + 10 * ldc
    flatA = np.full(batch * sA, np.nan)
    flatB = np.full(batch * sB, np.nan)
    flatC = np.full(batch * sC, SENTINEL)
    for b in range(batch):
        flatA[b * sA: b * sA + As[b][0].size] = As[b][0].ravel()
        flatB[b * sB: b * sB + Bs[b][0].size] = Bs[b][0].ravel()
        flatC[b * sC: b * sC + m * ldc].reshape(m, ldc)[:, :n] = rng.uniform(-1.0, 1.0, (m, n))
    dev = torch.device("cuda:0")
    tA, tB, tC = (torch.from_numpy(x.copy()).to(dev) for x in (flatA, flatB, flatC))
    r = lib.mi_gp_gemm_f64(transa, transb, m, n, k, -1.0, tA.data_ptr(), lda, tB.data_ptr(), ldb, 0.37, tC.data_ptr(), ldc,
                           tri, kmode, batch, sA, sB, sC, None)
    assert r == 0, lib.mi_gp_last_global_error()
    torch.cuda.synchronize()
    got = tC.cpu().numpy()
    for b in range(batch):
        C0 = flatC[b * sC: b * sC + m * ldc].reshape(m, ldc)
        _check(got[b * sC: b * sC + m * ldc].reshape(m, ldc), C0, ops[b][0], ops[b][1], -1.0, 0.37, tri, f"batch item {b}")
        assert _same_bits(got[b * sC + m * ldc: (b + 1) * sC], flatC[b * sC + m * ldc: (b + 1) * sC]), "gap after item written"
