"""The 128x128-tile GEMM kernel (small_below = 0 forces it) on every operand form: the NT form stages its operands into LDS by
LDS-DMA, the forms with a k-major operand through registers.  Checked against an fp64 reference within 2 k eps |alpha| |A||B|
+ |beta| |C| element-wise, and bit for bit against the 64x64-tile kernel where both compute the same k range in the same order
(uniform k), against the plain operand layout (k-segments), across the scheduling options (one workgroup per CU, the 64x64 tail)
and across the members of a batch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
BIG = 1 << 20  # small_below: every launch on the 64x64-tile kernel


def _lib():
    from andvaranaut_amd import _lib

    return _lib.load()


def _operand(rows, cols, kmajor, ld_pad, gen, dev):
    """rows x k logical operand X (row = output row / column, col = k).  Stored [rows][k] (row-major) or [k][rows] (k-major)
    with NaN in the padding columns past the leading dimension's used part."""
    import torch

    X = torch.randn(rows, cols, dtype=torch.float64, device=dev, generator=gen)
    if kmajor:
        store = torch.full((cols, rows + ld_pad), float("nan"), dtype=torch.float64, device=dev)
        store[:, :rows] = X.T
    else:
        store = torch.full((rows, cols + ld_pad), float("nan"), dtype=torch.float64, device=dev)
        store[:, :cols] = X
    return X, store


def _kmask(m, n, k, kmode, dev):
    """per (row of A, k) and (row of B, k) masks of the k range each tile takes (kmode 1..4), in 128-row tile units"""
    import torch

    kk = torch.arange(k, device=dev)
    ti = (torch.arange(m, device=dev) // 128)[:, None]
    tj = (torch.arange(n, device=dev) // 128)[:, None]
    ma = torch.ones(m, k, dtype=torch.bool, device=dev)
    mb = torch.ones(n, k, dtype=torch.bool, device=dev)
    if kmode == 1:
        mb = kk[None, :] >= 128 * tj
    elif kmode == 2:
        ma = kk[None, :] < 128 * (ti + 1)
    elif kmode == 3:
        ma = kk[None, :] >= 128 * ti
    elif kmode == 4:
        mb = kk[None, :] < 128 * (tj + 1)
    return ma, mb


def _gemm(transa, transb, m, n, k, alpha, Ast, Bst, beta, C, tri, kmode, small_below, tail=0, one_per_cu=0):
    lib = _lib()
    r = lib.mi_gp_gemm_f64_tuned(transa, transb, m, n, k, alpha, Ast.data_ptr(), Ast.stride(0), Bst.data_ptr(), Bst.stride(0),
                                 beta, C.data_ptr(), C.stride(0), tri, kmode, small_below, tail, 8, one_per_cu, None)
    assert r == 0, lib.mi_gp_last_global_error()


def _check(got, A, B, C0, alpha, beta, k, kmode, tri, m, n):
    import torch

    ma, mb = _kmask(m, n, k, kmode, A.device)
    Am, Bm = A * ma, B * mb
    prod = Am @ Bm.T
    ref = alpha * prod + (beta * C0 if beta != 0.0 else 0.0)
    bound = 2 * k * EPS * (abs(alpha) * (Am.abs() @ Bm.abs().T) + (abs(beta) * C0.abs() if beta != 0.0 else 0.0)) + 1e-300
    mask = torch.ones(m, n, dtype=torch.bool, device=A.device)
    if tri:  # tiles on and below the block diagonal are computed (whole tiles); the ones above are not touched
        t = torch.arange(m, device=A.device)[:, None] // 128 >= torch.arange(n, device=A.device)[None, :] // 128
        mask = t
        assert torch.equal(got[~t], C0[~t])
    err = ((got - ref).abs() / bound)[mask]
    assert torch.isfinite(got[mask]).all()
    assert err.max().item() <= 1.0, err.max().item()


@pytest.mark.parametrize("transa,transb", [(0, 1), (0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("kmode", [0, 1, 2, 3, 4])
def test_every_form_and_kmode_against_the_reference(transa, transb, kmode):
    import torch

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(11 * kmode + 3 * transa + transb)
    m, n = 640, 512
    k = {0: 352, 1: 544, 4: 544, 2: 672, 3: 672}[kmode]  # residues 96 / 32 / 32 / 32 / 32 of 128, >= n or m where needed
    tri = 1 if kmode in (0, 3) else 0
    A, Ast = _operand(m, k, transa == 1, 16, gen, dev)
    B, Bst = _operand(n, k, transb == 0, 16, gen, dev)
    C0 = torch.randn(m, n + 8, dtype=torch.float64, device=dev, generator=gen)
    C = C0.clone()
    _gemm(transa, transb, m, n, k, -1.0, Ast, Bst, 1.0, C, tri, kmode, 0)
    torch.cuda.synchronize()
    assert torch.equal(C[:, n:], C0[:, n:])
    _check(C[:, :n], A, B, C0[:, :n], -1.0, 1.0, k, kmode, tri, m, n)


@pytest.mark.parametrize("transa,transb", [(0, 1), (0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("k", [32, 64, 96, 128, 160, 224, 1056])
def test_k_residues_match_the_reference_and_the_64x64_tile_kernel(transa, transb, k):
    """uniform k: both kernels take the whole k range in ascending k4-steps on the same lane maps, so they agree bit for bit"""
    import torch

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(k + 7 * transa + transb)
    m, n = 768, 640
    A, Ast = _operand(m, k, transa == 1, 16, gen, dev)
    B, Bst = _operand(n, k, transb == 0, 16, gen, dev)
    C0 = torch.randn(m, n, dtype=torch.float64, device=dev, generator=gen)
    C, Cs = C0.clone(), C0.clone()
    _gemm(transa, transb, m, n, k, -1.0, Ast, Bst, 1.0, C, 0, 0, 0)
    _gemm(transa, transb, m, n, k, -1.0, Ast, Bst, 1.0, Cs, 0, 0, BIG)
    torch.cuda.synchronize()
    _check(C, A, B, C0, -1.0, 1.0, k, 0, 0, m, n)
    assert torch.equal(C, Cs)


@pytest.mark.parametrize("transa,transb", [(0, 1), (0, 0)])
def test_tail_and_one_per_cu_give_the_same_bits(transa, transb):
    """528 tiles of a triangle: one round of 512 on 128x128 tiles and a tail of 16 tiles finished on 64x64 tiles (tail_small),
    or all 528 on 128x128 tiles; one or two workgroups per CU.  Which kernel computes a tile never changes its bits."""
    import torch

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(5 + transb)
    m = n = 4096
    k = 288
    A, Ast = _operand(m, k, transa == 1, 32, gen, dev)
    B, Bst = (A, Ast) if transb == 1 else _operand(n, k, True, 32, gen, dev)
    C0 = torch.randn(m, n, dtype=torch.float64, device=dev, generator=gen)
    outs = []
    for tail, opc in ((0, 0), (1, 0), (0, 1), (1, 1)):
        C = C0.clone()
        _gemm(transa, transb, m, n, k, -1.0, Ast, Bst, 1.0, C, 1, 0, 0, tail, opc)
        outs.append(C)
    torch.cuda.synchronize()
    _check(outs[0], A, B, C0, -1.0, 1.0, k, 0, 1, m, n)
    assert torch.equal(outs[2], outs[0]) and torch.equal(outs[3], outs[1])
    low = torch.tril(torch.ones(m, n, dtype=torch.bool, device=dev))  # (the 64x64 tail skips the upper quadrant of diagonal tiles)
    assert torch.equal(outs[1][low], outs[0][low])


def test_beta_zero_never_reads_c():
    import torch

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(17)
    m, n, k = 1024, 896, 416
    A, Ast = _operand(m, k, False, 16, gen, dev)
    B, Bst = _operand(n, k, False, 16, gen, dev)
    for opc in (0, 1):
        C = torch.full((m, n), float("nan"), dtype=torch.float64, device=dev)
        _gemm(0, 1, m, n, k, 0.5, Ast, Bst, 0.0, C, 0, 0, 0, 0, opc)
        torch.cuda.synchronize()
        _check(C, A, B, torch.zeros_like(C), 0.5, 0.0, k, 0, 0, m, n)


@pytest.mark.parametrize("transa,transb", [(0, 1), (0, 0)])
def test_batch_of_three_with_nan_padded_strides(transa, transb):
    """mi_gp_gemm_f64, batch = 3 (blockIdx.z): the members sit in one allocation with NaN between them and NaN past every
    row's used columns; 3 x 352 tiles >= the default small_below, so the 128x128-tile kernel runs.  Each member must match the
    reference and a launch of its own (which runs on the same kernel when forced with small_below = 0)."""
    import torch

    dev = torch.device("cuda:0")
    lib = _lib()
    gen = torch.Generator(device=dev).manual_seed(23 + transb)
    m, n, k, nb = 4096, 1408, 160, 3
    a_rows, a_cols = (k, m + 16) if transa else (m, k + 16)
    b_rows, b_cols = (k, n + 16) if transb == 0 else (n, k + 16)
    sa, sb, sc = a_rows * a_cols + 1024, b_rows * b_cols + 512, m * (n + 8) + 256
    Abuf = torch.full((nb * sa,), float("nan"), dtype=torch.float64, device=dev)
    Bbuf = torch.full((nb * sb,), float("nan"), dtype=torch.float64, device=dev)
    Cbuf = torch.full((nb * sc,), float("nan"), dtype=torch.float64, device=dev)
    mats = []
    for z in range(nb):
        A, Ast = _operand(m, k, transa == 1, 16, gen, dev)
        B, Bst = _operand(n, k, transb == 0, 16, gen, dev)
        Abuf[z * sa: z * sa + a_rows * a_cols].view(a_rows, a_cols).copy_(Ast)
        Bbuf[z * sb: z * sb + b_rows * b_cols].view(b_rows, b_cols).copy_(Bst)
        Cz = Cbuf[z * sc: z * sc + m * (n + 8)].view(m, n + 8)
        Cz[:, :n] = torch.randn(m, n, dtype=torch.float64, device=dev, generator=gen)
        mats.append((A, B, Ast, Bst, Cz[:, :n].clone()))
    C_before = Cbuf.clone()
    r = lib.mi_gp_gemm_f64(transa, transb, m, n, k, -1.0, Abuf.data_ptr(), a_cols, Bbuf.data_ptr(), b_cols, 1.0, Cbuf.data_ptr(),
                           n + 8, 0, 0, nb, sa, sb, sc, None)
    assert r == 0, lib.mi_gp_last_global_error()
    torch.cuda.synchronize()
    for z, (A, B, Ast, Bst, C0) in enumerate(mats):
        Cz = Cbuf[z * sc: z * sc + m * (n + 8)].view(m, n + 8)
        _check(Cz[:, :n], A, B, C0, -1.0, 1.0, k, 0, 0, m, n)
        single = C0.clone()
        _gemm(transa, transb, m, n, k, -1.0, Ast, Bst, 1.0, single, 0, 0, 0)
        torch.cuda.synchronize()
        assert torch.equal(Cz[:, :n], single)
    # nothing outside the members' n used columns was written (NaN stays NaN: compare the NaN pattern and the finite values)
    untouched = torch.ones_like(Cbuf, dtype=torch.bool)
    for z in range(nb):
        untouched[z * sc: z * sc + m * (n + 8)].view(m, n + 8)[:, :n] = False
    assert torch.equal(torch.isnan(Cbuf[untouched]), torch.isnan(C_before[untouched]))


@pytest.mark.parametrize("kseg,k", [(128, 1024), (256, 768), (512, 512)])
def test_k_segments_on_the_dma_path(kseg, k):
    """mi_gp_gemm_nt_kseg forced onto the 128x128-tile kernel: the per-lane DMA sources jump with the segment, and the bits
    are those of the plain row-major layout"""
    import torch

    dev = torch.device("cuda:0")
    lib = _lib()
    gen = torch.Generator(device=dev).manual_seed(kseg + k)
    m, n = 2048, 1024
    P = torch.randn(m, k, dtype=torch.float64, device=dev, generator=gen)
    C0 = torch.randn(m, n, dtype=torch.float64, device=dev, generator=gen)
    stride = (m + 128) * kseg
    pieces = torch.full((k // kseg, stride), float("nan"), dtype=torch.float64, device=dev)
    for s in range(k // kseg):
        pieces[s, : m * kseg].view(m, kseg).copy_(P[:, s * kseg: (s + 1) * kseg])
    C1, C2 = C0.clone(), C0.clone()
    r = lib.mi_gp_gemm_nt_kseg(m, n, k, -1.0, pieces.data_ptr(), kseg, pieces.data_ptr(), kseg, kseg, stride, 1.0,
                               C1.data_ptr(), n, 1, 0, None)
    assert r == 0, lib.mi_gp_last_global_error()
    _gemm(0, 1, m, n, k, -1.0, P, P, 1.0, C2, 1, 0, 0)
    torch.cuda.synchronize()
    assert torch.equal(C1, C2)
    _check(C2, P, P[:n], C0, -1.0, 1.0, k, 0, 1, m, n)
