"""The three resident matrices every result passes through, read straight out of MiGP's tensors and judged by the element-wise
backward-error statistics of tests/resident_checks.py: the factor L with beta = L^-1 y as its last row (K_t / _bK), U = L^-T
(Z_t / _bZ) and the lower triangle of K^-1 = U U^T (W_t / _bW).  The rest of the suite sees them only through what is reduced
from them (the LML, a gradient of a dozen numbers, predictive moments), where a defect of one 128 x 128 tile is diluted.

K is the matrix the handle factored: assembled once per case with mi_gp_assemble_block over the whole padded square in the
matching noise form (the per-point diagonal added on the host), and itself held against oracle.noisy_cov within the
tolerance of test_gpu_blocks.test_assemble_block_matches_the_oracle.  Every product is a torch matmul (rocBLAS); the LAPACK
references (rho_ref of the U statistics, the LAPACK factor's rho_L) run on the host with SciPy.

Bounds (resident_checks.bound_*): rho_L <= (n + 1) + n; rho_W, rho_alpha <= 2 n; rho_U_left / rho_U_right <= 16 max(1, rho_ref)
with rho_ref the same statistic for X_ref = solve_triangular(L_device, I).  test_resident_checks_host.py shows that the
algorithm itself, in plain fp64, stays a factor 4 under each of them on every problem used here, and that planted faults
of one tile exceed them.

Measured on an MI355X (the -s output of this module; n is the padded size):

case                           n |  rho_L LAPACK  bound | U_left   ref  bound | U_rght   ref  bound |  rho_W rho_alpha  bound
-----------------------------------------------------------------------------------------------------------------------------
single-100                   128 |    5.6    2.5    257 |   2.00  0.72   16.0 |   2.00  0.50   16.0 |    0.0       1.7    256
single-300                   384 |   18.8    5.5    769 |   2.00  1.56   25.0 |   2.00  0.50   16.0 |    0.0       3.1    768
single-800                   896 |   26.5   15.8   1793 |   2.00  1.54   24.7 |   2.00  0.58   16.0 |    0.0       3.3   1792
single-1600                 1664 |   47.1   27.8   3329 |   2.00  2.14   34.3 |   2.00  1.08   17.2 |    0.0       5.9   3328
single-2600                 2688 |   40.0   39.4   5377 |   6.12  5.69   91.0 |   4.84  6.90  110.4 |    3.0      19.5   5376
single-2600-regrouped       2688 |   35.9   39.4   5377 |   6.20  6.75  108.0 |   5.20  6.42  102.7 |    3.5      18.2   5376
single-3400                 3456 |   53.2   52.6   6913 |   8.16  6.39  102.3 |   4.86  6.65  106.3 |    3.8      18.3   6912
single-4100                 4224 |   56.6   49.5   8449 |   5.62  5.54   88.6 |   4.21  4.43   70.9 |    4.2      12.7   8448
single-4100-regrouped       4224 |   48.3   49.5   8449 |   6.33  5.24   83.9 |   4.23  5.05   80.9 |    4.0      15.8   8448
conditional-800              896 |   23.7   18.6   1793 |   2.35  2.67   42.8 |   1.89  2.00   32.1 |
conditional-2600            2688 |   46.6   40.1   5377 |   4.87  4.19   67.1 |   3.78  3.43   54.9 |
batch-800-0                  896 |   23.4   15.9   1793 |   2.78  2.95   47.2 |   2.00  1.73   27.6 |    0.0             1792
batch-800-1                  896 |   22.2   20.0   1793 |   2.78  3.31   53.0 |   2.00  1.99   31.8 |    0.0             1792
batch-800-2                  896 |   19.7   18.5   1793 |   3.27  3.35   53.6 |   2.21  1.96   31.3 |    0.0             1792
batch-2600-0                2688 |   65.0   41.5   5377 |   6.85  6.81  108.9 |   4.31  4.50   71.9 |    4.7             5376
batch-2600-1                2688 |   61.2   54.5   5377 |   5.74  4.78   76.5 |   3.40  3.81   60.9 |    3.9             5376
batch-2600-2                2688 |   68.4   61.1   5377 |   5.03  4.71   75.3 |   3.30  3.55   56.8 |    4.3             5376
batch-800-0-beside-bad       896 |   23.4   15.9   1793 |   2.78  2.95   47.2 |   2.00  1.73   27.6 |    0.0             1792
batch-800-2-beside-bad       896 |   19.7   18.5   1793 |   3.27  3.35   53.6 |   2.21  1.96   31.3 |    0.0             1792
factor-batch-800-0           896 |   23.4   15.9   1793 |                     |                     |
factor-batch-800-1           896 |   22.2   20.0   1793 |                     |                     |
factor-batch-800-2           896 |   19.7   18.5   1793 |                     |                     |
append-250                   256 |   34.0    7.0    513 |   2.00  1.57   25.2 |   2.00  0.50   16.0 |
append-255                   256 |   34.0    7.0    513 |   2.00  1.57   25.2 |   2.00  0.50   16.0 |
append-258                   384 |   34.0    5.5    769 |   2.00  1.57   25.2 |   2.00  0.50   16.0 |

(The last bound column is 2 n, for rho_W and rho_alpha.  rho_W = 0.0: the device's product and rocBLAS's agree bit for bit there.
The U statistics of 2.00 at the small sizes sit on the diagonal, X_ii L_ii = 1 + 2 eps.  Every U statistic is within a small
factor of LAPACK's own: none needed the derived fallback bound.)
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.linalg as sla

import resident_checks as rc
from oracle import gp_oracle as orc
from test_gpu_blocks import EPS, _fold_sensitivity, _ids

pytestmark = pytest.mark.gpu

FORM_ID = {"marginal": 0, "conditional": 1}
DEV = "cuda:0"


def _t(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=2)
def _oracle_cov(name):
    """(oracle.noisy_cov without the per-point diagonal, the element-wise tolerance of the assembly test) of a problem."""
    p = next(q for q in rc.all_problems() if q.name == name)
    X, _, _ = rc.problem_data(p)
    kerns, ops = rc._kern(p.kernel)
    ref = orc.noisy_cov(X, kerns, ops, p.theta, form=p.form)
    s_r2, s_val = _fold_sensitivity(kerns, ops, p.theta, X, X)
    bound = 8.0 * EPS * (p.d + 4) * s_r2 + 8.0 * EPS * s_val + 4.0 * EPS * np.abs(ref)
    idx = np.arange(p.N)
    bound[idx, idx] += 4.0 * EPS * np.abs(ref[idx, idx])
    return ref, bound


def assembled_cov(gp, p, n, diag=None):
    """Kaug ((np + 1) x np, device) of the handle's first n points at p.theta: mi_gp_assemble_block over the padded square (the
    same kernel as the single-GPU assembly), checked against the oracle, + the per-point diagonal, + y^T as the last row."""
    import torch

    npad = rc.padded(n)
    kerns, ops = rc._kern(p.kernel)
    ids, opv = _ids(kerns, ops)
    K = torch.full((npad + 1, npad), float("nan"), dtype=torch.float64, device=DEV)
    th = _t(p.theta)
    torch.cuda.synchronize()
    r = gp.lib.mi_gp_assemble_block(p.d, len(kerns), ids, opv, th.data_ptr(), gp.X_t.data_ptr(), n, gp.X_t.data_ptr(), n, 0, 0,
                                    K.data_ptr(), npad, npad, npad, FORM_ID[p.form], None)
    assert r == 0, gp.lib.mi_gp_last_global_error()
    torch.cuda.synchronize()
    ref, bound = _oracle_cov(p.name)
    assert ref.shape == (n, n)
    err = np.abs(K[:n, :n].cpu().numpy() - ref)
    assert (err <= bound).all(), (p.name, "assembled K against oracle.noisy_cov", float(np.max(err / bound)))
    if diag is not None:
        K[:n, :n].diagonal().add_(_t(diag))
    K[npad] = 0.0
    K[npad, :n] = gp.y_t[:n]
    return K


def check(label, gp, p, Kbuf, Z=None, W=None, alpha=None, diag=None):
    """All statistics of one set of resident buffers (Kbuf: (np + 128) x lda, Z / W: np x lda or None).  Prints the measured
    row, then asserts every bound; a failure names the statistic, the case and the worst tile."""
    import torch

    n, npad = gp.n, rc.padded(gp.n)
    assert gp.np_ == npad
    Kaug = assembled_cov(gp, p, n, diag)
    Laug = torch.cat([Kbuf[:npad, :npad].tril(), Kbuf[npad:npad + 1, :npad]])
    L = Laug[:npad]
    got, bounds, worst = {}, {}, {}

    def measure(key, stat, bound, *args):
        got[key], bounds[key] = stat(*args), bound
        if not got[key] <= bound:
            worst[key] = rc.describe(rc.worst_tile(stat, *args))

    measure("rho_L", rc.rho_L, rc.bound_L(npad), Kaug, Laug)
    Kh = Kaug.cpu().numpy()
    Lr = sla.cholesky(Kh[:npad], lower=True, check_finite=False)
    Lr_aug = np.vstack([Lr, sla.solve_triangular(Lr, Kh[npad], lower=True, check_finite=False)])
    lapack_L = rc.rho_L(Kaug, _t(Lr_aug))
    del Kh, Lr, Lr_aug
    ref = {}
    if Z is not None:
        U = Z[:npad, :npad]
        assert not bool(U.tril(-1).any()), (label, "U holds a non-zero below its diagonal")
        Uref = _t(rc.reference_inverse(L.cpu().numpy())).T
        for key, stat in (("rho_U_left", rc.rho_U_left), ("rho_U_right", rc.rho_U_right)):
            ref[key] = stat(L, Uref)
            measure(key, stat, rc.bound_U(ref[key]), L, U)
        del Uref
        if W is not None:
            measure("rho_W", rc.rho_W, rc.bound_gemm(npad), U, W[:npad, :npad])
        if alpha is not None:
            a = torch.zeros(npad, dtype=torch.float64, device=DEV)
            a[:n] = _t(alpha)
            measure("rho_alpha", rc.rho_alpha, rc.bound_gemm(npad), U, Laug[npad], a)
    row = f"RESIDENT {label:24s} n {npad:5d} | rho_L {got['rho_L']:8.1f} (LAPACK {lapack_L:5.1f}) <= {bounds['rho_L']}"
    for key in ("rho_U_left", "rho_U_right"):
        if key in got:
            row += f" | {key} {got[key]:7.2f} (ref {ref[key]:5.2f}) <= {bounds[key]:.1f}"
    for key in ("rho_W", "rho_alpha"):
        if key in got:
            row += f" | {key} {got[key]:7.1f} <= {bounds[key]}"
    print(row)
    bad = {k: (got[k], bounds[k], worst[k]) for k in worst}
    assert not bad, (label, bad)
    return got


def alpha_of(gp):
    a = np.empty(gp.n)
    gp._check(gp.lib.mi_gp_alpha(gp.h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), "mi_gp_alpha")
    return a


def handle(p, **kw):
    from andvaranaut_amd import MiGP

    X, y, diag = rc.problem_data(p)
    gp = MiGP(X, y, p.kernel, device=0, **kw)
    if diag is not None:
        gp.set_diag(diag)
    return gp, diag


QUERY = 5  # points of the via_inverse predictions that make U resident


def query_points(p):
    return np.random.default_rng(p.seed).random((QUERY, p.d))


# ------------------------------------------------------------------------------------------ single lml_grad, marginal form
SINGLE_RUNS = [(p, regroup) for p in rc.SINGLE for regroup in ((False, True) if p.N in rc.REGROUP_SIZES else (False,))]


@pytest.mark.parametrize("p,regroup", SINGLE_RUNS, ids=[p.name + ("-regrouped" if r else "") for p, r in SINGLE_RUNS])
def test_lml_grad_leaves_L_U_Kinv_and_alpha(p, regroup):
    """Every statistic behind one mi_gp_lml_grad.  regroup: options 37, 35 and 32 at 0 -- no column mode, no extended panels, no
    thin kernel: other launches, the same bounds."""
    gp, _ = handle(p)
    try:
        if regroup:
            for opt in rc.REGROUP_OPTIONS:
                gp.set_option(opt, 0)
        val, _ = gp.lml_grad(p.theta)
        assert gp.info == 0 and np.isfinite(val)
        check(p.name + ("-regrouped" if regroup else ""), gp, p, gp.K_t, gp.Z_t, gp.W_t, alpha_of(gp))
    finally:
        gp.close()


def test_the_statistics_see_a_planted_fault_on_the_device():
    """The same torch products that pass the clean buffers fail a copy with one tile of U, or of L, scaled by 1 + 1e-9 (the host
    module plants the whole list of faults; this one shows that the device path of the statistics has the same eyes)."""
    import torch

    p = rc.SINGLE[1]
    gp, _ = handle(p)
    try:
        gp.lml_grad(p.theta)
        npad = gp.np_
        Kaug = assembled_cov(gp, p, gp.n)
        Laug = torch.cat([gp.K_t[:npad, :npad].tril(), gp.K_t[npad:npad + 1, :npad]])
        U = gp.Z_t[:npad, :npad].clone()
        Uref = _t(rc.reference_inverse(Laug[:npad].cpu().numpy())).T
        U[: rc.TILE, rc.TILE:2 * rc.TILE] *= 1.0 + 1e-9
        for stat, axis, where in ((rc.rho_U_left, 0, 1), (rc.rho_U_right, 1, 0)):  # (X = U^T: tile (1, 0) of X is the faulty one)
            w = rc.worst_tile(stat, Laug[:npad], U)
            assert w.value > 10 * rc.bound_U(stat(Laug[:npad], Uref)) and w.tile[axis] == where, (stat.__name__, rc.describe(w))
        assert rc.rho_W(U, gp.W_t[:npad, :npad]) > 10 * rc.bound_gemm(npad)
        Laug[rc.TILE:2 * rc.TILE, : rc.TILE] *= 1.0 + 1e-9
        assert rc.rho_L(Kaug, Laug) >= 10 * rc.bound_L(npad)
    finally:
        gp.close()


# ------------------------------------------------------------------------------------------ factor + predict through U
@pytest.mark.parametrize("p", rc.CONDITIONAL, ids=[p.name for p in rc.CONDITIONAL])
def test_factor_and_predict_via_inverse_leave_L_and_U(p):
    """The conditional form with a per-point diagonal; U comes from the stand-alone inverse_transpose (mi_gp_predict_u)."""
    gp, diag = handle(p)
    try:
        assert gp.factor(p.theta) == 0
        gp.predict(p.theta, query_points(p), via_inverse=True)
        check(p.name, gp, p, gp.K_t, gp.Z_t, diag=diag)
    finally:
        gp.close()


# ------------------------------------------------------------------------------------------ batches
@pytest.mark.parametrize("N", sorted(rc.BATCH_GRAD))
def test_lml_grad_batch_leaves_every_member(N):
    """Each member has its own L, U and K^-1 at the strides of mi_gp_set_batch."""
    ps = rc.BATCH_GRAD[N]
    gp, _ = handle(ps[0])
    try:
        vals, _ = gp.lml_grad_batch(np.stack([p.theta for p in ps]))
        assert np.isfinite(vals).all() and not gp.batch_info.any()
        for k, p in enumerate(ps):
            check(p.name, gp, p, gp._bK[k], gp._bZ[k], gp._bW[k])
    finally:
        gp.close()


def test_lml_grad_batch_with_a_bad_member_leaves_the_others():
    """The middle member's jitter makes its first pivot fail (info > 0, an ordinary return): members 0 and 2 must pass every
    statistic; nothing is asserted about the bad member's buffers."""
    ps = rc.BATCH_GRAD[800]
    thetas = np.stack([p.theta for p in ps])
    thetas[1, -1] = rc.BAD_MEMBER_JITTER
    gp, _ = handle(ps[0])
    try:
        vals, _ = gp.lml_grad_batch(thetas)
        assert gp.batch_info[1] > 0 and vals[1] == -np.inf
        assert gp.batch_info[0] == 0 and gp.batch_info[2] == 0
        for k in (0, 2):
            check(ps[k].name + "-beside-bad", gp, ps[k], gp._bK[k], gp._bZ[k], gp._bW[k])
    finally:
        gp.close()


def test_factor_batch_leaves_every_member():
    ps = rc.BATCH_FACTOR
    gp, _ = handle(ps[0], need_grad=False)
    try:
        assert not gp.factor_batch(np.stack([p.theta for p in ps])).any()
        for k, p in enumerate(ps):
            check(p.name, gp, p, gp._bK[k])
    finally:
        gp.close()


# ------------------------------------------------------------------------------------------ append
def test_append_extends_L_beta_and_U_in_place():
    """reserve(400), factor at n = 250 with U resident, + 5 points (n = 255), + 3 more (n = 258: np 256 -> 384, the beta row
    moves).  After each append L (with the moved beta row) and U meet their bounds against the grown conditional-form K, and
    the first n rows of L and U are bit for bit what they were."""
    from andvaranaut_amd import MiGP

    stages = rc.APPEND
    X, y, _ = rc.problem_data(stages[-1])
    n0 = stages[0].N
    gp = MiGP(X[:n0], y[:n0], stages[0].kernel, device=0, capacity=rc.APPEND_CAPACITY)
    try:
        theta = stages[0].theta
        assert gp.factor(theta) == 0
        gp.predict(theta, query_points(stages[0]), via_inverse=True)
        check(stages[0].name, gp, stages[0], gp.K_t, gp.Z_t)
        for p in stages[1:]:
            n_old, np_old = gp.n, gp.np_
            L_old, U_old = gp.K_t[:n_old, :np_old].clone(), gp.Z_t[:n_old, :n_old].clone()
            assert gp.append(X[n_old:p.N], y[n_old:p.N]) == 0
            assert gp.n == p.N and gp.append_refactors == 0
            assert bool((gp.K_t[:n_old, :np_old] == L_old).all()), (p.name, "the first n rows of L changed")
            assert bool((gp.Z_t[:n_old, :n_old] == U_old).all()), (p.name, "the leading n x n block of U changed")
            check(p.name, gp, p, gp.K_t, gp.Z_t)
        assert gp.np_ == 384
    finally:
        gp.close()
