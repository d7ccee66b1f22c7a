"""The sparse bound's gradients by the data on the device (include/mi_gp_sparse_data.h, MiSparseGP(data_grad=True)) against the
long-double dF/dy and dF/dX of tests/sgpr_data_grad_ref.py.

The tolerance is the project's gradient rule with cond = cond(Kuu) (sgpr_ref.tolerances): every entry within
max(1e-10, 200 cond eps) of max(|ref|, 1).  tests/test_sgpr_data_grad_host.py holds the CPU half: fp64 alone on the device's steps
uses at most 0.114 of it on dF/dX and 0.034 on dF/dy over the 30 cases.  Every case prints its ratios."""
import numpy as np
import pytest

import sgpr_data_grad_ref as DR
import sgpr_ref as R

pytestmark = pytest.mark.gpu

FOUR = "RBF+Matern52*Matern32+RatQuad"  # tests/test_gpu_sparse_zgrad.py's four components, at twice the plain length scales


def _sparse(X, y, Z, kernel, **kw):
    from andvaranaut_amd.sparse import MiSparseGP

    return MiSparseGP(X, y, Z, kernel, device=0, **kw)


def _same(a, b):
    return all((x is None and z is None) or np.array_equal(x, z) for x, z in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("case", DR.CASES, ids=R.case_id)
def test_gradients_by_the_data_against_long_double(case):
    X, y, Z, theta, _, chunk = DR.device_case(case)
    ref = DR.case_reference(case)
    sp = _sparse(X, y, Z, case[0], chunk=chunk, z_grad=True, data_grad=True)
    plain = _sparse(X, y, Z, case[0], chunk=chunk, z_grad=True)
    try:
        F, g, gy, gx, gz = sp.lml_grad_data(theta, want_z=True)
        assert sp.info == 0 and gy.shape == y.shape and gx.shape == X.shape and gz.shape == Z.shape
        ry, rx = DR.ratios(gy, gx, ref)
        print(R.case_id(case), "cond(Kuu) = %.2e" % ref["cond_Kuu"], "dF/dy ratio %.4f, dF/dX ratio %.4f" % (ry, rx))
        assert ry <= 1.0 and rx <= 1.0, (ry, rx)
        # the bound and its gradients by theta and Z are bit for bit those of an object without the data-side gradients
        F0, g0, gz0 = plain.lml_grad_z(theta)
        assert F == F0 and np.array_equal(g, g0) and np.array_equal(gz, gz0)
        assert _same(sp.lml_grad_z(theta), (F0, g0, gz0)) and _same(sp.lml_grad(theta), (F0, g0)) and sp.bound(theta) == F0
        # dF/dy alone: the same bits, and no dF/dX
        F1, g1, gy1, gx1 = sp.lml_grad_data(theta, want_x=False)
        assert gx1 is None and F1 == F and np.array_equal(g1, g) and np.array_equal(gy1, gy)
        with pytest.raises(ValueError, match="data_grad"):
            plain.lml_grad_data(theta)
    finally:
        sp.close()
        plain.close()


@pytest.mark.parametrize("kernel", ["RBF", "RBF+Matern32", FOUR])
def test_slab_counts_agree_within_the_tolerance_and_a_repeated_call_returns_the_same_bits(kernel):
    """(n, m, d, chunk) = (700, 200, 5, 256): four column blocks of Z against four, four and three row blocks of the chunks.
    xgrad_slabs = 1: one slab walks every block of Z; 2: two blocks per slab; the default: one block per slab."""
    case = (kernel, 700, 200, 5, 256, "subset")
    X, y, Z, theta, _, chunk = DR.device_case(case)
    if kernel == FOUR:
        theta = R.make_theta(kernel, 5, ls=2.0 * np.linspace(0.4, 1.5, 5))
    ref = DR.reference(X, y, Z, kernel, theta, ("slabs", kernel))
    ptol = R.tolerances(ref["cond_Kuu"])[1]
    out = []
    for slabs in (1, 2, None):
        sp = _sparse(X, y, Z, kernel, chunk=chunk, data_grad=True, xgrad_slabs=slabs)
        try:
            first = sp.lml_grad_data(theta)
            again = sp.lml_grad_data(theta)
        finally:
            sp.close()
        assert _same(first, again)
        ry, rx = DR.ratios(first[2], first[3], ref)
        print(kernel, "xgrad_slabs =", slabs, "cond(Kuu) = %.2e" % ref["cond_Kuu"], "dF/dy ratio %.4f, dF/dX ratio %.4f" % (ry, rx))
        assert ry <= 1.0 and rx <= 1.0, (slabs, ry, rx)
        out.append(first)
    for F, g, gy, gx in out[1:]:
        assert _same((F, g, gy), out[0][:3])  # the slabs regroup dF/dX's sums alone
        assert np.all(np.abs(gx - out[0][3]) <= ptol * np.maximum(np.abs(out[0][3]), 1.0))


def test_more_than_128_dimensions_take_two_windows():
    """d = 130 (n = 200, m = 70, RBF, four times the plain length scales: tests/test_gpu_sparse_zgrad.py's case).  Measured on
    the CPU: cond(Kuu) = 78, max |dF/dX| = 6.3 in the columns from 128 on, the fp64 restatement uses 0.007 of the tolerance."""
    n, m, d = 200, 70, 130
    X, y = R.problem(n, d, seed=n + m)
    Z = X[np.sort(np.random.default_rng(1).choice(n, m, replace=False))].copy()
    theta = R.make_theta("RBF", d, ls=4.0 * np.linspace(0.4, 1.5, d))
    ref = DR.reference(X, y, Z, "RBF", theta, "window")
    assert float(np.max(np.abs(ref["grad_x"][:, 128:]))) > 1.0  # the second window has something to get wrong
    sp = _sparse(X, y, Z, "RBF", data_grad=True)
    try:
        _, _, gy, gx = sp.lml_grad_data(theta)
    finally:
        sp.close()
    ry, rx = DR.ratios(gy, gx, ref)
    print("d = 130: cond(Kuu) = %.2e" % ref["cond_Kuu"], "dF/dy ratio %.4f, dF/dX ratio %.4f" % (ry, rx))
    assert ry <= 1.0 and rx <= 1.0, (ry, rx)


def test_a_bad_pivot_zeroes_the_gradients_by_the_data_and_the_object_stays_usable():
    """tests/test_gpu_sparse.py's case: rows 5 and 9 of Z are one point and jitter = 0, so pivot 10 of Kuu is not positive -- a
    numerical refusal, no device fault."""
    kernel, n, m, d = "Matern52", 300, 40, 3
    X, y = R.problem(n, d, seed=21)
    Z = X[:m].copy()
    Z[9] = Z[5]
    good = R.case_theta(kernel, d)
    bad = good.copy()
    bad[-1] = 0.0
    sp = _sparse(X, y, Z, kernel, z_grad=True, data_grad=True)
    fresh = _sparse(X, y, Z, kernel, z_grad=True, data_grad=True)
    try:
        one = sp.lml_grad_data(good, want_z=True)
        assert sp.info == 0 and one[2].any() and one[3].any()
        F, g, gy, gx, gz = sp.lml_grad_data(bad, want_z=True)
        assert sp.info == 10, sp.info
        assert F == -np.inf and not g.any() and not gy.any() and not gx.any() and not gz.any()
        assert gy.shape == (n,) and gx.shape == (n, d) and gz.shape == (m, d)
        # the library itself has zeroed the bound outputs
        assert not sp.gy_t.cpu().numpy().any() and not sp.gx_t.cpu().numpy().any()
        two = sp.lml_grad_data(good, want_z=True)
        assert sp.info == 0 and _same(two, fresh.lml_grad_data(good, want_z=True)) and _same(two, one)
    finally:
        sp.close()
        fresh.close()


def test_moved_data_and_inducing_points_give_the_bits_of_a_fresh_object_and_unbinding_restores_the_plain_call():
    kernel, n, m, d = "Matern52", 300, 40, 3
    X, y = R.problem(n, d, seed=21)
    Z = X[:m].copy()
    theta = R.case_theta(kernel, d)
    rng = np.random.default_rng(8)
    X2, y2, Z2 = X + 0.01 * rng.standard_normal(X.shape), y + 0.05 * rng.standard_normal(n), X[m:2 * m] + 0.02
    sp = _sparse(X, y, Z, kernel, z_grad=True, data_grad=True)
    fresh = _sparse(X2, y2, Z2, kernel, z_grad=True, data_grad=True)
    plain = _sparse(X2, y2, Z2, kernel, z_grad=True)
    try:
        before = sp.lml_grad_data(theta, want_z=True)
        sp.update_data(X=X2, y=y2)
        sp.set_inducing(Z2)
        after = sp.lml_grad_data(theta, want_z=True)
        assert _same(after, fresh.lml_grad_data(theta, want_z=True)) and not np.array_equal(after[3], before[3])
        # non-finite data are not uploaded: -inf and zeros until the next finite update, which restores the bits
        ybad = y2.copy()
        ybad[3] = np.nan
        sp.update_data(y=ybad)
        F, g, gy, gx = sp.lml_grad_data(theta)
        assert F == -np.inf and not g.any() and not gy.any() and not gx.any() and sp.bound(theta) == -np.inf
        sp.update_data(y=y2)
        assert _same(sp.lml_grad_data(theta, want_z=True), after)
        # unbinding through the library: the outputs are left alone and the gradient call is the plain one
        sp.gy_t.fill_(7.0)
        sp.gx_t.fill_(7.0)
        assert sp.lib.mi_gp_sparse_bind_data_grad(sp.h, None, None, 1) == 0
        assert _same(sp.lml_grad_z(theta), plain.lml_grad_z(theta))
        assert bool((sp.gy_t == 7.0).all()) and bool((sp.gx_t == 7.0).all())
        # a value-only call writes nothing either, bound or not
        assert sp.lib.mi_gp_sparse_bind_data_grad(sp.h, sp.gy_t.data_ptr(), sp.gx_t.data_ptr(), 1024) == 0
        assert sp.bound(theta) == after[0]
        assert bool((sp.gy_t == 7.0).all()) and bool((sp.gx_t == 7.0).all())
        assert _same(sp.lml_grad_data(theta, want_z=True), after)
        with pytest.raises(ValueError, match="keep its shape"):
            sp.update_data(X=X2[:-1])
    finally:
        sp.close()
        fresh.close()
        plain.close()
