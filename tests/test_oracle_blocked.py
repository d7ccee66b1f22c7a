"""The row-blocked oracle (oracle.gp_oracle.lml_all_blocked) against the whole-matrix one it restates, and cond2_spd against
np.linalg.cond.  The blocked form is what the large-shape GPU tests (tests/test_gpu_large_shapes.py) compare the device with
at 34-130 tile columns, where lml_grad / lml_grad_data would need ten N x N temporaries: here, at N <= 1200, every quantity
it returns must be the whole-matrix oracle's to 1e-12 per component (floor 1e-3 of the largest component)."""
import numpy as np
import pytest

from oracle import gp_oracle as orc

NAMES = ["RBF", "Matern52", "Matern32", "Exponential"]


def _close(a, b, rtol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = np.maximum(np.abs(b), 1e-3 * max(np.max(np.abs(b)), 1e-300))
    return float(np.max(np.abs(a - b) / scale)) <= rtol


def _case(N, d, kerns, ops, seed, gv=0.5, alpha=None, ls_scale=0.25):
    """A seeded problem; by default a well-conditioned one (short length scales, gv = 0.5: cond(K) of 1e1 .. 1e3), so that the
    two oracles' own forward errors (cond eps) stay below the 1e-12 the algebra is held to."""
    X, y = orc.synth_problem(N, d, seed=seed)
    rng = np.random.default_rng(seed)
    theta = orc.synth_theta(d, nkern=len(kerns), gv=gv)
    theta[: len(kerns) * d] *= rng.uniform(0.7, 1.6, len(kerns) * d) * ls_scale
    theta[len(kerns) * d : len(kerns) * d + len(kerns)] = rng.uniform(0.6, 1.8, len(kerns))
    if alpha is not None:
        theta[len(kerns) * d + len(kerns) : len(kerns) * d + 2 * len(kerns)] = alpha
    return X, y, theta


def _check(X, y, kerns, ops, theta, extra_diag=None, block=64, workers=None, predict=True):
    d = X.shape[1]
    rng = np.random.default_rng(X.shape[0])
    Xn = rng.random((37, d)) * 1.2 - 0.1
    Xg = rng.random((3, d))
    Xc = rng.random((20, d))
    kw = dict(Xnew=Xn, Xgrad=Xg, Xcov=Xc, form="conditional") if predict else {}
    b = orc.lml_all_blocked(X, y, kerns, ops, theta, extra_diag=extra_diag, block=block, workers=workers, **kw)
    ref, L, beta = orc.lml(X, y, kerns, ops, theta, form=kw.get("form", "marginal"), return_parts=True, extra_diag=extra_diag)
    assert abs(b["lml"] - ref) <= 1e-12 * abs(ref), (b["lml"], ref)
    assert abs(b["logdet"] - np.log(np.diag(L)).sum()) <= 1e-12 * abs(b["logdet"])
    assert abs(b["quad"] - beta @ beta) <= 1e-12 * abs(b["quad"])
    _, g = orc.lml_grad(X, y, kerns, ops, theta, form=kw.get("form", "marginal"), extra_diag=extra_diag)
    _, gy, gx = orc.lml_grad_data(X, y, kerns, ops, theta, form=kw.get("form", "marginal"), extra_diag=extra_diag)
    assert _close(b["grad"], g), (b["grad"], g)
    assert _close(b["gy"], gy)
    # (dLML/dx_i sums row i of W against dK/dx_i, and the terms cancel: the whole-matrix oracle's K^-1 = cho_solve(L, I) is
    # not symmetric to rounding, and its rows carry cond eps of the K^-1 entries into that sum -- 5e-12 at cond 8e2 measured)
    xtol = max(1e-12, 100.0 * orc.cond2_spd(b["L"]) * np.finfo(float).eps)
    assert _close(b["gX"], gx, xtol), np.abs(b["gX"] - gx).max()
    if predict:
        mu, var = orc.predict(X, y, Xn, kerns, ops, theta)
        assert _close(b["mu"], mu) and _close(b["var"], var)
        dmu, dvar = orc.predict_grad(X, y, Xg, kerns, ops, theta)
        assert _close(b["dmu"], dmu) and _close(b["dvar"], dvar)
        S = orc.sigma_joint(X, Xc, kerns, ops, theta, True)
        assert _close(b["cov"], S)
    return b


@pytest.mark.parametrize("kern", NAMES + ["RatQuad"])
@pytest.mark.parametrize("N,d,block", [(300, 3, 64), (517, 5, 100), (1200, 2, 256)])
def test_blocked_oracle_equals_the_whole_matrix_one_per_kernel(kern, N, d, block):
    X, y, theta = _case(N, d, [kern], [], seed=N + len(kern), alpha=1.7 if kern == "RatQuad" else None)
    _check(X, y, [kern], [], theta, block=block)


@pytest.mark.parametrize("kerns,ops", [
    (["RBF", "Matern52"], ["+"]),
    (["Matern32", "RBF"], ["*"]),
    (["Exponential", "Matern52", "RBF"], ["*", "+"]),
    (["RBF", "Matern32", "Matern52", "RBF"], ["+", "*", "*"]),
    (["Matern52", "RBF", "Exponential", "Matern32"], ["*", "+", "*"]),
])
def test_blocked_oracle_equals_the_whole_matrix_one_on_compositions(kerns, ops):
    N, d = 411, 4
    X, y, theta = _case(N, d, kerns, ops, seed=len(kerns) * 7 + len(ops[0]))
    _check(X, y, kerns, ops, theta, block=37)


def test_blocked_oracle_with_an_extra_diagonal_and_ragged_blocks():
    """extra_diag enters through K alone (the marginal form, as lml_grad takes it); blocks of 1, 7 and 1000 rows on 5 workers
    and one (the sums regroup: same values to rounding)."""
    N, d = 333, 3
    X, y, theta = _case(N, d, ["Matern52", "RBF"], ["+"], seed=5)
    diag = np.random.default_rng(1).uniform(1e-4, 5e-2, N)
    vals = [_check(X, y, ["Matern52", "RBF"], ["+"], theta, extra_diag=diag, block=blk, workers=w, predict=False)
            for blk, w in ((1, 5), (7, 1), (1000, 3))]
    xtol = max(1e-12, 100.0 * orc.cond2_spd(vals[0]["L"]) * np.finfo(float).eps)  # (see _check)
    for v in vals[1:]:
        assert _close(v["grad"], vals[0]["grad"]) and _close(v["gX"], vals[0]["gX"], xtol)


def test_blocked_oracle_predictions_from_the_marginal_factor_agree_to_rounding():
    """The default factor is the marginal form's (gv, then jitter, on the diagonal); predict's conditional form adds them the
    other way round.  The two differ by one rounding of the diagonal: far inside the GPU tests' 200 cond eps."""
    N, d = 700, 3
    X, y, theta = _case(N, d, ["Matern32"], [], seed=3)
    Xn = np.random.default_rng(2).random((50, d))
    b = orc.lml_all_blocked(X, y, ["Matern32"], [], theta, Xnew=Xn)
    mu, var = orc.predict(X, y, Xn, ["Matern32"], [], theta)
    cond = orc.cond2_spd(b["L"])
    eps = np.finfo(float).eps
    assert np.abs(b["mu"] - mu).max() <= 4 * cond * eps * max(np.abs(mu).max(), 1.0)
    assert np.abs(b["var"] - var).max() <= 4 * cond * eps * max(np.abs(var).max(), 1.0)


@pytest.mark.parametrize("N,d,kern,gv", [(200, 1, "RBF", 1e-5), (640, 3, "Matern52", 1e-3), (1000, 2, "Exponential", 1e-2),
                                         (1500, 6, "Matern32", 1e-4), (900, 1, "RatQuad", 1e-6)])
def test_cond2_spd_matches_numpy_cond(N, d, kern, gv):
    X, y, theta = _case(N, d, [kern], [], seed=N, gv=gv, ls_scale=1.0)
    K = orc.noisy_cov(X, [kern], [], theta)
    ref = np.linalg.cond(K)
    L = np.linalg.cholesky(K)
    got = orc.cond2_spd(L)
    assert abs(got - ref) <= 0.05 * ref, (got, ref)
