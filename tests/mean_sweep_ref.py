"""Host helpers of tests/test_gpu_mean_sweep.py (tested on the CPU by tests/test_mean_sweep_host.py): the case list of the
matrix-free mean sweep (option 53 of mi_gp_set_option, csrc/sweep_f64.hip), its query points, and the np.longdouble reference
of the mean -- the companion of grad_refs.predict_grad_reference, which is the gradient's reference and is used unchanged.
No GPU, no library import.

Every case runs ONE set of 1000 query points: grad_refs.predict_queries' five (a training point, a point 40 length scales
away, three in the cube) and 995 uniform ones.  The device is called with the first m of them for every m in M_VALUES.  The
np.longdouble references cost seconds per case at 1000 points (n d nkern extended-precision operations per point), so they are
formed at the 71 REF_POINTS only: all of the first 65 points (every point of the calls m = 1, 5, 63, 64, 65: every lane of a
wave and the first lane of the next), and of the larger calls both sides of the boundaries at 256 and 512, point 777 and the
last point (999).  The VALUES at the other 929 points are not checked against a reference: for them the tests show only that
they are finite and that they do not depend on m, on the position or on a repetition (bit equality between calls)."""
import functools

import numpy as np

import grad_refs as gr
from grad_refs import EPS, LD, TINY  # noqa: F401  (re-exported for the tests)
from oracle import gp_oracle as orc

EXTRA_CASES = [("RBF", 130, 128), ("Matern52+RBF", 65, 33), ("RBF", 64, 32), ("Matern52", 2500, 6)]
CASES = list(gr.PREDICT_CASES) + EXTRA_CASES
M_VALUES = (1, 5, 63, 64, 65, 257, 1000)
REF_POINTS = np.array(list(range(65)) + [255, 256, 511, 512, 777, 999])
FAMILIES = ("RBF", "Matern52", "Matern32", "Exponential", "RatQuad")


def problem(n, d, seed):
    X, y = orc.synth_problem(max(n, 3), d, seed=seed)
    return np.ascontiguousarray(X[:n]), np.ascontiguousarray(y[:n])


def queries(X, theta, d, seed):
    """The case's 1000 query points: predict_queries' five, then 995 uniform points of the cube."""
    five = gr.predict_queries(X, theta, d, seed)
    rest = np.random.default_rng(seed + 1).random((M_VALUES[-1] - five.shape[0], d))
    return np.ascontiguousarray(np.vstack([five, rest]))


def mean_reference(X, kernel, theta, Xn, alpha):
    """(sum_j alpha_j k(x*_p, x_j), sum_j |alpha_j k(x*_p, x_j)|) per query point, both (M,) np.longdouble: r2 in the direct form
    sum_m ((x*_m - x_jm) (1 / l_cm))^2 from the fp64 differences and the fp64 reciprocal the kernel forms, the oracle's
    base_kernel and its left-to-right +/* fold (the fold whose derivative is oracle._fold_coefs) in np.longdouble."""
    kerns, ops = gr.split(kernel)
    X = np.asarray(X, dtype=np.float64)
    Xn = np.asarray(Xn, dtype=np.float64)
    d, nk = X.shape[1], len(kerns)
    ls, kv, al, _, _ = orc.split_theta(theta, d, nk)
    il = 1.0 / ls
    diffs = Xn[:, None, :] - X[None, :, :]
    comps = []
    for c in range(nk):
        df = diffs.astype(LD) * il[c].astype(LD)
        r2 = np.sum(df * df, axis=-1)
        comps.append(LD(kv[c]) * orc.base_kernel(kerns[c], r2, LD(al[c])))
    terms = orc.combine(comps, ops) * np.asarray(alpha, dtype=np.float64).astype(LD)[None, :]
    return terms.sum(axis=1), np.abs(terms).sum(axis=1)


def mean_float64(X, kernel, theta, Xn, alpha, reverse=False):
    """The same sums in plain float64, j ascending (or descending with ``reverse``): (mean (M,), dmean (M, d)).  What a
    device may do at best; the host test holds it to a quarter of the bound the device is held to."""
    kerns, ops = gr.split(kernel)
    d, nk = X.shape[1], len(kerns)
    ls, kv, al, _, _ = orc.split_theta(theta, d, nk)
    il = 1.0 / ls
    order = np.arange(X.shape[0])[::-1] if reverse else np.arange(X.shape[0])
    diffs = Xn[:, None, :] - X[None, order, :]
    a = np.asarray(alpha, dtype=np.float64)[order]
    comps, dks = [], []
    for c in range(nk):
        df = diffs * il[c]
        r2 = np.sum(df * df, axis=-1)
        comps.append(kv[c] * orc.base_kernel(kerns[c], r2, al[c]))
        dks.append(kv[c] * orc.base_kernel_dr2(kerns[c], r2, al[c]))
    coefs = orc._fold_coefs(comps, ops)
    T = orc.combine(comps, ops)
    mean = np.zeros(Xn.shape[0])
    dmean = np.zeros((Xn.shape[0], d))
    w = np.zeros((Xn.shape[0], X.shape[0], d))
    for c in range(nk):
        w += ((coefs[c] * dks[c]) * a[None, :])[:, :, None] * (2.0 * il[c] * il[c])[None, None, :]
    w *= diffs
    for j in range(X.shape[0]):  # a sequential sum, as a thread of the kernel runs it
        mean += T[:, j] * a[j]
        dmean += w[:, j, :]
    return mean, dmean


@functools.lru_cache(maxsize=None)
def case_data(kernel, n, d):
    """Everything a case needs, computed once per process and not changed afterwards: the problem, theta, the 1000 queries,
    alpha_reference's (alpha, cond, ok, ratio) measured at REF_POINTS, and the references (mu, |mu| terms, dmu, |dmu| terms) at
    REF_POINTS."""
    X, y = problem(n, d, seed=7 * n + d)
    theta = gr.well_conditioned_theta(kernel, d)
    Xn = queries(X, theta, d, seed=n + d)
    Xr = np.ascontiguousarray(Xn[REF_POINTS])
    alpha, cond, ok, ratio = gr.alpha_reference(X, y, kernel, theta, Xr)
    mu, mag_mu = mean_reference(X, kernel, theta, Xr, alpha)
    dmu, mag_dmu = gr.predict_grad_reference(X, kernel, theta, Xr, alpha)
    for arr in (X, y, theta, Xn, Xr, alpha, mu, mag_mu, dmu, mag_dmu):
        arr.setflags(write=False)
    return dict(X=X, y=y, theta=theta, Xn=Xn, Xr=Xr, alpha=alpha, cond=cond, ok=bool(ok), alpha_ratio=ratio, mu=mu, mag_mu=mag_mu,
                dmu=dmu, mag_dmu=mag_dmu)


def bounds(case):
    """grad_refs.sum_bound with alpha's own forward error: (64 + 8 cond) eps sum |terms| + one subnormal quantum, for mu and d mu."""
    extra = 8.0 * case["cond"]
    return gr.sum_bound(case["mag_mu"], extra=extra), gr.sum_bound(case["mag_dmu"], extra=extra)


def families(kernel):
    return set(gr.split(kernel)[0])
