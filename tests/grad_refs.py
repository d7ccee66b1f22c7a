"""Host helpers of tests/test_gpu_grad_instantiations.py (tested on the CPU by tests/test_grad_refs_host.py): the launchers'
selection rule of csrc/grad_predict.hip restated, the case lists that pin every instantiation of the three gradient
kernels, and cond-free references of their sums in np.longdouble / 40-digit mpmath.  No GPU, no library import."""
import math
import os
import re

import numpy as np

from oracle import gp_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "andvaranaut_amd", "csrc", "grad_predict.hip")
EPS = np.finfo(np.float64).eps
TINY = 5e-324
LD = np.longdouble
NK_SLOTS = ("1", "2", "3", "4", "8")   # the NK of slot 0 .. 4
GX_WINDOWS = ("1", "2", "8")           # the NCH of column 0 .. 2


def split(kernel):
    return kernel.replace("*", "+").split("+"), [c for c in kernel if c in "+*"]


# ------------------------------------------------------------------------------------- the launchers' selection rule
def nk_slot(nk):
    return nk - 1 if nk <= 4 else 4


def has_ratquad(kerns):
    return any(k == "RatQuad" for k in kerns)


def contract_entry(kernel):
    kerns, _ = split(kernel)
    return nk_slot(len(kerns)), int(has_ratquad(kerns))


def grad_x_entry(kernel, d):
    kerns, _ = split(kernel)
    return nk_slot(len(kerns)), 0 if d <= 16 else 1 if d <= 32 else 2


def predict_entry(kernel):
    return (nk_slot(len(split(kernel)[0])),)


def table_shapes(text=None):
    """The declared extents of the three dispatch tables, read from the source text of grad_predict.hip."""
    if text is None:
        with open(SOURCE) as f:
            text = f.read()
    out = {}
    for name in ("GRAD_CONTRACT_KERNELS", "GRAD_X_KERNELS", "PREDICT_GRAD_KERNELS"):
        decl = re.findall(r"\b" + name + r"((?:\[\d+\])+)\s*=", text)
        assert len(decl) == 1, (name, decl)
        out[name] = tuple(int(v) for v in re.findall(r"\d+", decl[0]))
    return out


# ------------------------------------------------------------------------------------------------------ case lists
# Rational quadratics stand first, in the middle and last (dal[c] / al[c] are indexed by position), with + and with * on
# either side; five, six, seven and eight components all go through the <8> instantiations.
K5 = "RBF+Matern52*Matern32+Exponential*RBF"
K5Q = "Matern52*RatQuad+RBF*Matern32+Exponential"
K6 = "Matern32+RBF*Matern52+Exponential*RBF+Matern52"
K6Q = "RatQuad*RBF+Matern52*RatQuad+Matern32*Exponential"
K7 = "RBF*Matern52+Matern32+Exponential*RBF+Matern52*Matern32"
K7Q = "RBF+Matern52*Matern32+RatQuad*Exponential+RBF*Matern52"
K8 = "RBF+Matern52*Matern32+Exponential*RBF+Matern52*Matern32+Exponential"
K8Q = "Matern52*RBF+Matern32*Exponential+RBF*Matern52+Matern32+RatQuad"

# grad_contract_kernel through mi_gp_grad_contract_block: (kernel, d), n = 130 (three 64-row tiles, the last of 2 rows);
# d crosses the 32-dimension LDS chunk and the `staged` shortcut of one component with d <= 32
CONTRACT_N = 130
CONTRACT_CASES = [
    ("RBF", 32), ("Matern52", 33), ("RatQuad", 1), ("RatQuad", 65),
    ("Exponential+Matern32", 33), ("RatQuad*RBF", 32), ("Matern52+RatQuad", 1),
    ("RBF*Matern52+Matern32", 65), ("Matern32+RatQuad*Exponential", 33), ("RBF*RatQuad+Matern52", 1),
    ("RBF+Matern52*Matern32+Exponential", 32), ("RatQuad+RBF*Matern32*RatQuad", 33),
    (K5, 33), (K6Q, 1), (K7Q, 32), (K8, 65), (K8Q, 1),
]

# grad_x_kernel through the handle: (kernel, n, d).  Every table entry at n = 130 (grad_x_splits = 3: gx_reduce_kernel runs)
# with a d of its window column; every slot once at n = 1 and once at n = 65; d = 129 takes two windows, the second one
# dimension wide.
GRAD_X_CASES = [
    ("RBF", 130, 3), ("Matern52", 130, 17), ("RatQuad", 130, 129), ("Exponential", 1, 16), ("Matern32", 65, 33), ("RBF", 64, 32),
    ("RBF+Matern52", 130, 16), ("Matern32*RatQuad", 130, 32), ("RatQuad+Exponential", 130, 33), ("RBF*Matern52", 1, 3),
    ("Matern52+RBF", 65, 17), ("Matern32*RatQuad", 130, 129),
    ("Matern32*RBF+Matern52", 130, 16), ("RBF+Matern52*RatQuad", 130, 17), ("RatQuad*Matern52+RBF", 130, 129),
    ("RBF+RBF*Matern32", 1, 33), ("Exponential*Matern52+RBF", 65, 3),
    ("RBF+Matern52*Matern32+RatQuad", 130, 3), ("RBF*Matern52+Matern32*Exponential", 130, 32),
    ("RatQuad*RBF+Matern52+Matern32", 130, 33), ("RBF+Matern52*Matern32+Exponential", 1, 17),
    ("Matern52*RBF*Matern32+RBF", 65, 16),
    (K5, 130, 16), (K6Q, 130, 17), (K7, 130, 129), (K8Q, 130, 33), (K8, 1, 3), (K5Q, 65, 32), (K6, 64, 3), (K7Q, 130, 3),
    (K8, 130, 32),
]

# predict_grad_kernel: (kernel, n, d); n around the 256-thread stride, d around the 16-dimension register chunks.  d var is checked
# in every case (the device's own w rows); d mu where the oracle's alpha is as accurate as its bound assumes (alpha_reference_ok).
# RBF*RBF at n = 257: every term of the far query underflows, over a strided row loop.
K6N = "Matern32+RBF*Matern52+RatQuad*RBF+Matern52"
K7N = "RBF+Matern52*Matern32+RatQuad*Matern32+RBF*Matern52"
K8N = "Matern52*RBF+Matern32*RatQuad+RBF*Matern52+Matern32+RatQuad"
PREDICT_CASES = [
    ("RBF", 1, 16), ("Matern52", 600, 1), ("Matern32", 257, 17), ("Exponential", 257, 17),
    ("RatQuad*Matern32", 255, 17), ("Exponential+RBF", 257, 1), ("RBF*RBF", 257, 17),
    ("RBF+RatQuad*Matern52", 257, 40), ("RBF+Exponential*Matern52", 257, 40),
    ("RatQuad+RBF*Matern52+Matern32", 600, 16),
    (K5Q, 255, 1), (K6N, 257, 17), (K7N, 600, 40), (K7Q, 600, 40), (K8, 600, 1), (K8, 257, 16), (K8N, 255, 40), (K8N, 1, 16),
]


def case_id(case):
    return "-".join(str(v) for v in case)


def well_conditioned_theta(kernel, d):
    """synth_theta with gv = 0.3, kv = 1, the length scales times sqrt(max(d, 2) / 2) and alpha = 1.7 for a rational quadratic:
    cond of the noisy covariance stays below ~1e3 at the sizes used here."""
    kerns, _ = split(kernel)
    nk = len(kerns)
    th = orc.synth_theta(d, nkern=nk, kv=1.0, gv=0.3)
    th[: nk * d] *= math.sqrt(max(d, 2) / 2.0)
    for c, k in enumerate(kerns):
        if k == "RatQuad":
            th[nk * d + nk + c] = 1.7
    return th


def predict_queries(X, theta, d, seed):
    """Five query points: a training point (r2 = 0 exactly), one 40 length scales from the centre of the cube (the scaled
    distance of every component is 40: exp(-r2 / 2) underflows), three inside the cube."""
    ls = theta[:d]  # (the components share their length scales in synth_theta)
    far = 0.5 + 40.0 * ls / math.sqrt(d)
    inside = np.random.default_rng(seed).random((3, d))
    return np.ascontiguousarray(np.vstack([X[min(3, X.shape[0] - 1)], far, inside]))


# --------------------------------------------------------------------- longdouble references of the two data-side sums
def _fold_dk(kerns, ops, theta, diffs):
    """g = sum-ready factors of dK/dx: for differences diffs[..., m] = x_m - x'_m (fp64, any leading shape) returns the list
    over components of (coef_c kv_c k_c'(r2_c)) in np.longdouble and the components' 1 / l (fp64, as the kernels form it).
    r2 in the direct form sum_m ((x_m - x'_m) (1 / l_m))^2; the fold coefficients are oracle._fold_coefs'."""
    d = diffs.shape[-1]
    nk = len(kerns)
    ls, kv, alpha, _, _ = orc.split_theta(theta, d, nk)
    il = 1.0 / ls  # fp64: the kernels' own reciprocal
    comps, dks = [], []
    for c in range(nk):
        df = diffs.astype(LD) * il[c].astype(LD)
        r2 = np.sum(df * df, axis=-1)
        comps.append(LD(kv[c]) * orc.base_kernel(kerns[c], r2, LD(alpha[c])))
        dks.append(LD(kv[c]) * orc.base_kernel_dr2(kerns[c], r2, LD(alpha[c])))
    coefs = orc._fold_coefs(comps, ops)
    return [coefs[c] * dks[c] for c in range(nk)], il


def _contract(weights, kerns, ops, theta, diffs):
    """S[p, m] = sum_i weights[p, i] sum_c coef_c kv_c k_c'(r2_c) 2 diffs[p, i, m] / l_cm^2 in np.longdouble, and the sum of the
    absolute values of the same terms: both (P, d) np.longdouble."""
    g, il = _fold_dk(kerns, ops, theta, diffs)
    P, _, d = diffs.shape
    ref = np.zeros((P, d), dtype=LD)
    mag = np.zeros((P, d), dtype=LD)
    for c in range(len(kerns)):
        G = weights * g[c]
        for m in range(d):
            t = G * diffs[:, :, m].astype(LD) * (LD(2.0) * LD(il[c, m]) * LD(il[c, m]))
            ref[:, m] += t.sum(axis=1)
            mag[:, m] += np.abs(t).sum(axis=1)
    return ref, mag


def grad_x_reference(X, kernel, theta, Kinv, alpha):
    """gX_ref[i, m] = sum_j (alpha_i alpha_j - Kinv_ij) dK_ij/dx_im with dK_ij/dx_im = sum_c coef_c kv_c k_c'(r2_c)
    2 (x_im - x_jm) / l_cm^2, in np.longdouble from the given K^-1 (symmetric, full) and alpha; and the sum of the absolute
    values of the same terms.  Returns (gX_ref, abs_sum), both (n, d) np.longdouble."""
    kerns, ops = split(kernel)
    X = np.asarray(X, dtype=np.float64)
    a = np.asarray(alpha, dtype=np.float64).astype(LD)
    Wm = np.outer(a, a) - np.asarray(Kinv, dtype=np.float64).astype(LD)
    return _contract(Wm, kerns, ops, theta, X[:, None, :] - X[None, :, :])


def predict_grad_reference(X, kernel, theta, Xn, weights):
    """S[p, m] = sum_i weights[p, i] dk(x_i, x*_p)/dx*_pm in np.longdouble, dk/dx*_m = sum_c coef_c kv_c k_c'(r2_c)
    2 (x*_m - x_im) / l_cm^2, and the sum of the absolute values of the same terms: d mu with weights = alpha (one row,
    broadcast), d var with weights = -2 w_p.  Returns (S, abs_sum), both (M, d) np.longdouble."""
    kerns, ops = split(kernel)
    X = np.asarray(X, dtype=np.float64)
    Xn = np.asarray(Xn, dtype=np.float64)
    w = np.broadcast_to(np.asarray(weights, dtype=np.float64), (Xn.shape[0], X.shape[0])).astype(LD)
    return _contract(w, kerns, ops, theta, Xn[:, None, :] - X[None, :, :])


def alpha_reference(X, y, kernel, theta, Xn):
    """alpha from a host solve of the oracle's conditional-form covariance K, cond(K), and whether that alpha deserves the
    8 cond eps sum |terms| its d mu bound allows.  The oracle, like the device, forms the diagonal's r2_ii in the expansion
    form, where it is a rounding residue of a few eps |x / l|^2 and not 0; Exponential's dk/dr2 = -0.25 / r = -2.5e5 at r2 = 0
    turns that into ~1e-10 of the diagonal (nothing at d = 1, where -2 x^2 + (x^2 + x^2) is exact), independently on the two
    sides, and alpha inherits it.  Measured here: d mu moves by sum_i (alpha - alpha_0)_i dk_i/dx* when the diagonal is replaced
    by its value at r2_ii = 0 (alpha_0).  ok: that is at most HALF the allowance -- the device's residue is another of the
    same size.  Returns (alpha, cond, ok, the largest ratio of the move to the allowance)."""
    kerns, ops = split(kernel)
    d = X.shape[1]
    nk = len(kerns)
    _, kv, al, gv, jitter = orc.split_theta(theta, d, nk)
    K = orc.noisy_cov(X, kerns, ops, theta, form="conditional")
    cond = float(np.linalg.cond(K))
    alpha = np.linalg.solve(K, y)
    kd = kv[0] * orc.base_kernel(kerns[0], 0.0, al[0])
    for c in range(1, nk):
        kc = kv[c] * orc.base_kernel(kerns[c], 0.0, al[c])
        kd = kd + kc if ops[c - 1] == "+" else kd * kc
    K0 = K.copy()
    K0[np.diag_indices_from(K0)] = (kd + jitter) + np.sqrt(gv) ** 2
    move, _ = predict_grad_reference(X, kernel, theta, Xn, alpha - np.linalg.solve(K0, y))
    _, mag = predict_grad_reference(X, kernel, theta, Xn, alpha)
    ratio = float(np.max(np.abs(move) / (LD(8.0 * cond) * LD(EPS) * mag + LD(TINY))))
    return alpha, cond, ratio <= 0.5, ratio


def sum_bound(mag, extra=0.0):
    """(64 + extra) eps sum |terms| + one subnormal quantum (the output format's own resolution), np.longdouble."""
    return (LD(64.0) + LD(extra)) * LD(EPS) * mag + LD(TINY)


def max_ratio(got, ref, bound):
    """max |got - ref| / bound, as a float (inf for a non-finite result)."""
    got = np.asarray(got, dtype=np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float(np.max(np.abs(got.astype(LD) - ref) / bound))


# -------------------------------------------------------------------------------- 40-digit truths of the derivatives
def dk_truth(name, r2, alpha):
    """oracle.base_kernel_dr2's formulas in 40-digit mpmath, the 1e-12 under the root and Exponential's division by r
    included.  Returns (k', |exp argument| -- alpha for RatQuad --, the factor that multiplies exp(-argument) in k' -- 1 for
    RatQuad), all mpf."""
    import mpmath as mp

    mp.mp.dps = 40
    r2 = mp.mpf(float(r2))
    if name == "RBF":
        return -mp.exp(-r2 / 2) / 2, r2 / 2, mp.mpf(0.5)
    if name == "RatQuad":
        a = mp.mpf(float(alpha))
        return -mp.power(1 + r2 / 2 / a, -a - 1) / 2, a, mp.mpf(1)
    r = mp.sqrt(r2 + mp.mpf(1e-12))
    if name == "Matern52":
        s5 = mp.mpf(2.23606797749979)
        pre = mp.mpf(5.0 / 6.0) * (1 + s5 * r)
        return -pre * mp.exp(-s5 * r), s5 * r, pre
    if name == "Matern32":
        s3 = mp.mpf(1.7320508075688772)
        return -mp.mpf(1.5) * mp.exp(-s3 * r), s3 * r, mp.mpf(1.5)
    if name == "Exponential":
        pre = mp.mpf(0.25) / r
        return -pre * mp.exp(-r / 2), r / 2, pre
    raise ValueError(name)


def k_truth(name, r2, alpha):
    """oracle.base_kernel's formulas in 40-digit mpmath (mpf): the value, 1 - O(sqrt(1e-12)) at r2 = 0 for the Matern and
    Exponential families.  r2: a float, or an mpf taken as it is."""
    import mpmath as mp

    mp.mp.dps = 40
    r2 = r2 if isinstance(r2, mp.mpf) else mp.mpf(float(r2))
    if name == "RBF":
        return mp.exp(-r2 / 2)
    if name == "RatQuad":
        a = mp.mpf(float(alpha))
        return mp.power(1 + r2 / 2 / a, -a)
    r = mp.sqrt(r2 + mp.mpf(1e-12))
    if name == "Matern52":
        s5 = mp.mpf(2.23606797749979)
        return (1 + s5 * r + mp.mpf(5.0 / 3.0) * r * r) * mp.exp(-s5 * r)
    if name == "Matern32":
        s3 = mp.mpf(1.7320508075688772)
        return (1 + s3 * r) * mp.exp(-s3 * r)
    if name == "Exponential":
        return mp.exp(-r / 2)
    raise ValueError(name)


def ratquad_dalpha_truth(r2, alpha):
    """RatQuad's dk/dalpha = k (-log1p(u) + u / (1 + u)), u = r2 / (2 alpha), in 40-digit mpmath; and the size of the two
    terms that cancel, k (log1p(u) + u / (1 + u)).  Both mpf."""
    import mpmath as mp

    mp.mp.dps = 40
    r2, a = mp.mpf(float(r2)), mp.mpf(float(alpha))
    u = r2 / 2 / a
    k = mp.power(1 + u, -a)
    return k * (-mp.log1p(u) + u / (1 + u)), k * (mp.log1p(u) + u / (1 + u))
