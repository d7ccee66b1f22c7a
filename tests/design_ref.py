"""References of the design call (options 56 / 57 of mi_gp_set_option, MiGP.design): the greedy integrated-variance-reduction
selection in np.longdouble on explicit posterior covariances, a float64 restatement of the device's steps (row sums of G, the
candidate column from its history) and the inputs' gap condition.  Shared by tests/test_design_host.py (CPU) and
tests/test_gpu_design.py."""
import functools

import numpy as np
import scipy.linalg as sla

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)

# (n, Mc, Mr, d, b, kernel): the issue's shapes
CASES = [
    (130, 129, 65, 3, 8, "Matern52"),
    (257, 200, 130, 5, 16, "RBF+Matern32"),
    (130, 129, 65, 17, 8, "Matern52"),
    (130, 129, 0, 3, 8, "Matern52"),
    (130, 1, 1, 3, 1, "Matern52"),
    (130, 5, 65, 3, 8, "Matern52"),
]
MIN_GAP = 1e-4  # every GPU case: the best score leads the second best by this much, relatively, at every step


def case_id(c):
    return f"n{c[0]}-Mc{c[1]}-Mr{c[2]}-d{c[3]}-b{c[4]}-{c[5]}"


def split(kernel):
    kerns, ops, cur = [], [], ""
    for ch in kernel:
        if ch in "+*":
            kerns.append(cur)
            ops.append(ch)
            cur = ""
        else:
            cur += ch
    return kerns + [cur], ops


def make_theta(kernel, d, gv=1e-3, jitter=1e-6):
    """[ls(nkern * d), kv(nkern), alpha(nkern), gv, jitter]: ls = 0.4 sqrt(d), kv = 1.3 (a second component: 0.9 of both)"""
    nk = len(split(kernel)[0])
    ls = np.concatenate([np.full(d, 0.4 * np.sqrt(d) * (0.9 ** c)) for c in range(nk)])
    kv = np.array([1.3 * (0.9 ** c) for c in range(nk)])
    return np.concatenate([ls, kv, np.ones(nk), [gv, jitter]])


@functools.lru_cache(maxsize=None)
def case_data(n, Mc, Mr, d, b, kernel, gv=1e-3, seed=None):
    """Uniform points of [0, 1]^d; the outputs enter no criterion"""
    rng = np.random.default_rng(1000 * n + 10 * Mc + d if seed is None else seed)
    X, C, R = rng.random((n, d)), rng.random((Mc, d)), rng.random((Mr, d))
    y = np.sin(X.sum(1)) + 0.03 * rng.normal(size=n)
    return dict(X=X, y=y, C=C, R=R, theta=make_theta(kernel, d, gv), kernel=kernel, b=b)


def kmat(A, B, kernel, theta, dtype=LD):
    """k(A, B) in `dtype`, r2 in the direct form"""
    kerns, ops = split(kernel)
    nk, d = len(kerns), A.shape[1]
    th = np.asarray(theta, dtype=dtype)
    A, B = np.asarray(A, dtype=dtype), np.asarray(B, dtype=dtype)
    K = None
    for c, name in enumerate(kerns):
        u = (A[:, None, :] - B[None, :, :]) * (1 / th[c * d : (c + 1) * d])
        r2 = np.sum(u * u, axis=2)
        r = np.sqrt(r2 + dtype(1e-12))
        if name == "RBF":
            k = np.exp(-r2 / 2)
        elif name == "Matern52":
            s5 = np.sqrt(dtype(5.0))
            k = (1 + s5 * r + dtype(5.0) / 3 * r * r) * np.exp(-s5 * r)
        elif name == "Matern32":
            s3 = np.sqrt(dtype(3.0))
            k = (1 + s3 * r) * np.exp(-s3 * r)
        else:
            raise ValueError(name)
        k = th[nk * d + c] * k
        K = k if K is None else K + k if ops[c - 1] == "+" else K * k
    return K


def prior_diag(kernel, theta, d):
    kerns, ops = split(kernel)
    kv = theta[len(kerns) * d : len(kerns) * d + len(kerns)]
    kd = kv[0]
    for c in range(1, len(kerns)):
        kd = kd + kv[c] if ops[c - 1] == "+" else kd * kv[c]
    return kd


def noise_of(theta, noise):
    """v - var_latent: jitter, plus gv with `noise`"""
    return theta[-1] + (theta[-2] if noise else 0.0)


def chol_ld(K):
    """lower Cholesky factor in long double, column by column"""
    L = np.array(K, dtype=LD)
    n = len(L)
    for j in range(n):
        L[j, j] = np.sqrt(L[j, j] - np.dot(L[j, :j], L[j, :j]))
        if j + 1 < n:
            L[j + 1 :, j] = (L[j + 1 :, j] - L[j + 1 :, :j] @ L[j, :j]) / L[j, j]
    return np.tril(L)


def solve_lower_ld(L, B):
    """L^-1 B in long double"""
    A = np.array(B, dtype=LD)
    for i in range(len(L)):
        A[i] = (A[i] - L[i, :i] @ A[:i]) / L[i, i]
    return A


def posterior_ld(X, C, R, kernel, theta):
    """(cov(C, C) with the prior diagonal kd, cov(C, R)) of the latent function in long double; K_y = K + (jitter + gv) I"""
    d = X.shape[1]
    Ky = kmat(X, X, kernel, theta)
    Ky[np.diag_indices(len(X))] = LD(prior_diag(kernel, theta, d)) + LD(theta[-1]) + LD(theta[-2])
    L = chol_ld(Ky)
    Ac = solve_lower_ld(L, kmat(X, C, kernel, theta))
    Kcc = kmat(C, C, kernel, theta)
    Kcc[np.diag_indices(len(C))] = LD(prior_diag(kernel, theta, d))
    Scc = Kcc - Ac.T @ Ac
    Scr = None
    if len(R):
        Scr = kmat(C, R, kernel, theta) - Ac.T @ solve_lower_ld(L, kmat(X, R, kernel, theta))
    return Scc, Scr


def greedy(Scc, Scr, b, nz):
    """The greedy selection on explicit covariances (any dtype): (indices, gains, round-0 gains, smallest relative gap between
    the best and the second-best score over the steps; inf where a step has one candidate)"""
    Scc = Scc.copy()
    Scr = None if Scr is None else Scr.copy()
    Mc = len(Scc)
    alive = np.ones(Mc, dtype=bool)
    idx, gains, gains0, gap = [], [], None, np.inf
    for _ in range(b):
        v = np.diag(Scc) + nz
        ok = alive & np.isfinite(v.astype(np.float64)) & (v > 0)
        with np.errstate(all="ignore"):
            score = np.diag(Scc).copy() if Scr is None else np.mean(Scr * Scr, axis=1) / v
        if gains0 is None:
            gains0 = np.where(ok, score, np.nan)
        if not ok.any():
            break
        cand = np.where(ok, score, -np.inf)
        p = int(np.argmax(cand))
        if not cand[p] > 0:
            break
        rest = np.delete(cand, p)
        if len(rest) and np.isfinite(float(rest.max())):
            gap = min(gap, float((cand[p] - rest.max()) / cand[p]))
        idx.append(p)
        gains.append(cand[p])
        g = Scc[:, p].copy()
        if Scr is not None:
            Scr -= np.outer(g / v[p], Scr[p])
        Scc -= np.outer(g, g) / v[p]
        alive[p] = False
    return np.array(idx, dtype=np.int64), np.array(gains), gains0, gap


@functools.lru_cache(maxsize=None)
def reference(case, noise=True, gv=1e-3, seed=None):
    """The long-double selection of a case: dict(idx, gains, gains0, min_gap), gains in long double"""
    c = case_data(*case, gv=gv, seed=seed)
    Scc, Scr = posterior_ld(c["X"], c["C"], c["R"], c["kernel"], c["theta"])
    idx, gains, gains0, gap = greedy(Scc, Scr, c["b"], LD(noise_of(c["theta"], noise)))
    return dict(idx=idx, gains=gains, gains0=gains0, min_gap=gap)


def min_gap(case, **kw):
    return reference(case, **kw)["min_gap"]


APPEND_CASE = (258, 129, 65, 3, 8, "Matern52")  # the GPU test factorises its first 250 points and appends the last 8
COINCIDENT = (130, 129, 65, 3, 8, "Matern52")
DUP = (3, 7)  # candidate 7 repeats candidate 3; candidate 5 is training point 9


@functools.lru_cache(maxsize=None)
def coincident_case():
    """gv = 0 (v = var_latent + jitter): a candidate on a training point and a repeated candidate.  The repeated pair ties exactly,
    so the gap condition is that of the candidates without the repeat."""
    c = dict(case_data(*COINCIDENT, gv=0.0, seed=77))
    C = c["C"].copy()
    C[5] = c["X"][9]
    C[DUP[1]] = C[DUP[0]]
    c["C"] = C
    Scc, Scr = posterior_ld(c["X"], C, c["R"], c["kernel"], c["theta"])
    nz = LD(noise_of(c["theta"], True))
    idx, gains, gains0, _ = greedy(Scc, Scr, c["b"], nz)
    keep = np.delete(np.arange(len(C)), DUP[1])
    gap = greedy(Scc[np.ix_(keep, keep)], Scr[keep], c["b"], nz)[3]
    c["ref"] = dict(idx=idx, gains=gains, gains0=gains0, min_gap=gap)
    return c


def device_fp64(X, C, R, kernel, theta, b, noise=True):
    """The device's steps in float64 NumPy: A = L^-1 K(X, .), G = K(C, R) - A_C^T A_R, v = kd - |a_c|^2 + noise, then per step the
    score from the rows' sums of squares, the candidate column k(C, c*) - A_C . a_c* minus the history's contributions, and the
    rank-one pass.  (indices, gains, round-0 gains)"""
    d, Mc, Mr = X.shape[1], len(C), len(R)
    f = np.float64
    Ky = kmat(X, X, kernel, theta, f)
    Ky[np.diag_indices(len(X))] = prior_diag(kernel, theta, d) + theta[-1] + theta[-2]
    L = np.linalg.cholesky(Ky)
    Ac = sla.solve_triangular(L, kmat(X, C, kernel, theta, f), lower=True)
    nz = noise_of(theta, noise)
    v = prior_diag(kernel, theta, d) - np.sum(Ac * Ac, axis=0) + nz
    G = None
    if Mr:
        G = kmat(C, R, kernel, theta, f) - Ac.T @ sla.solve_triangular(L, kmat(X, R, kernel, theta, f), lower=True)
    alive = np.ones(Mc, dtype=bool)
    hist, vs, idx, gains, gains0 = [], [], [], [], None
    for _ in range(b):
        ok = alive & np.isfinite(v) & (v > 0)
        with np.errstate(all="ignore"):
            score = v - nz if G is None else np.sum(G * G, axis=1) / (Mr * v)
        if gains0 is None:
            gains0 = np.where(ok, score, np.nan)
        cand = np.where(ok, score, -np.inf)
        p = int(np.argmax(cand))
        if not (ok.any() and cand[p] > 0):
            break
        idx.append(p)
        gains.append(cand[p])
        alive[p] = False
        g = kmat(C, C[p : p + 1], kernel, theta, f)[:, 0] - Ac.T @ Ac[:, p]
        for h, vh in zip(hist, vs):
            g = g - h * (h[p] / vh)
        hist.append(g)
        vs.append(v[p])
        if G is not None:
            G[alive] -= np.outer(g[alive] / v[p], G[p])
        v[alive] -= g[alive] * (g[alive] / v[p])
    return np.array(idx, dtype=np.int64), np.array(gains), gains0


# tests/test_gpu_design_facade.py: 40 Latin-hypercube points, 16 more in 4 rounds of 4 at a fixed theta
FACADE = dict(seed=11, n0=40, nadd=16, batch=4, ncand=256, nref=128, ls=0.25, kv=1.0, gv=1e-4, jitter=1e-6)


def facade_points(priors, cfg=FACADE):
    """(start design, the 16 further Latin-hypercube points, the fresh 500-point set)"""
    from andvaranaut_amd.lhc import latin_sample

    return (latin_sample(priors, cfg["n0"], cfg["seed"]), latin_sample(priors, cfg["nadd"], cfg["seed"] + 100),
            latin_sample(priors, 500, cfg["seed"] + 200))


def cond_ky(X, kernel, theta):
    d = X.shape[1]
    Ky = kmat(X, X, kernel, theta, np.float64)
    Ky[np.diag_indices(len(X))] = prior_diag(kernel, theta, d) + theta[-1] + theta[-2]
    return float(np.linalg.cond(Ky))


def tolerance(X, kernel, theta, gains0):
    """The project's fp64 rule: each gain within max(1e-10, 200 cond(K_y) eps) of the largest round-0 gain"""
    return max(1e-10, 200.0 * cond_ky(X, kernel, theta) * EPS) * float(np.nanmax(np.asarray(gains0, dtype=np.float64)))


def mean_latent_variance(X, R, kernel, theta):
    """mean_r var_latent(r) in long double given observations at X (with K_y's diagonal kd + jitter + gv)"""
    d = X.shape[1]
    Ky = kmat(X, X, kernel, theta)
    Ky[np.diag_indices(len(X))] = LD(prior_diag(kernel, theta, d)) + LD(theta[-1]) + LD(theta[-2])
    A = solve_lower_ld(chol_ld(Ky), kmat(X, R, kernel, theta))
    return np.mean(LD(prior_diag(kernel, theta, d)) - np.sum(A * A, axis=0))
