"""Global sensitivity analysis from evaluations of a surrogate: active subspaces and derivative-based measures from gradients,
variance-based (Sobol) indices from a Saltelli design.  Pure NumPy: the evaluations come from elsewhere -- GPMCMC.predict_mean,
the matrix-free sweep of the posterior mean (MiGP.mean_sweep), or any other function."""
import numpy as np


def active_subspace_from_gradients(G, weights=None):
    """The active subspace of a gradient sample (Constantine 2015): C = sum_i w_i g_i g_i^T / sum_i w_i from the rows g_i of G
    (N, d), uniform weights by default.  Returns (eigenvalues (d,) in descending order, eigenvectors (d, d) in the columns, each
    with its largest component positive, C (d, d), dgsm (d,) = diag C -- the derivative-based global sensitivity measures
    nu_m = E[(df/dx_m)^2] of Sobol & Kucherenko 2009)."""
    G = np.asarray(G, dtype=np.float64)
    if G.ndim != 2 or G.shape[0] < 1:
        raise ValueError("G must be (N, d) with N >= 1")
    if not np.isfinite(G).all():
        raise ValueError("G must be finite")
    if weights is None:
        w = np.ones(G.shape[0])
    else:
        w = np.asarray(weights, dtype=np.float64).reshape(-1)
        if w.shape[0] != G.shape[0] or not np.isfinite(w).all() or (w < 0).any() or not w.sum() > 0:
            raise ValueError("weights must be N finite non-negative numbers with a positive sum")
    C = (G * w[:, None]).T @ G / w.sum()
    C = 0.5 * (C + C.T)
    lam, V = np.linalg.eigh(C)
    lam, V = lam[::-1].copy(), V[:, ::-1].copy()
    lam[lam < 0.0] = 0.0  # (rounding of a semi-definite matrix)
    big = np.argmax(np.abs(V), axis=0)
    V *= np.where(V[big, np.arange(V.shape[1])] < 0.0, -1.0, 1.0)[None, :]
    return lam, V, C, np.diag(C).copy()


def saltelli_design(A, B):
    """The (d + 2) M points of Saltelli's design from two independent base samples A, B (M, d): the rows of A, the rows of B, then
    for m = 0 .. d - 1 the rows of A with column m taken from B (AB_m)."""
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    if A.ndim != 2 or A.shape != B.shape:
        raise ValueError("A and B must be (M, d) arrays of one shape")
    M, d = A.shape
    out = np.empty(((d + 2) * M, d))
    out[:M] = A
    out[M : 2 * M] = B
    for m in range(d):
        blk = out[(2 + m) * M : (3 + m) * M]
        blk[:] = A
        blk[:, m] = B[:, m]
    return out


def split_saltelli(f, d):
    """The evaluations of a saltelli_design, in its order, as (fA (M,), fB (M,), fAB (d, M))."""
    f = np.asarray(f, dtype=np.float64).reshape(-1)
    if f.shape[0] % (d + 2) != 0:
        raise ValueError("the evaluations of a Saltelli design number (d + 2) M")
    M = f.shape[0] // (d + 2)
    return f[:M], f[M : 2 * M], f[2 * M :].reshape(d, M)


def sobol_from_evaluations(fA, fB, fAB):
    """First-order and total Sobol indices from the evaluations of a Saltelli design: fA, fB (M,), fAB (d, M) with row m the
    evaluations at AB_m.  First order by Saltelli et al. 2010 (table 2, b): V_m = mean(fB (fAB_m - fA)); total by Jansen 1999:
    VT_m = mean((fA - fAB_m)^2) / 2; both over the variance of the pooled fA, fB.  Returns (first (d,), total (d,), mean, var)."""
    fA = np.asarray(fA, dtype=np.float64).reshape(-1)
    fB = np.asarray(fB, dtype=np.float64).reshape(-1)
    fAB = np.atleast_2d(np.asarray(fAB, dtype=np.float64))
    if fA.shape != fB.shape or fAB.shape[1] != fA.shape[0]:
        raise ValueError("fA and fB must be (M,) and fAB (d, M)")
    pooled = np.concatenate([fA, fB])
    mean, var = float(pooled.mean()), float(pooled.var())
    if not var > 0.0:
        raise ValueError("the evaluations do not vary: the indices are undefined")
    first = np.mean(fB[None, :] * (fAB - fA[None, :]), axis=1) / var
    total = 0.5 * np.mean((fA[None, :] - fAB) ** 2, axis=1) / var
    return first, total, mean, var
