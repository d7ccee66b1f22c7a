"""References of the sparse inducing-point bound (include/mi_gp_sparse.h), for tests/test_sgpr_host.py,
tests/test_gpu_sparse.py.  No GPU, no device library, no oracle: the kernels are restated here (the cases take their k-means++
inducing points from the package's select_inducing, plain NumPy).

  bound_ld      the B-form in np.longdouble with a hand-written Cholesky and forward substitution: F, the analytic gradient
                (the header's textbook formulas, literally) and the predictive.  THE reference of the device tests.
  bound_dense   log N(y | 0, Qff + s I) - tr(Kff - Qff) / (2 s) in fp64 through NumPy's solvers: an independent cross-check.
  exact_lml     log N(y | 0, Kff + s I) in fp64.
  device_fp64   the device's algebra restated step by step in fp64 NumPy (expansion-form r2 in the assemblies, direct form in the
                contractions, chunked sums, the rewritten dF/ds): what fp64 alone costs against bound_ld.
"""
import numpy as np

LD = np.longdouble
EPS = np.finfo(np.float64).eps
SQRT5 = 2.23606797749979
SQRT3 = 1.7320508075688772


def split(kernel):
    return kernel.replace("*", "+").split("+"), [c for c in kernel if c in "+*"]


def num_theta(kernel, d):
    nk = len(split(kernel)[0])
    return nk * d + 2 * nk + 2


def make_theta(kernel, d, ls=None, kv=1.7, alpha=2.5, gv=1e-2, jitter=1e-6):
    """[ls | kv | alpha | gv | jitter] with every component on the same length scales (default linspace(0.4, 1.5, d))"""
    nk = len(split(kernel)[0])
    ls = np.linspace(0.4, 1.5, d) if ls is None else np.asarray(ls, dtype=np.float64)
    return np.concatenate([np.tile(ls, nk), np.full(nk, kv), np.full(nk, alpha), [gv, jitter]]).astype(np.float64)


def split_theta(theta, d, nk):
    theta = np.asarray(theta)
    return theta[: nk * d].reshape(nk, d), theta[nk * d: nk * d + nk], theta[nk * d + nk: nk * d + 2 * nk], theta[-2], theta[-1]


def problem(n, d, seed):
    """X uniform in [0, 1]^d, y = sin(3 sum x) + 0.1 eps, standardised"""
    rng = np.random.default_rng(seed)
    X = rng.random((n, d))
    y = np.sin(3.0 * X.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    return np.ascontiguousarray(X), (y - y.mean()) / y.std()


def base_kernel(name, r2, alpha):
    """(k, dk/dr2, dk/dalpha) of a base kernel at scaled squared distance r2, in r2's dtype; sqrt(r2 + 1e-12) for the Matern
    and Exponential families, as everywhere in the project"""
    dt = r2.dtype.type
    zero = np.zeros_like(r2)
    if name == "RBF":
        k = np.exp(-r2 / dt(2))
        return k, -k / dt(2), zero
    if name == "RatQuad":
        a = dt(alpha)
        u = r2 / dt(2) / a
        k = np.exp(-a * np.log1p(u))
        return k, -k / (dt(1) + u) / dt(2), k * (-np.log1p(u) + u / (dt(1) + u))
    r = np.sqrt(r2 + dt(1e-12))
    if name == "Matern52":
        s5 = dt(SQRT5)
        e = np.exp(-s5 * r)
        return (dt(1) + s5 * r + dt(5) / dt(3) * r * r) * e, -(dt(5) / dt(6)) * (dt(1) + s5 * r) * e, zero
    if name == "Matern32":
        s3 = dt(SQRT3)
        e = np.exp(-s3 * r)
        return (dt(1) + s3 * r) * e, -dt(1.5) * e, zero
    if name == "Exponential":
        e = np.exp(-r / dt(2))
        return e, -dt(0.25) * e / r, zero
    raise ValueError(name)


def _r2(X1, X2, ls, dt, expansion):
    A, B = X1.astype(dt) / ls.astype(dt), X2.astype(dt) / ls.astype(dt)
    if expansion:  # the assembly's form: -2 x.z + (|x|^2 + |z|^2), clamped at 0
        return np.maximum(-dt(2) * (A @ B.T) + ((A * A).sum(1)[:, None] + (B * B).sum(1)[None, :]), dt(0))
    r2 = np.zeros((A.shape[0], B.shape[0]), dtype=dt)
    for m in range(A.shape[1]):
        df = A[:, m, None] - B[None, :, m]
        r2 += df * df
    return r2


def fold(vals, ops):
    T = vals[0]
    for c in range(1, len(vals)):
        T = T + vals[c] if ops[c - 1] == "+" else T * vals[c]
    return T


def fold_coefs(vals, ops):
    """d fold / d vals[c] of the left-to-right fold"""
    nk = len(vals)
    pref, T = [np.ones_like(vals[0])], vals[0]
    for c in range(1, nk):
        pref.append(np.ones_like(T) if ops[c - 1] == "+" else T)
        T = T + vals[c] if ops[c - 1] == "+" else T * vals[c]
    out = []
    for c in range(nk):
        coef = pref[c]
        for c2 in range(c + 1, nk):
            if ops[c2 - 1] == "*":
                coef = coef * vals[c2]
        out.append(coef)
    return out


def cov(X1, X2, kernel, theta, dt=LD, expansion=False):
    """K(X1, X2) without any diagonal term"""
    kerns, ops = split(kernel)
    ls, kv, al, _, _ = split_theta(theta, X1.shape[1], len(kerns))
    return fold([dt(kv[c]) * base_kernel(kerns[c], _r2(X1, X2, ls[c], dt, expansion), al[c])[0] for c in range(len(kerns))], ops)


def prior_diag(kernel, theta, d, dt=LD):
    """the composite prior variance (every base kernel is 1 at r = 0 up to the 1e-12 under the root, which mi_gp_predict's kdiag
    ignores too) and its derivative by every kv_c"""
    kerns, ops = split(kernel)
    _, kv, _, _, _ = split_theta(theta, d, len(kerns))
    vals = [np.asarray(dt(kv[c])) for c in range(len(kerns))]
    return fold(vals, ops), fold_coefs(vals, ops)


def contract(Wt, X1, X2, kernel, theta, dt=LD):
    """g[k] = sum_ij Wt_ij dK(X1, X2)_ij / dtheta_k over the kernel parameters (direct-form r2); the gv and jitter slots stay 0"""
    kerns, ops = split(kernel)
    nk, d = len(kerns), X1.shape[1]
    ls, kv, al, _, _ = split_theta(theta, d, nk)
    parts = [base_kernel(kerns[c], _r2(X1, X2, ls[c], dt, False), al[c]) for c in range(nk)]
    coefs = fold_coefs([dt(kv[c]) * parts[c][0] for c in range(nk)], ops)
    g = np.zeros(nk * d + 2 * nk + 2, dtype=dt)
    Wt = Wt.astype(dt)
    for c in range(nk):
        wc = Wt * coefs[c]
        g[nk * d + c] = (wc * parts[c][0]).sum()
        g[nk * d + nk + c] = (wc * dt(kv[c]) * parts[c][2]).sum()
        G = wc * dt(kv[c]) * parts[c][1]
        for m in range(d):
            df = (X1[:, m, None].astype(dt) - X2[None, :, m].astype(dt)) / dt(ls[c, m])
            g[c * d + m] = (G * df * df).sum() * (dt(-2) / dt(ls[c, m]))
    return g


# ------------------------------------------------------------------------------------------------ long-double linear algebra
def cholesky_ld(A):
    """lower Cholesky factor, column by column in A's dtype; raises on a pivot that is not positive"""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        piv = A[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not piv > 0:
            raise np.linalg.LinAlgError(f"pivot {j + 1} is not positive")
        L[j, j] = np.sqrt(piv)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def forward_ld(L, M):
    """L^-1 M by forward substitution, row by row"""
    X = np.zeros_like(M)
    for i in range(L.shape[0]):
        X[i] = (M[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


# ---------------------------------------------------------------------------------------------------------- the reference
def bound_ld(X, y, Z, kernel, theta, grad=True, Xnew=None, pred_noise=False):
    """The B-form in np.longdouble.  Returns a dict: F, grad (jitter slot 0), cond_Kuu (fp64) and, with Xnew, mean and var."""
    kerns, _ = split(kernel)
    n, d = X.shape
    m = Z.shape[0]
    nk = len(kerns)
    _, _, _, gv, jitter = split_theta(theta, d, nk)
    s = LD(gv) + LD(jitter)
    yl = y.astype(LD)
    Kuu = cov(Z, Z, kernel, theta) + LD(jitter) * np.eye(m, dtype=LD)
    Kuf = cov(Z, X, kernel, theta)
    kdiag, dkdiag = prior_diag(kernel, theta, d)
    kappa = LD(n) * kdiag
    L = cholesky_ld(Kuu)
    A = forward_ld(L, Kuf)
    Psi = A @ A.T
    v = A @ yl
    yy = yl @ yl
    Im = np.eye(m, dtype=LD)
    B = Im + Psi / s
    LB = cholesky_ld(B)
    c = forward_ld(LB, v[:, None])[:, 0] / s
    out = {"cond_Kuu": float(np.linalg.cond(Kuu.astype(np.float64)))}
    out["F"] = (-LD(n) / 2 * np.log(2 * LD(np.pi) * s) - np.log(np.diag(LB)).sum() - yy / (2 * s) + (c @ c) / 2 - kappa / (2 * s)
                + np.trace(Psi) / (2 * s))
    LBinv = forward_ld(LB, Im)
    if grad:
        Linv = forward_ld(L, Im)
        Binv = LBinv.T @ LBinv
        ah = LBinv.T @ c
        R = ((Im - Binv - np.outer(ah, ah)) @ A + np.outer(ah, yl)) / s
        T = Linv.T @ R
        Guu = -(Linv.T @ (B - 2 * Im + Binv + np.outer(ah, ah)) @ Linv) / 2
        dFds = (-LD(n) / (2 * s) + yy / (2 * s * s) + kappa / (2 * s * s) - np.trace(Psi) / (2 * s * s)
                + np.trace(Binv @ Psi) / (2 * s * s) - (v @ Binv @ v) / (s * s * s) + (ah @ Psi @ ah) / (2 * s * s))
        g = contract(T, Z, X, kernel, theta) + contract(Guu, Z, Z, kernel, theta)
        for cc in range(nk):
            g[nk * d + cc] -= LD(n) / (2 * s) * dkdiag[cc]
        g[-2] = dFds
        g[-1] = 0
        out["grad"] = g
    if Xnew is not None:
        a = forward_ld(L, cov(Z, Xnew, kernel, theta))
        b = forward_ld(LB, a)
        out["mean"] = b.T @ c
        out["var"] = kdiag - (a * a).sum(0) + (b * b).sum(0) + (s if pred_noise else 0)
    return out


def bound_dense(X, y, Z, kernel, theta):
    """log N(y | 0, Qff + s I) - tr(Kff - Qff) / (2 s) in fp64, Qff = Kfu Kuu^-1 Kuf through NumPy's solvers"""
    n, d = X.shape
    nk = len(split(kernel)[0])
    _, _, _, gv, jitter = split_theta(theta, d, nk)
    s = gv + jitter
    f8 = np.float64
    Kuu = cov(Z, Z, kernel, theta, f8) + jitter * np.eye(Z.shape[0])
    Kuf = cov(Z, X, kernel, theta, f8)
    Qff = Kuf.T @ np.linalg.solve(Kuu, Kuf)
    C = Qff + s * np.eye(n)
    sign, logdet = np.linalg.slogdet(C)
    kdiag = float(prior_diag(kernel, theta, d, f8)[0])
    return -0.5 * n * np.log(2 * np.pi) - 0.5 * logdet - 0.5 * y @ np.linalg.solve(C, y) - (n * kdiag - np.trace(Qff)) / (2 * s)


def exact_lml(X, y, kernel, theta, dt=np.float64):
    """log N(y | 0, Kff + s I), the diagonal of Kff at the prior variance"""
    n, d = X.shape
    nk = len(split(kernel)[0])
    _, _, _, gv, jitter = split_theta(theta, d, nk)
    K = cov(X, X, kernel, theta, dt)
    K[np.diag_indices(n)] = prior_diag(kernel, theta, d, dt)[0]
    L = cholesky_ld(K + (dt(gv) + dt(jitter)) * np.eye(n, dtype=dt))
    b = forward_ld(L, y.astype(dt)[:, None])[:, 0]
    return -dt(n) / 2 * np.log(2 * dt(np.pi)) - np.log(np.diag(L)).sum() - (b @ b) / 2


# ---------------------------------------------------------------------------------- the device's algebra in fp64
def device_fp64(X, y, Z, kernel, theta, chunk=None, Xnew=None, pred_noise=False):
    """csrc/api_sparse.hip step by step in fp64 NumPy: the same matrices in the same roles, the chunks' sums in chunk order"""
    import scipy.linalg as sla

    f8 = np.float64
    kerns, _ = split(kernel)
    n, d = X.shape
    m = Z.shape[0]
    nk = len(kerns)
    _, _, _, gv, jitter = split_theta(theta, d, nk)
    s = gv + jitter
    chunk = n if chunk is None else chunk
    Kuu = cov(Z, Z, kernel, theta, f8, expansion=True)
    Kuu[np.diag_indices(m)] += jitter
    L = np.linalg.cholesky(Kuu)
    Psi, v, yy = np.zeros((m, m)), np.zeros(m), 0.0
    rows = []
    for i0 in range(0, n, chunk):
        Xc, yc = X[i0:i0 + chunk], y[i0:i0 + chunk]
        At = sla.solve_triangular(L, cov(Z, Xc, kernel, theta, f8, expansion=True), lower=True).T  # A_c^T, one row per point
        rows.append((Xc, yc, At))
        Psi += At.T @ At
        v += At.T @ yc
        yy += yc @ yc
    B = np.eye(m) + Psi / s
    LB = np.linalg.cholesky(B)
    UB = sla.solve_triangular(LB, np.eye(m), lower=True).T
    c = UB.T @ (v / s)
    kdiag, dkdiag = prior_diag(kernel, theta, d, f8)
    kappa = n * float(kdiag)
    out = {"F": -0.5 * n * (np.log(2 * np.pi) + np.log(s)) - np.log(np.diag(LB)).sum() - yy / (2 * s) + 0.5 * (c @ c)
           - (kappa - np.trace(Psi)) / (2 * s)}
    ah = UB @ c
    U = sla.solve_triangular(L, np.eye(m), lower=True).T
    Binv = UB @ UB.T
    H = np.eye(m) - Binv - np.outer(ah, ah)
    G0 = Psi / s - H
    M2 = (H @ U.T) / s
    W = U @ (G0 @ U.T)  # -2 Guu
    tv = (U @ ah) / s
    g = np.zeros(nk * d + 2 * nk + 2)
    for Xc, yc, At in rows:
        g += contract(At @ M2 + np.outer(yc, tv), Xc, Z, kernel, theta, f8)
    g += contract(-0.5 * W, Z, Z, kernel, theta, f8)
    for cc in range(nk):
        g[nk * d + cc] -= n / (2 * s) * float(dkdiag[cc])
    g[-2] = (-n / (2 * s) + yy / (2 * s * s) + (kappa - np.trace(Psi)) / (2 * s * s) + (m - np.trace(Binv)) / (2 * s)
             - (c @ c + ah @ ah) / (2 * s))
    g[-1] = 0.0
    out["grad"] = g
    if Xnew is not None:
        a = sla.solve_triangular(L, cov(Z, Xnew, kernel, theta, f8, expansion=True), lower=True)
        b = sla.solve_triangular(LB, a, lower=True)
        out["mean"] = b.T @ c
        out["var"] = float(kdiag) - (a * a).sum(0) + (b * b).sum(0) + (s if pred_noise else 0.0)
    return out


# ------------------------------------------------------------------------------- the cases of tests/test_gpu_sparse.py
# (n, m, d, chunk): one tile of m with n no multiple of 64 and one chunk; two ragged tiles of m, three chunks, the last one
# short; one past a tile in both sets with d past a block of 16
SHAPES = [(300, 40, 3, None), (700, 200, 5, 256), (257, 130, 17, None)]
KERNELS = ["RBF", "Matern52", "RBF+Matern32", "Matern52*Exponential", "RatQuad"]
DEVICE_CASES = [(k,) + s + (z,) for s in SHAPES for k in KERNELS for z in ("subset", "kmeanspp")]


# length-scale factors of the cases, by kernel and then by d (None: every d); case_theta says why
LS_FACTOR = {"Matern52*Exponential": {None: 100.0}, "RBF+Matern32": {None: 2.0, 5: 4.0}}


def case_id(case):
    return "-".join(str(v) for v in case)


def case_theta(kernel, d):
    """ls = linspace(0.4, 1.5, d), kv = 1.7, gv = 1e-2, jitter = 1e-6 (alpha = 2.5 for a rational quadratic).
    Matern52*Exponential takes 100 times these length scales: the assemblies form r2 in the expansion form, which leaves a
    rounding residue of a few eps |x / l|^2 where the reference's direct form gives 0 -- on Kuu's diagonal and at every inducing
    point that is a data point -- and Exponential's sqrt(r2 + 1e-12) turns a residue of 1e-15 into 2.5e-10 of the entry.  At the
    plain length scales the fp64 restatement alone misses the tolerances by up to 30x (measured: F 2.7, gradient 31, mean 6.7,
    variance 15.6 tolerances), at 30 times it uses up to 0.53 of one, at 100 times at most 0.03.
    RBF+Matern32 takes twice the length scales, four times at d = 5: at the plain ones dF/dkv of the RBF component at
    (n, m, d) = (700, 200, 5) is 0.39, what is left of three sums of the size n / (2 s) = 3.5e4, and fp64's 3.6e-10 on it is 0.28
    of a tolerance that cond(Kuu) = 2.9e4 makes 1.3e-9 (twice: 0.25 there; four times: 0.07 there, but 0.26 at d = 17)."""
    ls = np.linspace(0.4, 1.5, d)
    f = LS_FACTOR.get(kernel, {None: 1.0})
    return make_theta(kernel, d, ls=f.get(d, f[None]) * ls)


def device_case(case):
    """(X, y, Z, theta, Xnew, chunk) of a case (kernel, n, m, d, chunk, how Z is chosen)"""
    kernel, n, m, d, chunk, zsel = case
    X, y = problem(n, d, seed=n + m)
    if zsel == "subset":  # inducing points that are data points: r2 = 0 pairs in Kuf
        Z = X[np.sort(np.random.default_rng(1).choice(n, m, replace=False))].copy()
    else:
        from andvaranaut_amd.sparse import select_inducing

        Z = select_inducing(X, m, seed=3)
    Xnew = np.random.default_rng(2).random((100, d))
    return X, y, Z, case_theta(kernel, d), Xnew, chunk


_REFERENCES = {}


def reference(case):
    """bound_ld of a case, computed once per process and shared (callers must not change it)"""
    if case not in _REFERENCES:
        X, y, Z, theta, Xnew, _ = device_case(case)
        _REFERENCES[case] = bound_ld(X, y, Z, case[0], theta, Xnew=Xnew)
    return _REFERENCES[case]


def tolerances(cond):
    """the project's rule (tests/kfold_ref.py): (F and mean, gradient entries and variance)"""
    return max(1e-10, 20.0 * cond * EPS), max(1e-10, 200.0 * cond * EPS)


def error_ratios(got, ref, cond):
    """errors of a result dict against bound_ld's, each divided by its tolerance: F and the mean relative to max(|ref|, 1), every
    gradient entry relative to max(|ref|, 1), the variance relative to the reference variance"""
    vtol, ptol = tolerances(cond)
    out = {"F": float(abs(LD(got["F"]) - ref["F"]) / max(abs(ref["F"]), 1)) / vtol}
    if "grad" in got and "grad" in ref:
        out["grad"] = float(np.max(np.abs(np.asarray(got["grad"]).astype(LD) - ref["grad"]) / np.maximum(np.abs(ref["grad"]), 1))) / ptol
    if "mean" in got and "mean" in ref:
        out["mean"] = float(np.max(np.abs(np.asarray(got["mean"]).astype(LD) - ref["mean"]) / np.maximum(np.abs(ref["mean"]), 1))) / vtol
        out["var"] = float(np.max(np.abs(np.asarray(got["var"]).astype(LD) - ref["var"]) / ref["var"])) / ptol
    return out
