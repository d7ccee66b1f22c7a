"""NumPy reference of the joint GP over f and grad f (include/mi_gp_deriv.h): the covariance from the closed forms, the log marginal
likelihood, its theta gradient by the W contraction and the conditional.  Observation a = c n + i is component c (0: the value,
c >= 1: d f / d x_c) at point i; theta = [l(d), kv, alpha, gv, jitter]."""
import numpy as np

LOG_2PI = 1.8378770664093453
SQ5 = 2.23606797749979


def kders(kernel, s):
    """k and its first three derivatives by s = sum_m dl_m^2 / l_m^2 (r = sqrt(s + 1e-12) inside Matern)"""
    if kernel == "RBF":
        k = np.exp(-0.5 * s)
        return k, -0.5 * k, 0.25 * k, -0.125 * k
    if kernel != "Matern52":
        raise ValueError(kernel)
    r = np.sqrt(s + 1e-12)
    e = np.exp(-SQ5 * r)
    return (1.0 + SQ5 * r + 5.0 / 3.0 * r * r) * e, -(5.0 / 6.0) * (1.0 + SQ5 * r) * e, (25.0 / 12.0) * e, -(25.0 * SQ5 / 24.0) * e / r


def _geometry(X1, X2, theta):
    d = X1.shape[1]
    a = 1.0 / theta[:d] ** 2
    D = (X1[:, None, :] - X2[None, :, :]).transpose(2, 0, 1)  # (d, n1, n2): dl_c
    s = np.einsum("c,cij->ij", a, D * D)
    return d, a, D, s


def _join(B00, Bc0, B0c, Bcc, q1, q2):
    """the blocks in the observation layout: rows c n1 + i, columns c' n2 + j"""
    d, n1, n2 = Bc0.shape
    rows = [np.concatenate([B00] + ([B0c.transpose(1, 0, 2).reshape(n1, d * n2)] if q2 > 1 else []), axis=1)]
    if q1 > 1:
        left = Bc0.reshape(d * n1, n2)
        if q2 > 1:
            rows.append(np.concatenate([left, Bcc.transpose(0, 2, 1, 3).reshape(d * n1, d * n2)], axis=1))
        else:
            rows.append(left)
    return np.concatenate(rows, axis=0)


def cov(X1, q1, X2, q2, theta, kernel):
    """cov of the q1 components at X1 with the q2 components at X2 (each 1 or 1 + d), without any diagonal term"""
    d, a, D, s = _geometry(X1, X2, theta)
    kv = theta[d]
    k, k1, k2, _ = kders(kernel, s)
    aD = a[:, None, None] * D
    B00 = kv * k
    Bc0 = 2.0 * kv * k1[None] * aD
    B0c = -Bc0
    Bcc = -4.0 * kv * k2[None, None] * aD[:, None] * aD[None, :]
    for c in range(d):
        Bcc[c, c] -= 2.0 * kv * k1 * a[c]
    return _join(B00, Bc0, B0c, Bcc, q1, q2)


def diag_terms(n, d, theta, extra_diag=None):
    """gv + jitter on the value rows, the jitter alone on the derivative rows, the per-observation diagonal on both"""
    gv, jit = theta[d + 2], theta[d + 3]
    dg = np.full(n * (1 + d), jit)
    dg[:n] += gv
    if extra_diag is not None:
        dg = dg + extra_diag
    return dg


def train_cov(X, theta, kernel, extra_diag=None):
    n, d = X.shape
    K = cov(X, 1 + d, X, 1 + d, theta, kernel)
    K[np.diag_indices_from(K)] += diag_terms(n, d, theta, extra_diag)
    return K


def dcov_da(X, theta, kernel, p):
    """d K~ / d a_p (a_p = l_p^-2) over the joint training covariance"""
    d, a, D, s = _geometry(X, X, theta)
    kv = theta[d]
    _, k1, k2, k3 = kders(kernel, s)
    Dp2 = D[p] * D[p]
    aD = a[:, None, None] * D
    B00 = kv * k1 * Dp2
    Bc0 = 2.0 * kv * D * (k2 * Dp2)[None] * a[:, None, None]
    Bc0[p] += 2.0 * kv * D[p] * k1
    B0c = -Bc0
    Bcc = -4.0 * kv * (k3 * Dp2)[None, None] * aD[:, None] * aD[None, :]
    DD = D[:, None] * D[None, :]
    Bcc[p, :] -= 4.0 * kv * k2[None] * DD[p, :] * a[:, None, None]  # [c = p]: a_c'
    Bcc[:, p] -= 4.0 * kv * k2[None] * DD[:, p] * a[:, None, None]  # [c' = p]: a_c
    for c in range(d):
        Bcc[c, c] -= 2.0 * kv * k2 * Dp2 * a[c]
    Bcc[p, p] -= 2.0 * kv * k1
    return _join(B00, Bc0, B0c, Bcc, 1 + d, 1 + d)


def contract(X, theta, kernel, Wt, absolute=False):
    """g[p] = 1/2 sum_ab Wt_ab dK_ab/dtheta_p over the FULL symmetric Wt, p in the order l(d), kv, alpha (0), gv, jitter; with
    `absolute` also 1/2 sum_ab |Wt_ab dK_ab/dtheta_p|, the scale a rounding error of the sum is measured against"""
    n, d = X.shape
    g, ga = np.zeros(d + 4), np.zeros(d + 4)
    for p in range(d):
        T = Wt * dcov_da(X, theta, kernel, p) * (-2.0 / theta[p] ** 3)
        g[p], ga[p] = 0.5 * T.sum(), 0.5 * np.abs(T).sum()
    T = Wt * cov(X, 1 + d, X, 1 + d, theta, kernel) / theta[d]
    g[d], ga[d] = 0.5 * T.sum(), 0.5 * np.abs(T).sum()
    dw = np.diag(Wt)
    g[d + 2], ga[d + 2] = 0.5 * dw[:n].sum(), 0.5 * np.abs(dw[:n]).sum()
    g[d + 3], ga[d + 3] = 0.5 * dw.sum(), 0.5 * np.abs(dw).sum()
    return (g, ga) if absolute else g


def lml(X, yj, theta, kernel, extra_diag=None, grad=False):
    """the log marginal likelihood of the joint observations yj (and its theta gradient)"""
    K = train_cov(X, theta, kernel, extra_diag)
    L = np.linalg.cholesky(K)
    from scipy.linalg import solve_triangular

    beta = solve_triangular(L, yj, lower=True)
    val = -0.5 * beta @ beta - np.log(np.diag(L)).sum() - 0.5 * len(yj) * LOG_2PI
    if not grad:
        return val
    alpha = solve_triangular(L, beta, lower=True, trans="T")
    Li = solve_triangular(L, np.eye(len(yj)), lower=True)
    return val, contract(X, theta, kernel, np.outer(alpha, alpha) - Li.T @ Li)


def cond(X, theta, kernel, extra_diag=None):
    w = np.linalg.eigvalsh(train_cov(X, theta, kernel, extra_diag))
    return w[-1] / w[0]


def predict(X, yj, Xnew, theta, kernel, extra_diag=None, pred_noise=True):
    """mean and variance of the VALUE at Xnew"""
    from scipy.linalg import solve_triangular

    n, d = X.shape
    L = np.linalg.cholesky(train_cov(X, theta, kernel, extra_diag))
    A = solve_triangular(L, cov(Xnew, 1, X, 1 + d, theta, kernel).T, lower=True)
    beta = solve_triangular(L, yj, lower=True)
    return A.T @ beta, theta[d] - (A * A).sum(0) + (theta[d + 2] if pred_noise else 0.0)


def problem(n, d, seed, close_pair=True):
    """Points in the unit cube with one pair 1e-3 apart and one pair identical (n >= 4), values and gradients of a smooth function"""
    rng = np.random.default_rng(seed)
    X = rng.random((n, d))
    if close_pair and n >= 4:
        X[1] = X[0]
        X[3] = X[2]
        X[3, 0] += 1e-3
    w = rng.standard_normal(d)
    ph = X @ w
    y = np.sin(ph) + 0.1 * (X ** 2).sum(1)
    dY = np.cos(ph)[:, None] * w[None, :] + 0.2 * X
    return X, y, dY


def theta_for(d, kv=1.7, gv=1e-3, jitter=1e-6):
    ls = np.exp(np.linspace(np.log(0.4), np.log(1.5), d)) if d > 1 else np.array([0.4])
    return np.concatenate([ls, [kv, 1.0, gv, jitter]])
