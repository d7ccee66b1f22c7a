"""Host helpers of tests/test_paths_host.py and tests/test_gpu_path_sweep.py: np.longdouble restatements of the path sweep
(options 54 / 55 of mi_gp_set_option, csrc/paths_f64.hip) -- the evaluation of a path block with its element-wise bounds, the
conditioning's residual, and the whole draw of andvaranaut_amd/paths.py (features, residual, an accurate solve, the sweep).
No GPU, no library import."""
import numpy as np

import grad_refs as gr
from grad_refs import EPS, LD, TINY  # noqa: F401
from andvaranaut_amd import paths
from oracle import gp_oracle as orc

FAMILIES = ("RBF", "Matern52", "Matern32", "Exponential", "RatQuad")
SAMPLER_KERNELS = FAMILIES + ("RBF+Matern52*Matern32", "Matern52*RBF")


def header_offsets(F, d, ldw):
    """The offsets of include/mi_gp.h's option-54 paragraph, restated: Omega at 0, b at F d, W at F d + F, V at F d + F + F ldw."""
    return 0, F * d, F * d + F, F * d + F + F * ldw


def kernel_ld(X, kernel, theta, Xn):
    """k(x*_p, x_j) (M, n) in np.longdouble: r2 in the direct form from the fp64 differences and the fp64 reciprocal the device
    forms (mean_sweep_ref.mean_reference's restatement)."""
    kerns, ops = gr.split(kernel)
    d, nk = X.shape[1], len(kerns)
    ls, kv, al, _, _ = orc.split_theta(theta, d, nk)
    il = 1.0 / ls
    diffs = Xn[:, None, :] - X[None, :, :]
    comps = []
    for c in range(nk):
        df = diffs.astype(LD) * il[c].astype(LD)
        comps.append(LD(kv[c]) * orc.base_kernel(kerns[c], np.sum(df * df, axis=-1), LD(al[c])))
    return orc.combine(comps, ops)


def kernel_grad_ld(X, kernel, theta, Xn):
    """d k(x*_p, x_j) / d x*_pk (M, n, d) in np.longdouble: sum_c coef_c kv_c k_c'(r2_c) 2 (x*_k - x_jk) / l_ck^2
    (grad_refs._fold_dk, the reference of the gradient kernels)."""
    kerns, ops = gr.split(kernel)
    diffs = Xn[:, None, :] - X[None, :, :]
    g, il = gr._fold_dk(kerns, ops, theta, diffs)
    G = np.zeros(diffs.shape, dtype=LD)
    for c in range(len(kerns)):
        G += g[c][:, :, None] * diffs.astype(LD) * (LD(2.0) * il[c].astype(LD) * il[c].astype(LD))[None, None, :]
    return G


def feature_parts(omega, b, Xn):
    """(cos, sin, |b_i| + sum_u |om_iu x*_u|) of the phases b_i + om_i . x*_p, each (M, F) np.longdouble."""
    om, x = np.asarray(omega, dtype=np.float64).astype(LD), np.asarray(Xn, dtype=np.float64).astype(LD)
    ph = np.asarray(b, dtype=np.float64).astype(LD)[None, :] + x @ om.T
    return np.cos(ph), np.sin(ph), np.abs(np.asarray(b)).astype(LD)[None, :] + np.abs(x) @ np.abs(om).T


def eval_reference(X, kernel, theta, omega, b, W, V, Xn, grad=True, features_only=False):
    """The paths of a block at Xn in np.longdouble with their bounds: value (S, M), bound (S, M) and with ``grad`` gradient
    (S, M, d), bound (S, M, d).  Bound: grad_refs.sum_bound of sum |terms| over both sums, plus eps (d + 2) sum_i |W_is|
    (|b_i| + sum_u |om_iu x*_u|) for the rounding of the phase -- d + 1 roundings of the phase's own sum and the argument
    reduction's -- which cos and sin pass on with a slope of at most one; the gradient's with |om_ik| weights."""
    d = X.shape[1]
    Wl, Vl = np.asarray(W, dtype=np.float64).astype(LD), np.asarray(V, dtype=np.float64).astype(LD)
    C, Sn, phm = feature_parts(omega, b, Xn)
    val, mag = C @ Wl, np.abs(C) @ np.abs(Wl)
    phase = LD(EPS) * LD(d + 2) * (phm @ np.abs(Wl))
    if not features_only:
        K = kernel_ld(X, kernel, theta, Xn)
        val = val + K @ Vl
        mag = mag + np.abs(K) @ np.abs(Vl)
    out = [val.T, (gr.sum_bound(mag) + phase).T]
    if grad:
        S, M = Wl.shape[1], Xn.shape[0]
        g = np.zeros((S, M, d), dtype=LD)
        gb = np.zeros((S, M, d), dtype=LD)
        G = None if features_only else kernel_grad_ld(X, kernel, theta, Xn)
        om = np.asarray(omega, dtype=np.float64).astype(LD)
        for k in range(d):
            Sk = Sn * om[None, :, k]
            gk, mk = -(Sk @ Wl), np.abs(Sk) @ np.abs(Wl)
            pk = LD(EPS) * LD(d + 2) * ((phm * np.abs(om[None, :, k])) @ np.abs(Wl))
            if G is not None:
                gk = gk + G[:, :, k] @ Vl
                mk = mk + np.abs(G[:, :, k]) @ np.abs(Vl)
            g[:, :, k], gb[:, :, k] = gk.T, (gr.sum_bound(mk) + pk).T
        out += [g, gb]
    return tuple(out)


def residual_reference(X, y, omega, b, W, E):
    """R = y - Phi(X) W - E (n, S) in np.longdouble and the bound of the device's R: eval_reference's bound of Phi(X) W plus the
    two subtractions' roundings, 2 eps (|y| + |Phi W| + |E|)."""
    val, bound = eval_reference(X, "RBF", None, omega, b, W, np.zeros((X.shape[0], W.shape[1])), X, grad=False, features_only=True)
    yl, El = np.asarray(y, dtype=np.float64).astype(LD)[:, None], np.asarray(E, dtype=np.float64).astype(LD)
    R = yl - val.T - El
    return R, bound.T + LD(2.0) * LD(EPS) * (np.abs(yl) + np.abs(val.T) + np.abs(El))


def noisy_cov(X, kernel, theta, diag=None):
    """K_y, the matrix the device factorises (oracle.noisy_cov, conditional form)."""
    kerns, ops = gr.split(kernel)
    return orc.noisy_cov(X, kerns, ops, theta, form="conditional", extra_diag=diag)


def noise_part(X, kernel, theta, diag=None):
    """D = K_y - K_f (n, n) np.longdouble with K_f as the sweep forms it (kernel_ld): the noise, jitter and per-point diagonal,
    and the difference between the assembled matrix (r2 in the expansion form) and the sweep's (direct form) -- for the Matern
    and Exponential families the assembled diagonal is k at r2 + 1e-12 of a rounding residue, not of 0."""
    return noisy_cov(X, kernel, theta, diag).astype(LD) - kernel_ld(X, kernel, theta, X)


def accurate_solve(K, R):
    """K^-1 R in np.longdouble: an fp64 solve and two steps of iterative refinement with np.longdouble residuals."""
    Kl, Rl = np.asarray(K, dtype=np.float64).astype(LD), np.asarray(R).astype(LD)
    V = np.linalg.solve(K, Rl.astype(np.float64)).astype(LD)
    for _ in range(2):
        V = V + np.linalg.solve(K, (Rl - Kl @ V).astype(np.float64)).astype(LD)
    return V


def path_reference(X, y, kernel, theta, seed, S, F, Xn, precise=True):
    """The whole draw of MiGP.draw_paths(theta, S, F, seed) restated: paths.draw_block_parts' host draws, the residual, an
    accurate solve against oracle.noisy_cov and the sweep at Xn.  ``precise``: everything in np.longdouble (the reference of one
    device draw); otherwise the sums in float64 (the moments of thousands of paths).  Returns a dict: omega, b, W, E, kd, V
    (n, S), values (S, M)."""
    kerns, ops = gr.split(kernel)
    n, d = X.shape
    omega, b, W, E, kd = paths.draw_block_parts(kerns, ops, theta, d, n, S, F, seed)
    K = noisy_cov(X, kernel, theta)
    if precise:
        R, _ = residual_reference(X, y, omega, b, W, E)
        V = accurate_solve(K, R)
        values, _ = eval_reference(X, kernel, theta, omega, b, W, V.astype(np.float64), Xn, grad=False)
    else:
        R = y[:, None] - np.cos(b[None, :] + X @ omega.T) @ W - E
        V = np.linalg.solve(K, R)
        values = (np.cos(b[None, :] + Xn @ omega.T) @ W + orc.kernel_matrix(Xn, X, kerns, ops, theta) @ V).T
    return dict(omega=omega, b=b, W=W, E=E, kd=kd, V=V, values=values)


# ------------------------------------------------------------------------------------------------ the moment problem
MOMENT_KERNEL, MOMENT_N, MOMENT_D, MOMENT_F, MOMENT_S, MOMENT_DRAWS = "Matern52", 40, 2, 4096, 128, 32
MOMENT_SEEDS = tuple(7100 + i for i in range(MOMENT_DRAWS))


def moment_problem():
    """n = 40, d = 2, Matern52: (X, y, theta, the 12 test points, the oracle's posterior mean and latent variance there)."""
    X, y = orc.synth_problem(MOMENT_N, MOMENT_D, seed=21)
    theta = gr.well_conditioned_theta(MOMENT_KERNEL, MOMENT_D)
    Xt = np.random.default_rng(22).random((12, MOMENT_D))
    mu, var = orc.predict(X, y, Xt, [MOMENT_KERNEL], [], theta, pred_noise=False)
    return X, y, theta, Xt, mu, var


def moment_margins(values, mu, var):
    """values (paths, 12): (max |path mean - mu| in standard errors of the path mean, min and max of path variance / var)."""
    m, v = values.mean(axis=0), values.var(axis=0, ddof=1)
    z = np.abs(m - mu) / np.sqrt(v / values.shape[0])
    ratio = v / var
    return float(z.max()), float(ratio.min()), float(ratio.max())
