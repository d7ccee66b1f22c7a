"""Posterior sample paths by pathwise conditioning (Wilson et al. 2020, "Efficiently sampling functions from Gaussian process
posteriors"): a draw is a prior function draw from random Fourier features of the kernel's spectral measure plus a kernel-weighted
update, one weight per training point,

    f_s(x*) = sum_i W[i,s] cos(om_i . x* + b_i) + sum_j k(x*, x_j) V[j,s],      V[:,s] = K_y^-1 (y - prior_s(X) - eps_s),

with eps_s ~ N(0, K_y - K_f).  The host side, plain NumPy: the spectral samplers, the layout of the device's path block (options
54 / 55 of mi_gp_set_option, include/mi_gp.h) and the draw order.  ``PathDraw`` is what ``MiGP.draw_paths`` returns: a consistent
function that the device sweeps matrix-free over any points, in any number of calls, with its input gradient."""
import numpy as np

MAX_PATHS = 128      # option 54
MAX_D = 32           # the register windows of csrc/paths_f64.hip
TILE_VALUE = 16      # paths a thread carries without the gradient (PATH_TILE_VALUE)


def path_window(d):
    """The register window that runs for d <= 32 dimensions: 4, 16 or 32."""
    return 4 if d <= 4 else 16 if d <= 16 else 32


def path_tile(d, grad):
    """T, the paths a thread of csrc/paths_f64.hip carries: 16 without the gradient, 8 / 2 / 1 with it for the window 4 / 16 / 32."""
    return TILE_VALUE if not grad else {4: 8, 16: 2, 32: 1}[path_window(d)]


def check_counts(npaths, nfeatures):
    npaths, nfeatures = int(npaths), int(nfeatures)
    if not 1 <= npaths <= MAX_PATHS:
        raise ValueError(f"npaths must be 1..{MAX_PATHS}, got {npaths}")
    if not 16 <= nfeatures <= 65536 or nfeatures % 16:
        raise ValueError(f"nfeatures must be a multiple of 16 in 16..65536, got {nfeatures}")
    return npaths, nfeatures


def block_ldw(npaths):
    """The row stride of W and V that draw_paths uses: npaths rounded up to an even number."""
    return int(npaths) + (int(npaths) & 1)


def block_offsets(F, d, ldw, n):
    """Offsets (in doubles) of the parts of a path block, the formulas of include/mi_gp.h: Omega [F][d] at 0, b [F] at F d,
    W [F][ldw] at F d + F, V [n][ldw] at F d + F + F ldw; "len" is the block's length."""
    F, d, ldw, n = int(F), int(d), int(ldw), int(n)
    off = {"omega": 0, "b": F * d, "W": F * d + F, "V": F * d + F + F * ldw}
    off["len"] = off["V"] + n * ldw
    return off


def pack_block(omega, b, W, V, ldw):
    """The path block of Omega (F, d), b (F,), W (F, S) and V (n, S) as one float64 array; the padding columns hold zeros."""
    F, d = omega.shape
    n, S = V.shape
    off = block_offsets(F, d, ldw, n)
    blk = np.zeros(off["len"])
    blk[: F * d] = np.asarray(omega, dtype=np.float64).ravel()
    blk[off["b"] : off["W"]] = b
    blk[off["W"] : off["V"]].reshape(F, ldw)[:, :S] = W
    blk[off["V"] :].reshape(n, ldw)[:, :S] = V
    return blk


def unpack_block(blk, F, d, ldw, n, S):
    """(Omega, b, W, V) views of a block."""
    off = block_offsets(F, d, ldw, n)
    return (blk[: F * d].reshape(F, d), blk[off["b"] : off["W"]], blk[off["W"] : off["V"]].reshape(F, ldw)[:, :S],
            blk[off["V"] : off["len"]].reshape(n, ldw)[:, :S])


def _component_frequencies(name, l, alpha, F, rng):
    """F frequencies of one component's spectral measure, in the kernel forms of csrc/migp_math.h (r2 scaled by 1 / l): first
    z ~ N(0, I) of shape (F, d), then the family's mixing variable of shape (F,)."""
    l = np.asarray(l, dtype=np.float64)
    z = rng.standard_normal((F, l.shape[0])) / l[None, :]
    if name == "RBF":  # exp(-r2 / 2): Gaussian
        return z
    if name in ("Matern52", "Matern32", "Exponential"):  # multivariate t with 2 nu degrees of freedom
        nu2 = {"Matern52": 5.0, "Matern32": 3.0, "Exponential": 1.0}[name]
        g = rng.chisquare(nu2, F)
        om = z / np.sqrt(g / nu2)[:, None]
        return 0.5 * om if name == "Exponential" else om  # (k = exp(-r / 2) is the nu = 1/2 form at twice the length scale)
    if name == "RatQuad":  # a Gamma(alpha, scale 1 / alpha) mixture of Gaussians
        tau = rng.gamma(float(alpha), 1.0 / float(alpha), F)
        return z * np.sqrt(tau)[:, None]
    raise ValueError(f"unknown kernel {name!r}")


def spectral_frequencies(kerns, ops, ls, kv, alpha, F, rng):
    """F frequencies Omega (F, d) of the composite kernel's spectral measure and its prior variance kd, so that
    kd E[cos(om . (x - x'))] = k(x, x').  Per component, in the kernel forms of csrc/migp_math.h, with z ~ N(0, I): RBF
    om = z / l; Matern52 / Matern32 om = (z / l) / sqrt(g / 2 nu), g ~ chi2(2 nu); Exponential (k = exp(-r / 2)) the nu = 1/2 form with its frequencies halved;
    RatQuad om = (z / l) sqrt(tau), tau ~ Gamma(alpha, scale 1 / alpha).  The left-to-right fold, with T the fold so far and
    ``mass`` its total variance: '+' takes a frequency from T with probability mass / (mass + kv_c), else from component c, and
    sets mass += kv_c; '*' adds the two frequency draws and sets mass *= kv_c.  Draws from ``rng`` in component order: the
    component's z, its mixing variable, then (from the second component on, under '+') F uniforms."""
    ls = np.atleast_2d(np.asarray(ls, dtype=np.float64))
    kv = np.atleast_1d(np.asarray(kv, dtype=np.float64))
    alpha = np.ones_like(kv) if alpha is None else np.atleast_1d(np.asarray(alpha, dtype=np.float64))
    F = int(F)
    om = _component_frequencies(kerns[0], ls[0], alpha[0], F, rng)
    mass = float(kv[0])
    for c in range(1, len(kerns)):
        oc = _component_frequencies(kerns[c], ls[c], alpha[c], F, rng)
        if ops[c - 1] == "+":
            keep = rng.random(F) < mass / (mass + float(kv[c]))
            om = np.where(keep[:, None], om, oc)
            mass += float(kv[c])
        elif ops[c - 1] == "*":
            om = om + oc
            mass *= float(kv[c])
        else:
            raise ValueError(f"unknown operator {ops[c - 1]!r}")
    return np.ascontiguousarray(om), mass


def draw_block_parts(kerns, ops, theta, d, n, S, F, seed, diag=None):
    """The host draws of one block from np.random.Generator(np.random.Philox(seed)), in this order: Omega
    (spectral_frequencies), b ~ U[0, 2 pi) (F,), W = sqrt(2 kd / F) N(0, 1) (F, S), E = sqrt(gv + jitter + diag_j) N(0, 1) (n, S).
    Returns (Omega, b, W, E, kd).  The same seed gives the same block."""
    nk = len(kerns)
    theta = np.asarray(theta, dtype=np.float64)
    ls = theta[: nk * d].reshape(nk, d)
    kv = theta[nk * d : nk * d + nk]
    alpha = theta[nk * d + nk : nk * d + 2 * nk]
    gv, jitter = theta[nk * d + 2 * nk], theta[nk * d + 2 * nk + 1]
    rng = np.random.Generator(np.random.Philox(seed))
    omega, kd = spectral_frequencies(kerns, ops, ls, kv, alpha, F, rng)
    b = rng.random(F) * (2.0 * np.pi)
    W = np.sqrt(2.0 * kd / F) * rng.standard_normal((F, S))
    nv = np.full(n, gv + jitter) if diag is None else gv + jitter + np.asarray(diag, dtype=np.float64).reshape(-1)
    E = np.sqrt(nv)[:, None] * rng.standard_normal((n, S))
    return omega, b, W, E, kd


class PathDraw:
    """S posterior sample paths of one MiGP at one factorisation: the device block (Omega, b, W, V), S, F, ldw, the seed and the
    factorisation serial it was conditioned on.  ``evaluate`` sweeps the paths over any points; it raises RuntimeError once the
    MiGP has been factored again, appended to, given other data or closed -- the weights V belong to the factorisation that made
    them."""

    def __init__(self, gp, block, npaths, nfeatures, ldw, seed, serial):
        self.gp, self.block = gp, block
        self.npaths, self.nfeatures, self.ldw, self.seed, self.serial = npaths, nfeatures, ldw, seed, serial
        self.n, self.d = gp.n, gp.d

    def _live(self):
        if self.block is None:
            raise RuntimeError("this PathDraw was closed")
        if getattr(self.gp, "h", None) is None:
            raise RuntimeError("the MiGP of this PathDraw was closed")
        if self.gp._path_serial != self.serial:
            raise RuntimeError("the MiGP was factored, appended to or given other data since these paths were drawn: draw again")

    def host_block(self):
        """The block as the device holds it: (Omega (F, d), b (F,), W (F, S), V (n, S)) host copies."""
        self._live()
        blk = self.block.cpu().numpy()
        return tuple(np.array(a) for a in unpack_block(blk, self.nfeatures, self.d, self.ldw, self.n, self.npaths))

    def evaluate(self, Xnew, grad=False, chunk=1 << 20):
        """The paths at Xnew (M, d), converted inputs: values (S, M), and with ``grad`` (values, gradients (S, M, d)) w.r.t. the
        points.  The bits of a path at a point do not depend on the other points, on the other paths, on ``grad`` or on ``chunk``
        (a pass holds at most 2^26 output doubles)."""
        import torch

        self._live()
        gp, S, d = self.gp, self.npaths, self.d
        Xnew = np.ascontiguousarray(Xnew, dtype=np.float64)
        if Xnew.ndim != 2 or Xnew.shape[1] != d:
            raise ValueError("Xnew must be (m, d)")
        m = Xnew.shape[0]
        per = S * (1 + d if grad else 1)
        chunk = max(1, min(int(chunk), (1 << 26) // per))
        val = np.empty((S, m))
        dval = np.empty((S, m, d)) if grad else None
        gp.set_option(55, self.nfeatures)
        gp.set_option(54, S)
        try:
            with torch.cuda.device(gp.dev):
                for s in range(0, m, chunk):
                    mc = min(chunk, m - s)
                    nout = mc * per
                    pinned = mc * per <= gp.PINNED_IO_MAX_POINTS * (1 + d)
                    if pinned:  # (pinned I/O as in mean_sweep)
                        io = gp._pinned_io(mc * d + nout)
                        io_np = io.numpy()
                        io_np[: mc * d] = Xnew[s : s + mc].ravel()
                        x_p = io.data_ptr()
                        o_p = x_p + 8 * mc * d
                    else:
                        xn = torch.from_numpy(Xnew[s : s + mc]).to(gp.dev)
                        out = torch.empty(nout, dtype=torch.float64, device=gp.dev)
                        torch.cuda.synchronize(gp.dev)
                        x_p, o_p = xn.data_ptr(), out.data_ptr()
                    gp._check(gp.lib.mi_gp_predict_grad(gp.h, x_p, mc, self.block.data_ptr(), self.ldw, o_p, None, 0,
                                                        o_p + 8 * S * mc if grad else None, None), "mi_gp_predict_grad")
                    o = io_np[mc * d : mc * d + nout] if pinned else out.cpu().numpy()
                    val[:, s : s + mc] = o[: S * mc].reshape(S, mc)
                    if grad:
                        dval[:, s : s + mc] = o[S * mc :].reshape(S, mc, d)
        finally:
            gp.set_option(54, 0)
        return (val, dval) if grad else val

    def close(self):
        self.block = None
