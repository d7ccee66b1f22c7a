"""Sparse inducing-point GP regression for data sets whose n x n covariance one card cannot hold: Titsias' collapsed
variational bound (SGPR) over m << n inducing points, its exact theta gradient and the sparse predictive, streamed over the data
in chunks by libmi_gp_sparse.so (include/mi_gp_sparse.h).

The reference has no counterpart: "Sparse regression for large datasets" is an open item of its to-do list."""
import ctypes

import numpy as np
import torch

from . import _lib
from .backend import parse_kernel

MAX_INDUCING = 2048
DEFAULT_CHUNK = 8192
DEFAULT_ZGRAD_SLABS = 1024  # no cap of its own: the library's rule (row blocks of the chunk, 1024 workgroups, 64 MB) decides


def select_inducing(X, m, seed=None):
    """m distinct rows of X (converted inputs) by k-means++ seeding: the first uniformly, every further one with probability
    proportional to its squared distance to the nearest row chosen so far (D^2 sampling).  Plain NumPy, O(n m d).  Rows that
    coincide with a chosen one have distance 0 and are never drawn; with fewer than m distinct rows a ValueError is raised."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("X must be (n, d)")
    n = X.shape[0]
    m = int(m)
    if not 1 <= m <= n:
        raise ValueError(f"1 <= m <= n = {n} is required, got m = {m}")
    rng = np.random.default_rng(seed)
    idx = np.empty(m, dtype=np.int64)
    idx[0] = rng.integers(n)
    d2 = ((X - X[idx[0]]) ** 2).sum(axis=1)
    for k in range(1, m):
        total = d2.sum()
        if not total > 0.0:
            raise ValueError(f"X has only {k} distinct rows, {m} inducing points were asked for")
        idx[k] = rng.choice(n, p=d2 / total)
        d2 = np.minimum(d2, ((X - X[idx[k]]) ** 2).sum(axis=1))
        d2[idx[k]] = 0.0
    return np.ascontiguousarray(X[idx])


class MiSparseGP:
    """One data set, one set of inducing points and one kernel structure bound to one MI355X: the bound F(theta) <= LML, its
    gradient and the sparse predictive.  lml_grad has MiGP.lml_grad's signature, so HyperModel.logp_dlogp takes it unchanged.
    ``z_grad=True`` adds the exact gradient of the bound by the inducing locations: lml_grad_z returns (F, dF/dtheta, dF/dZ),
    set_inducing moves Z (lml_grad still returns (F, dF/dtheta) alone).  ``zgrad_slabs`` caps the slabs per chunk of its kernel
    (None: the library's rule); another count regroups sums, the same count returns the same bits."""

    def __init__(self, X, y, Z, kernel="RBF", device=0, chunk=None, z_grad=False, zgrad_slabs=None):
        if not torch.cuda.is_available():
            raise RuntimeError("MiSparseGP needs a ROCm GPU: the GP hot path has no CPU implementation")
        self.lib = _lib.load_sparse()
        X = np.ascontiguousarray(X, dtype=np.float64)
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
        Z = np.ascontiguousarray(Z, dtype=np.float64)
        if X.ndim != 2 or X.shape[0] != y.shape[0]:
            raise ValueError("X must be (n,d) and y (n,)")
        if Z.ndim != 2 or Z.shape[1] != X.shape[1]:
            raise ValueError("Z must be (m,d)")
        if not (np.isfinite(X).all() and np.isfinite(y).all() and np.isfinite(Z).all()):
            raise ValueError("X, y and Z must be finite")  # (the device exp clamps its argument: see MiGP.__init__)
        self.n, self.d = X.shape
        self.m = Z.shape[0]
        if not 1 <= self.m <= min(self.n, MAX_INDUCING):
            raise ValueError(f"1 <= m <= min(n, {MAX_INDUCING}) inducing points are supported, got m = {self.m}, n = {self.n}")
        self.kerns, self.ops = parse_kernel(kernel)
        self.nkern = len(self.kerns)
        self.ntheta = self.nkern * self.d + 2 * self.nkern + 2
        self.device = int(device)
        self.dev = torch.device("cuda", self.device)
        padded_n = (self.n + 127) // 128 * 128
        self.chunk = min(DEFAULT_CHUNK, padded_n) if chunk is None else int(chunk)
        if self.chunk <= 0 or self.chunk % 128:
            raise ValueError(f"chunk must be a positive multiple of 128, got {chunk}")
        cfg = _lib.MiGpSparseConfig()
        cfg.n, cfg.m, cfg.d, cfg.nkern = self.n, self.m, self.d, self.nkern
        for i, k in enumerate(self.kerns):
            cfg.kernel_ids[i] = _lib.KERNEL_IDS[k]
        for i, o in enumerate(self.ops):
            cfg.ops[i] = _lib.OP_IDS[o]
        cfg.device, cfg.chunk = self.device, self.chunk
        self.z_grad = bool(z_grad)
        if zgrad_slabs is not None and (not self.z_grad or int(zgrad_slabs) < 1):
            raise ValueError(f"zgrad_slabs needs z_grad=True and a count >= 1, got {zgrad_slabs}")
        cfg.zgrad_slabs = (DEFAULT_ZGRAD_SLABS if zgrad_slabs is None else int(zgrad_slabs)) if self.z_grad else 0
        h = ctypes.c_void_p()
        r = self.lib.mi_gp_sparse_create(ctypes.byref(cfg), ctypes.byref(h))
        if r != 0:
            raise RuntimeError(f"mi_gp_sparse_create failed ({r}): {self.lib.mi_gp_sparse_last_error(None).decode()}")
        self.h = h
        self.info = 0
        self._factored_theta = None
        self.work_len = int(self.lib.mi_gp_sparse_work(self.m, self.chunk))
        with torch.cuda.device(self.dev):
            self.X_t = torch.from_numpy(X).to(self.dev)
            self.y_t = torch.from_numpy(y).to(self.dev)
            self.Z_t = torch.from_numpy(Z).to(self.dev)
            self.work_t = torch.empty(self.work_len, dtype=torch.float64, device=self.dev)
            torch.cuda.synchronize(self.dev)
        self._bind()

    def _bind(self):
        self._factored_theta = None
        self._check(self.lib.mi_gp_sparse_set_data(self.h, self.X_t.data_ptr(), self.y_t.data_ptr(), self.n, self.Z_t.data_ptr(),
                                                   self.work_t.data_ptr(), self.work_len), "mi_gp_sparse_set_data")

    def set_inducing(self, Z):
        """Moves the inducing points: Z (m, d), converted inputs, is copied into the device buffer the library reads, the buffers
        are bound again (which resets the library's factored state and allocates nothing) and the predictive's state is dropped."""
        Z = np.ascontiguousarray(Z, dtype=np.float64)
        if Z.shape != (self.m, self.d) or not np.isfinite(Z).all():
            raise ValueError(f"Z must be a finite ({self.m}, {self.d}) array")
        with torch.cuda.device(self.dev):
            self.Z_t.copy_(torch.from_numpy(Z))
            torch.cuda.synchronize(self.dev)
        self._bind()

    def _check(self, r, what):
        if r < 0:
            raise RuntimeError(f"{what} failed ({r}): {self.lib.mi_gp_sparse_last_error(self.h).decode()}")
        return r

    def _theta(self, theta):
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if theta.shape != (self.ntheta,):
            raise ValueError(f"theta must have {self.ntheta} entries")
        return theta, theta.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def bound(self, theta):
        """F(theta): pass 1 alone.  -inf if Kuu or B is not positive definite (self.info > 0: the pivot, m + pivot for B)."""
        theta, tp = self._theta(theta)
        out = ctypes.c_double()
        self._factored_theta = None
        self.info = self._check(self.lib.mi_gp_sparse_bound_grad(self.h, tp, ctypes.byref(out), None), "mi_gp_sparse_bound_grad")
        return out.value

    def lml_grad(self, theta):
        """(F, dF/dtheta) at natural-scale theta, the jitter slot 0; (-inf, zeros) on a bad pivot."""
        F, grad = self._bound_grad(theta)
        return F, grad[: self.ntheta].copy() if self.z_grad else grad

    def lml_grad_z(self, theta):
        """(F, dF/dtheta, dF/dZ as an (m, d) array) at natural-scale theta and the current inducing points (z_grad=True);
        (-inf, zeros, zeros) on a bad pivot."""
        if not self.z_grad:
            raise ValueError("lml_grad_z needs MiSparseGP(..., z_grad=True)")
        F, grad = self._bound_grad(theta)
        return F, grad[: self.ntheta].copy(), grad[self.ntheta:].reshape(self.m, self.d).copy()

    def _bound_grad(self, theta):
        theta, tp = self._theta(theta)
        out = ctypes.c_double()
        grad = np.zeros(self.ntheta + (self.m * self.d if self.z_grad else 0))
        self._factored_theta = None
        self.info = self._check(self.lib.mi_gp_sparse_bound_grad(self.h, tp, ctypes.byref(out),
                                                                 grad.ctypes.data_as(ctypes.POINTER(ctypes.c_double))),
                                "mi_gp_sparse_bound_grad")
        return out.value, grad

    def factor(self, theta):
        """The state of the predictive at theta; returns the bad-pivot word (0: fine)."""
        theta, tp = self._theta(theta)
        self._factored_theta = None
        self.info = self._check(self.lib.mi_gp_sparse_factor(self.h, tp), "mi_gp_sparse_factor")
        if self.info == 0:
            self._factored_theta = theta.copy()
        return self.info

    def predict(self, theta, Xnew, pred_noise=True):
        """Sparse predictive mean and variance at Xnew (converted inputs)."""
        theta, _ = self._theta(theta)
        if self._factored_theta is None or not np.array_equal(self._factored_theta, theta):
            if self.factor(theta) != 0:
                raise np.linalg.LinAlgError(f"the sparse factorisation failed at pivot {self.info}")
        Xnew = np.ascontiguousarray(Xnew, dtype=np.float64)
        if Xnew.ndim != 2 or Xnew.shape[1] != self.d:
            raise ValueError("Xnew must be (m, d)")
        mq = Xnew.shape[0]
        with torch.cuda.device(self.dev):
            xn = torch.from_numpy(Xnew).to(self.dev)
            mu_t = torch.empty(mq, dtype=torch.float64, device=self.dev)
            var_t = torch.empty(mq, dtype=torch.float64, device=self.dev)
            torch.cuda.synchronize(self.dev)
            self._check(self.lib.mi_gp_sparse_predict(self.h, xn.data_ptr(), mq, mu_t.data_ptr(), var_t.data_ptr(),
                                                      1 if pred_noise else 0), "mi_gp_sparse_predict")
            return mu_t.cpu().numpy(), var_t.cpu().numpy()

    def last_error(self):
        return self.lib.mi_gp_sparse_last_error(self.h).decode()

    def close(self):
        if getattr(self, "h", None) is not None:
            self.lib.mi_gp_sparse_destroy(self.h)
            self.h = None
        self.X_t = self.y_t = self.Z_t = self.work_t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
