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
DEFAULT_XGRAD_SLABS = 1024  # likewise for dF/dX (column blocks of m, 1024 workgroups, 64 MB)


def select_inducing(X, m, seed=None, return_index=False):
    """m distinct rows of X (converted inputs) by k-means++ seeding: the first uniformly, every further one with probability
    proportional to its squared distance to the nearest row chosen so far (D^2 sampling).  Plain NumPy, O(n m d).  Rows that
    coincide with a chosen one have distance 0 and are never drawn; with fewer than m distinct rows a ValueError is raised.
    ``return_index=True`` returns (rows, their indices into X)."""
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
    rows = np.ascontiguousarray(X[idx])
    return (rows, idx) if return_index else rows


class MiSparseGP:
    """One data set, one set of inducing points and one kernel structure bound to one MI355X: the bound F(theta) <= LML, its
    gradient and the sparse predictive.  lml_grad has MiGP.lml_grad's signature, so HyperModel.logp_dlogp takes it unchanged.
    ``z_grad=True`` adds the exact gradient of the bound by the inducing locations: lml_grad_z returns (F, dF/dtheta, dF/dZ),
    set_inducing moves Z (lml_grad still returns (F, dF/dtheta) alone).  ``zgrad_slabs`` caps the slabs per chunk of its kernel
    (None: the library's rule); another count regroups sums, the same count returns the same bits.
    ``data_grad=True`` adds the gradients of the bound by the data (include/mi_gp_sparse_data.h; the object then runs on
    libmi_gp_sparse_data.so, the same code with one entry point more): lml_grad_data returns (F, dF/dtheta, dF/dy, dF/dX), which
    is MiGP.lml_grad_data's shape, and update_data overwrites the resident data in place -- what warps fitted with the
    hyper-parameters need.  ``xgrad_slabs`` caps the slabs of dF/dX's kernel as zgrad_slabs does for dF/dZ's.  Without data_grad
    every call returns the bits it returns without the argument."""

    def __init__(self, X, y, Z, kernel="RBF", device=0, chunk=None, z_grad=False, zgrad_slabs=None, data_grad=False,
                 xgrad_slabs=None):
        if not torch.cuda.is_available():
            raise RuntimeError("MiSparseGP needs a ROCm GPU: the GP hot path has no CPU implementation")
        self.data_grad = bool(data_grad)
        if xgrad_slabs is not None and (not self.data_grad or int(xgrad_slabs) < 1):
            raise ValueError(f"xgrad_slabs needs data_grad=True and a count >= 1, got {xgrad_slabs}")
        self.xgrad_slabs = DEFAULT_XGRAD_SLABS if xgrad_slabs is None else int(xgrad_slabs)
        self.lib = _lib.load_sparse_data() if self.data_grad else _lib.load_sparse()
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
            self.gy_t = self.gx_t = None
            if self.data_grad:
                self.gy_t = torch.zeros(self.n, dtype=torch.float64, device=self.dev)
                self.gx_t = torch.zeros((self.n, self.d), dtype=torch.float64, device=self.dev)
            torch.cuda.synchronize(self.dev)
        self._bad_X = self._bad_y = False
        self._bound_x = None  # whether dF/dX is bound beside dF/dy (None: nothing is bound)
        self._bind()
        if self.data_grad:
            self._bind_data_grad(True)

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

    def _bind_data_grad(self, want_x):
        """dF/dy's output and, with want_x, dF/dX's behind every later gradient call (None: unbound)"""
        if self._bound_x is not want_x:
            gy = None if want_x is None else self.gy_t.data_ptr()
            gx = self.gx_t.data_ptr() if want_x else None
            self._check(self.lib.mi_gp_sparse_bind_data_grad(self.h, gy, gx, self.xgrad_slabs), "mi_gp_sparse_bind_data_grad")
            self._bound_x = want_x

    def update_data(self, X=None, y=None):
        """Overwrites the resident inputs / outputs in place (same shapes) and binds the buffers again, as MiGP.update_data does
        for the dense handle and by its rule for non-finite data: a non-finite array is not uploaded, and until a finite one
        replaces it lml_grad, lml_grad_z, lml_grad_data and bound return -inf (zero gradients) like a bad pivot."""
        if X is not None:
            self._bad_X = not np.isfinite(np.asarray(X, dtype=np.float64)).all()
            if self._bad_X:
                X = None
        if y is not None:
            self._bad_y = not np.isfinite(np.asarray(y, dtype=np.float64)).all()
            if self._bad_y:
                y = None
        if X is None and y is None:
            self._factored_theta = None
            return
        with torch.cuda.device(self.dev):
            if X is not None:
                X = np.ascontiguousarray(X, dtype=np.float64)
                if X.shape != (self.n, self.d):
                    raise ValueError("X must keep its shape")
                self.X_t.copy_(torch.from_numpy(X))
            if y is not None:
                y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
                if y.shape != (self.n,):
                    raise ValueError("y must keep its shape")
                self.y_t.copy_(torch.from_numpy(y))
            torch.cuda.synchronize(self.dev)
        self._bind()

    def _bad_data(self):
        return self._bad_X or self._bad_y

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
        if self._bad_data():
            return -np.inf
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

    def lml_grad_data(self, theta, want_x=True, want_z=False):
        """(F, dF/dtheta, dF/dy, dF/dX or None[, dF/dZ with want_z]) at natural-scale theta (data_grad=True; want_z needs
        z_grad=True): MiGP.lml_grad_data's shape.  want_x=False binds dF/dy alone, so dF/dX's kernel does not run.
        (-inf, zeros, ...) on a bad pivot or non-finite data."""
        if not self.data_grad:
            raise ValueError("lml_grad_data needs MiSparseGP(..., data_grad=True)")
        if want_z and not self.z_grad:
            raise ValueError("lml_grad_data(want_z=True) needs MiSparseGP(..., z_grad=True)")
        self._bind_data_grad(bool(want_x))
        F, grad = self._bound_grad(theta)
        if np.isfinite(F):
            with torch.cuda.device(self.dev):
                gy = self.gy_t.cpu().numpy()
                gx = self.gx_t.cpu().numpy() if want_x else None
        else:
            gy, gx = np.zeros(self.n), (np.zeros((self.n, self.d)) if want_x else None)
        out = (F, grad[: self.ntheta].copy(), gy, gx)
        return out + (grad[self.ntheta:].reshape(self.m, self.d).copy(),) if want_z else out

    def _bound_grad(self, theta):
        theta, tp = self._theta(theta)
        out = ctypes.c_double()
        grad = np.zeros(self.ntheta + (self.m * self.d if self.z_grad else 0))
        self._factored_theta = None
        if self._bad_data():
            return -np.inf, grad
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
        self.X_t = self.y_t = self.Z_t = self.work_t = self.gy_t = self.gx_t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
