"""Gradient-enhanced GP: values AND gradients of the function at the training points (Rasmussen & Williams 9.4), on one MI355X.

The n runs in d dimensions become N = n (1 + d) observations [y ; dY[:, 0] ; .. ; dY[:, d-1]] of a joint GP over f and grad f.
The handle is the dense one of backend.MiGP under a gradient binding (include/mi_gp_deriv.h, libmi_gp_deriv.so): the same
factorisation, solves and reductions behind another covariance assembly, gradient contraction and cross-covariance."""
import ctypes

import numpy as np
import torch

from . import _lib

KERNELS = ("RBF", "Matern52")
MAX_D = 32


def joint_observations(y, dY):
    """[y ; dY[:, 0] ; .. ; dY[:, d-1]]: the value block, then one block per input dimension."""
    return np.concatenate([np.asarray(y, dtype=np.float64).reshape(-1), np.asarray(dY, dtype=np.float64).T.reshape(-1)])


class MiDerivGP:
    """A GP conditioned on y (n,) and dY (n, d) = dy/dx at X (n, d), all in converted space.  theta = [ls(d), kv, alpha, gv,
    jitter] as for MiGP; gv is the noise variance of the values.  ``grad_noise``: a fixed noise variance of the gradient
    observations, a scalar or (n, d) (None: the jitter alone)."""

    def __init__(self, X, y, dY, kernel="RBF", device=0, grad_noise=None):
        if not torch.cuda.is_available():
            raise RuntimeError("MiDerivGP needs a ROCm GPU: the GP hot path has no CPU implementation")
        if kernel not in KERNELS:
            raise ValueError(f"gradient observations need one kernel out of {KERNELS}, got {kernel!r}")
        X = np.ascontiguousarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        dY = np.asarray(dY, dtype=np.float64)
        if X.ndim != 2 or y.shape != (X.shape[0],) or dY.shape != X.shape:
            raise ValueError("X and dY must be (n, d) and y (n,)")
        if X.shape[1] > MAX_D:
            raise ValueError(f"gradient observations need d <= {MAX_D}, got {X.shape[1]}")
        if not (np.isfinite(X).all() and np.isfinite(y).all() and np.isfinite(dY).all()):
            raise ValueError("X, y and dY must be finite")
        self.lib = _lib.load_deriv()
        self.n, self.d = X.shape
        self.N = self.n * (1 + self.d)
        self.kernel = kernel
        self.device = int(device)
        self.dev = torch.device("cuda", self.device)
        cfg = _lib.MiGpConfig()
        cfg.n, cfg.d, cfg.nkern = self.N, self.d, 1
        cfg.kernel_ids[0] = _lib.KERNEL_IDS[kernel]
        cfg.device = self.device
        h = ctypes.c_void_p()
        r = self.lib.mi_gp_create(ctypes.byref(cfg), ctypes.byref(h))
        if r != 0:
            raise RuntimeError(f"mi_gp_create failed ({r}): {self.lib.mi_gp_last_global_error().decode()}")
        self.h = h
        self.np_ = int(self.lib.mi_gp_padded_n(h))
        self.ntheta = int(self.lib.mi_gp_num_theta(h))
        self.lda = self.np_ + 16
        self._check(self.lib.mi_gp_deriv_bind(self.h, self.n), "mi_gp_deriv_bind")
        with torch.cuda.device(self.dev):
            self.X_t = torch.from_numpy(X).to(self.dev)
            self.y_t = torch.from_numpy(joint_observations(y, dY)).to(self.dev)
            self.K_t = torch.empty((self.np_ + 128, self.lda), dtype=torch.float64, device=self.dev)
            self.Z_t = torch.zeros((self.np_, self.lda), dtype=torch.float64, device=self.dev)
            self.W_t = torch.zeros((self.np_, self.lda), dtype=torch.float64, device=self.dev)
            torch.cuda.synchronize(self.dev)
        b = _lib.MiGpBuffers()
        b.X_dev, b.y_dev, b.K_dev = self.X_t.data_ptr(), self.y_t.data_ptr(), self.K_t.data_ptr()
        b.lda = self.lda
        b.Z_dev, b.W_dev = self.Z_t.data_ptr(), self.W_t.data_ptr()
        self._check(self.lib.mi_gp_set_data(self.h, ctypes.byref(b)), "mi_gp_set_data")
        self._diag_t = None
        self._work = None
        self._factored_theta = None
        self.info = 0
        self.set_grad_noise(grad_noise)

    def _check(self, r, what):
        if r < 0:
            raise RuntimeError(f"{what} failed ({r}): {self.lib.mi_gp_last_error(self.h).decode()}")
        return r

    def _theta(self, theta):
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if theta.shape != (self.ntheta,):
            raise ValueError(f"theta must have {self.ntheta} entries")
        return theta, theta.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def set_grad_noise(self, grad_noise=None):
        """A fixed noise variance of the gradient observations (scalar or (n, d); None removes it): mi_gp_set_diag's vector
        over the N observations, zero on the value rows."""
        self._factored_theta = None
        if grad_noise is None:
            self._diag_t = None
            self._check(self.lib.mi_gp_set_diag(self.h, None), "mi_gp_set_diag")
            return
        g = np.broadcast_to(np.asarray(grad_noise, dtype=np.float64), (self.n, self.d))
        if not (np.isfinite(g).all() and (g >= 0).all()):
            raise ValueError("grad_noise must be finite and >= 0")
        diag = np.concatenate([np.zeros(self.n), g.T.reshape(-1)])
        with torch.cuda.device(self.dev):
            self._diag_t = torch.from_numpy(diag).to(self.dev)
            torch.cuda.synchronize(self.dev)
        self._check(self.lib.mi_gp_set_diag(self.h, self._diag_t.data_ptr()), "mi_gp_set_diag")

    def lml(self, theta):
        """The log marginal likelihood of the N observations; -inf if the joint covariance is not positive definite."""
        theta, tp = self._theta(theta)
        out = ctypes.c_double()
        self._factored_theta = None
        self.info = self._check(self.lib.mi_gp_lml(self.h, tp, ctypes.byref(out)), "mi_gp_lml")
        return out.value

    def lml_parts(self):
        """(sum log L_ii, |L^-1 y|^2) of the last evaluation that succeeded"""
        a, b = ctypes.c_double(), ctypes.c_double()
        self._check(self.lib.mi_gp_lml_parts(self.h, ctypes.byref(a), ctypes.byref(b)), "mi_gp_lml_parts")
        return a.value, b.value

    def lml_grad(self, theta):
        """(LML, dLML/dtheta); (-inf, zeros) if the joint covariance is not positive definite."""
        theta, tp = self._theta(theta)
        out = ctypes.c_double()
        grad = np.zeros(self.ntheta)
        self._factored_theta = None
        self.info = self._check(self.lib.mi_gp_lml_grad(self.h, tp, ctypes.byref(out), grad.ctypes.data_as(ctypes.POINTER(ctypes.c_double))),
                                "mi_gp_lml_grad")
        return out.value, grad

    def factor(self, theta):
        """Factorise for prediction (conditional form); returns LAPACK-style info."""
        theta, tp = self._theta(theta)
        self._factored_theta = None
        self.info = self._check(self.lib.mi_gp_factor(self.h, tp), "mi_gp_factor")
        if self.info == 0:
            self._factored_theta = theta.copy()
        return self.info

    def predict(self, theta, Xnew, pred_noise=True, chunk=4096):
        """Posterior mean and variance of the VALUE at Xnew (m, d), chunked over points."""
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if self._factored_theta is None or not np.array_equal(theta, self._factored_theta):
            if self.factor(theta) != 0:
                raise FloatingPointError(f"covariance not positive definite at pivot {self.info}")
        Xnew = np.ascontiguousarray(Xnew, dtype=np.float64)
        if Xnew.ndim != 2 or Xnew.shape[1] != self.d:
            raise ValueError("Xnew must be (m, d)")
        m = Xnew.shape[0]
        mean, var = np.empty(m), np.empty(m)
        with torch.cuda.device(self.dev):
            for s in range(0, m, chunk):
                mc = min(chunk, m - s)
                mp = (mc + 127) // 128 * 128
                if self._work is None or self._work.shape[0] < mp:
                    self._work = torch.empty((mp, self.lda), dtype=torch.float64, device=self.dev)
                xn = torch.from_numpy(Xnew[s : s + mc]).to(self.dev)
                mu_t = torch.empty(mc, dtype=torch.float64, device=self.dev)
                var_t = torch.empty(mc, dtype=torch.float64, device=self.dev)
                torch.cuda.synchronize(self.dev)
                self._check(self.lib.mi_gp_predict(self.h, xn.data_ptr(), mc, self._work.data_ptr(), self.lda, mu_t.data_ptr(),
                                                   var_t.data_ptr(), 1 if pred_noise else 0), "mi_gp_predict")
                mean[s : s + mc] = mu_t.cpu().numpy()
                var[s : s + mc] = var_t.cpu().numpy()
        return mean, var

    def last_error(self):
        return self.lib.mi_gp_last_error(self.h).decode()

    def close(self):
        if getattr(self, "h", None):
            with torch.cuda.device(self.dev):
                torch.cuda.synchronize(self.dev)
            self.lib.mi_gp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
