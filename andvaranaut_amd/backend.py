"""Device-side GP engine: owns the PyTorch-ROCm buffers and drives libmi_gp.so through ctypes.

Mirrors what the reference keeps inside its PyMC model object ``m``/``gp`` (gpmcmc.py:178,401):
the training inputs, the kernel structure, and a way to evaluate logp / dlogp / the conditional."""
import contextlib
import ctypes

import numpy as np
import torch

from . import _lib


def parse_kernel(kernel):
    """Kernel-string grammar of GPMCMC.change_model (gpmcmc.py:497-505): names joined by + or *."""
    import re

    kerns = re.split(r"[+*]", kernel)
    ops = [ch for ch in kernel if ch in "+*"]
    for k in kerns:
        if k not in _lib.KERNEL_IDS:
            raise Exception(f"Error: kernel string must contain only {list(_lib.KERNEL_IDS)}")
    if len(kerns) > _lib.MAX_KERN:
        raise Exception(f"Error: at most {_lib.MAX_KERN} kernel components are supported")
    return kerns, ops


def pack_theta(ls, kv, gv, jitter, alpha=None):
    """C-ABI theta layout: [ls(nkern*d), kv(nkern), alpha(nkern), gv, jitter]."""
    ls = np.atleast_2d(np.asarray(ls, dtype=np.float64))
    kv = np.atleast_1d(np.asarray(kv, dtype=np.float64))
    alpha = np.ones_like(kv) if alpha is None else np.atleast_1d(np.asarray(alpha, dtype=np.float64))
    return np.concatenate([ls.ravel(), kv, alpha, [float(gv), float(jitter)]])


class MiGP:
    """One GP data set + kernel structure bound to one MI355X and one HIP stream."""

    def __init__(self, X, y, kernel="RBF", device=0, panel_tiles=0, need_grad=True, capacity=None):
        if not torch.cuda.is_available():
            raise RuntimeError("MiGP needs a ROCm GPU: the GP hot path has no CPU implementation")
        self.lib = _lib.load()
        X = np.ascontiguousarray(X, dtype=np.float64)
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
        if X.ndim != 2 or X.shape[0] != y.shape[0]:
            raise ValueError("X must be (n,d) and y (n,)")
        if not (np.isfinite(X).all() and np.isfinite(y).all()):
            # the device exp clamps its argument (migp_math.h): a NaN input would come out as a finite covariance entry,
            # where the reference's PyTensor graph propagates NaN and the "posdef" check rejects the point
            raise ValueError("X and y must be finite")
        self._bad_data = False
        self.n, self.d = X.shape
        self.kerns, self.ops = parse_kernel(kernel)
        self.nkern = len(self.kerns)
        self.device = int(device)
        self.dev = torch.device("cuda", self.device)
        cfg = _lib.MiGpConfig()
        cfg.n, cfg.d, cfg.nkern = self.n, self.d, self.nkern
        for i, k in enumerate(self.kerns):
            cfg.kernel_ids[i] = _lib.KERNEL_IDS[k]
        for i, o in enumerate(self.ops):
            cfg.ops[i] = _lib.OP_IDS[o]
        cfg.device = self.device
        cfg.panel_tiles = int(panel_tiles)
        h = ctypes.c_void_p()
        r = self.lib.mi_gp_create(ctypes.byref(cfg), ctypes.byref(h))
        if r != 0:
            raise RuntimeError(f"mi_gp_create failed ({r}): {self.lib.mi_gp_last_global_error().decode()}")
        self.h = h
        self.np_ = int(self.lib.mi_gp_padded_n(h))
        self.ntheta = int(self.lib.mi_gp_num_theta(h))
        self.need_grad = bool(need_grad)
        self.append_refactors = 0  # capacity growths of append() (each one refactorises once)
        self.capacity = None
        if capacity is None:
            # leading dimension: padded n plus 16 doubles so that column panels are not power-of-two strided
            self.lda = self.np_ + 16
            with torch.cuda.device(self.dev):
                self.X_t = torch.from_numpy(X).to(self.dev)
                self.y_t = torch.from_numpy(y).to(self.dev)
                self.K_t = torch.empty((self.np_ + 128, self.lda), dtype=torch.float64, device=self.dev)
                self.Z_t = self.W_t = None
                if need_grad:
                    self.Z_t = torch.zeros((self.np_, self.lda), dtype=torch.float64, device=self.dev)
                    self.W_t = torch.zeros((self.np_, self.lda), dtype=torch.float64, device=self.dev)
                torch.cuda.synchronize(self.dev)
            self._bind()
        else:
            if int(capacity) < self.n:
                raise ValueError(f"capacity {capacity} < n = {self.n}")
            self._allocate(int(capacity), X, y, None)

    def _bind(self):
        b = _lib.MiGpBuffers()
        b.X_dev, b.y_dev, b.K_dev = self.X_t.data_ptr(), self.y_t.data_ptr(), self.K_t.data_ptr()
        b.lda = self.lda
        b.Z_dev = self.Z_t.data_ptr() if self.Z_t is not None else None
        b.W_dev = self.W_t.data_ptr() if self.Z_t is not None else None
        self._check(self.lib.mi_gp_set_data(self.h, ctypes.byref(b)), "mi_gp_set_data")

    @staticmethod
    def _padded(n):
        return (int(n) + 127) // 128 * 128

    def _allocate(self, capacity, X, y, diag):
        """Buffers for up to `capacity` points (the first n hold X, y and the optional diagonal), bound to the handle with
        mi_gp_set_data + mi_gp_reserve; X_t / y_t / _diag_t are views of the first n rows."""
        cp = self._padded(capacity)
        self.lda = cp + 16
        with torch.cuda.device(self.dev):
            self._X_store = torch.zeros((capacity, self.d), dtype=torch.float64, device=self.dev)
            self._y_store = torch.zeros(capacity, dtype=torch.float64, device=self.dev)
            self._X_store[: self.n].copy_(torch.as_tensor(X).to(self.dev))
            self._y_store[: self.n].copy_(torch.as_tensor(y).to(self.dev))
            self.K_t = None
            self.K_t = torch.empty((cp + 128, self.lda), dtype=torch.float64, device=self.dev)
            self.Z_t = self.W_t = None
            if self.need_grad:
                self.Z_t = torch.zeros((cp, self.lda), dtype=torch.float64, device=self.dev)
                self.W_t = torch.zeros((cp, self.lda), dtype=torch.float64, device=self.dev)
            self._diag_store = None
            if diag is not None:
                self._diag_store = torch.zeros(capacity, dtype=torch.float64, device=self.dev)
                self._diag_store[: self.n].copy_(torch.as_tensor(diag).to(self.dev))
            self._awork = None
            torch.cuda.synchronize(self.dev)
        self.capacity = capacity
        self._views()
        self._bind()
        self._check(self.lib.mi_gp_reserve(self.h, capacity), "mi_gp_reserve")
        if diag is not None:
            self._check(self.lib.mi_gp_set_diag(self.h, self._diag_t.data_ptr()), "mi_gp_set_diag")

    def _views(self):
        self.X_t = self._X_store[: self.n]
        self.y_t = self._y_store[: self.n]
        if getattr(self, "_diag_store", None) is not None:
            self._diag_t = self._diag_store[: self.n]

    def _check(self, r, what):
        if r < 0:
            raise RuntimeError(f"{what} failed ({r}): {self.lib.mi_gp_last_error(self.h).decode()}")
        return r

    def _theta(self, theta):
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if theta.shape != (self.ntheta,):
            raise ValueError(f"theta must have {self.ntheta} entries")
        return theta, theta.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def lml(self, theta):
        """LML at natural-scale theta; -inf if K is not positive definite (info > 0)."""
        self._no_trend("lml")
        self._no_outputs("lml")
        theta, tp = self._theta(theta)
        out = ctypes.c_double()
        self._factored_ok = False
        if self._bad_data:  # non-finite warped data: what PyMC turns into logp = -inf (update_data)
            self.info = 1
            return -np.inf
        self.info = self._check(self.lib.mi_gp_lml(self.h, tp, ctypes.byref(out)), "mi_gp_lml")
        return out.value

    def lml_parts(self):
        a, b = ctypes.c_double(), ctypes.c_double()
        self._check(self.lib.mi_gp_lml_parts(self.h, ctypes.byref(a), ctypes.byref(b)), "mi_gp_lml_parts")
        return a.value, b.value

    def lml_grad(self, theta):
        """(LML, dLML/dtheta) at natural-scale theta; (-inf, zeros) if K is not positive definite."""
        if self.Z_t is None:
            raise RuntimeError("this MiGP was created with need_grad=False")
        if self.nout > 1 and self._trend != 0:
            self._no_outputs("a trend")
        self._outcov_needs_points()
        if self._trend != 0 and self.get_option(48) == 1:
            self._no_trend("a cross-validation objective")
        if self.nout > 1 and self.get_option(48) == 1:
            self._no_outputs("a cross-validation objective")
        theta, tp = self._theta(theta)
        out = ctypes.c_double()
        grad = np.zeros(self.ntheta)
        gp_ = grad.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        self._factored_ok = False
        if self._bad_data:
            self.info = 1
            return -np.inf, grad
        self.info = self._check(self.lib.mi_gp_lml_grad(self.h, tp, ctypes.byref(out), gp_), "mi_gp_lml_grad")
        return out.value, grad

    OBJECTIVES = {"lml": 0, "loo": 1}

    def set_objective(self, objective):
        """What lml_grad returns (option 48 of mi_gp_set_option): "lml", the log marginal likelihood, or "loo", the leave-one-out
        log predictive density sum_i log p(y_i | y_-i) with its exact theta gradient.  lml, the batched evaluations,
        lml_grad_data's data-side gradients and kfold keep their meaning ("loo" has no batched form: lml_grad_batch raises)."""
        if objective not in self.OBJECTIVES:
            raise ValueError(f"objective must be one of {list(self.OBJECTIVES)}")
        self.set_option(48, self.OBJECTIVES[objective])

    TRENDS = {"none": 0, "constant": 1, "linear": 2}

    def set_trend(self, name):
        """The prior mean of the model (option 50 of mi_gp_set_option): "none", zero; "constant", h(x) = [1]; "linear",
        h(x) = [1, x_1 .. x_d] (d <= 127).  The coefficients carry a vague prior and are integrated out in closed form (Rasmussen &
        Williams section 2.7): theta keeps its layout.  lml_grad then returns the trend's marginal likelihood (eq. 2.45) and its
        exact theta gradient, factor + predict the trend's conditional (eqs. 2.41-2.42); every other evaluation raises
        ValueError until the trend is "none" again.  A change ends the resident factorisation."""
        if name not in self.TRENDS:
            raise ValueError(f"trend must be one of {list(self.TRENDS)}")
        if self.TRENDS[name] != self._trend:
            self.set_option(50, self.TRENDS[name])
            self._trend = self.TRENDS[name]
            self._factored_ok = False
            self._u_theta_ok = False

    _trend = 0

    def _no_trend(self, what):
        """Raised before the call by everything that has no form under a trend."""
        if self._trend != 0:
            name = [k for k, v in self.TRENDS.items() if v == self._trend][0]
            raise ValueError(f"{what} has no form under a trend (set_trend({name!r}) is in force): set_trend('none') first")

    nout = 1

    def set_outputs(self, Y):
        """The outputs of the model (option 51 of mi_gp_set_option): Y is (n, q) float64, finite, 1 <= q <= 128.  Under q >= 2 the q
        columns are modelled under ONE shared kernel and one noise, independent given theta: lml_grad returns the sum of the
        outputs' log marginal likelihoods and its exact theta gradient, factor + predict a mean of shape (m, q) and the variance
        (m,) every output shares; every other evaluation raises ValueError until set_outputs is called with one column, which
        returns to the single-output state.  The columns live in one (q, lda) tensor, output o in row o; the data are rebound,
        which ends the resident factorisation."""
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim == 1:
            Y = Y.reshape(-1, 1)
        if Y.ndim != 2 or Y.shape[0] != self.n or not 1 <= Y.shape[1] <= 128:
            raise ValueError(f"the outputs Y must be (n, q) with n = {self.n} and 1 <= q <= 128")
        if not np.isfinite(Y).all():
            raise ValueError("the outputs Y must be finite")
        q = Y.shape[1]
        with torch.cuda.device(self.dev):
            store = torch.zeros((q, self.lda), dtype=torch.float64, device=self.dev)
            store[:, : self.n].copy_(torch.from_numpy(np.ascontiguousarray(Y.T)))
            torch.cuda.synchronize(self.dev)
        self._Y_store = store
        if self.capacity is not None:  # (row 0 holds lda >= capacity doubles: room for appended points once q is 1 again)
            self._y_store = store[0]
        self.y_t = store[0, : self.n]
        self._bad_y = False
        self._bad_data = bool(getattr(self, "_bad_X", False))
        self._factored_ok = False
        self._u_theta_ok = False
        self._bind()
        self.set_option(51, q)
        self.nout = q

    OUTPUT_COVS = {"shared": 0, "integrated": 1}
    _outcov = 0

    def set_output_cov(self, name):
        """The covariance between the outputs of set_outputs (option 52 of mi_gp_set_option): "shared" (default), the outputs
        independent under one kernel variance; "integrated", vec(Y) ~ N(0, Sigma (x) K_y) with a q x q covariance Sigma between the
        outputs under the Jeffreys prior |Sigma|^-(q+1)/2, integrated out in closed form (the separable emulator of Conti &
        O'Hagan 2010).  Under "integrated" and q >= 2 outputs (n >= q + 2) lml_grad returns that marginal likelihood L_S and its
        exact theta gradient, and predict the same means with a variance of shape (m, q): column o is the shared variance times
        s_o = |L^-1 y_o|^2 / (n - q - 1).  L_S does not change under K_y -> c K_y: only their priors identify the overall scale
        of kv, gv and the jitter.  With one output the choice is inert.  A change ends the resident factorisation."""
        if name not in self.OUTPUT_COVS:
            raise ValueError(f"the output covariance must be one of {list(self.OUTPUT_COVS)}")
        if self.OUTPUT_COVS[name] != self._outcov:
            self.set_option(52, self.OUTPUT_COVS[name])  # (set_option keeps _outcov, the mirror predict reads, in step)

    def _outcov_needs_points(self):
        """Raised before the call: the integrated covariance of q outputs needs n >= q + 2."""
        if self._outcov and self.nout > 1 and self.n < self.nout + 2:
            raise ValueError(f"the integrated covariance of {self.nout} outputs (set_output_cov('integrated')) needs n >= q + 2 points, "
                             f"got n = {self.n}")

    def _no_outputs(self, what):
        """Raised before the call by everything that has no form under several outputs."""
        if self.nout > 1:
            raise ValueError(f"{what} has no form under several outputs (set_outputs with {self.nout} columns is in force): "
                             "call set_outputs with one column first")

    def loo_grad(self, theta):
        """(L_LOO, dL_LOO/dtheta) at natural-scale theta, whatever objective is set (it is the same afterwards); (-inf, zeros)
        if K is not positive definite or a diagonal entry of K^-1 is not positive (``info``)."""
        with self._options({48: 1}):
            return self.lml_grad(theta)

    def set_cv_block(self, b):
        """The fold size of the objective "loo" (option 49 of mi_gp_set_option): 1, leave-one-out, or 2..128, the leave-block-out
        log predictive density sum_f log p(y_I_f | y_-I_f) over the contiguous folds I_f = [f b, min((f + 1) b, n)) -- the sum of
        ``kfold``'s logp over these folds -- with its exact theta gradient.  No effect under the objective "lml"."""
        self.set_option(49, int(b))

    def cv_grad(self, theta, block):
        """(L_CV, dL_CV/dtheta) at natural-scale theta over contiguous folds of ``block`` points, whatever objective and fold size
        are set (they are the same afterwards); (-inf, zeros) if K or a fold's block of K^-1 is not positive definite (``info``:
        the 1-based index of the point at the bad pivot)."""
        with self._options({49: int(block), 48: 1}):
            return self.lml_grad(theta)

    # ------------------------------------------------------------------ batched evaluation
    def _ensure_batch(self, k, need_grad):
        """Device buffers for k problems in lockstep (mi_gp_set_batch): K (+ Z, W for the gradient) as ONE tensor each."""
        have = getattr(self, "_batch_k", 0)
        if have >= k and (not need_grad or self._bZ is not None):
            return
        k = max(k, have)
        with torch.cuda.device(self.dev):
            self._bK = torch.empty((k, self.np_ + 128, self.lda), dtype=torch.float64, device=self.dev)
            self._bZ = self._bW = None
            if need_grad or getattr(self, "_batch_grad", False):
                self._bZ = torch.zeros((k, self.np_, self.lda), dtype=torch.float64, device=self.dev)
                self._bW = torch.zeros((k, self.np_, self.lda), dtype=torch.float64, device=self.dev)
                self._batch_grad = True
            torch.cuda.synchronize(self.dev)
        b = _lib.MiGpBatchBuffers()
        b.K_dev = self._bK.data_ptr()
        b.Z_dev = self._bZ.data_ptr() if self._bZ is not None else None
        b.W_dev = self._bW.data_ptr() if self._bW is not None else None
        b.stride_k = (self.np_ + 128) * self.lda
        b.stride_zw = self.np_ * self.lda
        b.count = k
        self._check(self.lib.mi_gp_set_batch(self.h, ctypes.byref(b)), "mi_gp_set_batch")
        self._batch_k = k

    def _thetas(self, thetas):
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        if th.ndim != 2 or th.shape[1] != self.ntheta:
            raise ValueError(f"thetas must be (k, {self.ntheta})")
        return th

    def lml_batch(self, thetas):
        """LML at k hyper-parameter vectors of the same data in ONE lockstep evaluation (mi_gp_lml_batch): every launch
        carries blockIdx.z = problem.  Returns (k,) values, -inf where the covariance is not positive definite; the
        values are those lml() returns one at a time."""
        self._no_trend("lml_batch")
        self._no_outputs("lml_batch")
        th = self._thetas(thetas)
        k = th.shape[0]
        self._ensure_batch(k, False)
        self._factored_ok = False
        out = np.empty(k)
        info = np.zeros(k, dtype=np.int32)
        if self._bad_data:
            return np.full(k, -np.inf)
        dpt, ipt = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        self._check(self.lib.mi_gp_lml_batch(self.h, k, th.ctypes.data_as(dpt), out.ctypes.data_as(dpt), info.ctypes.data_as(ipt)),
                    "mi_gp_lml_batch")
        self.batch_info = info
        return out

    def lml_grad_batch(self, thetas):
        """(LML (k,), dLML/dtheta (k, ntheta)) at k hyper-parameter vectors in one lockstep evaluation
        (mi_gp_lml_grad_batch); rows of non-positive-definite problems are (-inf, zeros)."""
        self._no_trend("lml_grad_batch")
        self._no_outputs("lml_grad_batch")
        th = self._thetas(thetas)
        k = th.shape[0]
        self._ensure_batch(k, True)
        self._factored_ok = False
        out = np.empty(k)
        grad = np.zeros((k, self.ntheta))
        info = np.zeros(k, dtype=np.int32)
        if self._bad_data:
            return np.full(k, -np.inf), grad
        dpt, ipt = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        self._check(self.lib.mi_gp_lml_grad_batch(self.h, k, th.ctypes.data_as(dpt), out.ctypes.data_as(dpt),
                                                  grad.ctypes.data_as(dpt), info.ctypes.data_as(ipt)), "mi_gp_lml_grad_batch")
        self.batch_info = info
        return out, grad

    # ------------------------------------------------------------------ batched conditional (posterior predictive)
    def factor_batch(self, thetas):
        """Factorise k covariances in the conditional form (mi_gp_factor_batch), one theta each, in one lockstep evaluation.
        Returns the (k,) info array (0, or the 1-based first bad pivot).  The factors stay in the batch buffers for
        predict_batch; the single-evaluation factor is gone, so a later predict() refactorises."""
        self._no_trend("factor_batch")
        self._no_outputs("factor_batch")
        th = self._thetas(thetas)
        k = th.shape[0]
        self._ensure_batch(k, False)
        self._factored_ok = False
        self._u_theta_ok = False
        self._pred_count = 0
        if self._bad_data:
            raise FloatingPointError("the last update_data carried non-finite values: nothing to factorise")
        info = np.zeros(k, dtype=np.int32)
        dpt, ipt = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        self._check(self.lib.mi_gp_factor_batch(self.h, k, th.ctypes.data_as(dpt), info.ctypes.data_as(ipt)), "mi_gp_factor_batch")
        self.batch_info = info
        return info

    def predict_batch_capacity(self, m):
        """Draws that one factor_batch + predict_batch call holds for chunks of m points: K_p, its leaf inverses, the
        work block and the moments per draw against 80 % of the device's free memory (sized like the NUTS batch)."""
        mp = (min(int(m), 1 << 30) + 127) // 128 * 128
        have = getattr(self, "_batch_k", 0)
        per = ((self.np_ + 128) * self.lda + (self.np_ // 128 + 4) * 128 * 128 + mp * self.lda + 2 * mp) * 8
        if getattr(self, "_batch_grad", False):
            per += 2 * self.np_ * self.lda * 8  # (_ensure_batch grows U and K^-1 with K once they exist)
        free, _total = torch.cuda.mem_get_info(self.dev)
        held = have * per  # (buffers this handle holds already are reused, not added)
        return max(1, int((0.8 * free + held) // per))

    def predict_batch(self, thetas, Xnew, pred_noise=True, mixture=True, chunk=16384, max_batch=None):
        """Posterior mean / variance at Xnew under each of k hyper-parameter vectors (mi_gp_factor_batch +
        mi_gp_predict_batch): row p equals factor(thetas[p]) + predict(thetas[p], Xnew) bit for bit; rows of draws whose
        covariance is not positive definite are NaN (``self.batch_info``).  Chunked over draws by batch capacity (or
        ``max_batch``) and over points by ``chunk``.  Returns (means[k, m], vars[k, m]) and, with ``mixture``, also the
        equal-weight mixture (mix_mean[m], mix_var[m]) over the positive-definite draws: each draw-chunk's mixture
        comes from the device, chunks are combined here in chunk order (law of total variance)."""
        self._no_trend("predict_batch")
        self._no_outputs("predict_batch")
        th = self._thetas(thetas)
        k = th.shape[0]
        Xnew = np.ascontiguousarray(Xnew, dtype=np.float64)
        if Xnew.ndim != 2 or Xnew.shape[1] != self.d:
            raise ValueError("Xnew must be (m, d)")
        m = Xnew.shape[0]
        chunk = max(1, int(chunk))
        cap = self.predict_batch_capacity(min(chunk, m))
        if max_batch is not None:
            cap = max(1, min(cap, int(max_batch)))
        means = np.empty((k, m))
        vars_ = np.empty((k, m))
        info_all = np.zeros(k, dtype=np.int32)
        parts = []  # per draw-chunk: (positive-definite draws, mixture mean, mixture variance)
        with torch.cuda.device(self.dev):
            for b0 in range(0, k, cap):
                kc = min(cap, k - b0)
                info = self.factor_batch(th[b0 : b0 + kc])
                info_all[b0 : b0 + kc] = info
                mix_m, mix_v = np.empty(m), np.empty(m)
                for s in range(0, m, chunk):
                    mc = min(chunk, m - s)
                    mp = (mc + 127) // 128 * 128
                    work = getattr(self, "_bwork", None)
                    if work is None or work.numel() < kc * mp * self.lda:
                        self._bwork = None
                        self._bwork = torch.empty(kc * mp * self.lda, dtype=torch.float64, device=self.dev)
                        work = self._bwork
                    xn = torch.from_numpy(Xnew[s : s + mc]).to(self.dev)
                    out = torch.empty((2 * kc + 2, mc), dtype=torch.float64, device=self.dev)
                    torch.cuda.synchronize(self.dev)
                    mix = (out[2 * kc].data_ptr(), out[2 * kc + 1].data_ptr()) if mixture else (None, None)
                    self._check(self.lib.mi_gp_predict_batch(self.h, kc, xn.data_ptr(), mc, work.data_ptr(), self.lda, mp * self.lda,
                                                             out[0].data_ptr(), out[kc].data_ptr(), 1 if pred_noise else 0, *mix),
                                "mi_gp_predict_batch")
                    o = out.cpu().numpy()
                    means[b0 : b0 + kc, s : s + mc] = o[:kc]
                    vars_[b0 : b0 + kc, s : s + mc] = o[kc : 2 * kc]
                    if mixture:
                        mix_m[s : s + mc], mix_v[s : s + mc] = o[2 * kc], o[2 * kc + 1]
                parts.append((int(np.count_nonzero(info == 0)), mix_m, mix_v))
        self.batch_info = info_all
        if not mixture:
            return means, vars_
        parts = [p for p in parts if p[0] > 0]
        if not parts:
            return means, vars_, np.full(m, np.nan), np.full(m, np.nan)
        if len(parts) == 1:
            return means, vars_, parts[0][1], parts[0][2]
        # (relative to the first chunk's moments, as the device sums: chunks that all agree return those moments exactly)
        tot = sum(c for c, _, _ in parts)
        m0, v0 = parts[0][1], parts[0][2]
        mu = m0 + sum(c * (pm - m0) for c, pm, _ in parts) / tot
        var = v0 + sum(c * (pv - v0 + (pm - mu) ** 2) for c, pm, pv in parts) / tot
        return means, vars_, mu, var

    def lml_grad_data(self, theta, want_x=True):
        """(LML, dLML/dtheta, dLML/dy, dLML/dX) -- the data-side gradients drive the chain rule through
        warps (cwgp / iwgp) and free input rows (inverse_opt).  dLML/dX is None unless want_x."""
        self._no_trend("lml_grad_data")
        self._no_outputs("lml_grad_data")
        val, grad = self.lml_grad(theta)
        if not np.isfinite(val):
            return val, grad, np.zeros(self.n), (np.zeros((self.n, self.d)) if want_x else None)
        alpha = np.empty(self.n)
        self._check(self.lib.mi_gp_alpha(self.h, alpha.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), "mi_gp_alpha")
        gx = None
        if want_x:
            with torch.cuda.device(self.dev):
                if getattr(self, "_gx_t", None) is None:
                    self._gx_t = torch.empty((self.n, self.d), dtype=torch.float64, device=self.dev)
                    torch.cuda.synchronize(self.dev)
                self._check(self.lib.mi_gp_grad_x(self.h, self._gx_t.data_ptr()), "mi_gp_grad_x")
                gx = self._gx_t.cpu().numpy()
        return val, grad, -alpha, gx

    def update_data(self, X=None, y=None):
        """Overwrite the resident inputs / outputs in place (same shapes): warped data change at every
        posterior evaluation while the buffers, the handle and its streams stay.  Non-finite data (an overflowing warp)
        are not uploaded: until the next finite update lml / lml_grad return -inf like a non-positive-definite covariance
        (the reference's graph would produce NaN and PyMC's checks reject the point)."""
        if y is not None:
            self._no_outputs("update_data(y=...)")
        self._factored_ok = False
        # Each array carries its own state: a non-finite one is not uploaded and stays "bad" until a finite replacement
        # arrives, the finite member of a pair IS uploaded (round 4 dropped it: a later update of the other array then
        # evaluated against stale data).
        if X is not None:
            self._bad_X = not np.isfinite(np.asarray(X, dtype=np.float64)).all()
            if self._bad_X:
                X = None
        if y is not None:
            self._bad_y = not np.isfinite(np.asarray(y, dtype=np.float64)).all()
            if self._bad_y:
                y = None
        self._bad_data = bool(getattr(self, "_bad_X", False) or getattr(self, "_bad_y", False))
        if X is None and y is None:
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

    def set_diag(self, diag=None):
        """Per-point diagonal added to K at assembly (None removes it)."""
        self._factored_ok = False
        with torch.cuda.device(self.dev):
            if diag is None:
                self._diag_t = self._diag_store = None
                self._check(self.lib.mi_gp_set_diag(self.h, None), "mi_gp_set_diag")
                return
            diag = np.ascontiguousarray(np.asarray(diag, dtype=np.float64).reshape(-1))
            if diag.shape != (self.n,):
                raise ValueError("diag must have n entries")
            if self.capacity is None:
                self._diag_t = torch.from_numpy(diag).to(self.dev)
            else:  # (room for appended points: mi_gp_append writes their entries behind the first n)
                self._diag_store = torch.zeros(self.capacity, dtype=torch.float64, device=self.dev)
                self._diag_store[: self.n].copy_(torch.from_numpy(diag).to(self.dev))
                self._diag_t = self._diag_store[: self.n]
            torch.cuda.synchronize(self.dev)
            self._check(self.lib.mi_gp_set_diag(self.h, self._diag_t.data_ptr()), "mi_gp_set_diag")

    def factor(self, theta):
        """Factorise for prediction (conditional form); returns LAPACK-style info."""
        if self.nout > 1 and self._trend != 0:
            self._no_outputs("a trend")
        self._outcov_needs_points()
        theta, tp = self._theta(theta)
        self._factored_ok = False
        self._u_theta_ok = False
        self._pred_count = 0
        if self._bad_data:  # the resident arrays are not the caller's data (update_data refused a non-finite array)
            raise FloatingPointError("the last update_data carried non-finite values: nothing to factorise")
        self.info = self._check(self.lib.mi_gp_factor(self.h, tp), "mi_gp_factor")
        if self.info == 0:
            self._factored_ok, self._factored_theta = True, theta.copy()
        return self.info

    APPEND_CHUNK = 128  # points per mi_gp_append call

    def append(self, Xnew, ynew, diag=None):
        """Condition the resident factorisation (the last successful factor(), conditional form) on new points at the same
        theta (mi_gp_append, O(n^2 k) instead of an O(n^3) refactorisation), in chunks of 128 points.  ``diag``: the new
        points' entries of the per-point diagonal, required exactly when one is set.  When the capacity is exhausted the
        buffers grow about 1.5x and the handle is refactorised once at the factored theta (``append_refactors`` counts
        these).  Returns 0, or the LAPACK-style info of a chunk whose block is not positive definite: that chunk and the
        ones after it are not appended (``self.n`` says how many points are resident), the factor stays usable."""
        self._no_trend("append")
        self._no_outputs("append")
        Xnew = np.ascontiguousarray(np.atleast_2d(np.asarray(Xnew, dtype=np.float64)))
        ynew = np.ascontiguousarray(np.asarray(ynew, dtype=np.float64).reshape(-1))
        if Xnew.ndim != 2 or Xnew.shape[1] != self.d or Xnew.shape[0] != ynew.shape[0]:
            raise ValueError("Xnew must be (k, d) and ynew (k,)")
        if not (np.isfinite(Xnew).all() and np.isfinite(ynew).all()):
            raise ValueError("Xnew and ynew must be finite")
        has_diag = getattr(self, "_diag_t", None) is not None
        if (diag is not None) != has_diag:
            raise ValueError("diag must be given exactly when a per-point diagonal is set (set_diag)")
        if diag is not None:
            diag = np.ascontiguousarray(np.asarray(diag, dtype=np.float64).reshape(-1))
            if diag.shape != ynew.shape or not np.isfinite(diag).all():
                raise ValueError("diag must hold one finite entry per new point")
        if not getattr(self, "_factored_ok", False) or self._bad_data:
            raise RuntimeError("append() extends a factorisation: call factor() (or predict) first")
        total = ynew.shape[0]
        self.info = 0
        for s in range(0, total, self.APPEND_CHUNK):
            kc = min(self.APPEND_CHUNK, total - s)
            if self.capacity is None or self.n + kc > self.capacity:
                self._grow(max(self.n + total - s, int(np.ceil(1.5 * max(self.n, 1)))))
            with torch.cuda.device(self.dev):
                need = 4 * 128 * self.lda + 65600
                if getattr(self, "_awork", None) is None or self._awork.numel() < need:
                    self._awork = None
                    self._awork = torch.empty(need, dtype=torch.float64, device=self.dev)
                xn = torch.from_numpy(Xnew[s : s + kc]).to(self.dev)
                yn = torch.from_numpy(ynew[s : s + kc]).to(self.dev)
                dn = torch.from_numpy(diag[s : s + kc]).to(self.dev) if diag is not None else None
                torch.cuda.synchronize(self.dev)
                r = self._check(self.lib.mi_gp_append(self.h, xn.data_ptr(), yn.data_ptr(), dn.data_ptr() if dn is not None else None,
                                                      kc, self._awork.data_ptr(), self.lda), "mi_gp_append")
            if r != 0:
                self.info = r
                return r
            self.n += kc
            self.np_ = self._padded(self.n)
            self.__dict__["_path_serial"] = self._path_serial + 1  # (draw_paths: the weights of a PathDraw belong to the old n)
            self._views()
            self._gx_t = None  # (sized for n)
            self._drop_batch()
        return 0

    def logpdf(self, theta, Xnew, ynew, diag=None, grad=True):
        """Joint log predictive density of up to 128 trial points given the training data at theta (mi_gp_logpdf):
        log p(ynew | y, X, Xnew, theta) = LML(n + k) - LML(n), with its gradients w.r.t. the trial inputs and outputs --
        (logp, dX [k, d], dy [k]); dX and dy are None with ``grad=False``.  Nothing is committed: the resident factor serves any
        number of trial sets.  ``diag``: the trial points' entries of the per-point diagonal, required exactly when one is
        set.  A trial block that is not positive definite gives (-inf, zeros, zeros), ``self.info`` its pivot."""
        self._no_trend("logpdf")
        self._no_outputs("logpdf")
        Xnew = np.ascontiguousarray(np.atleast_2d(np.asarray(Xnew, dtype=np.float64)))
        ynew = np.ascontiguousarray(np.asarray(ynew, dtype=np.float64).reshape(-1))
        if Xnew.ndim != 2 or Xnew.shape[1] != self.d or Xnew.shape[0] != ynew.shape[0]:
            raise ValueError("Xnew must be (k, d) and ynew (k,)")
        k = ynew.shape[0]
        if not 1 <= k <= 128:
            raise ValueError("logpdf takes 1 to 128 trial points")
        if not (np.isfinite(Xnew).all() and np.isfinite(ynew).all()):
            raise ValueError("Xnew and ynew must be finite")
        has_diag = getattr(self, "_diag_t", None) is not None
        if (diag is not None) != has_diag:
            raise ValueError("diag must be given exactly when a per-point diagonal is set (set_diag)")
        if diag is not None:
            diag = np.ascontiguousarray(np.asarray(diag, dtype=np.float64).reshape(-1))
            if diag.shape != ynew.shape or not np.isfinite(diag).all():
                raise ValueError("diag must hold one finite entry per trial point")
        if grad and self.Z_t is None:
            raise RuntimeError("this MiGP was created with need_grad=False")
        self._ensure_factored(theta)
        nin = k * self.d + k + (k if diag is not None else 0)
        with torch.cuda.device(self.dev):
            need = int(self.lib.mi_gp_logpdf_work(self.lda))
            if getattr(self, "_lwork", None) is None or self._lwork.numel() < need:
                self._lwork = None
                self._lwork = torch.empty(need, dtype=torch.float64, device=self.dev)
                torch.cuda.synchronize(self.dev)
            # (pinned I/O as in predict(): this is the call inverse_opt's optimiser makes once per step)
            io = self._pinned_io(nin + k * self.d + k)
            io_np = io.numpy()
            io_np[: k * self.d] = Xnew.ravel()
            io_np[k * self.d : k * self.d + k] = ynew
            if diag is not None:
                io_np[k * self.d + k : nin] = diag
            base = io.data_ptr()
            out = ctypes.c_double()
            dx_p, dy_p = (base + 8 * nin, base + 8 * (nin + k * self.d)) if grad else (None, None)
            self.info = self._check(self.lib.mi_gp_logpdf(self.h, base, base + 8 * k * self.d,
                                                          base + 8 * (k * self.d + k) if diag is not None else None, k,
                                                          self._lwork.data_ptr(), self.lda, ctypes.byref(out), dx_p, dy_p),
                                    "mi_gp_logpdf")
            if grad:
                self._u_theta_ok = True
            if self.info != 0:
                return (-np.inf, np.zeros((k, self.d)), np.zeros(k)) if grad else (-np.inf, None, None)
            if not grad:
                return out.value, None, None
            o = io_np[nin : nin + k * self.d + k].copy()
        return out.value, o[: k * self.d].reshape(k, self.d), o[k * self.d :]

    KFOLD_MAX_PASS = 256  # folds per pass of mi_gp_kfold (one leaf workgroup per fold: one round on the chip's 256 CUs)

    def kfold(self, theta, folds, moments=True, resident=False):
        """Exact k-fold cross-validation at theta (mi_gp_kfold): for every fold -- a sequence of 1 to 128 distinct point indices;
        folds may overlap and need not cover the data; equal folds may be the rows of one 2-D array -- the hold-out predictive of its noisy observations given all other
        points, out of ONE gradient evaluation: (logp [nfolds], mean, var, info [nfolds]) with ``mean`` / ``var`` lists of
        one array per fold (its points in the fold's order; None with ``moments=False``), ``logp`` the joint log density of
        the fold's observations and ``info`` 0 or the 1-based position of the fold's first non-positive pivot (logp = -inf and
        NaN moments for that fold alone).  ``resident=True`` skips ``lml_grad(theta)``: K^-1 of the last ``lml_grad`` is used
        as it is (theta is ignored).  The hyper-parameters are the same for every fold: nothing is refitted."""
        self._no_trend("kfold")
        self._no_outputs("kfold")
        if self.Z_t is None:
            raise RuntimeError("this MiGP was created with need_grad=False")
        if isinstance(folds, np.ndarray) and folds.ndim == 2 and folds.shape[0] > 0:
            # equal folds as the rows of one array (leave-one-out of 16384 points: no Python loop over the folds)
            sizes = np.full(folds.shape[0], folds.shape[1])
            idx = np.ascontiguousarray(folds, dtype=np.int32).reshape(-1)
        else:
            folds = [np.asarray(f).reshape(-1) for f in folds]
            if not folds:
                raise ValueError("kfold needs at least one fold")
            sizes = np.array([len(f) for f in folds])
            idx = np.ascontiguousarray(np.concatenate(folds), dtype=np.int32)
        if sizes.min() < 1 or sizes.max() > 128:
            raise ValueError(f"every fold holds 1 to 128 points (got sizes {sizes.min()} to {sizes.max()})")
        if not resident:
            val, _ = self.lml_grad(theta)
            if not np.isfinite(val):
                raise FloatingPointError(f"covariance not positive definite at pivot {self.info}")
        nf, total = len(sizes), int(sizes.sum())
        ptr = np.zeros(nf + 1, dtype=np.int32)
        ptr[1:] = np.cumsum(sizes)
        info = np.zeros(nf, dtype=np.int32)
        ip = ctypes.POINTER(ctypes.c_int)
        with torch.cuda.device(self.dev):
            work_p, need = None, 0
            if sizes.max() > 1:  # (leave-one-out runs the closed form: no work block)
                need = int(self.lib.mi_gp_kfold_work(min(self.KFOLD_MAX_PASS, nf), total))
                if getattr(self, "_kwork", None) is None or self._kwork.numel() < need:
                    self._kwork = None
                    self._kwork = torch.empty(need, dtype=torch.float64, device=self.dev)
                work_p = self._kwork.data_ptr()
            out = torch.empty(nf + (2 * total if moments else 0), dtype=torch.float64, device=self.dev)
            torch.cuda.synchronize(self.dev)
            base = out.data_ptr()
            self._check(self.lib.mi_gp_kfold(self.h, nf, ptr.ctypes.data_as(ip), idx.ctypes.data_as(ip), work_p, need, base,
                                             base + 8 * nf if moments else None, base + 8 * (nf + total) if moments else None,
                                             info.ctypes.data_as(ip)), "mi_gp_kfold")
            o = out.cpu().numpy()
        if not moments:
            return o[:nf], None, None, info
        if sizes.min() == sizes.max():
            return o[:nf], list(o[nf : nf + total].reshape(nf, -1)), list(o[nf + total :].reshape(nf, -1)), info
        cuts = ptr[1:-1]
        return o[:nf], np.split(o[nf : nf + total], cuts), np.split(o[nf + total :], cuts), info

    def _drop_batch(self):
        """The batch buffers were sized for the old n: the next batch call re-creates them (mi_gp_append ended the batch state)."""
        self._bK = self._bZ = self._bW = self._bwork = None
        self._batch_k = 0
        self._batch_grad = False

    def _grow(self, need):
        """Re-allocate for at least `need` points (about 1.5x), rebind and refactorise once at the factored theta."""
        theta = self._factored_theta.copy()
        with torch.cuda.device(self.dev):
            X = self.X_t.clone()
            y = self.y_t.clone()
            diag = self._diag_t.clone() if getattr(self, "_diag_t", None) is not None else None
        self._drop_batch()
        self._work = self._work2 = None
        self._allocate(max(int(need), int(np.ceil(1.5 * self.n))), X, y, diag)
        self.np_ = self._padded(self.n)
        self.append_refactors += 1
        if self.factor(theta) != 0:
            raise FloatingPointError(f"covariance not positive definite at pivot {self.info} (refactorisation for append)")

    def _ensure_factored(self, theta):
        """Factorise unless the resident factor already belongs to this theta (BO sweeps, DE populations and
        refinement steps predict thousands of times at fixed hyper-parameters)."""
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if getattr(self, "_factored_ok", False) and np.array_equal(theta, self._factored_theta):
            return
        if self.factor(theta) != 0:
            raise FloatingPointError(f"covariance not positive definite at pivot {self.info}")

    def predict(self, theta, Xnew, pred_noise=True, chunk=16384, via_inverse=None):
        """Posterior mean and diagonal variance at Xnew (converted inputs), chunked over points.
        ``via_inverse``: use U = L^-T and one GEMM per chunk (mi_gp_predict_u) instead of the blocked triangular
        solve; default: when the gradient buffers exist and the sweep is large enough to pay for forming U
        (or U is already resident from an earlier sweep at this theta).  Under a trend (set_trend) the blocked solve is the only
        route: ``via_inverse=True`` raises ValueError.  Under several outputs the mean is (m, q); the variance is (m,), or (m, q)
        under set_output_cov("integrated")."""
        if via_inverse:
            self._no_trend("predict(via_inverse=True)")
            self._no_outputs("predict(via_inverse=True)")
        if self._trend != 0 or self.nout > 1:
            via_inverse = False
        self._ensure_factored(theta)
        Xnew = np.ascontiguousarray(Xnew, dtype=np.float64)
        if Xnew.ndim != 2 or Xnew.shape[1] != self.d:
            raise ValueError("Xnew must be (m, d)")
        m = Xnew.shape[0]
        if via_inverse is None:
            # U pays off for a large sweep, when it is already there, or from the third sweep on the same factor
            # (differential-evolution generations, refinement steps)
            self._pred_count = getattr(self, "_pred_count", 0) + 1
            via_inverse = self.Z_t is not None and (getattr(self, "_u_theta_ok", False) or 3 * m >= self.n
                                                    or self._pred_count >= 3)
        if via_inverse and self.Z_t is None:
            raise RuntimeError("this MiGP was created with need_grad=False")
        q = self.nout  # (q >= 2: mi_gp_predict writes q * mc means, output-major, and mc variances)
        qv = q if (self._outcov and q > 1) else 1  # (set_output_cov("integrated"): q * mc variances, output-major)
        mean = np.empty(m) if q == 1 else np.empty((m, q))
        var = np.empty(m) if qv == 1 else np.empty((m, q))
        with torch.cuda.device(self.dev):
            for s in range(0, m, chunk):
                mc = min(chunk, m - s)
                mp = (mc + 127) // 128 * 128
                rows = 2 * mp if via_inverse else mp
                if getattr(self, "_work", None) is None or self._work.shape[0] < rows:
                    self._work = torch.empty((rows, self.lda), dtype=torch.float64, device=self.dev)
                    torch.cuda.synchronize(self.dev)
                if mc <= self.PINNED_IO_MAX_POINTS:
                    # A few points (BO refinement steps, acquisition sweeps of small populations): the points go in and the
                    # moments come out through PINNED host memory the kernels address directly -- no torch copies, no torch
                    # synchronisation, one stream synchronisation inside the call (110 -> ~45 us per call at N = 512).  Same
                    # kernels on the same values: same bits as the device-buffer route below.
                    io = self._pinned_io(mc * self.d + (q + qv) * mc)
                    io_np = io.numpy()
                    io_np[: mc * self.d] = Xnew[s : s + mc].ravel()
                    base = io.data_ptr()
                    fn = self.lib.mi_gp_predict_u if via_inverse else self.lib.mi_gp_predict
                    self._check(fn(self.h, base, mc, self._work.data_ptr(), self.lda, base + 8 * mc * self.d,
                                   base + 8 * (mc * self.d + q * mc), 1 if pred_noise else 0),
                                "mi_gp_predict_u" if via_inverse else "mi_gp_predict")
                    if via_inverse:
                        self._u_theta_ok = True
                    mu = io_np[mc * self.d : mc * self.d + q * mc]
                    mean[s : s + mc] = mu if q == 1 else mu.reshape(q, mc).T
                    vr = io_np[mc * self.d + q * mc : mc * self.d + (q + qv) * mc]
                    var[s : s + mc] = vr if qv == 1 else vr.reshape(q, mc).T
                    continue
                xn = torch.from_numpy(Xnew[s : s + mc]).to(self.dev)
                mu_t = torch.empty(q * mc, dtype=torch.float64, device=self.dev)
                var_t = torch.empty(qv * mc, dtype=torch.float64, device=self.dev)
                torch.cuda.synchronize(self.dev)
                fn = self.lib.mi_gp_predict_u if via_inverse else self.lib.mi_gp_predict
                self._check(fn(self.h, xn.data_ptr(), mc, self._work.data_ptr(), self.lda, mu_t.data_ptr(),
                               var_t.data_ptr(), 1 if pred_noise else 0),
                            "mi_gp_predict_u" if via_inverse else "mi_gp_predict")
                if via_inverse:
                    self._u_theta_ok = True
                mean[s : s + mc] = mu_t.cpu().numpy() if q == 1 else mu_t.cpu().numpy().reshape(q, mc).T
                var[s : s + mc] = var_t.cpu().numpy() if qv == 1 else var_t.cpu().numpy().reshape(q, mc).T
        return mean, var

    def predict_grad(self, theta, Xnew, pred_noise=True, refactor=True):
        """Posterior mean / variance at a few points and their gradients w.r.t. the points:
        (mean[m], var[m], dmean[m,d], dvar[m,d]).  ``refactor=False`` reuses the resident factorisation
        (same theta as the previous predict / predict_grad call)."""
        self._no_trend("predict_grad")
        self._no_outputs("predict_grad")
        if self.Z_t is None:
            raise RuntimeError("this MiGP was created with need_grad=False")
        if refactor:
            self._factored_ok = False
        self._ensure_factored(theta)
        Xnew = np.ascontiguousarray(Xnew, dtype=np.float64)
        if Xnew.ndim != 2 or Xnew.shape[1] != self.d:
            raise ValueError("Xnew must be (m, d)")
        m = Xnew.shape[0]
        mp = (m + 127) // 128 * 128
        with torch.cuda.device(self.dev):
            if getattr(self, "_work2", None) is None or self._work2.shape[0] < 2 * mp:
                self._work2 = torch.empty((2 * mp, self.lda), dtype=torch.float64, device=self.dev)
                torch.cuda.synchronize(self.dev)
            if m <= self.PINNED_IO_MAX_POINTS:
                # (pinned I/O as in predict(): this is the call BO's refinement steps make once per optimiser iteration)
                nout = 2 * m + 2 * m * self.d
                io = self._pinned_io(m * self.d + nout)
                io_np = io.numpy()
                io_np[: m * self.d] = Xnew.ravel()
                base = io.data_ptr()
                o_p = base + 8 * m * self.d
                self._check(self.lib.mi_gp_predict_grad(self.h, base, m, self._work2.data_ptr(), self.lda, o_p, o_p + 8 * m,
                                                        1 if pred_noise else 0, o_p + 16 * m, o_p + 16 * m + 8 * m * self.d),
                            "mi_gp_predict_grad")
                o = io_np[m * self.d : m * self.d + nout].copy()
                return (o[:m], o[m : 2 * m], o[2 * m : 2 * m + m * self.d].reshape(m, self.d),
                        o[2 * m + m * self.d :].reshape(m, self.d))
            xn = torch.from_numpy(Xnew).to(self.dev)
            out = torch.empty((2 * m + 2 * m * self.d,), dtype=torch.float64, device=self.dev)
            torch.cuda.synchronize(self.dev)
            mu_p, var_p = out.data_ptr(), out.data_ptr() + 8 * m
            dmu_p, dvar_p = out.data_ptr() + 16 * m, out.data_ptr() + 16 * m + 8 * m * self.d
            self._check(self.lib.mi_gp_predict_grad(self.h, xn.data_ptr(), m, self._work2.data_ptr(), self.lda, mu_p, var_p,
                                                    1 if pred_noise else 0, dmu_p, dvar_p), "mi_gp_predict_grad")
            o = out.cpu().numpy()
        return (o[:m], o[m : 2 * m], o[2 * m : 2 * m + m * self.d].reshape(m, self.d),
                o[2 * m + m * self.d :].reshape(m, self.d))

    def mean_sweep(self, theta, Xnew, grad=False, chunk=1 << 20):
        """Posterior mean at Xnew (converted inputs) by the matrix-free sweep (option 53 of mi_gp_set_option): mu = sum_j k(x*, x_j)
        alpha_j, O(n d) per point with no work rows -- the route of sensitivity sweeps of 1e5 .. 1e7 points that read no variance.
        Returns mean (m,), or (mean, dmean (m, d)) with ``grad``: the gradient w.r.t. the points.  A point's bits do not depend on
        the other points, on its position or on ``chunk``.  d <= 128.  The option is 0 again afterwards."""
        self._no_trend("mean_sweep")
        self._no_outputs("mean_sweep")
        if self.Z_t is None:
            raise RuntimeError("this MiGP was created with need_grad=False")
        self._ensure_factored(theta)
        Xnew = np.ascontiguousarray(Xnew, dtype=np.float64)
        if Xnew.ndim != 2 or Xnew.shape[1] != self.d:
            raise ValueError("Xnew must be (m, d)")
        m, d = Xnew.shape
        chunk = max(1, int(chunk))
        mean = np.empty(m)
        dmean = np.empty((m, d)) if grad else None
        self.set_option(53, 1)
        try:
            with torch.cuda.device(self.dev):
                for s in range(0, m, chunk):
                    mc = min(chunk, m - s)
                    nout = mc + (mc * d if grad else 0)
                    if mc <= self.PINNED_IO_MAX_POINTS:  # (pinned I/O as in predict_grad)
                        io = self._pinned_io(mc * d + nout)
                        io_np = io.numpy()
                        io_np[: mc * d] = Xnew[s : s + mc].ravel()
                        x_p = io.data_ptr()
                        o_p = x_p + 8 * mc * d
                    else:
                        xn = torch.from_numpy(Xnew[s : s + mc]).to(self.dev)
                        out = torch.empty(nout, dtype=torch.float64, device=self.dev)
                        torch.cuda.synchronize(self.dev)
                        x_p, o_p = xn.data_ptr(), out.data_ptr()
                    self._check(self.lib.mi_gp_predict_grad(self.h, x_p, mc, None, 0, o_p, None, 0, o_p + 8 * mc if grad else None,
                                                            None), "mi_gp_predict_grad")
                    o = io_np[mc * d : mc * d + nout] if mc <= self.PINNED_IO_MAX_POINTS else out.cpu().numpy()
                    mean[s : s + mc] = o[:mc]
                    if grad:
                        dmean[s : s + mc] = o[mc:].reshape(mc, d)
        finally:
            self.set_option(53, 0)
        return (mean, dmean) if grad else mean

    # ---------------------------------------------------------------- posterior sample paths (options 54 / 55)
    # The factorisation serial: every assignment of _factored_ok -- factor(), update_data(), set_diag() and every call that
    # ends the factored state make one -- and every append() advance it.  A PathDraw remembers the serial it was conditioned on.
    @property
    def _factored_ok(self):
        return self.__dict__.get("_factored_flag", False)

    @_factored_ok.setter
    def _factored_ok(self, value):
        self.__dict__["_factored_flag"] = bool(value)
        self.__dict__["_path_serial"] = self.__dict__.get("_path_serial", 0) + 1

    @property
    def _path_serial(self):
        return self.__dict__.get("_path_serial", 0)

    def draw_paths(self, theta, npaths, nfeatures=4096, seed=None):
        """``npaths`` (1..128) posterior sample paths at theta by pathwise conditioning (paths.py; options 54 / 55 of
        mi_gp_set_option): a prior draw from ``nfeatures`` random Fourier features (a multiple of 16 in 16..65536) plus the
        update K(., X) K_y^-1 (y - prior(X) - eps), conditioned on the device against the resident factorisation.  Returns a
        paths.PathDraw, whose ``evaluate`` sweeps the draws matrix-free over any number of points, with their input gradients.
        The draws are of the latent f (add observation noise on the host).  Host draws come from
        np.random.Generator(np.random.Philox(seed)) in the order of paths.draw_block_parts: the same seed gives the same block;
        ``seed`` None takes one from the OS.  d <= 32.  Option 54 is 0 again afterwards."""
        from . import paths

        self._no_trend("draw_paths")
        self._no_outputs("draw_paths")
        if self.Z_t is None:
            raise RuntimeError("this MiGP was created with need_grad=False")
        if self.d > paths.MAX_D:
            raise ValueError(f"draw_paths needs d <= {paths.MAX_D}, got {self.d}")
        S, F = paths.check_counts(npaths, nfeatures)
        self._ensure_factored(theta)
        if seed is None:
            seed = int(np.random.SeedSequence().generate_state(2, dtype=np.uint64)[0])
        diag = self._diag_t.cpu().numpy() if getattr(self, "_diag_t", None) is not None else None
        omega, b, W, E, _ = paths.draw_block_parts(self.kerns, self.ops, self._factored_theta, self.d, self.n, S, F, seed, diag)
        ldw = paths.block_ldw(S)
        with torch.cuda.device(self.dev):
            block = torch.from_numpy(paths.pack_block(omega, b, W, E, ldw)).to(self.dev)
            torch.cuda.synchronize(self.dev)
            with self._options({55: F, 54: S}, leave={55: F, 54: 0}):  # the conditioning call: m = 0, pred_noise read as `condition`
                self._check(self.lib.mi_gp_predict_grad(self.h, None, 0, block.data_ptr(), ldw, None, None, 1, None, None),
                            "mi_gp_predict_grad")
        return paths.PathDraw(self, block, S, F, ldw, seed, self._path_serial)

    # ---------------------------------------------------------------- joint conditional and posterior draws
    # One call per request, nothing chunked: device memory bounds M.  predict_cov holds Sigma (mp^2 doubles, mp = M rounded up
    # to 128) beside the cross-covariance rows (mp x (padded n + 16)); sample_posterior adds mi_gp_sample_cov_work(M, s) =
    # mp / 128 * 16384 + 2 * ceil(s/128)*128 * mp doubles.  At N = 4096 and one draw that is ~8 GB at M = 30 000 and ~83 GB
    # at M = 100 000.

    def _prior_variance(self):
        """kd: the +/* fold of the components' kv, the composite prior variance (Stationary.diag == 1)."""
        th = self._factored_theta
        kv = th[self.nkern * self.d : self.nkern * self.d + self.nkern]
        kd = float(kv[0])
        for i, op in enumerate(self.ops):
            kd = kd + float(kv[i + 1]) if op == "+" else kd * float(kv[i + 1])
        return kd

    def _joint_device(self, Xnew, pred_noise):
        """mi_gp_predict_cov at the resident factor: (mean tensor [m], Sigma tensor [mp, mp] with its lower triangle set)."""
        Xnew = np.ascontiguousarray(Xnew, dtype=np.float64)
        if Xnew.ndim != 2 or Xnew.shape[1] != self.d:
            raise ValueError("Xnew must be (m, d)")
        if not np.isfinite(Xnew).all():
            raise ValueError("Xnew must be finite")
        m = Xnew.shape[0]
        if m < 1:
            raise ValueError("Xnew must hold at least one point")
        mp = (m + 127) // 128 * 128
        with torch.cuda.device(self.dev):
            if getattr(self, "_work", None) is None or self._work.shape[0] < mp:
                self._work = None
                self._work = torch.empty((mp, self.lda), dtype=torch.float64, device=self.dev)
            xn = torch.from_numpy(Xnew).to(self.dev)
            mu_t = torch.empty(m, dtype=torch.float64, device=self.dev)
            cov_t = torch.empty((mp, mp), dtype=torch.float64, device=self.dev)
            torch.cuda.synchronize(self.dev)
            self._check(self.lib.mi_gp_predict_cov(self.h, xn.data_ptr(), m, self._work.data_ptr(), self.lda, mu_t.data_ptr(),
                                                   cov_t.data_ptr(), mp, 1 if pred_noise else 0), "mi_gp_predict_cov")
        return mu_t, cov_t

    def predict_cov(self, theta, Xnew, pred_noise=True):
        """Posterior mean and JOINT covariance at Xnew (converted inputs): PyMC's gp.predict(Xnew, diag=False, pred_noise=...)
        -- Sigma = K(X*, X*) - A^T A with A = L^-1 K(X, X*), plus sqrt(gv)^2 I with pred_noise, else jitter I.  Returns
        (mu [M], cov [M, M]), cov symmetric (mirrored from the lower triangle the device computes); mu is predict()'s mean
        through the blocked solve, bit for bit."""
        self._no_trend("predict_cov")
        self._no_outputs("predict_cov")
        self._ensure_factored(theta)
        mu_t, cov_t = self._joint_device(Xnew, pred_noise)
        m = mu_t.shape[0]
        low = np.tril(cov_t[:m, :m].cpu().numpy())
        return mu_t.cpu().numpy(), low + np.tril(low, -1).T

    DESIGN_MAX_BATCH = 128  # points one design call selects (option 56)

    def design(self, theta, Xcand, Xref=None, batch=1, noise=True):
        """Greedy variance-reduction design at theta (options 56 / 57 of mi_gp_set_option): up to ``batch`` (1..128) of the
        candidates ``Xcand`` (converted inputs, (Mc, d)), each the one whose observation lowers the latent posterior variance
        averaged over the reference sample ``Xref`` (Mr, d) the most, given the ones chosen before it (integrated variance
        reduction, ALC: Cohn 1996).  The gain of c is mean_r cov(c, r)^2 / v(c) with v(c) = var_latent(c) + jitter, plus gv with
        ``noise`` -- exactly the drop of that average after ``append`` of one observation at c, whatever its value.
        ``Xref=None``: the plain maximum-variance criterion, gain = var_latent.  Returns (indices, gains, gains0): the chosen
        candidates in order (fewer than ``batch`` when no candidate is left or no gain is positive), their gains at the moment
        of choice and the round-0 gains of all candidates (NaN where v is not a finite positive number).  No resident state
        changes; both options are what they were afterwards."""
        self._no_trend("design")
        self._no_outputs("design")
        if getattr(self, "_diag_t", None) is not None:
            raise ValueError("design has no form under a per-point diagonal (set_diag is in force): set_diag(None) first")
        batch = int(batch)
        if not 1 <= batch <= self.DESIGN_MAX_BATCH:
            raise ValueError(f"batch must lie in 1..{self.DESIGN_MAX_BATCH}")
        Xcand = np.ascontiguousarray(Xcand, dtype=np.float64)
        if Xcand.ndim != 2 or Xcand.shape[1] != self.d or Xcand.shape[0] < 1:
            raise ValueError("Xcand must be (Mc, d) with Mc >= 1")
        if Xref is None:
            Xref = np.empty((0, self.d))
        Xref = np.ascontiguousarray(Xref, dtype=np.float64)
        if Xref.ndim != 2 or Xref.shape[1] != self.d:
            raise ValueError("Xref must be (Mr, d)")
        if not (np.isfinite(Xcand).all() and np.isfinite(Xref).all()):
            raise ValueError("Xcand and Xref must be finite")
        self._ensure_factored(theta)
        mc, mr = Xcand.shape[0], Xref.shape[0]
        mcp, mrp = self._padded(mc), self._padded(mr)
        with torch.cuda.device(self.dev):
            if getattr(self, "_work", None) is None or self._work.shape[0] < mcp + mrp:
                self._work = None
                self._work = torch.empty((mcp + mrp, self.lda), dtype=torch.float64, device=self.dev)
            xn = torch.from_numpy(np.concatenate([Xcand, Xref])).to(self.dev)
            out_t = torch.empty(mc + 2 * batch + 1, dtype=torch.float64, device=self.dev)
            g_t = torch.empty((mcp, mrp), dtype=torch.float64, device=self.dev) if mr else None
            torch.cuda.synchronize(self.dev)
            with self._options({57: mr, 56: batch}):
                self._check(self.lib.mi_gp_predict_cov(self.h, xn.data_ptr(), mc + mr, self._work.data_ptr(), self.lda, out_t.data_ptr(),
                                                       g_t.data_ptr() if mr else None, mrp, 1 if noise else 0), "mi_gp_predict_cov")
            o = out_t.cpu().numpy()
        count = int(o[-1])
        return o[mc : mc + count].astype(np.int64), o[mc + batch : mc + batch + count].copy(), o[:mc].copy()

    SAMPLE_JITTER_STEPS = (1e-12, 1e-10, 1e-8, 1e-6, 1e-4)  # extra diagonal (x kd) of sample_posterior's retries

    def sample_posterior(self, theta, Xnew, nsamples, seed=None, pred_noise=False, offset=None):
        """``nsamples`` joint draws of the posterior at Xnew (converted inputs), an (nsamples, M) array: mean + L_Sigma z with
        Sigma = predict_cov's joint covariance -- of the latent f by default (pred_noise=False, the target of Thompson
        sampling), of noisy observations with pred_noise=True.  z is the counter-based Philox stream of mi_gp_sample_cov:
        ``seed`` None takes one from the OS once per handle; the handle keeps the stream offset and advances it by every call,
        so repeated calls give fresh draws (``offset`` overrides it; the same seed and offset give the same bits).  If Sigma
        is not positive definite, it is rebuilt and factored again with an extra diagonal of 1e-12 kd, 1e-10 kd, ... up to
        1e-4 kd (kd the composite prior variance), then FloatingPointError.  ``self.sample_info`` records the seed, offset and
        extra jitter used."""
        self._no_trend("sample_posterior")
        self._no_outputs("sample_posterior")
        nsamples = int(nsamples)
        if nsamples < 1:
            raise ValueError("nsamples must be >= 1")
        self._ensure_factored(theta)
        if seed is None:
            if getattr(self, "_philox_seed", None) is None:
                self._philox_seed = int(np.random.SeedSequence().entropy) & (2 ** 64 - 1)
            seed = self._philox_seed
        seed = int(seed) & (2 ** 64 - 1)
        off = int(getattr(self, "_philox_offset", 0) if offset is None else offset)
        if not 0 <= off < 2 ** 64:
            raise ValueError("offset must lie in [0, 2^64)")
        mu_t, cov_t = self._joint_device(Xnew, pred_noise)
        m, mp = mu_t.shape[0], cov_t.shape[0]
        kd = self._prior_variance()
        need = int(self.lib.mi_gp_sample_cov_work(m, nsamples))
        with torch.cuda.device(self.dev):
            work = torch.empty(need, dtype=torch.float64, device=self.dev)
            draws = torch.empty((nsamples, m), dtype=torch.float64, device=self.dev)
            torch.cuda.synchronize(self.dev)
            jitters = (0.0,) + tuple(f * kd for f in self.SAMPLE_JITTER_STEPS)
            for attempt, ej in enumerate(jitters):
                if attempt > 0:  # the failed factorisation overwrote Sigma: rebuild it
                    mu_t, cov_t = self._joint_device(Xnew, pred_noise)
                r = self._check(self.lib.mi_gp_sample_cov(self.h, cov_t.data_ptr(), mp, m, mu_t.data_ptr(), ej, nsamples, seed, off,
                                                          draws.data_ptr(), m, work.data_ptr(), need), "mi_gp_sample_cov")
                if r == 0:
                    break
            else:
                raise FloatingPointError(f"joint covariance not positive definite with an extra diagonal of {jitters[-1]:.3g} "
                                         f"(pivot {r})")
            out = draws.cpu().numpy()
        self._philox_offset = (off + (nsamples * m + 3) // 4) % 2 ** 64
        self.sample_info = {"seed": seed, "offset": off, "extra_jitter": ej, "attempts": attempt + 1}
        return out

    PINNED_IO_MAX_POINTS = 256  # predict / predict_grad: up to this many points travel through pinned host memory

    def _pinned_io(self, nelem):
        """A pinned (page-locked, device-visible) host buffer of at least nelem doubles, grown on demand."""
        buf = getattr(self, "_pin_io", None)
        if buf is None or buf.numel() < nelem:
            buf = torch.empty(max(int(nelem), 4096), dtype=torch.float64).pin_memory()
            self._pin_io = buf
        return buf

    def set_option(self, what, value):
        """Per-handle tuning knobs (include/mi_gp.h: 0 look-ahead, 2 super-panel width, 7 small-tile threshold,
        8 one-workgroup-per-CU bulk updates, 14 tile order); unknown ids raise."""
        self._check(self.lib.mi_gp_set_option(self.h, int(what), int(value)), "mi_gp_set_option")
        if int(what) == 52 and int(value) != self._outcov:
            # (predict sizes its variance from this mirror of the option; a change ends the resident factorisation)
            self._outcov = int(value)
            self._factored_ok = False
            self._u_theta_ok = False

    @contextlib.contextmanager
    def _options(self, values, leave=None):
        """Options set for the length of a ``with`` block: ``values`` {id: value} are set in their order; on the way out, in
        reverse order, every id that was set gets back the value it had on entry, or the one ``leave`` {id: value} names for it.
        About 1 us of Python per use: mean_sweep and PathDraw.evaluate, whose calls take tens of us, set their option inline."""
        restore = []
        try:
            for what, value in values.items():
                old = leave[what] if leave and what in leave else self.get_option(what)
                self.set_option(what, value)
                restore.append((what, old))  # (a refused value changed nothing: nothing to put back)
            yield
        finally:
            for what, old in reversed(restore):
                self.set_option(what, old)

    def get_option(self, what, default=None):
        """Current value of a knob on this handle, the library's own defaults included (mi_gp_get_option; 40: 1 once the handle
        has switched its cross-stream edges to events by itself).  `default` for ids the library does not know."""
        out = ctypes.c_int()
        if self.lib.mi_gp_get_option(self.h, int(what), ctypes.byref(out)) != 0:
            return default
        return out.value

    def last_error(self):
        """Text of the handle's last error or notice (a demotion of the cross-stream edges is reported here once)."""
        return self.lib.mi_gp_last_error(self.h).decode()

    def set_profiling(self, level):
        self.lib.mi_gp_set_profiling(self.h, int(level))

    def timers(self):
        out = (ctypes.c_double * 17)()
        self.lib.mi_gp_timers(self.h, out, 17)
        keys = ["assemble_ms", "cholesky_ms", "reduce_ms", "total_ms", "gemm_ms", "gemm_flops", "gemm_launches",
                "trtri_ms", "lauum_ms", "contract_ms", "gemm_b_ms", "gemm_b_flops", "gemm_b_launches", "enqueue_ms",
                "logpdf_block_ms", "logpdf_weights_ms", "logpdf_grad_ms"]
        return dict(zip(keys, list(out)))

    def close(self):
        if getattr(self, "h", None) is not None:
            self.lib.mi_gp_destroy(self.h)  # synchronises the handle's streams first
            self.h = None
        # the device buffers the handle borrowed (a batch holds K-fold copies of K, U, K^-1)
        for name in ("_bK", "_bZ", "_bW", "_bwork", "K_t", "Z_t", "W_t", "_work", "_work2", "_gx_t", "_pin_io", "_awork", "_lwork", "_X_store",
                     "_y_store", "_diag_store", "_Y_store"):
            if hasattr(self, name):
                setattr(self, name, None)
        self._batch_k = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
