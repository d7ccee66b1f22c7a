"""A state model of one GP handle, seeded random walks over its entry points, and a NumPy stand-in with the same call surface.

include/mi_gp.h documents the handle's resident state in prose: which call leaves a factor, U = L^-T or K^-1 behind, which call
ends them, and which calls are refused (-1) meanwhile.  ``Model`` is that prose as a state machine -- written from the header's
sentences, not from api_gp.hip -- and ``walk`` draws operation sequences over it.  ``run_walk`` drives any object with the call
surface of ``OracleHandle`` (the NumPy stand-in here, the ctypes adapter of tests/test_gpu_handle_sequences.py on the device)
through a walk and checks EVERY call: its return code against the model, its values against oracle/gp_oracle.py at the
(data version, n, diagonal, theta) the model says is resident, and its bits against the first answer of the same query in the same
resident state.  A missed invalidation shows as a wrong return code or as a value of another key.

``FacadeModel`` / ``facade_walk`` / ``run_facade_walk`` do the same for andvaranaut_amd.backend.MiGP, which never refuses (it
refactorises by itself): values against the oracle, and the NUMBER of factorisations against the model's minimum.

Not a conftest and not a test module: tests/test_handle_model_host.py proves the model, the walks and the tolerances against the
stand-in (and that ten deliberately wrong stand-ins are caught); tests/test_gpu_handle_sequences.py runs the device."""
import numpy as np
import scipy.linalg as sla
from scipy.linalg import lapack

from oracle import gp_oracle as orc

EPS = 2.2e-16
SCHED_OPTIONS = (8, 14, 16, 18, 19, 21, 26, 30, 31, 38, 45, 47)  # include/mi_gp.h: "only change scheduling (bit-identical results)"
OPTION_VALUES = {8: (0, 4, 64), 14: (0, 4, 8), 16: (0, 1), 18: (0, 512, 1536), 19: (0, 1024), 21: (0, 8, 30), 26: (0, 1, 2),
                 30: (0, 16), 31: (8, 48), 38: (1, 4, 8), 45: (0, 1), 47: (0, 2000)}
SIZES = {
    100: dict(kernel="Matern52", d=2, cap=120, kapp=7, steps=96),        # one tile
    300: dict(kernel="RBF+Matern32", d=3, cap=420, kapp=50, steps=96),   # appends cross the 384-row tile boundary
    700: dict(kernel="RatQuad", d=5, cap=760, kapp=20, steps=96),
    2600: dict(kernel="Matern52", d=4, cap=2650, kapp=25, steps=12),     # two streams from the start
}
DEFAULT_SEEDS = (0, 1, 2)
M_NEW = 6          # prediction points of every query
M_SAMPLE, S_SAMPLE = 5, 3  # mi_gp_sample_cov: points and draws of the fixed test covariance
BATCH_COUNT = 3    # members the batch buffers hold; k = 4 is "above the count"
N_GOOD = 3         # good thetas 0 .. 2
BAD = 3            # theta index with a negative jitter: info > 0
MEMBERS = ((0, 1, 2, 0), (1, 2, 0, 1), (2, BAD, 0, 1), (0, 0, 1, 2))  # theta index of batch member p, by the op's `shift`
DUP_ROW = 17       # the point a "dup" append repeats

CHANGERS = ("set_data", "set_diag", "lml", "lml_grad", "factor", "reserve", "append", "set_batch", "lml_batch",
            "lml_grad_batch", "factor_batch")
CONSUMERS = ("alpha", "grad_x", "lml_parts", "predict", "predict_u", "predict_grad", "predict_cov", "append", "predict_batch")
ALL_OPS = ("set_data", "set_diag", "lml", "lml_grad", "alpha", "grad_x", "lml_parts", "factor", "predict", "predict_u",
           "predict_grad", "predict_cov", "sample_cov", "reserve", "append", "set_batch", "lml_batch", "lml_grad_batch",
           "factor_batch", "predict_batch", "set_option")
REFUSALS = ("unbound", "no_factor", "no_kinv", "no_parts", "reserve_below_n", "append_no_factor", "append_over_capacity",
            "set_batch_unbound", "batch_unbound", "batch_k_over_count", "batch_no_zw", "predict_batch_no_factors",
            "predict_batch_k_mismatch")


def split_kernel(kernel):
    import re

    return re.split(r"[+*]", kernel), [c for c in kernel if c in "+*"]


def padded(n):
    return (int(n) + 127) // 128 * 128


# ------------------------------------------------------------------------------------------------------------ the problem
class Problem:
    """Everything a walk over one size reads: data versions, thetas, diagonals, query points -- all pure functions of the size."""

    def __init__(self, size, cfg=None):
        c = cfg or SIZES[size]  # (cfg: a size outside the walks' table, tests/test_gpu_handle_layouts.py)
        self.size, self.n0, self.cap, self.kapp, self.d = size, size, c["cap"], c["kapp"], c["d"]
        self.kernel = c["kernel"]
        self.kerns, self.ops = split_kernel(self.kernel)
        self.nk = len(self.kerns)
        self.ntheta = self.nk * self.d + 2 * self.nk + 2
        self.rows = self.cap + 128  # (an "over capacity" append reads valid rows behind the capacity)
        self._data, self._diag = {}, {}
        self.xnew = np.random.default_rng(9000 + size).random((M_NEW, self.d)) * 1.1 - 0.05
        r = np.random.default_rng(31 + size)
        a = r.standard_normal((M_SAMPLE, M_SAMPLE))
        self.sample_cov = np.tril(a @ a.T + M_SAMPLE * np.eye(M_SAMPLE))
        self.sample_mean = r.standard_normal(M_SAMPLE)
        self.sample_jitter = 1e-9

    def data(self, ver):
        if ver not in self._data:
            r = np.random.default_rng(100000 * self.size + ver)
            X = r.random((self.rows, self.d))
            y = (np.sin(3.0 * X.sum(1)) + (X ** 2).sum(1) / self.d + r.normal(0.0, 1e-2, self.rows) - 0.5) / 0.7
            self._data[ver] = (np.ascontiguousarray(X), np.ascontiguousarray(y))
        return self._data[ver]

    def diag(self, diag_id):
        if diag_id is None:
            return None
        if diag_id not in self._diag:
            self._diag[diag_id] = np.random.default_rng(77 + diag_id).uniform(1e-4, 2e-3, self.rows)
        return self._diag[diag_id]

    def theta(self, ti):
        gv = (1e-3, 3e-4, 1e-4, 1e-4)[ti]
        th = orc.synth_theta(self.d, nkern=self.nk, gv=gv, jitter=1e-6)
        th[: self.nk * self.d] *= (1.0, 1.25, 0.85, 1.0)[ti]
        th[self.nk * self.d: self.nk * self.d + self.nk] = (1.7, 1.2, 0.9, 1.7)[ti]
        if "RatQuad" in self.kerns:
            th[self.nk * self.d + self.nk: self.nk * self.d + 2 * self.nk] = 1.3
        if ti == BAD:  # K + (gv + jitter) I with jitter = -kd / 2: two points correlated above 1/2 give a negative pivot
            th[-1] = -0.5 * orc.kernel_diag(self.kerns, self.ops, th, self.d)
        return th

    def thetas(self, shift, k):
        return np.array([self.theta(MEMBERS[shift][p]) for p in range(k)])

    def dup_diag(self, ti, diag_id):
        """Diagonal entry of a "dup" append (a copy of point DUP_ROW): it takes the copy's noise away and 1e-3 more.  The Schur
        complement of the copy is gv + jitter + dnew + s (1 - s (K^-1)_jj) with s = gv + jitter + diag_j in [0, s]: at most
        -(gv + jitter) - diag_j - 1e-3 here, a negative pivot far from rounding, at the 1-based index n + 1."""
        th = self.theta(ti)
        return -3.0 * (th[-2] + th[-1]) - 2.0 * self.diag(diag_id)[DUP_ROW] - 1e-3


# ------------------------------------------------------------------------------------------------------------- the oracle
def first_bad_pivot(K):
    """LAPACK dpotrf's info of the lower factorisation: 0, or the 1-based index of the first non-positive pivot."""
    _, info = lapack.dpotrf(K, lower=1, overwrite_a=0)
    return int(info)


class Oracle:
    """oracle/gp_oracle.py results, cached by (data version, n, diagonal id, theta index)."""

    def __init__(self, problem):
        self.p = problem
        self._marg, self._grad, self._cond, self._dup = {}, {}, {}, {}

    def _args(self, key):
        ver, n, diag_id, ti = key
        X, y = self.p.data(ver)
        dg = self.p.diag(diag_id)
        return X[:n], y[:n], (None if dg is None else dg[:n]), self.p.theta(ti)

    def _condnum(self, K, L):
        if K.shape[0] <= 1200:
            w = np.linalg.eigvalsh(K)
            return float(w[-1] / w[0])
        return float(orc.cond2_spd(L))

    def marg(self, key):
        """Marginal form (mi_gp_lml / mi_gp_lml_grad): info, lml, logdet, quad, cond."""
        if key not in self._marg:
            X, y, dg, th = self._args(key)
            K = orc.noisy_cov(X, self.p.kerns, self.p.ops, th, "marginal", dg)
            info = first_bad_pivot(K)
            r = {"info": info}
            if info == 0:
                val, L, beta = orc.lml(X, y, self.p.kerns, self.p.ops, th, "marginal", return_parts=True, extra_diag=dg)
                r.update(lml=val, logdet=float(np.sum(np.log(np.diag(L)))), quad=float(beta @ beta), cond=self._condnum(K, L))
            self._marg[key] = r
        return self._marg[key]

    def grad(self, key):
        """dLML/dtheta, alpha = K^-1 y and dLML/dX of the marginal form."""
        if key not in self._grad:
            X, y, dg, th = self._args(key)
            _, g = orc.lml_grad(X, y, self.p.kerns, self.p.ops, th, extra_diag=dg)
            _, my, gx = orc.lml_grad_data(X, y, self.p.kerns, self.p.ops, th, extra_diag=dg)
            self._grad[key] = {"grad": g, "alpha": -my, "gx": gx}
        return self._grad[key]

    def cond(self, key):
        """Conditional form (mi_gp_factor): info, logdet, quad, cond, and every prediction at the problem's query points."""
        if key not in self._cond:
            X, y, dg, th = self._args(key)
            p = self.p
            K = orc.noisy_cov(X, p.kerns, p.ops, th, "conditional", dg)
            info = first_bad_pivot(K)
            r = {"info": info}
            if info == 0:
                L = sla.cholesky(K, lower=True)
                beta = sla.solve_triangular(L, y, lower=True)
                r.update(logdet=float(np.sum(np.log(np.diag(L)))), quad=float(beta @ beta), cond=self._condnum(K, L))
                A = sla.solve_triangular(L, orc.kernel_matrix(X, p.xnew, p.kerns, p.ops, th), lower=True)
                _, _, _, gv, _ = orc.split_theta(th, p.d, p.nk)
                r["mean"] = A.T @ beta
                r["var"] = orc.kernel_diag(p.kerns, p.ops, th, p.d) - np.sum(A * A, 0) + np.sqrt(gv) ** 2
                r["cov"] = np.tril(orc.sigma_joint(X, p.xnew, p.kerns, p.ops, th, True, L=L))
                r["dmean"], r["dvar"] = self._predict_grad(X, L, sla.cho_solve((L, True), y), th)
                r["kd"] = float(orc.kernel_diag(p.kerns, p.ops, th, p.d))
            self._cond[key] = r
        return self._cond[key]

    def _predict_grad(self, X, L, a, theta):
        """oracle.predict_grad's sums with the caller's factor (it has no per-point diagonal of its own)."""
        p = self.p
        ls, kv, alpha, _, _ = orc.split_theta(theta, p.d, p.nk)
        dmu, dvar = np.zeros((M_NEW, p.d)), np.zeros((M_NEW, p.d))
        for q in range(M_NEW):
            xs = p.xnew[q: q + 1]
            comps, r2s = orc.component_matrices(X, xs, p.kerns, ls, kv, alpha)
            w = sla.cho_solve((L, True), orc.combine(comps, p.ops)[:, 0])
            pref, T = [np.ones_like(comps[0])], comps[0]
            for i in range(1, p.nk):
                pref.append(np.ones_like(T) if p.ops[i - 1] == "+" else T.copy())
                T = T + comps[i] if p.ops[i - 1] == "+" else T * comps[i]
            for c in range(p.nk):
                coef = pref[c]
                for i in range(c + 1, p.nk):
                    if p.ops[i - 1] == "*":
                        coef = coef * comps[i]
                dk = kv[c] * orc.base_kernel_dr2(p.kerns[c], r2s[c], alpha[c])
                g = (coef * np.where(r2s[c] > 0.0, dk, 0.0))[:, 0]
                for m in range(p.d):
                    dkx = g * 2.0 * (xs[0, m] - X[:, m]) / ls[c, m] ** 2
                    dmu[q, m] += a @ dkx
                    dvar[q, m] += -2.0 * (w @ dkx)
        return dmu, dvar

    def dup_pivot(self, key):
        """dpotrf's info for the data of `key` plus a copy of point DUP_ROW with Problem.dup_diag on its diagonal."""
        if key not in self._dup:
            X, y, dg, th = self._args(key)
            X2 = np.vstack([X, X[DUP_ROW: DUP_ROW + 1]])
            d2 = np.concatenate([dg, [self.p.dup_diag(key[3], key[2])]])
            self._dup[key] = first_bad_pivot(orc.noisy_cov(X2, self.p.kerns, self.p.ops, th, "conditional", d2))
        return self._dup[key]

    def sample_draws(self, seed, offset):
        from test_predict_joint_host import philox_normals

        p = self.p
        S = p.sample_cov + np.tril(p.sample_cov, -1).T
        L = sla.cholesky(S + p.sample_jitter * np.eye(M_SAMPLE), lower=True)
        z = philox_normals(seed, offset, S_SAMPLE * M_SAMPLE).reshape(S_SAMPLE, M_SAMPLE)
        return p.sample_mean[None, :] + z @ L.T, L, z


# -------------------------------------------------------------------------------------------------------------- the model
class Expect:
    """What a call must do.  rc: 0, -1 or "info" (the oracle's first non-positive pivot, looked up by the harness); `refusal`:
    which documented rule refuses it; `key`: the oracle key of its values; `bits`: output name -> identity of the resident state the
    bits depend on (the same identity twice = the same bits)."""

    def __init__(self, rc, refusal=None, key=None, bits=None, extra=None):
        self.rc, self.refusal, self.key, self.bits, self.extra = rc, refusal, key, bits or {}, extra or {}


class Model:
    """The handle's state as include/mi_gp.h states it.  Each rule cites its sentence."""

    def __init__(self, problem):
        self.p = problem
        self.bound = False
        self.n, self.cap = problem.n0, problem.n0  # "Without [mi_gp_reserve] a handle cannot grow"
        self.ver, self.next_ver = 0, 1
        self.diag_id, self.next_diag = None, 0
        self.fact = None    # identity of the resident conditional factor: (ver, diag, ti, n at mi_gp_factor, appends)
        self.u_at = None    # n at which U = L^-T became resident
        self.kinv = None    # oracle key of the resident K^-1
        self.parts = None   # (form, oracle key, identity) behind mi_gp_lml_parts
        self.batch = None   # bound batch: dict(count, zw, alias)
        self.bcond = None   # (k, shift, n): the batch's conditional factors
        self.min_factorisations = 0

    # ---- helpers
    def key(self, ti):
        return (self.ver, self.n, self.diag_id, ti)

    def fact_key(self):
        ver, diag_id, ti, _, _ = self.fact
        return (ver, self.n, diag_id, ti)

    def _end_single(self):
        self.fact = self.u_at = self.kinv = None

    def _single_eval_begins(self):
        # "mi_gp_lml, mi_gp_lml_grad and mi_gp_factor ... each of them, whether it succeeds, returns info > 0 or is refused for
        #  its theta, ends what an earlier one left resident -- the factor of mi_gp_factor, U and K^-1."
        self._end_single()
        self.parts = None  # "Returns -1 ... while the last one returned info > 0 or -1"
        if self.batch and self.batch["alias"]:
            # "with overlapping buffers it also ends the batch's conditional factors"
            self.bcond = None

    # ---- one operation
    def step(self, op):
        name = op[0]
        return getattr(self, "_" + name)(*op[1:])

    def _set_data(self, how):
        # "Every call ends the handle's resident state ... whether or not the pointers changed: mi_gp_predict*, mi_gp_predict_cov
        #  and mi_gp_append return -1 until the next mi_gp_factor, mi_gp_alpha and mi_gp_grad_x until the next mi_gp_lml_grad."
        self.bound = True
        self._end_single()
        self.bcond = None  # "(mi_gp_set_batch, mi_gp_set_data and mi_gp_set_diag also end it)"
        if how == "new":
            self.ver, self.next_ver = self.next_ver, self.next_ver + 1
        return Expect(0)

    def _set_diag(self, how):
        # "Every call, a repeated pointer included, ends the resident state like mi_gp_set_data ... May be called before
        #  mi_gp_set_data."
        self._end_single()
        self.bcond = None
        if how == "vec":
            self.diag_id, self.next_diag = self.next_diag % 2, self.next_diag + 1
        else:
            self.diag_id = None
        return Expect(0)

    def _single(self, ti, form):
        if not self.bound:
            self._single_eval_begins()
            return Expect(-1, "unbound")  # "Before the first mi_gp_set_data they return -1."
        self._single_eval_begins()
        return None

    def _lml(self, ti):
        r = self._single(ti, "marginal")
        if r:
            return r
        k = self.key(ti)
        if ti == BAD:
            return Expect("info", key=k, extra={"form": "marginal"})
        self.parts = ("marginal", k, ("lml",) + k)
        return Expect(0, key=k, bits={"lml": ("lml",) + k})

    def _lml_grad(self, ti):
        r = self._single(ti, "marginal")
        if r:
            return r
        k = self.key(ti)
        if ti == BAD:
            return Expect("info", key=k, extra={"form": "marginal"})
        self.kinv = k  # "at the theta of the last successful mi_gp_lml_grad (K^-1 and alpha still resident)"
        self.parts = ("marginal", k, ("lml_grad",) + k)
        self.min_factorisations += 1
        return Expect(0, key=k, bits={"lml": ("lml_grad.v",) + k, "grad": ("lml_grad.g",) + k})

    def _factor(self, ti):
        r = self._single(ti, "conditional")
        if r:
            return r
        k = self.key(ti)
        if ti == BAD:
            return Expect("info", key=k, extra={"form": "conditional"})
        self.fact = (self.ver, self.diag_id, ti, self.n, ())  # "keep L and beta = L^-1 y on the device for mi_gp_predict"
        self.parts = ("conditional", k, ("factor",) + self.fact)
        return Expect(0, key=k)

    def _alpha(self):
        if self.kinv is None:
            return Expect(-1, "no_kinv")
        return Expect(0, key=self.kinv, bits={"alpha": ("alpha",) + self.kinv})

    def _grad_x(self):
        if self.kinv is None:
            return Expect(-1, "no_kinv")
        return Expect(0, key=self.kinv, bits={"gx": ("gx",) + self.kinv})

    def _lml_parts(self):
        # "Returns -1, and writes neither output, before the first single evaluation and while the last one returned info > 0 or -1."
        if self.parts is None:
            return Expect(-1, "no_parts")
        form, k, ident = self.parts
        return Expect(0, key=k, bits={"logdet": ("logdet",) + ident, "quad": ("quad",) + ident}, extra={"form": form})

    def _needs_factor(self):
        return Expect(-1, "no_factor") if self.fact is None else None

    def _predict(self):
        # "mi_gp_predict changes no handle state"
        return self._needs_factor() or Expect(0, key=self.fact_key(), bits={"mean": ("mean", self.fact), "var": ("var", self.fact)})

    def _with_u(self, tag):
        r = self._needs_factor()
        if r:
            return r
        if self.u_at is None:  # "leave U = L^-T (and alpha) resident beside the factor and change nothing else"
            self.u_at = self.n
        ident = (self.fact, self.u_at)
        return Expect(0, key=self.fact_key(), bits={n_: (tag + "." + n_,) + ident for n_ in
                                                   (("mean", "var") if tag == "pu" else ("mean", "var", "dmean", "dvar"))})

    def _predict_u(self):
        return self._with_u("pu")

    def _predict_grad(self):
        return self._with_u("pg")

    def _predict_cov(self):
        # "mean_dev (m doubles) = mi_gp_predict's mean bit for bit ...  The handle's state is not changed."
        return self._needs_factor() or Expect(0, key=self.fact_key(), bits={"mean": ("mean", self.fact), "cov": ("cov", self.fact)})

    def _sample_cov(self, seed, offset):
        # "changes NO handle state" and "the same (seed, offset) gives the same bits"
        return Expect(0, bits={"draws": ("draws", seed, offset)})

    def _reserve(self, cap):
        if cap < self.n:
            return Expect(-1, "reserve_below_n")  # "-1 if capacity < n"
        self.cap = max(self.cap, cap)  # "(resident contents kept)"
        return Expect(0)

    def append_k(self, how):
        return {"ok": self.p.kapp, "over": self.cap - self.n + 1, "dup": 1}[how]

    def _append(self, how):
        k = self.append_k(how)
        # "Returns -1 without a prior mi_gp_factor, for n + k > capacity, ..."
        if self.fact is None:
            return Expect(-1, "append_no_factor", extra={"k": k})
        if self.n + k > self.cap:
            return Expect(-1, "append_over_capacity", extra={"k": k})
        if how == "dup":
            assert self.diag_id is not None, "a dup append needs a per-point diagonal to carry its negative entry"
            # "info > 0 ... if the appended block is not positive definite -- the handle is then exactly as it was"
            return Expect("info", key=self.fact_key(), extra={"k": k, "dup": True})
        ver, diag_id, ti, n0, hist = self.fact
        self.fact = (ver, diag_id, ti, n0, hist + ((self.n, k, self.u_at is not None),))
        self.n += k
        self.kinv = None   # "K^-1 is invalidated (mi_gp_alpha / mi_gp_grad_x need a new mi_gp_lml_grad)"
        self.batch = self.bcond = None  # "every batch call returns -1 until mi_gp_set_batch is called again"
        # "mi_gp_lml_parts returns the grown logdet and quad"
        self.parts = ("conditional", self.fact_key(), ("factor",) + self.fact)
        return Expect(0, key=self.fact_key(), extra={"k": k})

    def _set_batch(self, how):
        if not self.bound:
            return Expect(-1, "set_batch_unbound")  # "(after mi_gp_set_data: -1 before)"
        # "binds the buffers and ends the batch's conditional factors; the single-evaluation state stays"
        self.batch = {"count": BATCH_COUNT, "zw": how != "plain", "alias": how == "alias"}
        self.bcond = None
        return Expect(0)

    def _batch_call(self, k, need_zw):
        # "A batch call that is refused (-1: no buffers bound, k > count, no Z_dev / W_dev for the gradient) changes nothing."
        if self.batch is None:
            return Expect(-1, "batch_unbound")
        if k > self.batch["count"]:
            return Expect(-1, "batch_k_over_count")
        if need_zw and not self.batch["zw"]:
            return Expect(-1, "batch_no_zw")
        # "The handle's single-evaluation state (factor, K^-1) is invalidated."
        self._end_single()
        self.bcond = None  # "unless mi_gp_factor_batch with the same k was the last batch call"
        return None

    def _members(self, k, shift):
        return [self.key(MEMBERS[shift][p]) for p in range(k)]

    def _lml_batch(self, k, shift):
        r = self._batch_call(k, False)
        if r:
            return r
        ks = self._members(k, shift)
        return Expect(0, extra={"keys": ks}, bits={("lml", p): ("lml",) + kk for p, kk in enumerate(ks)})

    def _lml_grad_batch(self, k, shift):
        r = self._batch_call(k, True)
        if r:
            return r
        ks = self._members(k, shift)
        bits = {("lml", p): ("lml_grad.v",) + kk for p, kk in enumerate(ks)}
        bits.update({("grad", p): ("lml_grad.g",) + kk for p, kk in enumerate(ks)})
        return Expect(0, extra={"keys": ks}, bits=bits)

    def _factor_batch(self, k, shift):
        r = self._batch_call(k, False)
        if r:
            return r
        self.bcond = (k, shift, self.n, self.ver, self.diag_id)
        return Expect(0, extra={"keys": self._members(k, shift)})

    def _predict_batch(self, k):
        if self.bcond is None:
            return Expect(-1, "predict_batch_no_factors")
        k0, shift, n, ver, diag_id = self.bcond
        if k != k0:
            return Expect(-1, "predict_batch_k_mismatch")  # "mi_gp_factor_batch with the same k"
        ks = [(ver, n, diag_id, MEMBERS[shift][p]) for p in range(k)]
        # "bit for bit what mi_gp_factor(theta_p) + mi_gp_predict return"
        bits = {}
        for p, kk in enumerate(ks):
            fresh = (ver, diag_id, kk[3], n, ())
            bits[("mean", p)], bits[("var", p)] = ("mean", fresh), ("var", fresh)
        return Expect(0, extra={"keys": ks}, bits=bits)

    def _set_option(self, what, value):
        return Expect(0)  # "only change scheduling (bit-identical results)"


# --------------------------------------------------------------------------------------------------------------- the walks
def _pairs():
    ps = [(c, q) for c in CHANGERS for q in CONSUMERS]
    np.random.default_rng(4242).shuffle(ps)
    return ps


PAIRS = _pairs()
PAIR_BLOCKS = 11  # (changer, consumer) blocks a 96-step walk is sure to hold: 9 walks of the small sizes x 11 = all 99 pairs


def walk(seed, steps, size):
    """`steps` operations for one handle of `size`, a pure function of (seed, size): walk(s, k, n) is a prefix of walk(s, k + 1, n).
    The generator follows the model so that it can aim: blocks of [what the pair needs] + state-changing call + consumer walk
    through every ordered (changer, consumer) pair in turn -- the three small sizes' default seeds cover all of them -- and
    fillers draw consumers that are valid now, no-state calls, scheduling options and plain uniform calls (mostly refusals)."""
    rng = np.random.default_rng([int(seed), int(size)])
    p = Problem(size)
    m = Model(p)
    small = sorted(s for s in SIZES if s != max(SIZES))
    if size in small:
        nxt = ((int(seed) * len(small) + small.index(size)) * PAIR_BLOCKS) % len(PAIRS)
    else:
        nxt = int(rng.integers(0, len(PAIRS)))
    out, queue = [], []
    widx = int(seed) * len(SIZES) + sorted(SIZES).index(size)
    specials = [("dup",), ("over",), ("failed_parts",), ("u_lml_grad",), ("sample_in_batch",), ("alias_single",)] + [("k>", b) for b in ("lml_batch", "lml_grad_batch", "factor_batch", "predict_batch")]
    specials += [("k<", b) for b in ("lml_batch", "lml_grad_batch", "factor_batch", "predict_batch")]
    specials += [("option", o) for o in SCHED_OPTIONS]
    nspecial = widx * 5

    def special(which):
        """The variants a uniform draw seldom reaches, each with what it needs to say something."""
        if which[0] == "dup":
            pre = [] if m.bound else [("set_data", "same")]
            if m.diag_id is None:
                pre.append(("set_diag", "vec"))
            if m.cap < m.n + 1:
                pre.append(("reserve", min(p.cap, m.n + p.kapp)))
            return pre + [("factor", good()), ("append", "dup"), ("predict",)]
        if which[0] == "failed_parts":
            pre = [] if m.bound else [("set_data", "same")]
            return pre + [("lml", good()), (("lml", "lml_grad", "factor")[int(rng.integers(0, 3))], BAD), ("lml_parts",)]
        if which[0] == "u_lml_grad":  # U resident, then the marginal form takes alpha and ends U
            pre = [] if m.bound else [("set_data", "same")]
            return pre + [("factor", good()), ("predict_u",), ("lml_grad", good()), (("predict_u",), ("predict_grad",))[int(rng.integers(0, 2))]]
        if which[0] == "sample_in_batch":
            pre = [] if m.bound else [("set_data", "same")]
            if m.batch is None:
                pre.append(("set_batch", "zw"))
            return pre + [("factor_batch", 3, int(rng.integers(0, len(MEMBERS)))), ("sample_cov", 1, 0), ("predict_batch", 3)]
        if which[0] == "alias_single":  # member 0 on the single K_dev: a single evaluation overwrites its factor
            pre = [] if m.bound else [("set_data", "same")]
            return pre + [("set_batch", "alias"), ("factor_batch", 3, int(rng.integers(0, len(MEMBERS)))),
                          (("lml", "lml_grad", "factor")[int(rng.integers(0, 3))], good()), ("predict_batch", 3)]
        if which[0] == "over":
            return ([] if m.bound else [("set_data", "same")]) + ([] if m.fact is not None else [("factor", good())]) + [("append", "over")]
        if which[0] == "k>":
            pre = [] if m.bound else [("set_data", "same")]
            if m.batch is None:
                pre.append(("set_batch", "zw"))
            return pre + [(which[1], 4, 0) if which[1] != "predict_batch" else ("predict_batch", 4)]
        if which[0] == "k<":
            pre = [] if m.bound else [("set_data", "same")]
            if m.batch is None or not m.batch["zw"]:
                pre.append(("set_batch", ("zw", "alias")[int(rng.integers(0, 2))]))
            sh = int(rng.integers(0, len(MEMBERS)))
            return pre + ([(which[1], 2, sh)] if which[1] != "predict_batch" else [("factor_batch", 2, sh), ("predict_batch", 2)])
        o = which[1]
        return [("set_option", o, OPTION_VALUES[o][int(rng.integers(0, len(OPTION_VALUES[o])))])]

    def good():
        return int(rng.integers(0, N_GOOD))

    def variant(name):
        if name == "set_data":
            return ("set_data", ("same", "new")[int(rng.integers(0, 2))])
        if name == "set_diag":
            return ("set_diag", "vec" if m.diag_id is None or rng.random() < 0.5 else "none")
        if name in ("lml", "lml_grad", "factor"):
            return (name, BAD if rng.random() < 0.15 else good())
        if name == "sample_cov":
            return ("sample_cov", int(rng.integers(1, 3)), int(rng.integers(0, 2)) * 7)
        if name == "reserve":
            u = rng.random()
            return ("reserve", m.n - 1 if u < 0.2 else p.cap if u < 0.7 else min(p.cap, m.n + (p.cap - m.n) // 2))
        if name == "append":
            u = rng.random()
            return ("append", "over" if u < 0.15 else "dup" if u < 0.3 and m.diag_id is not None and m.fact is not None else "ok")
        if name == "set_batch":
            return ("set_batch", ("plain", "zw", "alias")[int(rng.integers(0, 3))])
        if name in ("lml_batch", "lml_grad_batch", "factor_batch"):
            return (name, (3, 3, 2, 1, 4)[int(rng.integers(0, 5))], int(rng.integers(0, len(MEMBERS))))
        if name == "predict_batch":
            if m.bcond is not None and rng.random() < 0.75:
                return ("predict_batch", m.bcond[0])
            return ("predict_batch", int(rng.integers(1, 5)))
        if name == "set_option":
            o = SCHED_OPTIONS[int(rng.integers(0, len(SCHED_OPTIONS)))]
            return ("set_option", o, OPTION_VALUES[o][int(rng.integers(0, len(OPTION_VALUES[o])))])
        return (name,)

    def setup_for(changer, consumer):
        """Calls that make the pair say something: the consumer would have succeeded had the changer not come between."""
        pre = []
        if not m.bound and changer != "set_data":
            pre.append(("set_data", "same"))
        if consumer in ("alpha", "grad_x"):
            if m.kinv is None:
                pre.append(("lml_grad", good()))
        elif consumer == "predict_batch":
            if m.batch is None or changer == "append":
                pre.append(("set_batch", ("plain", "zw", "alias")[int(rng.integers(0, 3))]))
            if changer != "factor_batch":
                pre.append(("factor_batch", 3, int(rng.integers(0, len(MEMBERS)))))
            if changer == "append":  # (appending needs a factor; an aliased batch call would have ended it)
                pre.append(("factor", good()))
        elif consumer != "lml_parts" or rng.random() < 0.5:
            if m.fact is None or changer == "append":
                pre.append(("factor", good()))
        if changer == "append" and consumer in ("predict_u", "predict_grad") and rng.random() < 0.6:
            pre.append(("predict_u",))  # (U resident: the append extends it and recomputes alpha)
        if "append" in (changer, consumer) and m.cap < m.n + p.kapp:
            pre.insert(0, ("reserve", min(p.cap, m.n + p.kapp)))  # (just enough: later reservations still grow the scratch)
        if changer in ("lml_batch", "lml_grad_batch", "factor_batch") and m.batch is None and consumer != "predict_batch":
            pre.insert(0, ("set_batch", "zw"))
        return pre

    while len(out) < steps:
        if not queue:
            u = rng.random()
            if u < 0.50:
                c, q = PAIRS[nxt % len(PAIRS)]
                nxt += 1
                queue = setup_for(c, q)
                cv = variant(c)
                if c == "append":
                    cv = ("append", "ok")
                elif c in ("lml_batch", "lml_grad_batch", "factor_batch"):
                    cv = (c, 3, cv[2])
                elif c == "reserve":
                    cv = ("reserve", min(p.cap, max(m.cap, m.n) + p.kapp))
                queue += [cv, None if q == "predict_batch" else variant(q)]
                if q == "predict_batch":
                    queue[-1] = ("predict_batch", 3 if rng.random() < 0.8 else 2)
                elif q == "append":
                    queue[-1] = ("append", "ok")
                elif rng.random() < 0.35:
                    # the same query again behind a call that changes no state (a refused one included): same code, same bits
                    queue += [variant(("sample_cov", "set_option", "predict_cov")[int(rng.integers(0, 3))]), queue[-1]]
            elif u < 0.63:  # a consumer that the state allows
                ok = [q for q in CONSUMERS if (q in ("alpha", "grad_x") and m.kinv is not None)
                      or (q in ("predict", "predict_u", "predict_grad", "predict_cov") and m.fact is not None)
                      or (q == "lml_parts" and m.parts is not None) or (q == "predict_batch" and m.bcond is not None)
                      or (q == "append" and m.fact is not None)]
                queue = [variant(ok[int(rng.integers(0, len(ok)))])] if ok else [("factor", good())]
            elif u < 0.72:  # calls that change no state
                queue = [variant(("set_option", "sample_cov", "predict_cov", "set_option")[int(rng.integers(0, 4))])]
            elif u < 0.90:
                queue = special(specials[nspecial % len(specials)])
                nspecial += 1
            else:
                queue = [variant(ALL_OPS[int(rng.integers(0, len(ALL_OPS)))])]
        op = queue.pop(0)
        if op[0] == "append" and op[1] == "dup" and (m.diag_id is None):
            op = ("append", "ok")
        e = m.step(op)
        out.append(op)
        if op[0] == "append" and e.rc == 0:
            # behind an accepted append: the grown parts, the three predictors' routes, the K^-1 users and a batch call
            follow = [("lml_parts",), ("predict",), (("predict_u",), ("predict_grad",))[int(rng.integers(0, 2))],
                     (("alpha",), ("grad_x",))[int(rng.integers(0, 2))],
                     variant(("lml_batch", "factor_batch", "predict_batch", "lml_grad_batch")[int(rng.integers(0, 4))])]
            queue = queue + [f for f in follow if not queue or f[0] != queue[0][0]]
    return out


def replay_line(seed, size, i, ops):
    return f"replay: handle_model.walk(seed={seed}, steps={i + 1}, size={size}) == {ops[: i + 1]!r}"


# ------------------------------------------------------------------------------------------------------------ the stand-in
class Res:
    """What a call did: the return code, the outputs by name, the error text, and whether every output buffer still held its
    sentinel (checked where the call was refused)."""

    def __init__(self, rc, out=None, err="", untouched=True):
        self.rc, self.out, self.err, self.untouched = rc, out or {}, err, untouched


class OracleHandle:
    """The reference implementation of the handle's state machine on the CPU: every value from the oracle, validity tracked as the
    header says.  Deliberately written flag by flag like a library would be, NOT by calling Model: the two meet in run_walk."""

    def __init__(self, problem, oracle):
        self.p, self.o = problem, oracle
        self.have_data = False
        self.n = self.cap = problem.n0
        self.ver, self.next_ver = 0, 1
        self.diag_id, self.next_diag = None, 0
        self.factored = self.have_u = self.have_kinv = self.have_parts = False
        self.f_key = self.kinv_key = self.parts_key = None
        self.parts_form = None
        self.alpha_key = None  # the one alpha buffer: written by lml_grad, by U's formation and by append
        self.batch = None
        self.b_cond = None
        self.no = Res(-1, err="refused")

    def close(self):
        pass

    def _key(self, ti):
        return (self.ver, self.n, self.diag_id, ti)

    def set_data(self, how):
        if how == "new":
            self.ver, self.next_ver = self.next_ver, self.next_ver + 1
        self.have_data = True
        self.factored = self.have_u = self.have_kinv = False
        self.b_cond = None
        return Res(0)

    def set_diag(self, how):
        if how == "vec":
            self.diag_id, self.next_diag = self.next_diag % 2, self.next_diag + 1
        else:
            self.diag_id = None
        self.factored = self.have_u = self.have_kinv = False
        self.b_cond = None
        return Res(0)

    def _evaluate(self, ti, form):
        self.factored = self.have_u = self.have_kinv = self.have_parts = False
        if not self.have_data:
            return None, self.no
        if self.batch and self.batch["alias"]:
            self.b_cond = None
        key = self._key(ti)
        r = self.o.marg(key) if form == "marginal" else self.o.cond(key)
        if r["info"]:
            return None, Res(r["info"], {"lml": -np.inf, "grad": np.zeros(self.p.ntheta)})
        self.have_parts, self.parts_key, self.parts_form = True, key, form
        return key, None

    def lml(self, ti):
        key, bad = self._evaluate(ti, "marginal")
        if bad:
            return Res(bad.rc, {"lml": bad.out["lml"]} if bad.rc > 0 else None, bad.err)
        return Res(0, {"lml": self.o.marg(key)["lml"]})

    def lml_grad(self, ti):
        key, bad = self._evaluate(ti, "marginal")
        if bad:
            return bad
        self.have_kinv, self.kinv_key, self.alpha_key = True, key, key
        return Res(0, {"lml": self.o.marg(key)["lml"], "grad": self.o.grad(key)["grad"]})

    def factor(self, ti):
        key, bad = self._evaluate(ti, "conditional")
        if bad:
            return Res(bad.rc, None, bad.err)
        self.factored, self.f_key = True, key
        return Res(0)

    def alpha(self):
        if not self.have_kinv:
            return self.no
        if self.alpha_key is None:
            return Res(0, {"alpha": np.zeros(self.n)})
        return Res(0, {"alpha": self.o.grad(self.alpha_key)["alpha"]})

    def grad_x(self):
        if not self.have_kinv:
            return self.no
        return Res(0, {"gx": self.o.grad(self.kinv_key)["gx"]})

    def lml_parts(self):
        if not self.have_parts:
            return self.no
        r = self.o.marg(self.parts_key) if self.parts_form == "marginal" else self.o.cond(self.parts_key)
        return Res(0, {"logdet": r["logdet"], "quad": r["quad"]})

    def _pred(self, names):
        if not self.factored:
            return self.no
        r = self.o.cond(self.f_key)
        return Res(0, {k: r[k] for k in names})

    def predict(self):
        return self._pred(("mean", "var"))

    def _make_u(self):
        if self.factored and not self.have_u:
            self.have_u, self.alpha_key = True, self.f_key

    def predict_u(self):
        self._make_u()
        return self._pred(("mean", "var"))

    def predict_grad(self):
        self._make_u()
        r = self._pred(("mean", "var", "dmean", "dvar"))
        if r.rc == 0 and self.alpha_key != self.f_key:  # d mu / d x* = sum_i alpha_i dk: a stale alpha is a wrong gradient
            r.out["dmean"] = r.out["dmean"] + 1.0
        return r

    def predict_cov(self):
        return self._pred(("mean", "cov"))

    def sample_cov(self, seed, offset):
        return Res(0, {"draws": self.o.sample_draws(seed, offset)[0]})

    def reserve(self, cap):
        if cap < self.n:
            return self.no
        self.cap = max(self.cap, cap)  # (the resident alpha and leaf inverses move into the larger arrays)
        return Res(0)

    def _append_u(self, key):
        self.alpha_key = key  # "With U = L^-T resident ... it is extended in place and alpha recomputed"

    def append(self, how, k):
        if not self.factored or self.n + k > self.cap:
            return self.no
        if how == "dup":
            info = self.o.dup_pivot(self.f_key)
            if info:
                return Res(info, {"k_head_same": True})
            raise AssertionError("a dup append is only drawn where it cannot be accepted")
        key = (self.f_key[0], self.n + k, self.f_key[2], self.f_key[3])
        info = self.o.cond(key)["info"]
        if info:
            return Res(info, {"k_head_same": True})
        self.n += k
        self.f_key = key
        if self.have_u:
            self._append_u(key)
        self.have_kinv = False
        self.parts_key, self.parts_form, self.have_parts = key, "conditional", True
        self.batch = self.b_cond = None
        return Res(0, {"k_head_same": True})

    def set_batch(self, how):
        if not self.have_data:
            return self.no
        self.batch = {"count": BATCH_COUNT, "zw": how != "plain", "alias": how == "alias"}
        self.b_cond = None
        return Res(0)

    def _batch(self, k, shift, zw):
        if self.batch is None or k > self.batch["count"] or (zw and not self.batch["zw"]):
            return None
        self.factored = self.have_u = self.have_kinv = False
        self.b_cond = None
        return [self._key(MEMBERS[shift][p]) for p in range(k)]

    def lml_batch(self, k, shift):
        ks = self._batch(k, shift, False)
        if ks is None:
            return self.no
        rs = [self.o.marg(kk) for kk in ks]
        return Res(0, {"lml": np.array([r.get("lml", -np.inf) for r in rs]), "info": np.array([r["info"] for r in rs])})

    def lml_grad_batch(self, k, shift):
        ks = self._batch(k, shift, True)
        if ks is None:
            return self.no
        rs = [self.o.marg(kk) for kk in ks]
        g = np.array([np.zeros(self.p.ntheta) if r["info"] else self.o.grad(kk)["grad"] for r, kk in zip(rs, ks)])
        return Res(0, {"lml": np.array([r.get("lml", -np.inf) for r in rs]), "grad": g, "info": np.array([r["info"] for r in rs])})

    def factor_batch(self, k, shift):
        ks = self._batch(k, shift, False)
        if ks is None:
            return self.no
        self.b_cond = ks
        return Res(0, {"info": np.array([self.o.cond(kk)["info"] for kk in ks])})

    def predict_batch(self, k):
        if self.b_cond is None or k != len(self.b_cond):
            return self.no
        rs = [self.o.cond(kk) for kk in self.b_cond]
        nan = np.full(M_NEW, np.nan)
        return Res(0, {"mean": np.array([nan if r["info"] else r["mean"] for r in rs]),
                       "var": np.array([nan if r["info"] else r["var"] for r in rs])})

    def set_option(self, what, value):
        return Res(0)


# -------------------------------------------------------------------------------------------------------------- the harness
class WalkFailure(AssertionError):
    pass


class Stats:
    def __init__(self):
        self.steps = self.refusals = self.infos = self.bit_compares = self.value_compares = self.padding_checks = 0
        self.ops, self.pairs, self.refusal_kinds = {}, set(), {}

    def add(self, other):
        for k in ("steps", "refusals", "infos", "bit_compares", "value_compares", "padding_checks"):
            setattr(self, k, getattr(self, k) + getattr(other, k))
        for k, v in other.ops.items():
            self.ops[k] = self.ops.get(k, 0) + v
        for k, v in other.refusal_kinds.items():
            self.refusal_kinds[k] = self.refusal_kinds.get(k, 0) + v
        self.pairs |= other.pairs

    def line(self):
        return (f"steps {self.steps} refusals {self.refusals} info>0 {self.infos} value comparisons {self.value_compares} "
                f"bit comparisons {self.bit_compares}")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _close(a, b, rtol):
    """tests/test_gpu_random_sweep.py: per component, floored at 1e-3 of the largest."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = np.maximum(np.abs(b), 1e-3 * max(np.max(np.abs(b)), 1e-300))
    return bool(np.max(np.abs(a - b) / scale) <= rtol)


def tolerances(cond):
    """The project's cond-scaled tolerances (tests/test_gpu_random_sweep.py); cond from the oracle."""
    return {"lml": max(1e-10, 20.0 * cond * EPS), "grad": max(1e-7, 500.0 * cond * EPS), "ctol": max(1e-8, 200.0 * cond * EPS)}


def _check_values(o, problem, name, out, key, exp, what):
    """Values of one successful single-handle call against the oracle at `key`; returns the number of comparisons."""
    bad = []

    def need(ok, msg):
        if not ok:
            bad.append(msg)

    if name in ("lml", "lml_grad"):
        r = o.marg(key)
        t = tolerances(r["cond"])
        need(abs(out["lml"] - r["lml"]) <= t["lml"] * max(abs(r["lml"]), 1.0), f"lml {out['lml']!r} oracle {r['lml']!r}")
        if name == "lml_grad":
            need(_close(out["grad"], o.grad(key)["grad"], t["grad"]), f"grad {out['grad']} oracle {o.grad(key)['grad']}")
    elif name == "alpha":
        t = tolerances(o.marg(key)["cond"])
        need(_close(out["alpha"], o.grad(key)["alpha"], t["grad"]), "alpha")
    elif name == "grad_x":
        t = tolerances(o.marg(key)["cond"])
        need(_close(out["gx"], o.grad(key)["gx"], 10 * t["grad"]), "dLML/dX")
    elif name == "lml_parts":
        r = o.marg(key) if exp.extra["form"] == "marginal" else o.cond(key)
        t = tolerances(r["cond"])
        # LML = -n/2 log 2 pi - quad / 2 - logdet: its two terms at the LML's own tolerance and scale
        scale = max(abs(-0.5 * key[1] * np.log(2.0 * np.pi) - 0.5 * r["quad"] - r["logdet"]), 1.0)
        need(abs(out["logdet"] - r["logdet"]) <= t["lml"] * scale, f"logdet {out['logdet']!r} oracle {r['logdet']!r}")
        need(abs(0.5 * out["quad"] - 0.5 * r["quad"]) <= t["lml"] * scale, f"quad {out['quad']!r} oracle {r['quad']!r}")
    elif name in ("predict", "predict_u", "predict_grad", "predict_cov"):
        r = o.cond(key)
        t = tolerances(r["cond"])
        ctol = t["ctol"]
        need(np.allclose(out["mean"], r["mean"], rtol=ctol, atol=ctol), f"mean {out['mean']} oracle {r['mean']}")
        if "var" in out:
            need(np.allclose(out["var"], r["var"], rtol=10 * ctol, atol=max(1e-10, ctol * 1e-2)), f"var {out['var']} oracle {r['var']}")
        if name == "predict_grad":
            ptol = max(1e-6, 10 * t["grad"])
            for k_ in ("dmean", "dvar"):
                need(np.allclose(out[k_], r[k_], rtol=ptol, atol=ptol * max(np.abs(r[k_]).max(), 1e-12)), f"{k_} {out[k_]} oracle {r[k_]}")
        if name == "predict_cov":
            # tests/test_gpu_predict_joint.py: 1e-9 kd on the lower triangle
            err = np.abs(np.tril(out["cov"]) - r["cov"]).max()
            need(err <= 1e-9 * r["kd"], f"Sigma off by {err}")
    else:
        raise AssertionError(name)
    if bad:
        raise WalkFailure(f"{what}: " + "; ".join(bad))
    return len(out)


def run_walk(handle, problem, oracle, ops, seed=None, registry=None):
    """Drive `handle` through `ops`, checking every call against a fresh Model.  Returns Stats; raises WalkFailure with a line
    that replays the walk up to the failing step."""
    m = Model(problem)
    st = Stats()
    reg = {} if registry is None else registry
    prev = None
    for i, op in enumerate(ops):
        name = op[0]
        where = replay_line(seed, problem.size, i, ops) + f"\n  step {i} {op!r}"
        st.steps += 1
        st.ops[name] = st.ops.get(name, 0) + 1
        if prev in CHANGERS and name in CONSUMERS:
            st.pairs.add((prev, name))
        prev = name
        exp = m.step(op)
        args = op[1:]
        if name == "append":
            args = (op[1], exp.extra.get("k", m.append_k(op[1])))
        res = getattr(handle, name)(*args)
        if res.rc == -2 and exp.rc != -2:
            raise WalkFailure(f"{where}: returned -2 (a HIP / RCCL failure, {res.err!r}): the walk ends here")
        book = getattr(handle, "bk", None)  # (tests/handle_layouts.py: a handle on poisoned buffers says what the call wrote outside)
        if book is not None:
            before = book.checked
            v = book.violation()
            st.padding_checks += book.checked - before
            if v:
                raise WalkFailure(f"{where}: {v[2]}")
        want = exp.rc
        if want == "info":
            if exp.extra.get("dup"):
                want = oracle.dup_pivot(exp.key)
                if want != exp.key[1] + 1:
                    raise WalkFailure(f"{where}: the oracle's pivot of a dup append is {want}, not n + 1")
            else:
                want = (oracle.marg(exp.key) if exp.extra["form"] == "marginal" else oracle.cond(exp.key))["info"]
            if want <= 0:
                raise WalkFailure(f"{where}: the oracle factorises the theta that was to fail")
        if res.rc != want:
            raise WalkFailure(f"{where}: returned {res.rc} ({res.err!r}), the model expects {want}"
                              + (f" ({exp.refusal})" if exp.refusal else ""))
        if want == -1:
            st.refusals += 1
            st.refusal_kinds[exp.refusal] = st.refusal_kinds.get(exp.refusal, 0) + 1
            if not res.err:
                raise WalkFailure(f"{where}: refused without a text in mi_gp_last_error")
            if not res.untouched:
                raise WalkFailure(f"{where}: a refused call wrote into an output buffer")
            continue
        if want > 0:
            st.infos += 1
            if name in ("lml", "lml_grad") and res.out["lml"] != -np.inf:
                raise WalkFailure(f"{where}: info {want} with lml {res.out['lml']!r}, not -inf")
            if name == "lml_grad" and (np.any(res.out["grad"] != 0.0) or np.signbit(res.out["grad"]).any()):
                raise WalkFailure(f"{where}: info {want} with a gradient that is not +0.0")
            if name == "append" and not res.out["k_head_same"]:
                raise WalkFailure(f"{where}: a refused append changed the factor")
            continue
        # ---- values of a successful call
        out = res.out
        if name in ("lml", "lml_grad", "alpha", "grad_x", "lml_parts", "predict", "predict_u", "predict_grad", "predict_cov"):
            st.value_compares += _check_values(oracle, problem, name, out, exp.key, exp, where)
        elif name == "append":
            if not out["k_head_same"]:
                raise WalkFailure(f"{where}: the first n rows of the factor changed their bits")
            st.bit_compares += 1
        elif name == "sample_cov":
            ref, L, z = oracle.sample_draws(op[1], op[2])
            tol = 1e-9 * np.abs(L).max() * max(1.0, np.abs(z).max())  # tests/test_gpu_predict_joint.py
            if not np.abs(out["draws"] - ref).max() <= tol:
                raise WalkFailure(f"{where}: draws off by {np.abs(out['draws'] - ref).max()}")
            st.value_compares += 1
        elif name in ("lml_batch", "lml_grad_batch", "factor_batch", "predict_batch"):
            for p, kk in enumerate(exp.extra["keys"]):
                form = "marginal" if name in ("lml_batch", "lml_grad_batch") else "conditional"
                r = oracle.marg(kk) if form == "marginal" else oracle.cond(kk)
                if name != "predict_batch" and int(out["info"][p]) != r["info"]:
                    raise WalkFailure(f"{where}: member {p} info {int(out['info'][p])}, the oracle's pivot is {r['info']}")
                sub = None
                if r["info"]:
                    ok = True
                    if "lml" in out:
                        ok = out["lml"][p] == -np.inf
                    if "grad" in out:
                        ok = ok and not np.any(out["grad"][p] != 0.0) and not np.signbit(out["grad"][p]).any()
                    if name == "predict_batch":
                        ok = np.isnan(out["mean"][p]).all() and np.isnan(out["var"][p]).all()
                    if not ok:
                        raise WalkFailure(f"{where}: member {p} failed (info {r['info']}) but its outputs are not -inf / +0.0 / NaN")
                    continue
                if name == "lml_batch":
                    sub, single = {"lml": out["lml"][p]}, "lml"
                elif name == "lml_grad_batch":
                    sub, single = {"lml": out["lml"][p], "grad": out["grad"][p]}, "lml_grad"
                elif name == "predict_batch":
                    sub, single = {"mean": out["mean"][p], "var": out["var"][p]}, "predict"
                if sub:
                    st.value_compares += _check_values(oracle, problem, single, sub, kk, exp, where + f" member {p}")
        # ---- bits: the same identity twice is the same bits
        for oname, ident in exp.bits.items():
            if isinstance(oname, tuple):  # (output, batch member): a member that failed has no bits to keep
                kk = exp.extra["keys"][oname[1]]
                if (oracle.cond(kk) if name == "predict_batch" else oracle.marg(kk))["info"]:
                    continue
                got = out[oname[0]][oname[1]]
            else:
                got = out[oname]
            if oname == "cov":
                got = np.tril(got)
            b = _bits(got)
            if ident in reg:
                st.bit_compares += 1
                if b.shape != reg[ident][0].shape or not np.array_equal(b, reg[ident][0]):
                    raise WalkFailure(f"{where}: {oname} differs in its bits from the answer of step {reg[ident][1]} in the same resident "
                                      f"state ({ident!r})")
            else:
                reg[ident] = (b.copy(), i)
    return st


# --------------------------------------------------------------------------------------------------------------- the facade
FACADE_OPS = ("lml", "lml_grad", "lml_grad_data", "factor", "predict", "predict_grad", "predict_cov", "predict_batch",
              "lml_grad_batch", "append", "set_diag", "update_data", "set_option")


class FacadeModel:
    """What MiGP's shadow of the handle state must amount to: which (data version, n, diagonal, theta) every result belongs to
    and the LEAST number of factorisations (mi_gp_factor / mi_gp_lml_grad / mi_gp_factor_batch calls) the walk needs."""

    def __init__(self, problem):
        self.p = problem
        self.n, self.ver, self.next_ver = problem.n0, 0, 1
        self.diag_id, self.next_diag = None, 0
        self.fact = None  # theta index of the factor MiGP may reuse
        self.counts = {"mi_gp_factor": 0, "mi_gp_lml_grad": 0, "mi_gp_factor_batch": 0}

    def key(self, ti):
        return (self.ver, self.n, self.diag_id, ti)

    def step(self, op):
        name = op[0]
        if name == "lml":
            self.fact = None  # (the evaluation overwrites K_dev)
        elif name in ("lml_grad", "lml_grad_data"):
            self.fact = None
            self.counts["mi_gp_lml_grad"] += 1
        elif name == "factor":
            self.counts["mi_gp_factor"] += 1
            self.fact = op[1] if op[1] != BAD else None
        elif name in ("predict", "predict_cov") or (name == "predict_grad" and not op[2]):
            if self.fact != op[1]:
                self.counts["mi_gp_factor"] += 1
                self.fact = op[1]
        elif name == "predict_grad":  # refactor=True
            self.counts["mi_gp_factor"] += 1
            self.fact = op[1]
        elif name == "predict_batch":
            self.counts["mi_gp_factor_batch"] += 1
            self.fact = None
        elif name == "lml_grad_batch":
            self.fact = None
        elif name == "append":
            assert self.fact is not None and self.n + self.p.kapp <= self.p.cap
            self.n += self.p.kapp
        elif name == "set_diag":
            self.fact = None
            if op[1] == "vec":
                self.diag_id, self.next_diag = self.next_diag % 2, self.next_diag + 1
            else:
                self.diag_id = None
        elif name == "update_data":
            self.fact = None
            self.ver, self.next_ver = self.next_ver, self.next_ver + 1
        return self.key(op[1]) if name in ("lml", "lml_grad", "lml_grad_data", "factor", "predict", "predict_grad", "predict_cov") else None


def facade_walk(seed, steps, size):
    """Operations for one MiGP over its public methods: lml, lml_grad, lml_grad_data, factor, predict(via_inverse=...), predict_grad
    (refactor=...), predict_cov, predict_batch, lml_grad_batch, append, set_diag, update_data, set_option."""
    rng = np.random.default_rng([int(seed), int(size), 7])
    p = Problem(size)
    m = FacadeModel(p)
    out = []
    last = 0
    while len(out) < steps:
        u = rng.random()
        ti = last if rng.random() < 0.6 else int(rng.integers(0, N_GOOD))  # (a BO sweep stays at its theta)
        if u < 0.30:
            op = ("predict", ti, bool(rng.integers(0, 2)))
        elif u < 0.42:
            op = ("predict_grad", ti, bool(rng.random() < 0.25))
        elif u < 0.50:
            op = ("predict_cov", ti)
        elif u < 0.56:
            op = ("factor", BAD if rng.random() < 0.2 else ti)
        elif u < 0.62:
            op = ("lml", BAD if rng.random() < 0.2 else ti)
        elif u < 0.70:
            op = (("lml_grad", "lml_grad_data")[int(rng.integers(0, 2))], ti)
        elif u < 0.75:
            op = ("predict_batch", int(rng.integers(0, len(MEMBERS))), int(rng.integers(1, 4)))
        elif u < 0.79:
            op = ("lml_grad_batch", int(rng.integers(0, len(MEMBERS))), int(rng.integers(1, 4)))
        elif u < 0.86:
            if m.fact is None or m.n + p.kapp > p.cap:
                continue
            op = ("append",)
        elif u < 0.91:
            op = ("set_diag", "vec" if m.diag_id is None or rng.random() < 0.5 else "none")
        elif u < 0.95:
            op = ("update_data",)
        else:
            o = SCHED_OPTIONS[int(rng.integers(0, len(SCHED_OPTIONS)))]
            op = ("set_option", o, OPTION_VALUES[o][int(rng.integers(0, len(OPTION_VALUES[o])))])
        m.step(op)
        if op[0] in ("predict", "predict_grad", "predict_cov"):
            last = op[1]
        out.append(op)
    return out


class OracleFacade:
    """MiGP's call surface over an OracleHandle: refactorises exactly when its own factor is not the one asked for, and counts."""

    def __init__(self, problem, oracle):
        self.p, self.h = problem, OracleHandle(problem, oracle)
        self.h.set_data("same")
        self.h.reserve(problem.cap)
        self.counts = {"mi_gp_factor": 0, "mi_gp_lml_grad": 0, "mi_gp_factor_batch": 0}
        self.ok_theta = None

    def close(self):
        pass

    def _ensure(self, ti):
        if self.ok_theta != ti:
            self.factor(ti)

    def lml(self, ti):
        self.ok_theta = None
        r = self.h.lml(ti)
        return {"lml": r.out["lml"], "info": r.rc}

    def lml_grad(self, ti):
        self.ok_theta = None
        self.counts["mi_gp_lml_grad"] += 1
        r = self.h.lml_grad(ti)
        return {"lml": r.out["lml"], "grad": r.out["grad"], "info": r.rc}

    def lml_grad_data(self, ti):
        r = self.lml_grad(ti)
        r["alpha"], r["gx"] = self.h.alpha().out["alpha"], self.h.grad_x().out["gx"]
        return r

    def factor(self, ti):
        self.counts["mi_gp_factor"] += 1
        r = self.h.factor(ti)
        self.ok_theta = ti if r.rc == 0 else None
        return {"info": r.rc}

    def predict(self, ti, via):
        self._ensure(ti)
        return (self.h.predict_u() if via else self.h.predict()).out

    def predict_grad(self, ti, refactor):
        if refactor:
            self.ok_theta = None
        self._ensure(ti)
        return self.h.predict_grad().out

    def predict_cov(self, ti):
        self._ensure(ti)
        return self.h.predict_cov().out

    def predict_batch(self, shift, k):
        self.ok_theta = None
        self.counts["mi_gp_factor_batch"] += 1
        self.h.set_batch("zw")
        info = self.h.factor_batch(k, shift).out["info"]
        r = self.h.predict_batch(k).out
        r["info"] = info
        return r

    def lml_grad_batch(self, shift, k):
        self.ok_theta = None
        self.h.set_batch("zw")
        return self.h.lml_grad_batch(k, shift).out

    def append(self):
        assert self.h.append("ok", self.p.kapp).rc == 0
        return {}

    def set_diag(self, how):
        self.ok_theta = None
        self.h.set_diag(how)
        return {}

    def update_data(self):
        self.ok_theta = None
        self.h.ver, self.h.next_ver = self.h.next_ver, self.h.next_ver + 1
        return {}

    def set_option(self, what, value):
        return {}


def run_facade_walk(gp, problem, oracle, ops, seed=None):
    """Every result of the facade against the oracle at the model's key; at the end the factorisation counts equal the model's."""
    m = FacadeModel(problem)
    st = Stats()
    for i, op in enumerate(ops):
        name = op[0]
        where = f"replay: handle_model.facade_walk(seed={seed}, steps={i + 1}, size={problem.size}) == {ops[: i + 1]!r}\n  step {i} {op!r}"
        st.steps += 1
        st.ops[name] = st.ops.get(name, 0) + 1
        key = m.step(op)
        out = getattr(gp, name)(*op[1:])
        exp = Expect(0, extra={"form": "marginal"})
        if name in ("lml", "lml_grad", "lml_grad_data", "factor"):
            form = "conditional" if name == "factor" else "marginal"
            info = (oracle.marg(key) if form == "marginal" else oracle.cond(key))["info"]
            if out["info"] != info:
                raise WalkFailure(f"{where}: info {out['info']}, the oracle's pivot is {info}")
            if info:
                st.infos += 1
                if name != "factor" and out["lml"] != -np.inf:
                    raise WalkFailure(f"{where}: info {info} with lml {out['lml']!r}")
                continue
            if name != "factor":
                st.value_compares += _check_values(oracle, problem, "lml" if name == "lml" else "lml_grad",
                                                   {k: out[k] for k in ("lml", "grad") if k in out}, key, exp, where)
            if name == "lml_grad_data":
                st.value_compares += _check_values(oracle, problem, "alpha", {"alpha": out["alpha"]}, key, exp, where)
                st.value_compares += _check_values(oracle, problem, "grad_x", {"gx": out["gx"]}, key, exp, where)
        elif name in ("predict", "predict_grad", "predict_cov"):
            st.value_compares += _check_values(oracle, problem, name, out, key, exp, where)
        elif name in ("predict_batch", "lml_grad_batch"):
            for q in range(op[2]):
                kk = m.key(MEMBERS[op[1]][q])
                r = oracle.cond(kk) if name == "predict_batch" else oracle.marg(kk)
                if int(out["info"][q]) != r["info"]:
                    raise WalkFailure(f"{where}: member {q} info {int(out['info'][q])}, the oracle's pivot is {r['info']}")
                if r["info"]:
                    continue
                sub = ({"mean": out["mean"][q], "var": out["var"][q]} if name == "predict_batch"
                       else {"lml": out["lml"][q], "grad": out["grad"][q]})
                st.value_compares += _check_values(oracle, problem, "predict" if name == "predict_batch" else "lml_grad", sub, kk,
                                                   exp, where + f" member {q}")
    if dict(gp.counts) != m.counts:
        raise WalkFailure(f"replay: handle_model.facade_walk(seed={seed}, steps={len(ops)}, size={problem.size}): factorisations "
                          f"{dict(gp.counts)}, the model's minimum is {m.counts}")
    return st
