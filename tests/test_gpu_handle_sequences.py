"""Seeded random call sequences on ONE handle against the state model of tests/handle_model.py.

Almost every other GPU test creates a handle, calls one or two entry points in a hand-picked order and closes it.  Here one handle
per (size, seed) lives through a whole walk over the C-ABI -- set_data, set_diag, the three single evaluations, the K^-1 users,
the five predictors, reserve, append (accepted, over capacity, without a factor, not positive definite), the batch calls with k
below / at / above the count on plain, Z/W and ALIASED buffers, and the scheduling-only options -- and EVERY call is checked:
  * its return code equals the model's (0, -1, or the oracle's first non-positive pivot); a -1 leaves a text in mi_gp_last_error and
    every output buffer's sentinel in place; info > 0 comes with lml = -inf and a +0.0 gradient;
  * its values meet the oracle at the (data version, n, diagonal, theta) the model says is resident, within the cond-scaled
    tolerances of tests/test_gpu_random_sweep.py and tests/test_gpu_predict_joint.py (no tolerance of its own);
  * its bits equal the first answer of the same query in the same resident state, whatever no-state calls came between; batch
    members equal the single evaluations, mi_gp_predict_cov's mean mi_gp_predict's, mi_gp_predict_batch's rows mi_gp_factor +
    mi_gp_predict, and an accepted append leaves the first n rows of the factor alone.
The same kind of walk then goes through MiGP's public methods: the facade never refuses, so every result must meet the oracle and
the NUMBER of mi_gp_factor / mi_gp_lml_grad / mi_gp_factor_batch calls must equal the model's minimum -- the shadow of the handle
state in backend.py is neither stale nor kept right by always refactorising.

tests/test_handle_model_host.py runs this harness against a NumPy stand-in and shows that broken rules are caught.  A failure
prints one line that handle_model.walk() replays.  A return of -2 ends the module: nothing more is started on the GPU.
HANDLE_WALK_SEEDS=<count> and HANDLE_WALK_STEPS=<steps> extend a run; HANDLE_WALK_REPORT=<path> appends one JSON line per walk."""
import ctypes
import json
import os
import time

import numpy as np
import pytest

import handle_layouts as HL
import handle_model as H

pytestmark = pytest.mark.gpu

SEEDS = list(range(int(os.environ.get("HANDLE_WALK_SEEDS", str(len(H.DEFAULT_SEEDS))))))
DP = ctypes.POINTER(ctypes.c_double)
IP = ctypes.POINTER(ctypes.c_int)
SENTINEL = -7.25e77
_STATE = {"stop": None, "oracles": {}}


def _steps(size):
    return int(os.environ.get("HANDLE_WALK_STEPS", str(H.SIZES[size]["steps"])))


def _setup(size):
    if size not in _STATE["oracles"]:
        p = H.Problem(size)
        _STATE["oracles"][size] = (p, H.Oracle(p))
    return _STATE["oracles"][size]


def _report(**kw):
    path = os.environ.get("HANDLE_WALK_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(kw) + "\n")


def _guard():
    if _STATE["stop"]:
        pytest.fail(f"not started: an earlier walk ended in a HIP failure ({_STATE['stop']})")


class TorchBackend:
    """handle_layouts.Book on the device: flat float64 tensors, strided views, the comparison of the int64 view on the GPU."""

    def __init__(self, torch, dev):
        self.torch, self.dev = torch, dev

    def alloc(self, total, bits):
        t = self.torch.zeros(total, dtype=self.torch.float64, device=self.dev)
        if bits is not None:
            t.view(self.torch.int64).fill_(int(bits))
        return t

    def bits(self, flat):
        return flat.view(self.torch.int64)

    def index(self, idx):
        return self.torch.from_numpy(idx).to(self.dev)

    def strided(self, flat, shape, strides, off):
        return flat.as_strided(shape, strides, off)

    def any_changed(self, pairs, want):
        return self.torch.stack([(b[i] != want).any() for b, i in pairs]).cpu().tolist()

    def first_changed(self, b, i, want):
        return int(i[self.torch.nonzero(b[i] != want)[0, 0]])


class RawHandle:
    """handle_model's call surface over the C-ABI: the test's own torch buffers, allocated once for the capacity, under one
    layout of tests/handle_layouts.py (every allocation, pointer, lda, ldw and stride comes from it; `bk` is its bookkeeping,
    which run_walk asks after every call what was written outside the writable regions)."""

    def __init__(self, problem, layout=HL.DEFAULT):
        import torch

        from andvaranaut_amd import _lib

        assert torch.cuda.is_available()
        self.torch, self.p, self.lib = torch, problem, _lib.load()
        p = problem
        self.dev = torch.device("cuda", 0)
        cfg = _lib.MiGpConfig()
        cfg.n, cfg.d, cfg.nkern = p.n0, p.d, p.nk
        for i, k in enumerate(p.kerns):
            cfg.kernel_ids[i] = _lib.KERNEL_IDS[k]
        for i, o in enumerate(p.ops):
            cfg.ops[i] = _lib.OP_IDS[o]
        cfg.device, cfg.panel_tiles = 0, 0
        h = ctypes.c_void_p()
        assert self.lib.mi_gp_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, self.lib.mi_gp_last_global_error()
        self.h, self._lib_mod = h, _lib
        self.n, self.ver, self.next_ver, self.diag_id, self.next_diag, self.f_ti = p.n0, 0, 1, None, 0, None
        capp = H.padded(p.cap)
        self.capp, self.layout = capp, layout
        with torch.cuda.device(self.dev):
            bk = self.bk = HL.Book(layout, capp, TorchBackend(torch, self.dev))
            self.lda, self.ldw = bk.lda, bk.ldw
            self.X = bk.vector("X", p.rows * p.d).view(p.rows, p.d)
            self.y = bk.vector("y", p.rows)
            self.dg = bk.vector("diag", p.rows)
            self.Xpool, self.ypool, self.dpool = bk.vector("Xpool", p.rows * p.d).view(p.rows, p.d), bk.vector("ypool", p.rows), bk.vector("dpool", p.rows)
            self.Kall = bk.matrix("K", capp + 128, "K", H.BATCH_COUNT)  # [0] is the single K_dev (the aliased batch's member 0)
            self.Z = bk.matrix("Z", capp, "ZW")
            self.W = bk.matrix("W", capp, "ZW")
            self.bK = bk.matrix("batch K", capp + 128, "K", H.BATCH_COUNT)
            self.bZ = bk.matrix("batch Z", capp, "ZW", H.BATCH_COUNT)
            self.bW = bk.matrix("batch W", capp, "ZW", H.BATCH_COUNT)
            self.work = bk.matrix("work", 2 * 128, "work")
            self.bwork = bk.matrix("batch work", 128, "work", H.BATCH_COUNT + 1)
            self.awork = bk.vector("append work", 4 * 128 * self.ldw + 65600, big=True)
            self.xn = bk.vector("Xnew", H.M_NEW * p.d).view(H.M_NEW, p.d)
            self.xn.copy_(torch.from_numpy(p.xnew))
            self.out = bk.vector("out", 8 * H.M_NEW * (p.d + 2))
            self.mix = bk.vector("mix", 2 * H.M_NEW)
            self.cov = bk.vector("cov", 128 * 128, big=True).view(128, 128)
            self.gx = bk.vector("gx", p.rows * p.d).view(p.rows, p.d)
            self.scov = bk.vector("sample cov", 128 * 128, big=True).view(128, 128)
            self.smean = bk.vector("sample mean", H.M_SAMPLE)
            self.smean.copy_(torch.from_numpy(p.sample_mean))
            self.draws = bk.vector("draws", H.S_SAMPLE * H.M_SAMPLE).view(H.S_SAMPLE, H.M_SAMPLE)
            self.swork_len = int(self.lib.mi_gp_sample_cov_work(H.M_SAMPLE, H.S_SAMPLE))
            self.swork = bk.vector("sample work", self.swork_len, big=True)
            self.dnew = bk.vector("diag new", 1)
            self._pool()
            self.X[: self.n].copy_(self.Xpool[: self.n])
            self.y[: self.n].copy_(self.ypool[: self.n])
            torch.cuda.synchronize(self.dev)

    def close(self):
        if self.h is not None:
            self.lib.mi_gp_destroy(self.h)
            self.h = None

    # ---- helpers
    def _pool(self):
        X, y = self.p.data(self.ver)
        self.Xpool.copy_(self.torch.from_numpy(X))
        self.ypool.copy_(self.torch.from_numpy(y))

    def _sync(self):
        self.torch.cuda.synchronize(self.dev)

    def _err(self):
        return self.lib.mi_gp_last_error(self.h).decode()

    def _res(self, rc, out, bufs):
        """rc < 0: nothing is returned and every buffer must still hold its sentinel."""
        if rc < 0:
            clean = all(bool((b == SENTINEL).all()) for b in bufs)
            return H.Res(rc, None, self._err(), clean)
        return H.Res(rc, out, self._err())

    def _theta(self, ti):
        th = np.ascontiguousarray(self.p.theta(ti))
        return th, th.ctypes.data_as(DP)

    def _fill(self, *tensors):
        for t in tensors:
            t.fill_(SENTINEL) if hasattr(t, "fill_") else t.fill(SENTINEL)
        self._sync()

    # ---- the entry points
    def set_data(self, how):
        if how == "new":
            self.ver, self.next_ver = self.next_ver, self.next_ver + 1
            self._pool()
            self.X[: self.n].copy_(self.Xpool[: self.n])
            self.y[: self.n].copy_(self.ypool[: self.n])
            self._sync()
        b = self._lib_mod.MiGpBuffers()
        b.X_dev, b.y_dev, b.K_dev, b.lda = self.X.data_ptr(), self.y.data_ptr(), self.Kall.data_ptr(), self.lda
        b.Z_dev, b.W_dev = self.Z.data_ptr(), self.W.data_ptr()
        return H.Res(self.lib.mi_gp_set_data(self.h, ctypes.byref(b)), None, self._err())

    def set_diag(self, how):
        if how == "vec":
            self.diag_id, self.next_diag = self.next_diag % 2, self.next_diag + 1
            self.dpool.copy_(self.torch.from_numpy(self.p.diag(self.diag_id)))
            self.dg[: self.n].copy_(self.dpool[: self.n])
            self._sync()
            return H.Res(self.lib.mi_gp_set_diag(self.h, self.dg.data_ptr()), None, self._err())
        self.diag_id = None
        return H.Res(self.lib.mi_gp_set_diag(self.h, None), None, self._err())

    def lml(self, ti):
        _, tp = self._theta(ti)
        v = ctypes.c_double(SENTINEL)
        rc = self.lib.mi_gp_lml(self.h, tp, ctypes.byref(v))
        return self._res(rc, {"lml": v.value}, [np.array(v.value)])

    def lml_grad(self, ti):
        _, tp = self._theta(ti)
        v, g = ctypes.c_double(SENTINEL), np.full(self.p.ntheta, SENTINEL)
        rc = self.lib.mi_gp_lml_grad(self.h, tp, ctypes.byref(v), g.ctypes.data_as(DP))
        return self._res(rc, {"lml": v.value, "grad": g}, [np.array(v.value), g])

    def factor(self, ti):
        _, tp = self._theta(ti)
        rc = self.lib.mi_gp_factor(self.h, tp)
        if rc == 0:
            self.f_ti = ti
        return self._res(rc, None, [])

    def alpha(self):
        a = np.full(self.n, SENTINEL)
        rc = self.lib.mi_gp_alpha(self.h, a.ctypes.data_as(DP))
        return self._res(rc, {"alpha": a}, [a])

    def grad_x(self):
        self._fill(self.gx)
        rc = self.lib.mi_gp_grad_x(self.h, self.gx.data_ptr())
        return self._res(rc, {"gx": self.gx[: self.n].cpu().numpy()} if rc == 0 else None, [self.gx])

    def lml_parts(self):
        a, b = ctypes.c_double(SENTINEL), ctypes.c_double(SENTINEL)
        rc = self.lib.mi_gp_lml_parts(self.h, ctypes.byref(a), ctypes.byref(b))
        return self._res(rc, {"logdet": a.value, "quad": b.value}, [np.array([a.value, b.value])])

    def _predict(self, fn, grad=False):
        m, d = H.M_NEW, self.p.d
        self._fill(self.out)
        o = self.out.data_ptr()
        args = [self.h, self.xn.data_ptr(), m, self.work.data_ptr(), self.ldw, o, o + 8 * m, 1]
        if grad:
            args += [o + 16 * m, o + 16 * m + 8 * m * d]
        rc = fn(*args)
        if rc != 0:
            return self._res(rc, None, [self.out])
        v = self.out.cpu().numpy()
        out = {"mean": v[:m].copy(), "var": v[m: 2 * m].copy()}
        if grad:
            out["dmean"], out["dvar"] = v[2 * m: 2 * m + m * d].reshape(m, d).copy(), v[2 * m + m * d: 2 * m + 2 * m * d].reshape(m, d).copy()
        return H.Res(0, out, self._err())

    def predict(self):
        return self._predict(self.lib.mi_gp_predict)

    def predict_u(self):
        return self._predict(self.lib.mi_gp_predict_u)

    def predict_grad(self):
        return self._predict(self.lib.mi_gp_predict_grad, True)

    def predict_cov(self):
        m = H.M_NEW
        self._fill(self.out, self.cov)
        rc = self.lib.mi_gp_predict_cov(self.h, self.xn.data_ptr(), m, self.work.data_ptr(), self.ldw, self.out.data_ptr(),
                                        self.cov.data_ptr(), 128, 1)
        if rc != 0:
            return self._res(rc, None, [self.out, self.cov])
        return H.Res(0, {"mean": self.out[:m].cpu().numpy(), "cov": np.tril(self.cov[:m, :m].cpu().numpy())}, self._err())

    def sample_cov(self, seed, offset):
        m = H.M_SAMPLE
        self.scov.zero_()
        self.scov[:m, :m].copy_(self.torch.from_numpy(self.p.sample_cov))
        self._fill(self.draws)
        rc = self.lib.mi_gp_sample_cov(self.h, self.scov.data_ptr(), 128, m, self.smean.data_ptr(), self.p.sample_jitter, H.S_SAMPLE,
                                       seed, offset, self.draws.data_ptr(), m, self.swork.data_ptr(), self.swork_len)
        return self._res(rc, {"draws": self.draws.cpu().numpy()} if rc == 0 else None, [self.draws])

    def reserve(self, cap):
        return H.Res(self.lib.mi_gp_reserve(self.h, cap), None, self._err())

    def append(self, how, k):
        n = self.n
        if how == "dup":
            x, y = self.Xpool[H.DUP_ROW: H.DUP_ROW + 1], self.ypool[H.DUP_ROW: H.DUP_ROW + 1]
            self.dnew.fill_(self.p.dup_diag(self.f_ti if self.f_ti is not None else 0, self.diag_id))
            dn = self.dnew
        else:
            x, y = self.Xpool[n: n + k], self.ypool[n: n + k]
            dn = self.dpool[n: n + k] if self.diag_id is not None else None
        head = self.torch.tril(self.Kall[0, :n, :n]).view(self.torch.int64).clone()
        self._sync()
        rc = self.lib.mi_gp_append(self.h, x.data_ptr(), y.data_ptr(), dn.data_ptr() if dn is not None else None, k,
                                   self.awork.data_ptr(), self.ldw)
        same = bool(self.torch.equal(head, self.torch.tril(self.Kall[0, :n, :n]).view(self.torch.int64)))
        if rc == 0:
            self.n += k
        return H.Res(rc, {"k_head_same": same}, self._err(), same)

    def set_batch(self, how):
        b = self._lib_mod.MiGpBatchBuffers()
        b.K_dev = (self.Kall if how == "alias" else self.bK).data_ptr()
        b.Z_dev = self.bZ.data_ptr() if how != "plain" else None
        b.W_dev = self.bW.data_ptr() if how != "plain" else None
        b.stride_k, b.stride_zw, b.count = self.bk.stride("K"), self.bk.stride("batch Z"), H.BATCH_COUNT
        return H.Res(self.lib.mi_gp_set_batch(self.h, ctypes.byref(b)), None, self._err())

    def _batch_eval(self, which, k, shift):
        th = np.ascontiguousarray(self.p.thetas(shift, k))
        v, g = np.full(k, SENTINEL), np.full((k, self.p.ntheta), SENTINEL)
        info = np.full(k, -99, dtype=np.int32)
        tp, vp, gp_, ip = th.ctypes.data_as(DP), v.ctypes.data_as(DP), g.ctypes.data_as(DP), info.ctypes.data_as(IP)
        if which == "lml":
            rc, out, bufs = self.lib.mi_gp_lml_batch(self.h, k, tp, vp, ip), {"lml": v, "info": info}, [v]
        elif which == "grad":
            rc, out, bufs = self.lib.mi_gp_lml_grad_batch(self.h, k, tp, vp, gp_, ip), {"lml": v, "grad": g, "info": info}, [v, g]
        else:
            rc, out, bufs = self.lib.mi_gp_factor_batch(self.h, k, tp, ip), {"info": info}, []
        if rc < 0 and not (info == -99).all():
            return H.Res(rc, None, self._err(), False)
        return self._res(rc, out, bufs)

    def lml_batch(self, k, shift):
        return self._batch_eval("lml", k, shift)

    def lml_grad_batch(self, k, shift):
        return self._batch_eval("grad", k, shift)

    def factor_batch(self, k, shift):
        return self._batch_eval("factor", k, shift)

    def predict_batch(self, k, mix=False):
        m = H.M_NEW
        self._fill(self.out, self.mix)
        o, x = self.out.data_ptr(), self.mix.data_ptr()
        rc = self.lib.mi_gp_predict_batch(self.h, k, self.xn.data_ptr(), m, self.bwork.data_ptr(), self.ldw, self.bk.stride("batch work"), o,
                                          o + 8 * k * m, 1, x if mix else None, x + 8 * m if mix else None)
        if rc != 0:
            return self._res(rc, None, [self.out, self.mix])
        v = self.out.cpu().numpy()
        out = {"mean": v[: k * m].reshape(k, m).copy(), "var": v[k * m: 2 * k * m].reshape(k, m).copy()}
        if mix:
            w = self.mix.cpu().numpy()
            out["mix_mean"], out["mix_var"] = w[:m].copy(), w[m:].copy()
        return H.Res(0, out, self._err())

    def set_option(self, what, value):
        return H.Res(self.lib.mi_gp_set_option(self.h, what, value), None, self._err())


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("size", list(H.SIZES))
def test_raw_walk(size, seed):
    _guard()
    p, o = _setup(size)
    ops = H.walk(seed, _steps(size), size)
    t0 = time.time()
    h = RawHandle(p)
    try:
        st = H.run_walk(h, p, o, ops, seed)
    except H.WalkFailure as e:
        if "returned -2" in str(e):
            _STATE["stop"] = str(e).splitlines()[-1]
        raise
    finally:
        h.close()
    print(f"raw walk size {size} seed {seed}: {st.line()} in {time.time() - t0:.1f} s")
    _report(kind="raw", size=size, seed=seed, steps=st.steps, refusals=st.refusals, infos=st.infos, value_compares=st.value_compares,
            bit_compares=st.bit_compares, seconds=time.time() - t0)
    assert st.steps == len(ops)


class _CountingLib:
    """The library with mi_gp_factor, mi_gp_lml_grad and mi_gp_factor_batch counted (everything else passes through)."""

    COUNTED = ("mi_gp_factor", "mi_gp_lml_grad", "mi_gp_factor_batch")

    def __init__(self, lib):
        self._lib = lib
        self.counts = {k: 0 for k in self.COUNTED}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in self.COUNTED:
            return fn

        def counted(*a):
            self.counts[name] += 1
            return fn(*a)

        return counted


class FacadeHandle:
    """handle_model's facade surface over MiGP's public methods."""

    def __init__(self, problem):
        from andvaranaut_amd import MiGP

        self.p = problem
        X, y = problem.data(0)
        self.gp = MiGP(X[: problem.n0], y[: problem.n0], problem.kernel, capacity=problem.cap)
        self.gp.lib = _CountingLib(self.gp.lib)
        self.counts = self.gp.lib.counts
        self.ver, self.next_ver, self.diag_id, self.next_diag = 0, 1, None, 0

    def close(self):
        self.gp.close()

    def lml(self, ti):
        v = self.gp.lml(self.p.theta(ti))
        return {"lml": v, "info": self.gp.info}

    def lml_grad(self, ti):
        v, g = self.gp.lml_grad(self.p.theta(ti))
        return {"lml": v, "grad": g, "info": self.gp.info}

    def lml_grad_data(self, ti):
        v, g, dy, dx = self.gp.lml_grad_data(self.p.theta(ti))
        return {"lml": v, "grad": g, "alpha": -dy, "gx": dx, "info": self.gp.info}

    def factor(self, ti):
        return {"info": self.gp.factor(self.p.theta(ti))}

    def predict(self, ti, via):
        mu, var = self.gp.predict(self.p.theta(ti), self.p.xnew, via_inverse=via)
        return {"mean": mu, "var": var}

    def predict_grad(self, ti, refactor):
        mu, var, dm, dv = self.gp.predict_grad(self.p.theta(ti), self.p.xnew, refactor=refactor)
        return {"mean": mu, "var": var, "dmean": dm, "dvar": dv}

    def predict_cov(self, ti):
        mu, cov = self.gp.predict_cov(self.p.theta(ti), self.p.xnew)
        return {"mean": mu, "cov": np.tril(cov)}

    def predict_batch(self, shift, k):
        mu, var = self.gp.predict_batch(self.p.thetas(shift, k), self.p.xnew, mixture=False)
        return {"mean": mu, "var": var, "info": self.gp.batch_info}

    def lml_grad_batch(self, shift, k):
        v, g = self.gp.lml_grad_batch(self.p.thetas(shift, k))
        return {"lml": v, "grad": g, "info": self.gp.batch_info}

    def append(self):
        n, k = self.gp.n, self.p.kapp
        X, y = self.p.data(self.ver)
        dg = self.p.diag(self.diag_id)
        assert self.gp.append(X[n: n + k], y[n: n + k], diag=None if dg is None else dg[n: n + k]) == 0
        assert self.gp.append_refactors == 0
        return {}

    def set_diag(self, how):
        if how == "vec":
            self.diag_id, self.next_diag = self.next_diag % 2, self.next_diag + 1
            self.gp.set_diag(self.p.diag(self.diag_id)[: self.gp.n])
        else:
            self.diag_id = None
            self.gp.set_diag(None)
        return {}

    def update_data(self):
        self.ver, self.next_ver = self.next_ver, self.next_ver + 1
        X, y = self.p.data(self.ver)
        self.gp.update_data(X[: self.gp.n], y[: self.gp.n])
        return {}

    def set_option(self, what, value):
        self.gp.set_option(what, value)
        return {}


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("size", [s for s in H.SIZES if s != max(H.SIZES)])
def test_facade_walk(size, seed):
    """(The three small sizes: the facade adds nothing size-dependent to the handle, and the oracle's gradients at N = 2600 are the
    module's most expensive part.)"""
    _guard()
    p, o = _setup(size)
    ops = H.facade_walk(seed, _steps(size), size)
    t0 = time.time()
    gp = FacadeHandle(p)
    try:
        st = H.run_facade_walk(gp, p, o, ops, seed)
    except RuntimeError as e:
        if "(-2)" in str(e):
            _STATE["stop"] = str(e)
        raise
    finally:
        gp.close()
    print(f"facade walk size {size} seed {seed}: {st.line()}; factorisations {gp.counts} in {time.time() - t0:.1f} s")
    _report(kind="facade", size=size, seed=seed, steps=st.steps, value_compares=st.value_compares, counts=gp.counts,
            seconds=time.time() - t0)
