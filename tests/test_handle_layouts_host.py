"""The layout harness without a GPU (tests/handle_layouts.py): the properties of the layout table, the bookkeeping's "what was
written outside", and a NumPy stand-in for the handle that really keeps its factor, U = L^-T, the batch's factors and its work
rows in flat strided arrays allocated by the Book -- honouring lda, ldw, the strides and the pointer offsets -- so that a layout
slip changes what it returns.  The stand-in passes seed 0's default walks under every layout, bit for bit against the default
layout's answers; five planted slips are each caught by handle_model.run_walk under the layout named for them and by none of
its checks under `default`.  That is the evidence that tests/test_gpu_handle_layouts.py would catch the same slip in the library."""
import numpy as np
import pytest
import scipy.linalg as sla

import handle_layouts as HL
import handle_model as H
from oracle import gp_oracle as orc

SEED = 0
SMALL = [s for s in H.SIZES if s != max(H.SIZES)]
_ORACLES, _REGISTRY = {}, {}


def _setup(size):
    if size not in _ORACLES:
        p = H.Problem(size)
        _ORACLES[size] = (p, H.Oracle(p))
    return _ORACLES[size]


# ------------------------------------------------------------------------------------------------------- the table
def test_layout_table_properties():
    capps = [HL.padded(H.SIZES[s]["cap"]) for s in SMALL]
    assert set(HL.LAYOUTS) >= {"default", "tight", "even", "wide", "offset"}
    for ly in HL.LAYOUTS.values():
        for capp in capps:
            bk = HL.Book(ly, capp)
            assert bk.lda % 2 == 0 and bk.ldw % 2 == 0 and bk.lda >= capp and bk.ldw >= capp, (ly, capp)
            bk.matrix("K", capp + 128, "K", 3), bk.matrix("Z", capp, "ZW", 3), bk.matrix("work", 128, "work", 3)
            assert bk.stride("K") % 2 == 0 and bk.stride("K") >= (capp + 128) * bk.lda
            assert bk.stride("Z") % 2 == 0 and bk.stride("Z") >= capp * bk.lda
            assert bk.stride("work") % 2 == 0 and bk.stride("work") >= 128 * bk.ldw
            assert ly.off_big % 2 == 0  # (an even ld implies 16-byte rows only from a 16-byte base)
    d, capp = HL.DEFAULT, 512
    assert (d.lda(capp), d.ldw(capp), d.fill, d.off_big, d.off_small, d.tail) == (capp + 16, capp + 16, "zeros", 0, 0, 0)
    assert any(ly.ldw(capp) < ly.lda(capp) for ly in HL.LAYOUTS.values())
    assert any(ly.ldw(capp) > ly.lda(capp) for ly in HL.LAYOUTS.values())
    assert any(ly.lda(capp) % 4 == 2 for ly in HL.LAYOUTS.values())
    assert any(ly.off_small % 2 == 1 for ly in HL.LAYOUTS.values())
    for size in (100, 700):  # no padding column at all: np == capp == lda
        assert HL.padded(size) == HL.padded(H.SIZES[size]["cap"]) == HL.LAYOUTS["tight"].lda(HL.padded(H.SIZES[size]["cap"]))
    assert all(HL.LAYOUTS[k].fill == "nan" for k in HL.NON_DEFAULT)


def test_book_reports_every_kind_of_outside_write():
    bk = HL.Book(HL.LAYOUTS["offset"], 128)
    K = bk.matrix("K", 256, "K", 2)
    v = bk.vector("out", 7)
    s = bk.specs["K"]
    assert (s.off, s.ld, s.stride) == (2, 144, 258 * 144) and bk.specs["out"].off == 1
    assert np.isnan(bk.flat["K"]).all() and (bk.flat["K"].view(np.int64) == HL.NAN_BITS).all()
    K[:, :, :128] = 1.0  # the writable region
    v[:] = 2.0
    assert bk.violation() is None and bk.checked == len(s.outside()) + len(bk.specs["out"].outside())
    assert len(s.outside()) == s.total - 2 * 256 * 128
    for name, flat_index, word in (("K", 1, "in front of the pointer"), ("K", 2 + 5 * 144 + 128, "row 5 column 128"),
                                   ("K", 2 + 256 * 144 + 3, "behind member 0's last row"),
                                   ("K", s.total - 1, "behind member 1's last row"), ("out", 0, "in front"), ("out", 8, "behind")):
        keep = bk.flat[name][flat_index]
        bk.flat[name][flat_index] = np.nan  # (another NaN: only the bits tell)
        got = bk.violation()
        assert got and got[:2] == (name, flat_index) and word in got[2] and "offset" in got[2], (name, flat_index, got)
        bk.flat[name].view(np.int64)[flat_index] = HL.NAN_BITS
        assert keep != keep and bk.violation() is None
    assert HL.Book(HL.DEFAULT, 128).matrix("K", 256, "K").shape == (256, 144)


# ---------------------------------------------------------------------------------------------------- the stand-in
class LayoutStandIn(H.OracleHandle):
    """OracleHandle's state machine with the conditional path computed THROUGH the buffers: mi_gp_factor / mi_gp_factor_batch
    write L and the beta row into K (lda), mi_gp_predict / _predict_cov / _predict_batch solve in the work rows (ldw, stride_work),
    mi_gp_predict_u / _predict_grad build U's upper triangle in Z, mi_gp_append commits its rows into K and y, y is read at its
    offset.  `slip` plants one layout mistake."""

    def __init__(self, problem, oracle, layout, slip=None):
        super().__init__(problem, oracle)
        p, self.slip = problem, slip
        capp = HL.padded(p.cap)
        bk = self.bk = HL.Book(layout, capp)
        self.lda, self.ldw = bk.lda, bk.ldw
        self.y = bk.vector("y", p.rows)
        bk.matrix("K", capp + 128, "K", H.BATCH_COUNT)
        bk.matrix("batch K", capp + 128, "K", H.BATCH_COUNT)
        bk.matrix("Z", capp, "ZW")
        bk.matrix("work", 2 * 128, "work")
        bk.matrix("batch work", 128, "work", H.BATCH_COUNT + 1)
        self.out = bk.vector("out", 2 * H.M_NEW)
        self.u_stale = False

    # ---- raw access: rows `ld` apart from the buffer's pointer, as a kernel would address them
    def _rows(self, name, ld, r0, nrows, ncols, member=0):
        s = self.bk.specs[name]
        base = s.off + member * s.stride + r0 * ld
        assert base + (nrows - 1) * ld + ncols <= s.total
        return np.lib.stride_tricks.as_strided(self.bk.flat[name][base:], (nrows, ncols), (8 * ld, 8))

    def _read_y(self, n):
        if self.slip == "y_pair_load":  # a 16-byte load: the address' low four bits are dropped
            s = self.bk.specs["y"]
            return np.array(self.bk.flat["y"][s.off & ~1: (s.off & ~1) + n])
        return np.array(self.y[:n])

    def _load_y(self):
        self.y[: self.n] = self.p.data(self.ver)[1][: self.n]

    def _write_factor(self, name, member, key):
        X, _, dg, th = self.o._args(key)
        n, npad = key[1], HL.padded(key[1])
        L = sla.cholesky(orc.noisy_cov(X, self.p.kerns, self.p.ops, th, "conditional", dg), lower=True, check_finite=False)
        self._rows(name, self.lda, 0, n, n, member)[:] = np.tril(L)
        self._rows(name, self.lda, npad, 1, n, member)[0] = sla.solve_triangular(L, self._read_y(n), lower=True, check_finite=False)
        if self.slip == "column_np":
            self._rows(name, self.lda, 3, 1, npad + 1, member)[0, npad] = 1.0

    def _factor_of(self, name, member, n):
        return (np.tril(np.array(self._rows(name, self.lda, 0, n, n, member))),
                np.array(self._rows(name, self.lda, HL.padded(n), 1, n, member)[0]))

    def _cross(self, key):
        X, _, _, th = self.o._args(key)
        _, _, _, gv, _ = orc.split_theta(th, self.p.d, self.p.nk)
        return orc.kernel_matrix(X, self.p.xnew, self.p.kerns, self.p.ops, th), orc.kernel_diag(self.p.kerns, self.p.ops, th, self.p.d), gv

    def _reduce(self, name, member, n, beta, kd, gv):
        ld = self.lda if self.slip == "work_read_lda" else self.ldw
        A = np.array(self._rows(name, ld, 0, H.M_NEW, n, member))
        self.out[: H.M_NEW] = A @ beta
        self.out[H.M_NEW:] = kd - np.sum(A * A, 1) + np.sqrt(gv) ** 2
        return np.array(self.out[: H.M_NEW]), np.array(self.out[H.M_NEW:])

    def _solve_predict(self, kname, wname, member, key):
        """mi_gp_predict's three steps: K(X*, X) rows into the work block, A = L^-1 K(X, X*) in place, the reduction."""
        n = key[1]
        L, beta = self._factor_of(kname, member, n)
        kx, kd, gv = self._cross(key)
        W = self._rows(wname, self.ldw, 0, H.M_NEW, n, member)
        W[:] = kx.T
        W[:] = sla.solve_triangular(L, np.array(W).T, lower=True, check_finite=False).T
        return self._reduce(wname, member, n, beta, kd, gv)

    def _build_u(self):
        n = self.n
        L, _ = self._factor_of("K", 0, n)
        U = sla.solve_triangular(L, np.eye(n), lower=True, check_finite=False).T
        iu = np.triu_indices(n)
        self._rows("Z", self.lda, 0, n, n)[iu] = U[iu]  # (only the upper triangle is ever written)
        self.u_stale = False

    def _u_predict(self):
        n = self.n
        Z = np.array(self._rows("Z", self.lda, 0, n, n))
        U = Z if self.slip == "u_reads_unwritten" else np.triu(Z)
        _, beta = self._factor_of("K", 0, n)
        kx, kd, gv = self._cross(self.f_key)
        self._rows("work", self.ldw, 128, H.M_NEW, n)[:] = kx.T
        self._rows("work", self.ldw, 0, H.M_NEW, n)[:] = np.array(self._rows("work", self.ldw, 128, H.M_NEW, n)) @ U
        return self._reduce("work", 0, n, beta, kd, gv)

    # ---- the entry points that touch the buffers
    def set_data(self, how):
        r = super().set_data(how)
        self._load_y()
        return r

    def factor(self, ti):
        r = super().factor(ti)
        if r.rc == 0:
            self._write_factor("K", 0, self.f_key)
        return r

    def predict(self):
        if not self.factored:
            return self.no
        return H.Res(0, dict(zip(("mean", "var"), self._solve_predict("K", "work", 0, self.f_key))))

    def predict_cov(self):
        r = super().predict_cov()
        if r.rc == 0:
            r.out["mean"] = self._solve_predict("K", "work", 0, self.f_key)[0]
        return r

    def _make_u(self):
        if self.factored and not self.have_u:
            self._build_u()
        super()._make_u()

    def predict_u(self):
        r = super().predict_u()
        if r.rc == 0:
            r.out["mean"], r.out["var"] = self._u_predict()
        return r

    def predict_grad(self):
        r = super().predict_grad()
        if r.rc == 0:
            r.out["mean"], r.out["var"] = self._u_predict()
        return r

    def _append_u(self, key):
        super()._append_u(key)
        self.u_stale = True

    def append(self, how, k):
        n, old = self.n, self.f_key
        r = super().append(how, k)
        if r.rc != 0 or self.n == n:
            return r
        X, y, dg, th = self.o._args(self.f_key)
        n2, npad, npad2 = self.n, HL.padded(n), HL.padded(self.n)
        Kf = orc.noisy_cov(X, self.p.kerns, self.p.ops, th, "conditional", dg)
        L11, beta1 = self._factor_of("K", 0, n)
        L21 = sla.solve_triangular(L11, Kf[:n, n:], lower=True, check_finite=False).T
        L22 = sla.cholesky(Kf[n:, n:] - L21 @ L21.T, lower=True, check_finite=False)
        beta2 = sla.solve_triangular(L22, y[n:] - L21 @ beta1, lower=True, check_finite=False)
        ld = self.ldw if self.slip == "commit_ldw" else self.lda  # the commit of the new rows
        self._rows("K", ld, n, k, n2)[:] = np.hstack([L21, L22])
        self._rows("K", self.lda, npad2, 1, n2)[0] = np.concatenate([beta1, beta2])  # (the beta row moves along)
        self.y[n: n2] = y[n:]
        if self.u_stale:
            self._build_u()
        assert old[1] == n
        return r

    def _batch_k(self):
        return "K" if self.batch["alias"] else "batch K"

    def factor_batch(self, k, shift):
        r = super().factor_batch(k, shift)
        if r.rc == 0:
            for m, key in enumerate(self.b_cond):
                if r.out["info"][m] == 0:
                    self._write_factor(self._batch_k(), m, key)
        return r

    def predict_batch(self, k):
        r = super().predict_batch(k)
        if r.rc == 0:
            for m, key in enumerate(self.b_cond):
                if self.o.cond(key)["info"] == 0:
                    r.out["mean"][m], r.out["var"][m] = self._solve_predict(self._batch_k(), "batch work", m, key)
        return r


def _walk(size, layout, slip=None):
    p, o = _setup(size)
    ops = H.walk(SEED, H.SIZES[size]["steps"], size)
    if size not in _REGISTRY:  # the default layout's answers, once per size
        _REGISTRY[size] = {}
        H.run_walk(LayoutStandIn(p, o, HL.DEFAULT), p, o, ops, SEED, registry=_REGISTRY[size])
    reg = dict(_REGISTRY[size])  # (a failing walk must not leave its answers behind)
    return H.run_walk(LayoutStandIn(p, o, HL.LAYOUTS[layout], slip), p, o, ops, SEED, registry=reg)


@pytest.mark.parametrize("size", SMALL)
@pytest.mark.parametrize("layout", list(HL.LAYOUTS))
def test_stand_in_passes_under_every_layout(layout, size):
    st = _walk(size, layout)
    print(f"{layout} size {size}: {st.line()} padding elements {st.padding_checks}")
    assert st.steps == H.SIZES[size]["steps"] and st.value_compares > 0
    assert st.bit_compares >= sum(1 for _ in _REGISTRY[size])  # every answer of the default walk was met again
    assert (st.padding_checks > 0) == (layout != "default")


# slip -> (the layout named for it, the layouts that cannot see it)
SLIPS = {
    "work_read_lda": ("even", ("default", "tight")),          # 1. predict reads the work rows with lda instead of ldw
    "commit_ldw": ("wide", ("default", "tight")),             # 2. append's commit writes its rows with ldw instead of lda
    "column_np": ("tight", ("default",)),                     # 3. one element at column np is written
    "u_reads_unwritten": ("even", ("default",)),              # 4. U's build reads a tile that was never written
    "y_pair_load": ("offset", ("default", "tight", "even", "wide")),  # 5. y is read with a 16-byte-aligned pair load
}


def _caught(slip, layout):
    out = []
    for size in SMALL:
        try:
            _walk(size, layout, slip)
        except H.WalkFailure as e:
            out.append((size, str(e)))
    return out


@pytest.mark.parametrize("slip", list(SLIPS))
def test_a_planted_slip_is_caught_under_its_layout_and_not_under_default(slip):
    named, blind = SLIPS[slip]
    caught = _caught(slip, named)
    print(slip, named, [(s, m.splitlines()[1][:160]) for s, m in caught])
    assert caught, f"{slip}: every seed-0 walk passed under {named}"
    assert all(m.startswith("replay: handle_model.walk(seed=0") for _, m in caught)
    for layout in blind:
        assert not _caught(slip, layout), f"{slip} is visible under {layout}"


def test_the_column_np_slip_is_seen_where_there_is_no_padding_column():
    """np == capp == lda at sizes 100 and 700: the element lands in the next row (tight: a wrong value) or in the padding (every
    other poisoned layout: the bookkeeping names it)."""
    sizes = {s for s, _ in _caught("column_np", "tight")}
    assert sizes >= {100, 700}, sizes
    msgs = _caught("column_np", "wide")
    assert {s for s, _ in msgs} >= {100, 700} and all("was written (layout wide)" in m for s, m in msgs if s in (100, 700)), msgs
