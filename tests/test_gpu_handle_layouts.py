"""One GP handle under every buffer layout include/mi_gp.h allows (tests/handle_layouts.py).

The rest of the suite runs one point of that space: lda = np + 16 (every row on a 128-byte boundary), the same value passed as
every ldw, exact strides, pointers at the start of zero-filled allocations.  Here the walks of tests/handle_model.py go over
RawHandle (tests/test_gpu_handle_sequences.py) on `tight` (lda = ldw = capp: no padding column at sizes 100 and 700), `even`
(ld % 4 == 2, ldw > lda, gaps), `wide` (ldw < lda, other gaps) and `offset` (matrices 16 bytes, vectors / points / outputs 8 bytes
into their allocation) buffers, every allocation filled with one NaN bit pattern, and every call is checked three ways:
  * against the oracle at the module's cond-scaled tolerances (handle_model.run_walk);
  * for unchanged bits outside the region the header lets the library write (padding columns, gaps, head, tail);
  * bit for bit against the `default` layout's answer to the same query in the same state -- no launcher reads a leading
    dimension, stride or pointer to choose a kernel, tile form or k order, so the arithmetic per element cannot depend on them.
Directed cases add the schedules the walks do not reach at these sizes, two appends across a tile boundary with and without U
resident, a batch with a failed member and the mixture outputs, and the refusals of every ldw / lda / stride_work.
tests/test_handle_layouts_host.py shows on a NumPy stand-in that the harness catches planted layout slips.  A return of -2 ends
the module (and test_gpu_handle_sequences's: they share its state).  One record per test goes to handle_layouts.json in the
directory $MIGP_TEST_RECORD_DIR names (default: test_records/ in the repository root)."""
import ctypes
import json
import os
import time

import numpy as np
import pytest
from conftest import ROOT

import handle_layouts as HL
import handle_model as H
import test_gpu_handle_sequences as S

pytestmark = pytest.mark.gpu

SEED = 0
RECORD = {}
_DEFAULT = {}  # (size, what) -> what the default layout answered: the walks' registry, the directed cases' results
DP = ctypes.POINTER(ctypes.c_double)


def _record(test, **kw):
    RECORD[test] = kw
    out = os.environ.get("MIGP_TEST_RECORD_DIR") or os.path.join(ROOT, "test_records")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "handle_layouts.json"), "w") as f:
        json.dump(RECORD, f, indent=1, sort_keys=True)


def _run(p, o, ops, layout, registry, seed=None):
    """One handle under `layout` through `ops`; returns (Stats, handle) -- the caller closes it."""
    S._guard()
    h = S.RawHandle(p, HL.LAYOUTS[layout])
    try:
        return H.run_walk(h, p, o, ops, seed, registry=registry), h
    except H.WalkFailure as e:
        h.close()
        if "returned -2" in str(e):
            S._STATE["stop"] = str(e).splitlines()[-1]
        raise H.WalkFailure(f"layout {layout}: {e}") from None


def _default_registry(p, o, ops, what, seed=None):
    """The default layout's answers to `ops`, once per (size, what), shared by every layout."""
    key = (p.size, what)
    if key not in _DEFAULT:
        reg = {}
        st, h = _run(p, o, ops, "default", reg, seed)
        h.close()
        assert st.padding_checks == 0
        _DEFAULT[key] = reg
    return dict(_DEFAULT[key])  # (a failing walk must not leave its answers behind)


def _finish(test, layout, size, st, t0, **more):
    print(f"{test}: {st.line()} padding elements {st.padding_checks} in {time.time() - t0:.1f} s")
    _record(test, layout=layout, size=size, steps=st.steps, bit_compares=st.bit_compares, value_compares=st.value_compares,
            padding_checks=st.padding_checks, seconds=round(time.time() - t0, 2), **more)


def test_the_device_bookkeeping_names_an_outside_write():
    """handle_layouts.Book on the torch backend (the NumPy one: tests/test_handle_layouts_host.py): padding, gap, head and tail."""
    S._guard()
    import torch

    bk = HL.Book(HL.LAYOUTS["offset"], 128, S.TorchBackend(torch, torch.device("cuda", 0)))
    K, v = bk.matrix("K", 256, "K", 2), bk.vector("out", 7)
    assert bool(torch.isnan(bk.flat["K"]).all()) and K.data_ptr() == bk.flat["K"].data_ptr() + 16 and v.data_ptr() % 16 == 8
    K[:, :, :128] = 1.0
    v.fill_(2.0)
    assert bk.violation() is None and bk.checked > 0
    for name, i in (("K", 1), ("K", 2 + 5 * 144 + 128), ("K", 2 + 256 * 144 + 3), ("K", bk.specs["K"].total - 1), ("out", 0), ("out", 8)):
        bk.flat[name][i] = float("nan")  # (another NaN: only the bits tell)
        got = bk.violation()
        assert got and got[:2] == (name, i), (name, i, got)
        bk.flat[name].view(torch.int64)[i] = HL.NAN_BITS
    assert bk.violation() is None


# --------------------------------------------------------------------------------------------------------- a. the walks
def _layout_walk(layout, size, test):
    p, o = S._setup(size)
    ops = H.walk(SEED, S._steps(size), size)
    reg = _default_registry(p, o, ops, "walk", SEED)
    answers = len(reg)
    t0 = time.time()
    st, h = _run(p, o, ops, layout, reg, SEED)
    h.close()
    _finish(test, layout, size, st, t0)
    assert st.steps == len(ops)
    assert st.bit_compares >= answers > 0 and st.value_compares > 0 and st.padding_checks > 0


@pytest.mark.parametrize("size", [100, 300, 700])
@pytest.mark.parametrize("layout", HL.NON_DEFAULT)
def test_layout_walk(layout, size):
    _layout_walk(layout, size, f"walk[{layout}-{size}]")


def test_layout_walk_on_two_streams():
    """Size 2600 (its 12 steps, two streams from the start) under `even`."""
    _layout_walk("even", 2600, "walk[even-2600]")


# ----------------------------------------------------------------------------- b. the schedules the walks do not reach
SCHED_DEFAULTS = {0: 1, 2: 0, 26: 2, 32: 2048, 35: 32, 37: 24, 46: 31}
SCHED_SETS = [("panels", {37: 0, 2: 2}), ("lookahead", {0: 2}), ("events", {26: 0})]
# the option combinations of tests/test_gpu_stream_edges.py's 32 / 35 / 37 / 46 test
SCHED_SETS += [(f"r5-{i}", dict(zip((32, 35, 37, 46), c))) for i, c in enumerate(
    [(2048, 32, 24, 31), (0, 32, 24, 31), (2048, 0, 24, 31), (2048, 32, 0, 31), (0, 0, 0, 31), (2048, 64, 34, 31), (64, 8, 12, 31),
     (2048, 32, 24, 34), (2048, 32, 12, 40)])]
SCHED_SIZES = {700: None, 1100: dict(kernel="Matern52", d=4, cap=1100, kapp=1, steps=0)}  # 6 and 9 tile columns


def _sched_setup(size):
    if SCHED_SIZES[size] is None:
        return S._setup(size)
    if ("sched", size) not in S._STATE["oracles"]:
        p = H.Problem(size, SCHED_SIZES[size])
        S._STATE["oracles"][("sched", size)] = (p, H.Oracle(p))
    return S._STATE["oracles"][("sched", size)]


def _sched_answers(p, layout):
    """name -> {output: bits} of mi_gp_lml, mi_gp_lml_grad, mi_gp_factor + mi_gp_predict + mi_gp_predict_u per option set, the
    values under the library's defaults, and the padding elements checked."""
    S._guard()
    h = S.RawHandle(p, HL.LAYOUTS[layout])
    got, values, calls = {}, {}, 0
    try:
        assert h.set_data("same").rc == 0
        for name, opts in [("defaults", {})] + SCHED_SETS:
            for k, v in {**SCHED_DEFAULTS, **opts}.items():
                assert h.set_option(k, v).rc == 0
            for call, args in (("lml", (0,)), ("lml_grad", (0,)), ("factor", (0,)), ("predict", ()), ("predict_u", ())):
                r = getattr(h, call)(*args)
                if r.rc == -2:
                    S._STATE["stop"] = f"{layout} {name} {call}: {r.err}"
                assert r.rc == 0, (layout, name, call, r.rc, r.err)
                v = h.bk.violation()
                assert v is None, (layout, name, call, v[2])
                calls += 1
                for oname, val in r.out.items():
                    got[(name, call, oname)] = H._bits(val)
                if name == "defaults":
                    values[call] = r.out
    finally:
        h.close()
    return got, values, h.bk.checked, calls


@pytest.mark.parametrize("size", list(SCHED_SIZES))
@pytest.mark.parametrize("layout", ["tight", "even", "wide"])
def test_schedules_return_the_default_layouts_bits(layout, size):
    p, o = _sched_setup(size)
    key = (0, p.n0, None, 0)
    if (size, "sched") not in _DEFAULT:
        got, values, _, _ = _sched_answers(p, "default")
        n = 0
        for call, out in values.items():  # once per size: the defaults against the oracle (tests/test_gpu_random_sweep.py's tolerances)
            n += H._check_values(o, p, call, out, key, H.Expect(0), f"size {size} default layout {call}") if out else 0
        assert n > 0
        _DEFAULT[(size, "sched")] = got
    ref = _DEFAULT[(size, "sched")]
    t0 = time.time()
    got, _, checked, calls = _sched_answers(p, layout)
    assert set(got) == set(ref) and len(got) == 7 * (len(SCHED_SETS) + 1)
    diff = [k for k in ref if not np.array_equal(ref[k], got[k])]
    print(f"schedules[{layout}-{size}]: {calls} calls, {len(got)} bit comparisons, padding elements {checked} in {time.time() - t0:.1f} s")
    _record(f"schedules[{layout}-{size}]", layout=layout, size=size, steps=calls, bit_compares=len(got), value_compares=0,
            padding_checks=checked, seconds=round(time.time() - t0, 2))
    assert not diff, f"layout {layout} size {size}: bits differ from the default layout's for (option set, call, output) {diff}"
    assert checked > 0


# ------------------------------------------------------------------------------------- c. append across a tile boundary
APPEND_OPS = {
    "without_u": [("set_data", "same"), ("reserve", 420), ("factor", 0), ("append", "ok"), ("append", "ok"), ("lml_parts",),
                  ("predict",), ("predict_u",), ("predict_grad",)],
    "with_u": [("set_data", "same"), ("reserve", 420), ("factor", 1), ("predict_u",), ("append", "ok"), ("append", "ok"),
               ("lml_parts",), ("predict",), ("predict_u",), ("predict_grad",)],
}


@pytest.mark.parametrize("u", list(APPEND_OPS))
@pytest.mark.parametrize("layout", ["wide", "tight"])
def test_two_appends_across_the_tile_boundary(layout, u):
    """300 -> 350 -> 400 crosses row 384 in the second append (the beta row moves, the padded size grows by a tile): the grown
    parts against the oracle, the three predictors against the oracle and the default layout's bits, nothing written outside.
    (Seed 0's size-300 walk appends too, but not twice in a row from 300 in both states of U.)"""
    p, o = S._setup(300)
    ops = APPEND_OPS[u]
    reg = _default_registry(p, o, ops, "append_" + u)
    answers = len(reg)
    t0 = time.time()
    st, h = _run(p, o, ops, layout, reg)
    n = h.n
    h.close()
    _finish(f"append[{layout}-{u}]", layout, 300, st, t0)
    assert n == 400 and st.steps == len(ops) and st.refusals == 0 and st.infos == 0
    assert st.bit_compares >= answers + 2 and st.value_compares > 0 and st.padding_checks > 0


# --------------------------------------------------------------------------------------------------------------- d. batch
BATCH_SHIFT = 2  # handle_model.MEMBERS[2] = (2, BAD, 0, 1): member 1 fails
BATCH_OPS = [("set_data", "same"), ("lml_grad", 2), ("lml_grad", 0), ("factor", 2), ("predict",), ("factor", 0), ("predict",),
             ("set_batch", "zw"), ("lml_grad_batch", 3, BATCH_SHIFT), ("factor_batch", 3, BATCH_SHIFT), ("predict_batch", 3)]


@pytest.mark.parametrize("layout", ["wide", "offset"])
def test_batch_with_a_failed_member_and_the_mixture(layout):
    """Three members at N = 300, the middle one with a theta that is not positive definite: members equal the single evaluations
    bit for bit (the registry holds them from the same walk), the failed member's rows are NaN, the mixture is the documented
    two-pass formula over the two good members and the default layout's bits; gaps and padding keep their fill."""
    assert H.MEMBERS[BATCH_SHIFT][1] == H.BAD
    p, o = S._setup(300)
    key = ("batch", 300)
    if key not in _DEFAULT:
        reg = {}
        st, h = _run(p, o, BATCH_OPS, "default", reg)
        r = h.predict_batch(3, mix=True)
        h.close()
        assert r.rc == 0
        _DEFAULT[key] = (reg, r.out)
    reg, ref = dict(_DEFAULT[key][0]), _DEFAULT[key][1]
    t0 = time.time()
    st, h = _run(p, o, BATCH_OPS, layout, reg)
    try:
        r = h.predict_batch(3, mix=True)
        v = h.bk.violation()
    finally:
        h.close()
    _finish(f"batch[{layout}]", layout, 300, st, t0)
    assert r.rc == 0 and v is None, (r.rc, r.err, v)
    assert st.bit_compares >= 2 * 2 + 2 * 2 and st.padding_checks > 0  # lml + grad and mean + var of the two good members
    for name in ("mean", "var", "mix_mean", "mix_var"):
        assert np.array_equal(H._bits(r.out[name]), H._bits(ref[name])), name
    assert np.isnan(r.out["mean"][1]).all() and np.isnan(r.out["var"][1]).all()
    good = [0, 2]
    mu, var = r.out["mean"][good], r.out["var"][good]
    mm = mu[0] + (mu - mu[0]).sum(0) / 2  # sums relative to the first member's moments
    mv = var[0] + (var - var[0]).sum(0) / 2 + ((mu - mm) ** 2).sum(0) / 2
    assert np.allclose(r.out["mix_mean"], mm, rtol=1e-13, atol=1e-13 * np.abs(mu).max())
    assert np.allclose(r.out["mix_var"], mv, rtol=1e-12, atol=1e-13 * np.abs(mv).max())


# ----------------------------------------------------------------------------------------------------------- e. refusals
def test_bad_leading_dimensions_and_strides_are_refused():
    """ldw = np - 2 and np + 1 at every entry point that takes one, lda in mi_gp_set_data, stride_work odd or too small: -1 with
    a text, the outputs' sentinels in place, nothing written outside.  (mi_gp_set_batch's strides: tests/test_gpu_batch_sweep.py.)"""
    S._guard()
    p, o = S._setup(300)
    h = S.RawHandle(p, HL.LAYOUTS["even"])
    lib, t0, n = h.lib, time.time(), 0
    m, npad = H.M_NEW, HL.padded(p.n0)
    try:
        for op in (("set_data", "same"), ("reserve", p.cap), ("set_batch", "zw"), ("factor_batch", 3, 0), ("factor", 0), ("predict_u",)):
            assert getattr(h, op[0])(*op[1:]).rc == 0, (op, h._err())
        good = h.predict().out
        o_, x, w = h.out.data_ptr(), h.xn.data_ptr(), h.work.data_ptr()
        sw = h.bk.stride("batch work")

        def refused(rc, text, *bufs):
            assert rc == -1 and text in h._err(), (rc, h._err(), text)
            assert all(bool((b == S.SENTINEL).all()) for b in bufs)
            assert h.bk.violation() is None
            return 1

        for ldw in (npad - 2, npad + 1):
            for fn, extra in ((lib.mi_gp_predict, ()), (lib.mi_gp_predict_u, ()), (lib.mi_gp_predict_grad, (o_ + 16 * m, o_ + 16 * m + 8 * m * p.d))):
                h._fill(h.out)
                n += refused(fn(h.h, x, m, w, ldw, o_, o_ + 8 * m, 1, *extra), "ldw must be even and >= padded n", h.out)
            h._fill(h.out, h.cov)
            n += refused(lib.mi_gp_predict_cov(h.h, x, m, w, ldw, o_, h.cov.data_ptr(), 128, 1), "ldw must be even and >= padded n", h.out, h.cov)
            h._fill(h.out)
            n += refused(lib.mi_gp_predict_batch(h.h, 3, x, m, h.bwork.data_ptr(), ldw, sw, o_, o_ + 8 * 3 * m, 1, None, None),
                         "ldw must be even and >= padded n", h.out)
        for stride in (128 * h.ldw - 2, 128 * h.ldw + 1):
            h._fill(h.out)
            n += refused(lib.mi_gp_predict_batch(h.h, 3, x, m, h.bwork.data_ptr(), h.ldw, stride, o_, o_ + 8 * 3 * m, 1, None, None),
                         "stride_work must be even and >=", h.out)
        np2 = HL.padded(p.n0 + 100)  # 300 + 100 rows: padded(n + k) = 512
        for ldw in (np2 - 2, np2 + 1):
            head = h.Kall[0].clone()
            rc = lib.mi_gp_append(h.h, h.Xpool[p.n0:].data_ptr(), h.ypool[p.n0:].data_ptr(), None, 100, h.awork.data_ptr(), ldw)
            n += refused(rc, "ldw must be even and >= padded(n + k)")
            assert h.torch.equal(head.view(h.torch.int64), h.Kall[0].view(h.torch.int64))
        # the refusals changed no state: the factor, U and the batch's factors answer as before
        again = h.predict().out
        assert all(np.array_equal(H._bits(good[k]), H._bits(again[k])) for k in good)
        assert h.predict_u().rc == 0 and h.predict_batch(3).rc == 0
        b = h._lib_mod.MiGpBuffers()
        b.X_dev, b.y_dev, b.K_dev, b.Z_dev, b.W_dev = h.X.data_ptr(), h.y.data_ptr(), h.Kall.data_ptr(), h.Z.data_ptr(), h.W.data_ptr()
        for lda in (npad - 2, npad + 1):
            b.lda = lda
            n += refused(lib.mi_gp_set_data(h.h, ctypes.byref(b)), "lda must be even and >= padded n")
        assert h.predict().rc == 0  # (a refused mi_gp_set_data keeps the binding and the resident state)
    finally:
        h.close()
    _record("refusals[even]", layout="even", size=300, steps=n, bit_compares=len(good), value_compares=0,
            padding_checks=h.bk.checked, seconds=round(time.time() - t0, 2))
    assert n == 2 * 5 + 2 + 2 + 2
