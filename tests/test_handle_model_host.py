"""The handle's state model without a GPU (tests/handle_model.py): the header's sentences about resident state as asserts on the
model, the whole harness of tests/test_gpu_handle_sequences.py against the NumPy stand-in for every default seed and size, the
conditions the default walks must meet, and deliberately wrong stand-ins -- one documented rule broken each -- that the harness
must catch within the default seeds.  That last part is the evidence that the device test would catch the same slip in the
library or in MiGP's shadow of the state."""
import os
import re

import numpy as np
import pytest
from conftest import ROOT

import handle_model as H

_ORACLES = {}


def _setup(size):
    if size not in _ORACLES:
        p = H.Problem(size)
        _ORACLES[size] = (p, H.Oracle(p))
    return _ORACLES[size]


def _header():
    with open(os.path.join(ROOT, "include", "mi_gp.h")) as f:
        text = f.read()
    return re.sub(r"\s+", " ", re.sub(r"\n\s*\*", " ", text))


# ---------------------------------------------------------------------------------------------- a. the header's sentences
def _model(*ops):
    m = H.Model(H.Problem(100))
    last = None
    for op in ops:
        last = m.step(op)
    return m, last


SENTENCES = [
    # (sentence of include/mi_gp.h, operations, the call it rules on, expected return, refusal)
    ("mi_gp_predict*, mi_gp_predict_cov and mi_gp_append return -1 until the next mi_gp_factor",
     [("set_data", "same"), ("factor", 0), ("set_data", "same")], ("predict",), -1),
    ("mi_gp_predict*, mi_gp_predict_cov and mi_gp_append return -1 until the next mi_gp_factor",
     [("set_data", "same"), ("reserve", 120), ("factor", 0), ("set_data", "same")], ("append", "ok"), -1),
    ("mi_gp_alpha and mi_gp_grad_x until the next mi_gp_lml_grad",
     [("set_data", "same"), ("lml_grad", 0), ("set_data", "new")], ("alpha",), -1),
    ("Before the first mi_gp_set_data they return -1", [], ("lml", 0), -1),
    ("ends what an earlier one left resident -- the factor of mi_gp_factor, U and K^-1",
     [("set_data", "same"), ("factor", 0), ("lml", 1)], ("predict_cov",), -1),
    ("ends what an earlier one left resident -- the factor of mi_gp_factor, U and K^-1",
     [("set_data", "same"), ("lml_grad", 0), ("factor", 1)], ("grad_x",), -1),
    ("ends what an earlier one left resident -- the factor of mi_gp_factor, U and K^-1",
     [("set_data", "same"), ("factor", 0), ("factor", H.BAD)], ("predict",), -1),
    ("Returns -1, and writes neither output, before the first single evaluation and while the last one returned info > 0 or -1",
     [("set_data", "same"), ("lml", 0), ("lml", H.BAD)], ("lml_parts",), -1),
    ("mi_gp_set_data, mi_gp_set_diag and the batch calls leave them",
     [("set_data", "same"), ("lml", 0), ("set_diag", "vec"), ("set_data", "new")], ("lml_parts",), 0),
    ("Every call, a repeated pointer included, ends the resident state like mi_gp_set_data",
     [("set_data", "same"), ("factor", 0), ("predict_u",), ("set_diag", "none")], ("predict_u",), -1),
    ("The handle's single-evaluation state (factor, K^-1) is invalidated",
     [("set_data", "same"), ("set_batch", "plain"), ("factor", 0), ("lml_batch", 2, 0)], ("predict",), -1),
    ("The handle's single-evaluation state (factor, K^-1) is invalidated",
     [("set_data", "same"), ("set_batch", "zw"), ("lml_grad", 0), ("lml_grad_batch", 2, 0)], ("alpha",), -1),
    ("A batch call that is refused (-1: no buffers bound, k > count, no Z_dev / W_dev for the gradient) changes nothing",
     [("set_data", "same"), ("set_batch", "plain"), ("factor", 0), ("lml_batch", 4, 0), ("lml_grad_batch", 2, 0)], ("predict",), 0),
    ("(after mi_gp_set_data: -1 before)", [], ("set_batch", "zw"), -1),
    ("the single-evaluation state stays", [("set_data", "same"), ("factor", 0), ("set_batch", "alias")], ("predict",), 0),
    ("so with overlapping buffers it also ends the batch's conditional factors",
     [("set_data", "same"), ("set_batch", "alias"), ("factor_batch", 3, 0), ("lml", 0)], ("predict_batch", 3), -1),
    ("Without overlap single evaluations leave them",
     [("set_data", "same"), ("set_batch", "zw"), ("factor_batch", 3, 0), ("lml_grad", 0)], ("predict_batch", 3), 0),
    ("Returns -1 unless mi_gp_factor_batch with the same k was the last batch call",
     [("set_data", "same"), ("set_batch", "zw"), ("factor_batch", 3, 0)], ("predict_batch", 2), -1),
    ("Returns -1 unless mi_gp_factor_batch with the same k was the last batch call",
     [("set_data", "same"), ("set_batch", "zw"), ("factor_batch", 3, 0), ("lml_batch", 3, 0)], ("predict_batch", 3), -1),
    ("(mi_gp_set_batch, mi_gp_set_data and mi_gp_set_diag also end it)",
     [("set_data", "same"), ("set_batch", "zw"), ("factor_batch", 3, 0), ("set_batch", "zw")], ("predict_batch", 3), -1),
    ("(mi_gp_set_batch, mi_gp_set_data and mi_gp_set_diag also end it)",
     [("set_data", "same"), ("set_batch", "zw"), ("factor_batch", 3, 0), ("set_diag", "vec")], ("predict_batch", 3), -1),
    ("mi_gp_predict changes no handle state", [("set_data", "same"), ("lml_grad", 0), ("predict",)], ("alpha",), 0),
    ("The handle's state is not changed", [("set_data", "same"), ("factor", 0), ("predict_cov",)], ("predict_grad",), 0),
    ("changes NO handle state: the resident factor, U, K^-1, the batch state and the append capacity stay valid",
     [("set_data", "same"), ("set_batch", "zw"), ("factor_batch", 2, 0), ("sample_cov", 1, 0)], ("predict_batch", 2), 0),
    ("-1 if capacity < n", [("set_data", "same")], ("reserve", 99), -1),
    ("Without it a handle cannot grow (mi_gp_append returns -1)", [("set_data", "same"), ("factor", 0)], ("append", "ok"), -1),
    ("(resident contents kept)", [("set_data", "same"), ("lml_grad", 0), ("reserve", 120)], ("alpha",), 0),
    ("(resident contents kept)", [("set_data", "same"), ("factor", 0), ("predict_u",), ("reserve", 120)], ("predict_grad",), 0),
    ("Returns -1 without a prior mi_gp_factor, for n + k > capacity",
     [("set_data", "same"), ("reserve", 110), ("factor", 0), ("append", "ok")], ("append", "ok"), -1),
    ("mi_gp_predict, _predict_u and _predict_grad continue without a refactorisation",
     [("set_data", "same"), ("reserve", 120), ("factor", 0), ("append", "ok")], ("predict_u",), 0),
    ("mi_gp_lml_parts returns the grown logdet and quad",
     [("set_data", "same"), ("reserve", 120), ("factor", 0), ("append", "ok")], ("lml_parts",), 0),
    ("K^-1 is invalidated (mi_gp_alpha / mi_gp_grad_x need a new mi_gp_lml_grad)",
     [("set_data", "same"), ("reserve", 120), ("factor", 0), ("append", "ok")], ("grad_x",), -1),
    ("every batch call returns -1 until mi_gp_set_batch is called again",
     [("set_data", "same"), ("set_batch", "zw"), ("reserve", 120), ("factor", 0), ("append", "ok")], ("lml_batch", 1, 0), -1),
    ("the handle is then exactly as it was",
     [("set_data", "same"), ("set_diag", "vec"), ("reserve", 120), ("factor", 0), ("append", "dup")], ("predict",), 0),
]


@pytest.mark.parametrize("i", range(len(SENTENCES)))
def test_header_sentence(i):
    sentence, ops, call, want = SENTENCES[i]
    assert re.sub(r"\s+", " ", sentence) in _header(), f"include/mi_gp.h no longer says: {sentence}"
    _, e = _model(*ops, call)
    assert e.rc == want, (sentence, ops, call, e.rc, e.refusal)


def test_append_keeps_the_model_on_the_grown_problem():
    m, e = _model(("set_data", "same"), ("reserve", 120), ("factor", 1), ("predict_u",), ("append", "ok"), ("predict_grad",))
    assert m.n == 107 and e.key == (0, 107, None, 1)
    # the bits of the grown factor are not those of a fresh factorisation at n + k, nor of an append without U
    m2, e2 = _model(("set_data", "same"), ("reserve", 120), ("factor", 1), ("append", "ok"), ("predict_grad",))
    assert e.bits["mean"] != e2.bits["mean"] and e.key == e2.key


# ------------------------------------------------------------------------------------------------------------ c. the walks
def _default_walks():
    return [(seed, size, H.walk(seed, H.SIZES[size]["steps"], size)) for size in H.SIZES for seed in H.DEFAULT_SEEDS]


def test_walks_are_deterministic_prefix_stable_and_full_length():
    for seed, size, ops in _default_walks():
        steps = H.SIZES[size]["steps"]
        assert len(ops) == steps, (seed, size)  # no walk ends before step `steps`
        assert ops == H.walk(seed, steps, size)
        assert H.walk(seed, steps // 2, size) == ops[: steps // 2]  # (the replay line of a failure relies on this)


def _model_stats():
    tot = H.Stats()
    for seed, size, ops in _default_walks():
        m, st, prev = H.Model(H.Problem(size)), H.Stats(), None
        for op in ops:
            e = m.step(op)
            st.steps += 1
            st.ops[op[0]] = st.ops.get(op[0], 0) + 1
            if prev in H.CHANGERS and op[0] in H.CONSUMERS:
                st.pairs.add((prev, op[0]))
            prev = op[0]
            if e.rc == -1:
                st.refusals += 1
                st.refusal_kinds[e.refusal] = st.refusal_kinds.get(e.refusal, 0) + 1
        tot.add(st)
    return tot


def test_walk_conditions():
    st = _model_stats()
    few = {o: st.ops.get(o, 0) for o in H.ALL_OPS if st.ops.get(o, 0) < 5}
    assert not few, f"operations drawn fewer than 5 times over the default seeds: {few}"
    missing = [(c, q) for c in H.CHANGERS for q in H.CONSUMERS if (c, q) not in st.pairs]
    assert not missing, f"(state-changing, state-consuming) pairs that never occur: {missing}"
    unknown = set(st.refusal_kinds) - set(H.REFUSALS)
    assert not unknown, unknown
    never = [r for r in H.REFUSALS if r not in st.refusal_kinds]
    assert not never, f"refusals the model knows that no default walk meets: {never}"
    assert st.refusals <= 0.35 * st.steps, (st.refusals, st.steps)


def test_walks_draw_every_variant_the_issue_names():
    seen = set()
    for _, _, ops in _default_walks():
        for op in ops:
            seen.add(op[:2] if op[0] in ("set_data", "set_diag", "append", "set_batch") else op[:1])
            if op[0] in ("lml", "lml_grad", "factor") and op[1] == H.BAD:
                seen.add((op[0], "bad"))
            if op[0] in ("lml_batch", "lml_grad_batch", "factor_batch", "predict_batch"):
                seen.add((op[0], "k<" if op[1] < H.BATCH_COUNT else "k=" if op[1] == H.BATCH_COUNT else "k>"))
            if op[0] == "set_option":
                seen.add(("option", op[1]))
    want = {("set_data", "same"), ("set_data", "new"), ("set_diag", "vec"), ("set_diag", "none"), ("append", "ok"),
            ("append", "over"), ("append", "dup"), ("set_batch", "plain"), ("set_batch", "zw"), ("set_batch", "alias"),
            ("factor", "bad"), ("lml", "bad"), ("lml_grad", "bad")}
    want |= {(b, k) for b in ("lml_batch", "lml_grad_batch", "factor_batch", "predict_batch") for k in ("k<", "k=", "k>")}
    want |= {("option", o) for o in H.SCHED_OPTIONS}
    assert not want - seen, want - seen


def test_the_failing_theta_fails_far_from_rounding():
    """The pivot the oracle reports for the negative-jitter theta is negative by a margin no rounding reaches."""
    import scipy.linalg as sla

    from oracle import gp_oracle as orc

    for size in H.SIZES:
        p = H.Problem(size)
        X, _ = p.data(0)
        K = orc.noisy_cov(X[: p.n0], p.kerns, p.ops, p.theta(H.BAD), "conditional")
        info = H.first_bad_pivot(K)
        assert 1 < info <= 64, (size, info)
        j = info - 1
        L = sla.cholesky(K[:j, :j], lower=True)
        r = sla.solve_triangular(L, K[:j, j], lower=True)
        assert K[j, j] - r @ r < -1e-3, (size, info, K[j, j] - r @ r)


# --------------------------------------------------------------------------------------- b. the harness against the stand-in
@pytest.mark.parametrize("size", list(H.SIZES))
def test_stand_in_passes_every_default_walk(size):
    p, o = _setup(size)
    tot = H.Stats()
    for seed in H.DEFAULT_SEEDS:
        tot.add(H.run_walk(H.OracleHandle(p, o), p, o, H.walk(seed, H.SIZES[size]["steps"], size), seed))
    print(f"size {size}: {tot.line()}")
    assert tot.bit_compares > 0 and tot.value_compares > 0


@pytest.mark.parametrize("size", [s for s in H.SIZES if s != max(H.SIZES)])
def test_facade_stand_in_passes_every_default_walk(size):
    p, o = _setup(size)
    for seed in H.DEFAULT_SEEDS:
        ops = H.facade_walk(seed, H.SIZES[size]["steps"], size)
        assert len(ops) == H.SIZES[size]["steps"]
        H.run_facade_walk(H.OracleFacade(p, o), p, o, ops, seed)


def test_facade_walks_use_every_public_method():
    seen = {}
    for size in H.SIZES:
        for seed in H.DEFAULT_SEEDS:
            for op in H.facade_walk(seed, H.SIZES[size]["steps"], size):
                seen[op[0]] = seen.get(op[0], 0) + 1
    assert set(seen) == set(H.FACADE_OPS), set(H.FACADE_OPS) - set(seen)


# ------------------------------------------------------------------------------------------------- d. wrong stand-ins
class SetDiagKeepsFactor(H.OracleHandle):
    def set_diag(self, how):
        keep = (self.factored, self.have_u)
        r = super().set_diag(how)
        self.factored, self.have_u = keep
        return r


class AppendKeepsOldAlpha(H.OracleHandle):
    def _append_u(self, key):
        pass


class ReserveDropsAlpha(H.OracleHandle):
    def reserve(self, cap):
        grows = cap > self.cap and cap >= self.n
        r = super().reserve(cap)
        if grows:
            self.alpha_key = None
        return r


class BatchKeepsSingleFactor(H.OracleHandle):
    def _batch(self, k, shift, zw):
        keep = self.factored
        ks = super()._batch(k, shift, zw)
        self.factored = keep
        return ks


class LmlGradKeepsU(H.OracleHandle):
    """U survives mi_gp_lml_grad, so the predictors that read U go on answering from it."""

    def lml_grad(self, ti):
        keep = self.have_u
        r = super().lml_grad(ti)
        self.have_u = keep
        return r

    def _pred_u(self, names):
        if self.have_u and not self.factored:
            return H.Res(0, {k: self.o.cond(self.f_key)[k] for k in names})
        return None

    def predict_u(self):
        return self._pred_u(("mean", "var")) or super().predict_u()

    def predict_grad(self):
        return self._pred_u(("mean", "var", "dmean", "dvar")) or super().predict_grad()


class PredictCovEndsFactor(H.OracleHandle):
    def predict_cov(self):
        r = super().predict_cov()
        self.factored = False
        return r


class SampleCovEndsBatch(H.OracleHandle):
    def sample_cov(self, seed, offset):
        self.b_cond = None
        return super().sample_cov(seed, offset)


class AliasedFactorBatchKeepsFactored(H.OracleHandle):
    def factor_batch(self, k, shift):
        keep = self.factored and bool(self.batch) and self.batch["alias"]
        r = super().factor_batch(k, shift)
        if r.rc == 0 and keep:
            self.factored = True
        return r


class AliasedSingleKeepsBatchFactors(H.OracleHandle):
    def _evaluate(self, ti, form):
        keep = self.b_cond
        r = super()._evaluate(ti, form)
        self.b_cond = keep
        return r


class PartsSurviveAFailure(H.OracleHandle):
    def _evaluate(self, ti, form):
        keep = self.have_parts
        r = super()._evaluate(ti, form)
        if r[0] is None and self.have_data:
            self.have_parts = keep
        return r


WRONG = [SetDiagKeepsFactor, AppendKeepsOldAlpha, ReserveDropsAlpha, BatchKeepsSingleFactor, LmlGradKeepsU, PredictCovEndsFactor,
         SampleCovEndsBatch, AliasedFactorBatchKeepsFactored, AliasedSingleKeepsBatchFactors, PartsSurviveAFailure]


@pytest.mark.parametrize("cls", WRONG, ids=[c.__name__ for c in WRONG])
def test_a_wrong_stand_in_is_caught(cls):
    """One documented rule broken: some default walk of the three small sizes must fail on it."""
    caught = []
    for size in [s for s in H.SIZES if s != max(H.SIZES)]:
        p, o = _setup(size)
        for seed in H.DEFAULT_SEEDS:
            try:
                H.run_walk(cls(p, o), p, o, H.walk(seed, H.SIZES[size]["steps"], size), seed)
            except H.WalkFailure as e:
                caught.append((size, seed, str(e).splitlines()[-1][:160]))
    print(cls.__name__, len(caught), caught[:2])
    assert caught, f"{cls.__name__}: every default walk passed"


class ShadowMissesSetDiag(H.OracleFacade):
    def set_diag(self, how):
        keep = self.ok_theta
        super().set_diag(how)
        self.ok_theta = keep


class ShadowAlwaysRefactors(H.OracleFacade):
    def _ensure(self, ti):
        self.factor(ti)


@pytest.mark.parametrize("cls", [ShadowMissesSetDiag, ShadowAlwaysRefactors], ids=["misses_set_diag", "always_refactors"])
def test_a_wrong_facade_shadow_is_caught(cls):
    caught = 0
    for size in [s for s in H.SIZES if s != max(H.SIZES)]:
        p, o = _setup(size)
        for seed in H.DEFAULT_SEEDS:
            try:
                H.run_facade_walk(cls(p, o), p, o, H.facade_walk(seed, H.SIZES[size]["steps"], size), seed)
            except (H.WalkFailure, KeyError):
                caught += 1
    assert caught
