"""Several outputs under one shared kernel (option 51 of mi_gp_set_option) on the host: the tail's algebra in NumPy against the
per-output oracle sum, the option's place in the header, the facades' refusals (raised before any device call: there is no
device here), the state of GPMCMC, and the build without csrc/api_multi.hip -- the schedule-trace program -- which refuses
51 = 2 and 51 = 128, accepts 51 = 1 and enqueues the same records under it as without the option."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest
import scipy.stats as st

import loo_ref
import multi_output_ref as ref
import sched_check as C
import sched_trace_harness as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REFUSED_ENTRIES = ("mi_gp_lml", "mi_gp_lml_batch", "mi_gp_lml_grad_batch", "mi_gp_factor_batch", "mi_gp_predict_batch", "mi_gp_predict_u",
                   "mi_gp_predict_grad", "mi_gp_predict_cov", "mi_gp_append", "mi_gp_logpdf", "mi_gp_kfold", "mi_gp_alpha", "mi_gp_grad_x")


def _target(x):  # (module level: the object that holds it is pickled below)
    return np.array([x[0] - x[1], x[0] * x[1], np.sin(x[0])])


# cases of loo_ref.CASES: one tile with a diagonal, a ragged size in 33 dimensions, a two-tile Matern, the composite kernel
@pytest.mark.parametrize("i,q", [(2, 2), (3, 17), (4, 3), (8, 5), (9, 128)])
def test_the_tails_algebra_is_the_per_output_oracle_sum(i, q):
    kernel, n, d, with_diag, gv = loo_ref.CASES[i]
    X, Y, theta, diag, cond = ref.problem(kernel, n, d, q, with_diag, gv, 70 + i)
    want_v, want_g = ref.oracle_sum(X, Y, kernel, theta, diag)
    v, g, quad = ref.tail(X, Y, kernel, theta, diag)
    rv, rg = loo_ref.value_ratio(v, want_v, cond), loo_ref.grad_ratio(g, want_g, cond)
    print(loo_ref.CASES[i], "q = %d" % q, "error / bound: value %.3g gradient %.3g" % (rv, rg))
    assert rv <= 1.0 and rg <= 1.0
    assert quad.shape == (q,) and (quad > 0).all()
    assert abs(g[-1] - g[-2]) <= 1e-12 * abs(g[-1])
    # one output: the tail is the ordinary evaluation
    v1, g1, _ = ref.tail(X, Y[:, :1], kernel, theta, diag)
    o1 = ref.oracle_sum(X, Y[:, :1], kernel, theta, diag)
    assert loo_ref.value_ratio(v1, o1[0], cond) <= 1.0 and loo_ref.grad_ratio(g1, o1[1], cond) <= 1.0


def test_option_51_is_documented_and_the_abi_keeps_its_entries():
    from andvaranaut_amd import MiGP, _lib

    assert len(_lib.EXPORTS) == 57
    assert MiGP.TRENDS == {"none": 0, "constant": 1, "linear": 2} and MiGP.OBJECTIVES == {"lml": 0, "loo": 1}
    text = open(os.path.join(ROOT, "include", "mi_gp.h")).read()
    m = re.search(r"\n \*   50 \(not a tuning knob\) the TREND.*?\n \*   51 \(not a tuning knob\) the OUTPUTS(.*?)\n \* 8, 14, 16,", text, re.S)
    assert m, "the option 51 block of include/mi_gp.h, between option 50's block and the scheduling line"
    block = m.group(1)
    assert "\n *   5" not in block and "\n *   4" not in block  # (no other option's block inside it)
    for word in ("o * lda", "o * m + i", "L_MO", "q K^-1 - V V^T", "V = K_y^-1 Y", "beta = q", "1..128", "mi_gp_reserve", "mi_gp_lml_parts",
                 "option 48 = 1", "50 != 0", "mi_gp_factor under option", "pinned", "Out of scope", "coregionalisation", "q > 128"):
        assert word in block, word
    for entry in REFUSED_ENTRIES:
        assert re.search(r"\b%s\b(?!_)" % entry, block), entry
    for doc, word in (("README.md", "option 51"), ("DESIGN.md", "option 51"), ("INTEGRATION.md", "set_outputs")):
        assert word in open(os.path.join(ROOT, doc)).read(), (doc, word)


def test_a_null_handle_and_values_out_of_range_return_minus_one(tmp_path):
    from andvaranaut_amd import _lib

    lib = _lib.load()
    for v in (1, 2, 128, 0, 129):
        assert lib.mi_gp_set_option(None, 51, v) == -1
    out = ctypes.c_int(7)
    assert lib.mi_gp_get_option(None, 51, ctypes.byref(out)) == -1 and out.value == 7
    # on a handle (the host-only program): 0, 129 and -1 are refused as out of range, 1 is taken
    prog = H.build_trace_program()
    (cfg, recs, end), = C.split_evaluations(H.run_traces(prog, [H.config_line(3, "lml_grad", options={51: 0})], tmp_path))
    assert cfg["refused"] == ["51=0"] and end["ret"] == 0
    for bad in (129, -1):
        (cfg, _, _), = C.split_evaluations(H.run_traces(prog, [H.config_line(3, "lml_grad", options={51: bad})], tmp_path))
        assert cfg["refused"] == ["51=%d" % bad]


def test_the_facades_refuse_before_any_device_call():
    from andvaranaut_amd import GPMCMC, MiGP, uniform

    priors = [st.uniform(loc=0, scale=2), st.uniform(loc=1, scale=0.5)]
    g = GPMCMC(kernel="RBF", noise=True, xconrevs=[uniform(priors[0]), uniform(priors[1])], yconrevs=[None] * 3, nx=2, ny=3,
               priors=priors, target=_target, parallel=False, nproc=1, verbose=False)
    g.sample(nsamps=12, seed=1)
    assert g.outputs == "first"
    for kw in (dict(method="mcmc_mean"), dict(method="mcmc_map"), dict(method="none"), dict(objective="loo"),
               dict(objective="kfold", nfolds=3), dict(trend="constant"), dict(iwgp=True), dict(cwgp=True)):
        with pytest.raises(ValueError, match="outputs"):
            g.fit(outputs="all", **kw)
    with pytest.raises(ValueError, match="outputs"):
        g.fit(outputs="every")
    g1 = GPMCMC(kernel="RBF", noise=True, xconrevs=[uniform(priors[0]), uniform(priors[1])], yconrevs=[None], nx=2, ny=1,
                priors=priors, target=lambda x: np.array([x[0]]), parallel=False, nproc=1, verbose=False)
    with pytest.raises(ValueError, match="outputs"):
        g1.fit(outputs="all")  # (ny = 1)
    assert g.outputs == "first" and g.hypers is None
    # under a fit of every output (the state alone: nothing here reaches a device)
    g.outputs = "all"
    x = np.ones((3, 2))
    for call in (lambda: g.predict(x, EI=True), lambda: g.BO(), lambda: g.inverse_opt(np.ones(1)), lambda: g.predict_joint(x),
                 lambda: g.sample_posterior(x), lambda: g.log_predictive(x, np.ones(3)), lambda: g.predict_posterior(x, None),
                 lambda: g.cv_stats(), lambda: g.test_stats()):
        with pytest.raises(ValueError, match="outputs"):
            call()
    # the choice survives pickling (save_object pickles the object's state) and change_model resets it
    assert pickle.loads(pickle.dumps(g)).outputs == "all"
    g.change_model(kernel="Matern52")
    assert g.outputs == "first"
    # MiGP: every refused evaluation raises before it looks at its arguments or its handle
    gp = MiGP.__new__(MiGP)
    assert gp.nout == 1
    gp.nout = 3
    gp.Z_t = object()
    for call in (lambda: gp.lml(None), lambda: gp.lml_batch(None), lambda: gp.lml_grad_batch(None), lambda: gp.factor_batch(None),
                 lambda: gp.predict_batch(None, None), lambda: gp.lml_grad_data(None), lambda: gp.append(None, None),
                 lambda: gp.logpdf(None, None, None), lambda: gp.kfold(None, None), lambda: gp.predict(None, None, via_inverse=True),
                 lambda: gp.predict_grad(None, None), lambda: gp.predict_cov(None, None), lambda: gp.sample_posterior(None, None, 1),
                 lambda: gp.update_data(y=np.zeros(3))):
        with pytest.raises(ValueError, match="outputs"):
            call()
    gp._trend = 1  # (a trend and several outputs together: lml_grad and factor have no form)
    for call in (lambda: gp.lml_grad(None), lambda: gp.factor(None)):
        with pytest.raises(ValueError, match="outputs"):
            call()
    gp.h = None  # (nothing for __del__ to destroy)


def test_a_build_without_the_tail_refuses_several_outputs_and_option_1_changes_no_record(tmp_path):
    prog = H.build_trace_program()
    sets = [(c, e) for c in (3, 24, 33) for e in ("lml_grad", "factor")]
    runs = {}
    for opt in (None, 1, 2, 128):
        lines = [H.config_line(c, e, options=None if opt is None else {51: opt}) for c, e in sets]
        runs[opt] = C.split_evaluations(H.run_traces(prog, lines, tmp_path))
        assert len(runs[opt]) == len(sets)
    for opt in (1, 2, 128):
        for (cfg, recs, end), (cfg0, recs0, end0) in zip(runs[opt], runs[None]):
            assert cfg["refused"] == ([] if opt == 1 else ["51=%d" % opt]), (opt, cfg["refused"])
            assert end["ret"] == 0 and recs == recs0 and len(recs) > 0
