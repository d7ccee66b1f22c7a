"""The between-output covariance integrated out (option 52 of mi_gp_set_option) on the host: the tail's algebra in NumPy against the
forward-mode definition, its q = 1 form against quadrature over the scale, the option's block in the header, the facades' refusals
(raised before any device call: there is no device here), the state of GPMCMC, and the build without csrc/api_multi.hip -- the
schedule-trace program -- which refuses 52 = 1, accepts 52 = 0 and enqueues the same records under it as without the option."""
import os
import pickle
import re

import numpy as np
import pytest
import scipy.stats as st

import loo_ref
import multi_output_ref as mo
import output_cov_ref as ref
import sched_check as C
import sched_trace_harness as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _target(x):  # (module level: the object that holds it is pickled below)
    return np.array([x[0] - x[1], x[0] * x[1], np.sin(x[0])])


@pytest.mark.parametrize("i,q", ref.CASES)
def test_the_tails_algebra_is_the_forward_definition(i, q):
    kernel, n, d, with_diag, gv = loo_ref.CASES[i]
    X, Y, theta, diag, cond_k = mo.problem(kernel, n, d, q, with_diag, gv, 70 + i)
    want_v, want_g, cond_s = ref.forward(X, Y, kernel, theta, diag)
    cond = max(cond_k, cond_s)
    v, g = ref.tail(X, Y, kernel, theta, diag)
    rv, rg = loo_ref.value_ratio(v, want_v, cond), loo_ref.grad_ratio(g, want_g, cond)
    print(loo_ref.CASES[i], "q = %d" % q, "cond(K) %.3g cond(S) %.3g" % (cond_k, cond_s), "error / bound: value %.3g gradient %.3g" % (rv, rg))
    assert rv <= 1.0 and rg <= 1.0
    assert abs(g[-1] - g[-2]) <= 1e-12 * abs(g[-1])  # d/d jitter = d/d gv
    assert n >= q + 2


def test_one_output_is_the_scale_integrated_out_by_quadrature():
    """q = 1: L_S = log int N(y; 0, s K_y) / s ds, on 12 points"""
    X, Y, theta, _, _ = mo.problem("RBF", 12, 2, 1, False, 1e-2, 5)
    v, _ = ref.tail(X, Y, "RBF", theta)
    want = ref.quadrature_q1(X, Y[:, 0], "RBF", theta)
    print("q = 1 on 12 points: closed form %.12f quadrature %.12f" % (v, want))
    assert abs(v - want) <= 1e-10 * abs(want)


def test_the_value_is_invariant_to_the_scale_of_the_covariance_and_to_mixing():
    """L_S(c K_y) = L_S(K_y), so kv g_kv + gv g_gv + jitter g_jitter = 0 for one component without a per-point diagonal (case 4);
    L_S(Y M) = L_S(Y) - n log|det M| and the gradient is that of Y"""
    kernel, n, d, with_diag, gv = loo_ref.CASES[4]
    X, Y, theta, diag, cond_k = mo.problem(kernel, n, d, 3, with_diag, gv, 74)
    assert diag is None
    v, g, cond_s = ref.forward(X, Y, kernel, theta)
    terms = np.array([theta[d] * g[d], theta[-2] * g[-2], theta[-1] * g[-1]])
    bound = max(1e-7, 500.0 * max(cond_k, cond_s) * loo_ref.EPS) * np.abs(terms).max()
    print("scale invariance: sum %.3g of terms up to %.3g, bound %.3g" % (terms.sum(), np.abs(terms).max(), bound))
    assert abs(terms.sum()) <= bound
    M = np.random.default_rng(3).normal(size=(3, 3)) + 2.0 * np.eye(3)
    vm, gm, cond_m = ref.forward(X, Y @ M, kernel, theta)
    cond = max(cond_k, cond_s, cond_m)
    assert loo_ref.value_ratio(vm, v - n * np.linalg.slogdet(M)[1], cond) <= 1.0 and loo_ref.grad_ratio(gm, g, cond) <= 1.0


def test_option_52_is_documented_behind_the_options_closing_paragraph():
    from andvaranaut_amd import MiGP, _lib

    assert len(_lib.EXPORTS) == 57
    assert MiGP.TRENDS == {"none": 0, "constant": 1, "linear": 2} and MiGP.OBJECTIVES == {"lml": 0, "loo": 1}
    assert MiGP.OUTPUT_COVS == {"shared": 0, "integrated": 1}
    text = open(os.path.join(ROOT, "include", "mi_gp.h")).read()
    m = re.search(r"\n \* Unknown ids return -1\..*?\n \* Option 52 \(not a tuning knob\) the OUTPUT COVARIANCE(.*?)\*/\nMI_GP_API int mi_gp_set_option",
                  text, re.S)
    assert m, "the option 52 block of include/mi_gp.h, behind the closing paragraph of the options comment"
    block = m.group(1)
    assert "\n *   5" not in block and "\n *   4" not in block  # (no other option's block inside it)
    for word in ("Sigma", "Jeffreys", "Conti", "S = Y^T V", "C_S", "L_S", "Gamma_q", "lgamma", "n V S^-1 V^T - q K_y^-1", "sqrt(n) V C_S^-T",
                 "q W - Q Q^T", "n >= q + 2", "n + j", "s_o = |b_o|^2 / (n - q - 1)", "var_dev[o * m + i]", "n - q + 1", "mi_gp_reserve",
                 "c K_y", "inert", "option 51", "Out of scope", "off-diagonal", "reading Sigma", "q = 1", "batched", "sharded",
                 "mi_gp_set_data", "bit for bit"):
        assert word in block, word
    # option 51's block still ends at the scheduling line
    assert re.search(r"\n \*   51 \(not a tuning knob\) the OUTPUTS(.*?)\n \* 8, 14, 16,", text, re.S)
    for doc, word in (("README.md", "option 52"), ("DESIGN.md", "option 52"), ("INTEGRATION.md", "set_output_cov"),
                      (os.path.join("profiles", "NOTES_output_cov.md"), "option 52")):
        assert word in open(os.path.join(ROOT, doc)).read(), (doc, word)


def test_the_facades_refuse_before_any_device_call():
    from andvaranaut_amd import GPMCMC, MiGP, uniform

    priors = [st.uniform(loc=0, scale=2), st.uniform(loc=1, scale=0.5)]
    g = GPMCMC(kernel="RBF", noise=True, xconrevs=[uniform(priors[0]), uniform(priors[1])], yconrevs=[None] * 3, nx=2, ny=3,
               priors=priors, target=_target, parallel=False, nproc=1, verbose=False)
    g.sample(nsamps=4, seed=1)
    assert g.outputs == "first" and g.output_cov == "shared"
    with pytest.raises(ValueError, match="output_cov must be one of"):
        g.fit(outputs="all", output_cov="free")
    with pytest.raises(ValueError, match="output_cov='integrated' needs outputs='all'"):
        g.fit(output_cov="integrated")  # (the first output alone)
    with pytest.raises(ValueError, match="needs at least ny \\+ 2 = 5 points, got 4"):
        g.fit(outputs="all", output_cov="integrated")  # (4 points, 3 outputs)
    # every refusal of outputs="all" stays, whatever the covariance and however few the points: with 4 points (the refusal of the
    # combination comes before the count of the points) and with 6, each on the text of that refusal
    no_form = "outputs='all' needs method='map', objective='lml', trend=None and neither iwgp nor cwgp"
    for nsamps in (0, 2):
        if nsamps:
            g.sample(nsamps=nsamps, seed=2)
            assert len(g.x) == 6
        for cov in ("shared", "integrated"):
            for kw in (dict(method="mcmc_mean"), dict(method="mcmc_map"), dict(method="none"), dict(objective="loo"),
                       dict(objective="kfold", nfolds=3), dict(trend="constant"), dict(iwgp=True), dict(cwgp=True)):
                with pytest.raises(ValueError) as e:
                    g.fit(outputs="all", output_cov=cov, **kw)
                assert str(e.value) == no_form, (nsamps, cov, kw, str(e.value))
            with pytest.raises(ValueError, match="outputs must be 'first' or 'all'"):
                g.fit(outputs="every", output_cov=cov)
    g1 = GPMCMC(kernel="RBF", noise=True, xconrevs=[uniform(priors[0]), uniform(priors[1])], yconrevs=[None], nx=2, ny=1,
                priors=priors, target=lambda x: np.array([x[0]]), parallel=False, nproc=1, verbose=False)
    with pytest.raises(ValueError, match="outputs='all' needs ny >= 2"):
        g1.fit(outputs="all", output_cov="integrated")
    assert g.outputs == "first" and g.output_cov == "shared" and g.hypers is None
    # the choice survives pickling and change_model resets it
    g.outputs, g.output_cov = "all", "integrated"
    back = pickle.loads(pickle.dumps(g))
    assert back.outputs == "all" and back.output_cov == "integrated"
    x = np.ones((3, 2))
    for call in (lambda: g.predict(x, EI=True), lambda: g.BO(), lambda: g.inverse_opt(np.ones(1)), lambda: g.predict_joint(x),
                 lambda: g.sample_posterior(x), lambda: g.log_predictive(x, np.ones(3)), lambda: g.predict_posterior(x, None),
                 lambda: g.cv_stats(), lambda: g.test_stats()):
        with pytest.raises(ValueError, match="has no form under outputs='all'"):
            call()
    g.change_model(kernel="Matern52")
    assert g.outputs == "first" and g.output_cov == "shared"
    # MiGP: a name that is none, and too few points, before the handle is looked at
    gp = MiGP.__new__(MiGP)
    assert gp._outcov == 0
    with pytest.raises(ValueError, match="output covariance"):
        gp.set_output_cov("free")
    gp.set_output_cov("shared")  # (the current value: no call)
    gp._outcov, gp.nout, gp.n = 1, 3, 4
    gp.Z_t = object()
    for call in (lambda: gp.lml_grad(None), lambda: gp.factor(None)):
        with pytest.raises(ValueError, match="q \\+ 2"):
            call()
    # set_option keeps the mirror that predict sizes its variance from in step with the handle's option (a stand-in library: no
    # device here), and ends the facade's factored state with it
    class _Lib:
        calls = []

        def mi_gp_set_option(self, h, what, value):
            self.calls.append((what, value))
            return 0

    gp.lib, gp.h, gp._outcov, gp._factored_ok = _Lib(), None, 0, True
    gp.set_option(52, 1)
    assert gp._outcov == 1 and not gp._factored_ok and gp.lib.calls == [(52, 1)]
    gp._factored_ok = True
    gp.set_output_cov("integrated")  # (the current value: no call)
    gp.set_option(7, 3)  # (another option: the mirror and the factored state stay)
    assert gp._outcov == 1 and gp._factored_ok and gp.lib.calls == [(52, 1), (7, 3)]
    gp.set_output_cov("shared")
    assert gp._outcov == 0 and not gp._factored_ok and gp.lib.calls[-1] == (52, 0)
    gp._outcov = 1
    gp.nout = 1  # (one output: inert, the call goes on to look at theta)
    with pytest.raises(Exception) as e:
        gp.factor(None)
    assert "q + 2" not in str(e.value)
    gp.h = None  # (nothing for __del__ to destroy)


def test_a_build_without_the_tail_refuses_the_covariance_and_option_0_changes_no_record(tmp_path):
    prog = H.build_trace_program()
    sets = [(c, e) for c in (3, 24) for e in ("lml_grad", "factor")]
    runs = {}
    for name, opts in (("none", None), ("0", {52: 0}), ("1", {52: 1}), ("2", {52: 2}), ("-1", {52: -1}), ("q", {51: 3}), ("0 q", {52: 0, 51: 3})):
        runs[name] = C.split_evaluations(H.run_traces(prog, [H.config_line(c, e, options=opts) for c, e in sets], tmp_path))
        assert len(runs[name]) == len(sets)
    for name, refused in (("0", []), ("1", ["52=1"]), ("2", ["52=2"]), ("-1", ["52=-1"]), ("q", ["51=3"]), ("0 q", ["51=3"])):
        for (cfg, recs, end), (_, recs0, _) in zip(runs[name], runs["none"]):
            assert cfg["refused"] == refused, (name, cfg["refused"])
            assert end["ret"] == 0 and recs == recs0 and len(recs) > 0
