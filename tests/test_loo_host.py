"""Host checks for the leave-one-out objective (option 48, MiGP.loo_grad, GPMCMC.fit(objective="loo")): the three references of
tests/loo_ref.py against each other on the GPU test's own cases, the facade's refusals, the option's place in the C-ABI and its
refusal in a build without the tail (the schedule-trace program)."""
import os
import re

import numpy as np
import pytest
import scipy.stats as st

import loo_ref as ref
from conftest import ROOT


@pytest.mark.parametrize("i", range(len(ref.CASES)))
def test_refit_forward_and_reverse_references_agree(i):
    """The definition (one refit per point), R & W eq. 5.13 and the device's reverse-mode algebra, in float64 NumPy, at the bounds
    of the GPU test: the references alone stay inside them."""
    X, y, kernel, theta, diag, cond = ref.case(i)
    v_refit, (v_f, g_f), (v_r, g_r) = ref.case_refs(i)
    rv = max(ref.value_ratio(v_f, v_refit, cond), ref.value_ratio(v_r, v_refit, cond))
    rg = ref.grad_ratio(g_r, g_f, cond)
    print(ref.CASES[i], "cond %.3g" % cond, "error / bound: value %.3g gradient (reverse vs forward) %.3g" % (rv, rg))
    assert rv <= 1.0 and rg <= 1.0, (rv, rg)
    assert len(g_f) == len(theta) and g_f[-1] == pytest.approx(g_f[-2], rel=1e-12)  # d/d jitter = d/d gv


@pytest.mark.parametrize("i", [3, 9])
def test_forward_gradient_agrees_with_central_differences(i):
    X, y, kernel, theta, diag, cond = ref.case(i)
    _, (_, g) = ref.case_refs(i)[:2]
    rng = np.random.default_rng(i)
    for _ in range(3):
        u = rng.standard_normal(len(theta)) * theta  # (a relative direction: every parameter is positive)
        u[-1] = 0.0  # (the jitter of 1e-6 has no room for a step)
        h = 1e-5
        vp = ref.loo_forward(X, y, kernel, theta + h * u, diag)[0]
        vm = ref.loo_forward(X, y, kernel, theta - h * u, diag)[0]
        fd = (vp - vm) / (2 * h)
        # truncation h^2 and rounding cond eps / h of a value of size ~n
        assert abs(fd - g @ u) <= 1e-5 * max(abs(g @ u), np.abs(g * u).max()), (fd, g @ u)


def _facade():
    from andvaranaut_amd import GPMCMC, normal, uniform

    priors = [st.uniform(loc=0, scale=2), st.uniform(loc=1, scale=0.5)]
    fun = lambda x: np.array([x[0] ** 2 - x[0] - x[1] ** 2 * x[0] + x[1]])  # noqa: E731
    g = GPMCMC(kernel="RBF", noise=True, xconrevs=[uniform(priors[0]), normal(priors[1])], yconrevs=[None], nx=2, ny=1,
               priors=priors, target=fun, parallel=False, nproc=1, verbose=False)
    g.sample(nsamps=12, seed=1)
    return g


def test_fit_refuses_the_loo_objective_outside_a_plain_map_fit_before_any_device_call():
    g = _facade()
    for kw in ({"method": "mcmc_mean"}, {"method": "mcmc_map"}, {"method": "none"}, {"cwgp": True}, {"iwgp": True}):
        with pytest.raises(ValueError, match="objective"):
            g.fit(objective="loo", **kw)
    with pytest.raises(ValueError, match="objective"):
        g.fit(objective="cv")
    assert g.gp is None and g.hypers is None  # nothing was created, nothing stored


def test_option_48_is_documented_and_no_entry_point_was_added():
    from andvaranaut_amd import _lib
    from andvaranaut_amd.backend import MiGP

    header = open(os.path.join(ROOT, "include", "mi_gp.h")).read()
    assert re.search(r"^ \*   48 .*OBJECTIVE of mi_gp_lml_grad", header, flags=re.M)
    assert "leave-one-out" in header and "eq. 5.13" in header
    assert len(_lib.EXPORTS) == 57
    assert MiGP.OBJECTIVES == {"lml": 0, "loo": 1}


def test_a_build_without_the_tail_refuses_the_option_and_enqueues_the_same_evaluation(tmp_path):
    """The schedule-trace program links api_gp.hip without api_loo.hip: 48 = 1 is refused (and 48 = 0, 48 = 2 as everywhere), and
    the evaluation behind the refusal is the ordinary one, launch for launch."""
    import sched_trace_harness as H

    prog = H.build_trace_program()
    lines = [H.config_line(ntc, "lml_grad", options=o) for ntc in (3, 24) for o in ({}, {48: 1}, {48: 0}, {48: 2})]
    import sched_check as C

    # (one process per configuration: the stand-ins number streams and events per process)
    evs = [ev for line in lines for ev in C.split_evaluations(H.run_traces(prog, [line], tmp_path))]
    assert len(evs) == len(lines)
    for k in range(0, len(evs), 4):
        (cfg0, recs0, end0), (cfg1, recs1, end1), (cfg2, recs2, end2), (cfg3, recs3, end3) = evs[k : k + 4]
        assert cfg0["refused"] == [] and cfg1["refused"] == ["48=1"] and cfg2["refused"] == [] and cfg3["refused"] == ["48=2"]
        assert end0["ret"] == end1["ret"] == end2["ret"] == end3["ret"] == 0
        assert recs1 == recs0 and recs2 == recs0 and recs3 == recs0 and len(recs0) > 10
