"""Host checks for the k-fold cross-validation objective (option 49, MiGP.cv_grad, GPMCMC.fit(objective="kfold")): the three
references of tests/cv_objective_ref.py against each other on the GPU test's own cases, the facade's refusals, the option's place
in the C-ABI and its refusal in a build without the tail (the schedule-trace program)."""
import os
import re

import numpy as np
import pytest
import scipy.stats as st

import cv_objective_ref as ref
import loo_ref
from conftest import ROOT


@pytest.mark.parametrize("i,b", ref.PAIRS)
def test_refit_forward_and_reverse_references_agree(i, b):
    """The definition (one refit per fold), the forward-mode gradient and the device's reverse-mode algebra, in float64 NumPy, at
    the bounds of the GPU test: the references alone stay inside them."""
    X, y, kernel, theta, diag, cond = loo_ref.case(i)
    v_refit, (v_f, g_f), (v_r, g_r) = ref.case_refs(i, b)
    rv = max(loo_ref.value_ratio(v_f, v_refit, cond), loo_ref.value_ratio(v_r, v_refit, cond))
    rg = loo_ref.grad_ratio(g_r, g_f, cond)
    print(loo_ref.CASES[i], "b = %d" % b, "cond %.3g" % cond, "error / bound: value %.3g gradient (reverse vs forward) %.3g" % (rv, rg))
    assert rv <= 1.0 and rg <= 1.0, (rv, rg)
    assert len(g_f) == len(theta) and g_f[-1] == pytest.approx(g_f[-2], rel=1e-12)  # d/d jitter = d/d gv


def test_one_fold_is_the_marginal_likelihood_and_single_points_are_leave_one_out():
    """The two ends of the family, in the references: b >= n is the LML (oracle), and the forward form with blocks of one point is
    loo_ref's."""
    from oracle import gp_oracle as orc

    X, y, kernel, theta, diag, cond = loo_ref.case(2)  # n = 128
    kerns, ops = ref.kfold_ref.split_kernel(kernel)
    K = orc.noisy_cov(X, kerns, ops, theta, "marginal", diag)
    sign, logdet = np.linalg.slogdet(K)
    lml = -0.5 * y @ np.linalg.solve(K, y) - 0.5 * logdet - 0.5 * len(y) * ref.LOG_2PI
    assert loo_ref.value_ratio(ref.case_refs(2, 128)[1][0], lml, cond) <= 1.0
    v1, g1 = ref.cv_forward(X, y, kernel, theta, 1, diag)
    v0, (vf, gf), _ = loo_ref.case_refs(2)
    assert loo_ref.value_ratio(v1, v0, cond) <= 1.0 and loo_ref.grad_ratio(g1, gf, cond) <= 1.0


@pytest.mark.parametrize("i,b", [(3, 37), (9, 100)])
def test_forward_gradient_agrees_with_central_differences(i, b):
    X, y, kernel, theta, diag, cond = loo_ref.case(i)
    _, (_, g) = ref.case_refs(i, b)[:2]
    rng = np.random.default_rng(i)
    for _ in range(3):
        u = rng.standard_normal(len(theta)) * theta  # (a relative direction: every parameter is positive)
        u[-1] = 0.0  # (the jitter of 1e-6 has no room for a step)
        h = 1e-5
        vp = ref.cv_forward(X, y, kernel, theta + h * u, b, diag)[0]
        vm = ref.cv_forward(X, y, kernel, theta - h * u, b, diag)[0]
        fd = (vp - vm) / (2 * h)
        # truncation h^2 and rounding cond eps / h of a value of size ~n
        assert abs(fd - g @ u) <= 1e-5 * max(abs(g @ u), np.abs(g * u).max()), (fd, g @ u)


def _facade(nsamps=12):
    from andvaranaut_amd import GPMCMC, normal, uniform

    priors = [st.uniform(loc=0, scale=2), st.uniform(loc=1, scale=0.5)]
    fun = lambda x: np.array([x[0] ** 2 - x[0] - x[1] ** 2 * x[0] + x[1]])  # noqa: E731
    g = GPMCMC(kernel="RBF", noise=True, xconrevs=[uniform(priors[0]), normal(priors[1])], yconrevs=[None], nx=2, ny=1,
               priors=priors, target=fun, parallel=False, nproc=1, verbose=False)
    g.sample(nsamps=nsamps, seed=1)
    return g


def test_fit_refuses_the_kfold_objective_before_any_device_call():
    g = _facade()
    for kw in ({"method": "mcmc_mean"}, {"method": "mcmc_map"}, {"method": "none"}, {"cwgp": True}, {"iwgp": True}):
        with pytest.raises(ValueError, match="objective"):
            g.fit(objective="kfold", **kw)
    for k in (1, 0, -3, 2.5, "loo"):
        with pytest.raises(ValueError, match="nfolds"):
            g.fit(objective="kfold", nfolds=k)
    with pytest.raises(ValueError, match="nfolds"):
        g.fit(objective="kfold", nfolds=13)  # more folds than points
    with pytest.raises(ValueError, match="objective"):
        g.fit(objective="cv")
    assert g.gp is None and g.hypers is None  # nothing was created, nothing stored


def test_fit_names_the_smallest_admissible_nfolds_when_a_fold_would_exceed_128_points():
    g = _facade(nsamps=300)  # (ceil(300 / 2) = 150 points per fold)
    with pytest.raises(ValueError, match=r"objective.*smallest admissible nfolds is 3"):
        g.fit(objective="kfold", nfolds=2)
    assert g.gp is None and g.hypers is None
    assert g._kfold_plan("map", False, False, 3, 0)[0] == 100


def test_the_fold_plan_is_a_seeded_partition_into_blocks():
    g = _facade()
    b, perm = g._kfold_plan("map", False, False, 5, 7)
    assert b == 3 and np.array_equal(np.sort(perm), np.arange(12))  # ceil(12 / 5) = 3: four folds of three points
    assert np.array_equal(perm, g._kfold_plan("map", False, False, 5, 7)[1])
    assert not np.array_equal(perm, g._kfold_plan("map", False, False, 5, 8)[1])


def test_option_49_is_documented_and_no_entry_point_was_added():
    from andvaranaut_amd import _lib
    from andvaranaut_amd.backend import MiGP

    header = open(os.path.join(ROOT, "include", "mi_gp.h")).read()
    assert re.search(r"^ \*   49 .*FOLD SIZE", header, flags=re.M)
    assert "leave-block-out" in header and "option 49" in header
    assert not re.search(r"Out of scope: k-fold gradients", header)
    assert len(_lib.EXPORTS) == 57
    assert MiGP.OBJECTIVES == {"lml": 0, "loo": 1}
    assert callable(MiGP.set_cv_block) and callable(MiGP.cv_grad)


def test_a_build_without_the_tail_refuses_a_block_and_enqueues_the_same_evaluation(tmp_path):
    """The schedule-trace program links api_gp.hip without api_loo.hip: 49 = 37 is refused, 49 = 1 (the default) is accepted, 0 and
    129 are refused as everywhere, and the evaluation is the ordinary one, launch for launch."""
    import sched_check as C
    import sched_trace_harness as H

    prog = H.build_trace_program()
    lines = [H.config_line(ntc, "lml_grad", options=o) for ntc in (3, 24) for o in ({}, {49: 37}, {49: 1}, {49: 0}, {49: 129})]
    # (one process per configuration: the stand-ins number streams and events per process)
    evs = [ev for line in lines for ev in C.split_evaluations(H.run_traces(prog, [line], tmp_path))]
    assert len(evs) == len(lines)
    for k in range(0, len(evs), 5):
        cfgs, recs, ends = zip(*evs[k : k + 5])
        assert [c["refused"] for c in cfgs] == [[], ["49=37"], [], ["49=0"], ["49=129"]]
        assert all(e["ret"] == 0 for e in ends)
        assert all(r == recs[0] for r in recs) and len(recs[0]) > 10
