"""The host side of the design call (options 56 / 57 of mi_gp_set_option, MiGP.design, GPMCMC.propose_samples /
adaptive_sample) on the CPU: the exact identities of the criterion, the fp64 error budget of the device's steps against the
long-double reference, the gap condition of the GPU cases, the facade's refusals and the seed of the facade's GPU test."""
import os

import numpy as np
import pytest
import scipy.stats as st

import design_ref as dr
from andvaranaut_amd import _lib
from andvaranaut_amd.gpmcmc import GPMCMC
from andvaranaut_amd.lhc import latin_sample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [dr.case_id(c) for c in dr.CASES]


def test_case_list_is_the_issues():
    assert [c[:5] for c in dr.CASES] == [(130, 129, 65, 3, 8), (257, 200, 130, 5, 16), (130, 129, 65, 17, 8), (130, 129, 0, 3, 8),
                                         (130, 1, 1, 3, 1), (130, 5, 65, 3, 8)]
    assert dr.CASES[1][5] == "RBF+Matern32" and dr.MIN_GAP == 1e-4
    th = dr.make_theta("Matern52", 3)
    assert np.allclose(th[:3], 0.4 * np.sqrt(3)) and th[3] == 1.3 and th[-2:].tolist() == [1e-3, 1e-6]


@pytest.mark.parametrize("case", [c for c in dr.CASES if c[2] > 0], ids=[dr.case_id(c) for c in dr.CASES if c[2] > 0])
def test_sum_of_gains_is_the_drop_of_the_mean_variance_after_a_refit(case):
    """sum gains = mean_r var_latent(r | X) - mean_r var_latent(r | X and the chosen points): a brute-force refit in long double"""
    c = dr.case_data(*case)
    ref = dr.reference(case)
    before = dr.mean_latent_variance(c["X"], c["R"], c["kernel"], c["theta"])
    after = dr.mean_latent_variance(np.vstack([c["X"], c["C"][ref["idx"]]]), c["R"], c["kernel"], c["theta"])
    err = abs(float(np.sum(ref["gains"]) - (before - after)))
    print(f"{dr.case_id(case)}: sum of gains {float(np.sum(ref['gains'])):.6e}, drop {float(before - after):.6e}, difference {err:.2e}")
    assert err <= 1e-12
    # and step by step: the k-th gain is the drop from k - 1 to k appended points
    prev = before
    for k, p in enumerate(ref["idx"][:3]):
        cur = dr.mean_latent_variance(np.vstack([c["X"], c["C"][ref["idx"][: k + 1]]]), c["R"], c["kernel"], c["theta"])
        assert abs(float(ref["gains"][k] - (prev - cur))) <= 1e-12
        prev = cur
    assert len(ref["idx"]) == min(case[4], case[1]) and len(set(ref["idx"])) == len(ref["idx"])


def test_the_variance_criterion_is_a_pivoted_cholesky():
    """Mr = 0: the chosen sequence is the pivot order of a diagonally pivoted Cholesky of cov(C, C) + noise I, the gains its pivots
    less the noise"""
    case = dr.CASES[3]
    c = dr.case_data(*case)
    ref = dr.reference(case)
    Scc, _ = dr.posterior_ld(c["X"], c["C"], c["R"], c["kernel"], c["theta"])
    nz = dr.LD(dr.noise_of(c["theta"], True))
    S = Scc + nz * np.eye(len(Scc), dtype=dr.LD)
    piv, dg = [], []
    for _ in range(case[4]):
        dd = np.diag(S).copy()
        dd[piv] = -np.inf
        p = int(np.argmax(dd))
        piv.append(p)
        dg.append(S[p, p])
        S = S - np.outer(S[:, p], S[:, p]) / S[p, p]
    assert piv == ref["idx"].tolist()
    assert np.abs((np.array(dg) - nz - ref["gains"]).astype(np.float64)).max() <= 1e-15


@pytest.mark.parametrize("case", dr.CASES, ids=IDS)
def test_float64_steps_stay_within_half_of_the_tolerance(case):
    """device_fp64 -- the device's steps in float64 NumPy -- against the long-double reference: the same sequence, every gain and
    round-0 gain within half of max(1e-10, 200 cond(K_y) eps) of the largest round-0 gain"""
    c = dr.case_data(*case)
    ref = dr.reference(case)
    idx, gains, gains0 = dr.device_fp64(c["X"], c["C"], c["R"], c["kernel"], c["theta"], c["b"])
    tol = dr.tolerance(c["X"], c["kernel"], c["theta"], ref["gains0"])
    r1 = float(np.abs(gains - ref["gains"].astype(np.float64)).max() / tol)
    r0 = float(np.abs(gains0 - ref["gains0"].astype(np.float64)).max() / tol)
    print(f"{dr.case_id(case)}: cond {dr.cond_ky(c['X'], c['kernel'], c['theta']):.3g}, tolerance {tol:.3e}, gains error / tolerance "
          f"{r1:.2e}, round-0 error / tolerance {r0:.2e}, min gap {ref['min_gap']:.3e}")
    assert idx.tolist() == ref["idx"].tolist()
    assert r1 <= 0.5 and r0 <= 0.5


@pytest.mark.parametrize("case", dr.CASES, ids=IDS)
def test_gpu_cases_meet_the_gap_condition(case):
    """a condition on the inputs: at every step the best score leads the second best by >= 1e-4 relative (inf: one candidate)"""
    assert dr.min_gap(case) >= dr.MIN_GAP
    assert dr.min_gap(case, noise=False) >= dr.MIN_GAP


def test_gap_condition_of_the_further_gpu_cases():
    """after an append across a tile (n = 250 -> 258), and gv = 0 with a candidate on a training point and a repeated candidate"""
    assert dr.min_gap(dr.APPEND_CASE) >= dr.MIN_GAP
    c = dr.coincident_case()
    ref = c["ref"]
    print(f"coincident case: min gap {ref['min_gap']:.3e}, chosen {ref['idx'].tolist()}, gain of the candidate on a training point "
          f"{float(ref['gains0'][5]):.3e} of {float(np.nanmax(ref['gains0'].astype(np.float64))):.3e}")
    assert ref["min_gap"] >= dr.MIN_GAP
    assert 5 not in ref["idx"] and dr.DUP[1] not in ref["idx"]
    assert ref["gains0"][dr.DUP[0]] == ref["gains0"][dr.DUP[1]]
    idx, gains, gains0 = dr.device_fp64(c["X"], c["C"], c["R"], c["kernel"], c["theta"], c["b"])
    tol = dr.tolerance(c["X"], c["kernel"], c["theta"], ref["gains0"])
    assert idx.tolist() == ref["idx"].tolist()
    assert np.abs(gains - ref["gains"].astype(np.float64)).max() <= 0.5 * tol


def test_exports_are_unchanged():
    assert len(_lib.EXPORTS) == 57


def test_options_are_documented_in_the_header():
    text = open(os.path.join(ROOT, "include", "mi_gp.h")).read()
    assert "Option 56" in text and "Option 57" in text and "DESIGN CALL" in text


# ------------------------------------------------------------------------------------------------ the facade's refusals
def _model(**kw):
    return GPMCMC(nx=2, ny=1, priors=[st.uniform(0, 1), st.uniform(0, 1)], target=lambda x: np.array([np.sin(3 * x[0]) + x[1] ** 2]),
                  verbose=False, **kw)


def test_adaptive_sampler_needs_a_fit():
    m = _model()
    for call in (lambda: m.propose_samples(4), lambda: m.adaptive_sample(4)):
        with pytest.raises(Exception, match="fit the GP before"):
            call()


@pytest.mark.parametrize("state,match", [(dict(inducing=np.zeros((3, 2))), "sparse fit"), (dict(trend="linear"), "trend"),
                                         (dict(outputs="all"), "outputs='all'")])
def test_adaptive_sampler_refuses_before_any_device_call(state, match):
    m = _model()
    m.hypers, m.m = {"l": np.ones(2)}, object()  # (a fitted object's marks: the refusals come first and touch neither)
    for k, v in state.items():
        setattr(m, k, v)
    assert m.gp is None
    for call in (lambda: m.propose_samples(4), lambda: m.adaptive_sample(4)):
        with pytest.raises(ValueError, match=match):
            call()
    assert m.gp is None


def test_bad_arguments_are_refused():
    m = _model()
    m.hypers, m.m = {"l": np.ones(2)}, object()
    with pytest.raises(Exception, match="integer > 0"):
        m.propose_samples(0)
    with pytest.raises(ValueError, match="criterion"):
        m.propose_samples(2, criterion="ei")
    with pytest.raises(ValueError, match="batch"):
        m.adaptive_sample(2, batch=0)
    assert m.gp is None


# ------------------------------------------------------------------------------------------------ the facade test's seed
def test_facade_seed_shows_the_gain_in_numpy():
    """The condition of the facade's GPU test: at its fixed theta, 16 points chosen by the reference's greedy selection (4 rounds
    of 4, candidates and references drawn as propose_samples draws them) leave a smaller mean posterior variance over the fresh
    500-point set than 16 further Latin-hypercube points."""
    cfg = dr.FACADE
    priors = [st.uniform(0, 1), st.uniform(0, 1)]
    x0, xl, xt = dr.facade_points(priors)
    theta = np.array([cfg["ls"], cfg["ls"], cfg["kv"], 1.0, cfg["gv"], cfg["jitter"]])
    X = x0.copy()
    for rnd in range(cfg["nadd"] // cfg["batch"]):
        C = latin_sample(priors, cfg["ncand"], cfg["seed"] + 2 * rnd)
        R = latin_sample(priors, cfg["nref"], cfg["seed"] + 2 * rnd + 1)
        Scc, Scr = dr.posterior_ld(X, C, R, "Matern52", theta)
        idx, _, _, gap = dr.greedy(Scc, Scr, cfg["batch"], dr.LD(dr.noise_of(theta, True)))
        assert gap >= dr.MIN_GAP
        X = np.vstack([X, C[idx]])
    adaptive = float(dr.mean_latent_variance(X, xt, "Matern52", theta))
    lhc = float(dr.mean_latent_variance(np.vstack([x0, xl]), xt, "Matern52", theta))
    print(f"mean latent variance over 500 fresh points: adaptive {adaptive:.5e}, Latin hypercube {lhc:.5e}")
    assert adaptive < 0.9 * lhc
