"""The host side of the mean sweep (option 53 of mi_gp_set_option) and of andvaranaut_amd/sensitivity.py, on the CPU: the
references and bounds of tests/mean_sweep_ref.py are validated before the device meets them (a plain float64 evaluation stays
within a quarter of the bound), the case list keeps enough asserted cases, the sensitivity estimators satisfy their exact
identities and a statistical check against the Ishigami function's closed-form indices, and the option is documented where the
header tests of the earlier options leave room for it."""
import ctypes
import os
import re

import numpy as np
import pytest

import grad_refs as gr
import mean_sweep_ref as ms
import sched_check as C
import sched_trace_harness as H
from andvaranaut_amd import sensitivity as sens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [gr.case_id(c) for c in ms.CASES]


def test_case_list_is_the_issues():
    assert ms.CASES[: len(gr.PREDICT_CASES)] == gr.PREDICT_CASES
    assert ms.CASES[len(gr.PREDICT_CASES):] == [("RBF", 130, 128), ("Matern52+RBF", 65, 33), ("RBF", 64, 32), ("Matern52", 2500, 6)]
    assert ms.M_VALUES == (1, 5, 63, 64, 65, 257, 1000)
    # every call's last point, both sides of every workgroup boundary and every point of the calls up to 65 have a reference
    assert set(range(65)) <= set(ms.REF_POINTS) and {m - 1 for m in ms.M_VALUES} <= set(ms.REF_POINTS)
    assert {255, 256, 511, 512} <= set(ms.REF_POINTS) and ms.REF_POINTS.max() == 999


@pytest.mark.parametrize("kernel,n,d", ms.CASES, ids=IDS)
def test_float64_evaluation_stays_within_a_quarter_of_the_bound(kernel, n, d):
    """mu and d mu summed in plain float64, j ascending and j descending, from the reference's own alpha: error / bound <= 1/4
    at every reference point, whether or not the case is asserted on the device.  The queries are the issue's: the first five
    are predict_queries', the training point among them."""
    case = ms.case_data(kernel, n, d)
    X, Xn = case["X"], case["Xn"]
    assert Xn.shape == (1000, d) and np.array_equal(Xn[0], X[min(3, n - 1)])
    assert np.array_equal(Xn[:5], gr.predict_queries(X, case["theta"], d, seed=n + d))
    b_mu, b_dmu = ms.bounds(case)
    for reverse in (False, True):
        mu, dmu = ms.mean_float64(X, kernel, case["theta"], case["Xr"], case["alpha"], reverse=reverse)
        r_mu, r_dmu = gr.max_ratio(mu, case["mu"], b_mu), gr.max_ratio(dmu, case["dmu"], b_dmu)
        print(f"{kernel} n={n} d={d} cond={case['cond']:.0f} {'descending' if reverse else 'ascending'}: mu error / bound {r_mu:.4f}, "
              f"d mu error / bound {r_dmu:.4f} ({'asserted' if case['ok'] else 'printed'} on the device: alpha's diagonal residue is "
              f"{case['alpha_ratio']:.4f} of its allowance)")
        assert r_mu <= 0.25 and r_dmu <= 0.25, (r_mu, r_dmu)
    gone = ms.LD(ms.TINY) * ms.LD(2.0) ** -64
    assert (mu[case["mag_mu"] < gone] == 0.0).all()


def test_three_quarters_of_the_cases_and_every_family_are_asserted():
    ok = [c for c in ms.CASES if ms.case_data(*c)["ok"]]
    print(f"{len(ok)} of {len(ms.CASES)} cases asserted; printed only: {[gr.case_id(c) for c in ms.CASES if c not in ok]}")
    assert 4 * len(ok) >= 3 * len(ms.CASES)
    seen = set().union(*[ms.families(c[0]) for c in ok])
    assert seen == set(ms.FAMILIES), seen
    # the window forms of the kernel (d <= 4, <= 16, <= 32, wide) and every component-count slot are among the asserted cases
    forms = {0 if d <= 4 else 1 if d <= 16 else 2 if d <= 32 else 3 for _, _, d in ok}
    assert forms == {0, 1, 2, 3}
    assert {gr.nk_slot(len(gr.split(k)[0])) for k, _, _ in ok} == {0, 1, 2, 3, 4}


# ------------------------------------------------------------------------------------------------ sensitivity.py
def test_rank_one_gradient_field_has_one_eigenvalue_and_its_vector():
    rng = np.random.default_rng(0)
    a = np.array([3.0, -4.0, 0.0, 12.0])  # |a| = 13
    s = rng.normal(size=200)
    lam, V, Cm, dgsm = sens.active_subspace_from_gradients(s[:, None] * a[None, :])
    e2 = np.mean(s * s)
    assert abs(lam[0] - 169.0 * e2) <= 1e-12 * 169.0 * e2 and np.abs(lam[1:]).max() <= 1e-12 * lam[0]
    assert np.abs(V[:, 0] - a / 13.0).max() <= 1e-12  # (sign: the largest component, 12 / 13, is positive)
    assert np.allclose(dgsm, a * a * e2, rtol=1e-12, atol=0) and np.array_equal(dgsm, np.diag(Cm))
    assert (np.diff(lam) <= 0).all() and np.allclose(V.T @ V, np.eye(4), atol=1e-12)
    # weights: doubling a row's weight equals repeating the row
    G = rng.normal(size=(5, 3))
    w = np.array([1.0, 2.0, 1.0, 1.0, 1.0])
    l1, V1, C1, _ = sens.active_subspace_from_gradients(G, w)
    l2, V2, C2, _ = sens.active_subspace_from_gradients(np.vstack([G, G[1:2]]))
    assert np.allclose(C1, C2, rtol=1e-13, atol=1e-15) and np.allclose(l1, l2, rtol=1e-12) and np.allclose(V1, V2, atol=1e-10)
    assert (V1[np.argmax(np.abs(V1), axis=0), np.arange(3)] > 0).all()


def test_saltelli_design_shape_and_columns():
    rng = np.random.default_rng(1)
    M, d = 7, 3
    A, B = rng.random((M, d)), rng.random((M, d))
    D = sens.saltelli_design(A, B)
    assert D.shape == ((d + 2) * M, d)
    assert np.array_equal(D[:M], A) and np.array_equal(D[M: 2 * M], B)
    for m in range(d):
        blk = D[(2 + m) * M: (3 + m) * M]
        assert np.array_equal(blk[:, m], B[:, m])
        assert np.array_equal(np.delete(blk, m, axis=1), np.delete(A, m, axis=1))
    fA, fB, fAB = sens.split_saltelli(np.arange((d + 2) * M, dtype=float), d)
    assert fA.shape == (M,) and fB[0] == M and fAB.shape == (d, M) and fAB[1, 0] == 3 * M
    # an additive function of independent inputs: the design's own sample gives first = total for each input up to sampling
    # error, and a function of one input alone gives exact zeros for the others
    f = lambda x: 3.0 * x[:, 1]  # noqa: E731
    first, total, mean, var = sens.sobol_from_evaluations(*sens.split_saltelli(f(D), d))
    assert first[0] == 0.0 and first[2] == 0.0 and total[0] == 0.0 and total[2] == 0.0 and total[1] > 0.0


def _ishigami(x, a=7.0, b=0.1):
    return np.sin(x[:, 0]) + a * np.sin(x[:, 1]) ** 2 + b * x[:, 2] ** 4 * np.sin(x[:, 0])


def test_sobol_estimators_against_ishigami_closed_form():
    """Ishigami (a = 7, b = 0.1) on [-pi, pi]^3: V = a^2/8 + b pi^4/5 + b^2 pi^8/18 + 1/2, V1 = (1 + b pi^4/5)^2 / 2, V2 = a^2/8,
    V3 = 0, VT1 = V1 + 8 b^2 pi^8 / 225, VT2 = V2, VT3 = 8 b^2 pi^8 / 225.  16 replicate seeds of M = 4096: the mean of the
    replicates lies within 5 of ITS standard errors (the replicates' own standard deviation / sqrt(16)) of the truth, index by
    index -- a measurement against replicates, not a constant."""
    a, b, pi = 7.0, 0.1, np.pi
    V = a * a / 8 + b * pi ** 4 / 5 + b * b * pi ** 8 / 18 + 0.5
    V1, V2, VT3 = 0.5 * (1 + b * pi ** 4 / 5) ** 2, a * a / 8, 8 * b * b * pi ** 8 / 225
    truth_first = np.array([V1, V2, 0.0]) / V
    truth_total = np.array([V1 + VT3, V2, VT3]) / V
    firsts, totals = [], []
    for seed in range(16):
        sa, sb = np.random.SeedSequence(seed).spawn(2)
        A = np.random.default_rng(sa).uniform(-pi, pi, (4096, 3))
        B = np.random.default_rng(sb).uniform(-pi, pi, (4096, 3))
        first, total, _, _ = sens.sobol_from_evaluations(*sens.split_saltelli(_ishigami(sens.saltelli_design(A, B)), 3))
        firsts.append(first)
        totals.append(total)
    for name, est, truth in (("first", np.array(firsts), truth_first), ("total", np.array(totals), truth_total)):
        se = est.std(axis=0, ddof=1) / np.sqrt(est.shape[0])
        z = (est.mean(axis=0) - truth) / se
        print(f"Ishigami {name}: mean {est.mean(axis=0)}, truth {truth}, standard error {se}, z {z}")
        assert (se > 0).all() and (np.abs(z) <= 5.0).all(), (name, z)


# ----------------------------------------------------------------------------------------------- option 53, host level
def test_option_53_on_a_null_handle_and_in_the_host_only_program(tmp_path):
    from andvaranaut_amd import _lib

    assert len(_lib.EXPORTS) == 57
    lib = _lib.load()
    for v in (0, 1, 2, -1):
        assert lib.mi_gp_set_option(None, 53, v) == -1
    out = ctypes.c_int(7)
    assert lib.mi_gp_get_option(None, 53, ctypes.byref(out)) == -1 and out.value == 7
    assert lib.mi_gp_predict_grad(None, None, 1, None, 0, None, None, 0, None, None) == -1
    # the host-only schedule-trace program links api_gp.hip without api_sweep.hip: 1 is refused ("not part of this build"), 2
    # is out of range, 0 is taken
    prog = H.build_trace_program()
    for value, refused in ((1, ["53=1"]), (2, ["53=2"]), (0, [])):
        (cfg, _, end), = C.split_evaluations(H.run_traces(prog, [H.config_line(3, "lml_grad", options={53: value})], tmp_path))
        assert cfg["refused"] == refused and end["ret"] == 0, (value, cfg["refused"])


def test_option_53_is_documented_behind_mi_gp_get_option():
    text = open(os.path.join(ROOT, "include", "mi_gp.h")).read()
    # the options comment still ends with option 52's block, and option 51's block at the scheduling paragraph
    m = re.search(r"\n \* Option 52 \(not a tuning knob\) the OUTPUT COVARIANCE(.*?)\*/\nMI_GP_API int mi_gp_set_option", text, re.S)
    assert m and "Option 53" not in m.group(1) and "*/" not in m.group(1)
    assert "\n * 8, 14, 16," in text and "Option 53" not in text[: text.index("MI_GP_API int mi_gp_set_option")]
    m = re.search(r"MI_GP_API int mi_gp_get_option\(mi_gp_handle\* h, int what, int\* value\);\n/\* Option 53 \(not a tuning knob\) the MEAN "
                  r"SWEEP(.*?)\*/\n", text, re.S)
    assert m, "the option 53 comment of include/mi_gp.h, behind the declaration of mi_gp_get_option"
    block = m.group(1)
    for word in ("mi_gp_predict_grad", "bit for bit", "m >= 1", "mean_dev", "dmean_dev", "NULL", "work_dev", "pinned", "option 50",
                 "option 51", "d <= 128", "make_u_resident", "direct form", "index order", "position", "Out of scope",
                 "not part of this build"):
        assert word in block, word
    for doc, word in (("README.md", "option 53"), ("DESIGN.md", "option 53"), ("INTEGRATION.md", "mean_sweep")):
        assert word in open(os.path.join(ROOT, doc)).read(), (doc, word)
