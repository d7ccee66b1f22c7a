"""The host side of tests/test_gpu_grad_instantiations.py: its case lists cover every entry of the three dispatch tables of
csrc/grad_predict.hip, and its longdouble / mpmath references agree with the oracle where the oracle is accurate."""
import itertools

import numpy as np
import pytest

import grad_refs as gr
from oracle import gp_oracle as orc


# ------------------------------------------------------------------------------------------ coverage of the tables
def test_table_shapes_are_those_the_cases_were_written_for():
    shapes = gr.table_shapes()
    assert shapes == {"GRAD_CONTRACT_KERNELS": (5, 2), "GRAD_X_KERNELS": (5, 3), "PREDICT_GRAD_KERNELS": (5,)}, shapes
    assert len(gr.NK_SLOTS) == 5 and len(gr.GX_WINDOWS) == 3


def test_table_shapes_reads_a_grown_table():
    text = open(gr.SOURCE).read().replace("GRAD_X_KERNELS[5][3] =", "GRAD_X_KERNELS[6][4] =")
    assert gr.table_shapes(text)["GRAD_X_KERNELS"] == (6, 4)


def _all_entries(shape):
    return set(itertools.product(*[range(s) for s in shape]))


def test_case_lists_cover_every_table_entry():
    shapes = gr.table_shapes()
    hit = {"GRAD_CONTRACT_KERNELS": {gr.contract_entry(k) for k, _ in gr.CONTRACT_CASES},
           "GRAD_X_KERNELS": {gr.grad_x_entry(k, d) for k, n, d in gr.GRAD_X_CASES if n == 130},
           "PREDICT_GRAD_KERNELS": {gr.predict_entry(k) for k, _, _ in gr.PREDICT_CASES}}
    for name, shape in shapes.items():
        missing = _all_entries(shape) - hit[name]
        assert not missing, (name, sorted(missing))


def test_case_lists_hold_every_component_count_and_every_ratquad_position():
    for cases in (gr.CONTRACT_CASES, gr.GRAD_X_CASES, gr.PREDICT_CASES):
        counts = {len(gr.split(c[0])[0]) for c in cases}
        assert counts >= set(range(1, 9)), counts
        first = middle = last = False
        sides = set()  # (side of the rational quadratic, operator)
        for c in cases:
            kerns, ops = gr.split(c[0])
            for i, k in enumerate(kerns):
                if k != "RatQuad" or len(kerns) == 1:
                    continue
                first |= i == 0
                last |= i == len(kerns) - 1
                middle |= 0 < i < len(kerns) - 1
                if i > 0:
                    sides.add(("left", ops[i - 1]))
                if i < len(kerns) - 1:
                    sides.add(("right", ops[i]))
        assert first and middle and last
        assert sides == {("left", "+"), ("left", "*"), ("right", "+"), ("right", "*")}, sides


def test_case_lists_hold_the_shapes_at_which_the_kernels_branch():
    assert {d for _, d in gr.CONTRACT_CASES} == {1, 32, 33, 65}
    assert {n for _, n, _ in gr.GRAD_X_CASES} == {1, 64, 65, 130}
    assert {d for _, _, d in gr.GRAD_X_CASES} == {3, 16, 17, 32, 33, 129}
    for slot in range(5):  # each slot once at n = 1 and once at n = 65
        ns = {n for k, n, d in gr.GRAD_X_CASES if gr.grad_x_entry(k, d)[0] == slot}
        assert {1, 65} <= ns, (slot, ns)
    assert {n for _, n, _ in gr.PREDICT_CASES} == {1, 255, 257, 600}
    assert {d for _, _, d in gr.PREDICT_CASES} == {1, 16, 17, 40}
    assert max(n for _, n, _ in gr.PREDICT_CASES) <= 600


def test_selection_rule_at_its_thresholds():
    assert [gr.nk_slot(k) for k in range(1, 9)] == [0, 1, 2, 3, 4, 4, 4, 4]
    assert [gr.grad_x_entry("RBF", d)[1] for d in (1, 16, 17, 32, 33, 129)] == [0, 0, 1, 1, 2, 2]
    assert gr.contract_entry("RBF+Matern52") == (1, 0) and gr.contract_entry("RBF+RatQuad") == (1, 1)


# --------------------------------------------------------------------------------- the references against the oracle
@pytest.mark.parametrize("kernel,n,d", [("RBF+Matern52*RatQuad", 40, 3), (gr.K6Q, 33, 5)])
def test_grad_x_reference_reproduces_the_oracle(kernel, n, d):
    kerns, ops = gr.split(kernel)
    X, y = orc.synth_problem(n, d, seed=n + d)
    theta = gr.well_conditioned_theta(kernel, d)
    K = orc.noisy_cov(X, kerns, ops, theta)
    Kinv = np.linalg.inv(K)
    Kinv = 0.5 * (Kinv + Kinv.T)
    ref, mag = gr.grad_x_reference(X, kernel, theta, Kinv, np.linalg.solve(K, y))
    _, gy, gX = orc.lml_grad_data(X, y, kerns, ops, theta)
    assert np.abs(ref.astype(np.float64) - gX).max() <= 1e-10 * np.abs(gX).max()
    assert (mag >= np.abs(ref)).all() and (mag > 0).all()


@pytest.mark.parametrize("kernel,n,d", [("Matern32*RatQuad+Exponential", 30, 2), (gr.K5, 25, 17)])
def test_predict_grad_reference_reproduces_the_oracle(kernel, n, d):
    kerns, ops = gr.split(kernel)
    X, y = orc.synth_problem(n, d, seed=n)
    theta = gr.well_conditioned_theta(kernel, d)
    Xn = gr.predict_queries(X, theta, d, seed=1)[2:]
    K = orc.noisy_cov(X, kerns, ops, theta, form="conditional")
    a = np.linalg.solve(K, y)
    w = np.linalg.solve(K, orc.kernel_matrix(X, Xn, kerns, ops, theta)).T
    dmu, dvar = orc.predict_grad(X, y, Xn, kerns, ops, theta)
    rm, _ = gr.predict_grad_reference(X, kernel, theta, Xn, a)
    rv, _ = gr.predict_grad_reference(X, kernel, theta, Xn, -2.0 * w)
    assert np.abs(rm.astype(np.float64) - dmu).max() <= 1e-10 * np.abs(dmu).max()
    assert np.abs(rv.astype(np.float64) - dvar).max() <= 1e-10 * np.abs(dvar).max()


def test_queries_hold_a_training_point_and_a_point_forty_length_scales_away():
    d = 17
    X, _ = orc.synth_problem(50, d, seed=0)
    theta = gr.well_conditioned_theta("RBF", d)
    Xn = gr.predict_queries(X, theta, d, seed=0)
    assert Xn.shape == (5, d) and (Xn[0] == X[3]).all()
    r = np.sqrt((((Xn[1] - 0.5) / theta[:d]) ** 2).sum())
    assert abs(r - 40.0) < 1e-9
    assert ((Xn[2:] >= 0) & (Xn[2:] <= 1)).all()


def test_well_conditioned_theta_keeps_cond_small():
    for kernel, n, d in [("RBF", 130, 3), ("RBF+Matern52*RatQuad", 130, 17), (gr.K8, 200, 33)]:
        kerns, ops = gr.split(kernel)
        X, _ = orc.synth_problem(n, d, seed=n + d)
        assert np.linalg.cond(orc.noisy_cov(X, kerns, ops, gr.well_conditioned_theta(kernel, d))) < 2e3


@pytest.mark.parametrize("name", ["RBF", "Matern52", "Matern32", "Exponential", "RatQuad"])
def test_mpmath_derivatives_against_the_oracle_and_a_difference_quotient(name):
    import mpmath as mp

    mp.mp.dps = 40
    for r2 in (0.0, 2.0 ** -20, 0.37, 5.0, 90.0):
        dk, arg, pre = gr.dk_truth(name, r2, 1.7)
        ref = float(orc.base_kernel_dr2(name, np.float64(r2), 1.7))
        assert abs(float(dk) - ref) <= 1e-13 * abs(ref) + 1e-300, (name, r2)
        if name != "RatQuad":
            assert abs(-pre * mp.exp(-arg) - dk) <= mp.mpf(10) ** -35 * abs(dk)
    # k' is the derivative of the value formula: central difference in 40 digits (Matern / Exponential through r2 + 1e-12)
    def value(r2):
        return gr.k_truth(name, r2, 1.7)

    h = mp.mpf(10) ** -12
    for r2 in (0.37, 5.0):
        fd = (value(mp.mpf(r2) + h) - value(mp.mpf(r2) - h)) / (2 * h)
        dk = gr.dk_truth(name, r2, 1.7)[0]
        # (5 / 3 and 5 / 6 are fp64 constants in the formulas: the Matern52 pair is consistent to their rounding only)
        assert abs(fd - dk) <= mp.mpf(10) ** -14 * abs(dk), (name, r2)


def test_mpmath_dalpha_against_a_difference_quotient_and_the_oracle():
    import mpmath as mp

    mp.mp.dps = 40
    h = mp.mpf(10) ** -15
    for r2, a in ((2.0 ** -20, 0.5), (1.0, 2.0), (2.0 ** 20, 8.0)):
        f = lambda al: mp.power(1 + mp.mpf(r2) / 2 / al, -al)
        fd = (f(mp.mpf(a) + h) - f(mp.mpf(a) - h)) / (2 * h)
        t, big = gr.ratquad_dalpha_truth(r2, a)
        assert abs(fd - t) <= mp.mpf(10) ** -10 * abs(t)  # (40 digits less the 15 of h, of a value near 1)
        assert big >= abs(t)
    X = np.array([[0.0], [1.5]])
    theta = orc.pack_theta([[1.0]], [1.7], 0.1, 1e-6, alpha=[2.0])
    got = orc.dK_dtheta(X, ["RatQuad"], [], theta)[2][1, 0]
    assert abs(got - 1.7 * float(gr.ratquad_dalpha_truth(2.25, 2.0)[0])) <= 1e-14 * abs(got)


def _alpha_ok(kernel, n, d):
    X, y = orc.synth_problem(max(n, 3), d, seed=7 * n + d)
    X, y = X[:n], y[:n]
    theta = gr.well_conditioned_theta(kernel, d)
    return gr.alpha_reference(X, y, kernel, theta, gr.predict_queries(X, theta, d, seed=n + d))[2:]


def test_d_mu_is_asserted_for_every_predict_grad_entry_and_count():
    """alpha_reference_ok leaves d mu unasserted only where an Exponential component meets d > 1; what remains still covers
    the five table entries and five to eight components."""
    slots, counts = set(), set()
    for kernel, n, d in gr.PREDICT_CASES:
        ok, dev = _alpha_ok(kernel, n, d)
        assert ok == (d == 1 or "Exponential" not in kernel), (kernel, n, d, dev)
        if ok:
            slots.add(gr.predict_entry(kernel)[0])
            counts.add(len(gr.split(kernel)[0]))
    assert slots == set(range(5)) and counts >= {5, 6, 7, 8}, (slots, counts)
    assert any("Exponential" in k and d > 16 for k, _, d in gr.PREDICT_CASES)  # d var meets Exponential and the 16-dimension chunks


@pytest.mark.parametrize("name", ["RBF", "Matern52", "Matern32", "Exponential", "RatQuad"])
def test_mpmath_values_against_the_oracle(name):
    for r2 in (0.0, 0.37, 90.0):
        ref = float(orc.base_kernel(name, np.float64(r2), 1.7))
        assert abs(float(gr.k_truth(name, r2, 1.7)) - ref) <= 1e-14 * abs(ref), (name, r2)
