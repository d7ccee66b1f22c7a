"""GPMCMC.propose_samples / adaptive_sample on the GPU: on a 2-D test function, 16 adaptively chosen points (4 rounds of 4 at fixed
hyper-parameters) leave a smaller mean posterior variance over a fresh 500-point set than 16 further Latin-hypercube points
(tests/test_design_host.py shows in NumPy that the seed has this property); propose_samples leaves the object as it found it and
its points respect the priors' intervals and the constraints."""
import numpy as np
import pytest
import scipy.stats as st

from design_ref import FACADE, facade_points

pytestmark = pytest.mark.gpu

PRIORS = [st.uniform(0, 1), st.uniform(0, 1)]


def _target(x):
    return np.array([np.sin(5.0 * x[0]) * np.cos(3.0 * x[1]) + 0.5 * x[0] * x[1]])


@pytest.fixture(scope="module")
def fitted():
    """40 Latin-hypercube points, a MAP fit for the model object, then the test's fixed hyper-parameters"""
    from andvaranaut_amd.gpmcmc import GPMCMC

    x0, xl, xt = facade_points(PRIORS)
    g = GPMCMC(kernel="Matern52", noise=True, nx=2, ny=1, priors=PRIORS, target=_target, verbose=False)
    g.set_data(x0, np.array([_target(r) for r in x0]))
    g.fit(method="map")
    g.hypers = {"l": np.full(2, FACADE["ls"]), "kv": np.array([FACADE["kv"]]), "gv": np.array([FACADE["gv"]])}
    yield g, x0, xl, xt
    if g.gp is not None:
        g.gp.close()


def test_propose_samples_leaves_the_object_as_it_found_it(fitted):
    g, x0, _, xt = fitted
    before = g.predict(xt, return_var=True)
    n_before, x_before = g.gp.n, g.x.copy()
    xs, gains = g.propose_samples(6, ncand=200, nref=100, seed=3)
    assert xs.shape == (6, 2) and gains.shape == (6,) and (gains > 0).all() and (np.diff(gains) < 0).any()
    assert ((xs >= 0) & (xs <= 1)).all() and len({tuple(r) for r in xs}) == 6
    after = g.predict(xt, return_var=True)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert g.gp.n == n_before and np.array_equal(g.x, x_before)
    assert g.gp.get_option(56) == 0 and g.gp.get_option(57) == 0
    # the same seed proposes the same points; "var" needs no reference set
    xs2, gains2 = g.propose_samples(6, ncand=200, nref=100, seed=3)
    assert np.array_equal(xs, xs2) and np.array_equal(gains, gains2)
    xv, gv = g.propose_samples(3, criterion="var", ncand=200, seed=3)
    assert xv.shape == (3, 2) and (np.diff(gv) <= 0).all()


def test_more_than_one_device_batch_appends_and_restores(fitted):
    g, _, _, xt = fitted
    before = g.predict(xt, return_var=True)
    xs, gains = g.propose_samples(130, ncand=300, nref=64, seed=5)
    assert xs.shape == (130, 2) and len({tuple(r) for r in xs}) == 130 and (gains > 0).all()
    after = g.predict(xt, return_var=True)
    assert g.gp.n == len(g.x) == FACADE["n0"]
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_proposed_points_respect_the_constraints(fitted):
    g = fitted[0]
    g.constraints = {"constraints": [lambda x: x[0] + x[1]], "lower_bounds": [0.0], "upper_bounds": [1.1]}
    try:
        xs, _ = g.propose_samples(8, ncand=200, nref=100, seed=4)
    finally:
        g.constraints = None
    assert len(xs) == 8 and (xs.sum(1) <= 1.1).all() and ((xs >= 0) & (xs <= 1)).all()


def test_adaptive_points_beat_a_latin_hypercube_of_the_same_size(fitted):
    from andvaranaut_amd import MiGP

    g, x0, xl, xt = fitted
    cfg = FACADE
    theta = g._theta_from_hypers(g.hypers, cfg["jitter"])
    g.adaptive_sample(cfg["nadd"], batch=cfg["batch"], refit=False, seed=cfg["seed"], ncand=cfg["ncand"], nref=cfg["nref"],
                      jitter=cfg["jitter"])
    assert len(g.x) == cfg["n0"] + cfg["nadd"] and np.array_equal(g.x[: cfg["n0"]], x0) and g.y.shape == (len(g.x), 1)
    assert np.array_equal(g.y[cfg["n0"]:, 0], [_target(r)[0] for r in g.x[cfg["n0"]:]])
    adaptive = g._ensure_gp().predict(theta, xt, pred_noise=False)[1].mean()
    assert g.gp.n == len(g.x)
    xa = np.vstack([x0, xl])
    other = MiGP(xa, np.array([_target(r)[0] for r in xa]), "Matern52", device=0)
    try:
        lhc = other.predict(theta, xt, pred_noise=False)[1].mean()
    finally:
        other.close()
    print(f"mean latent variance over 500 fresh points: adaptive {adaptive:.5e}, Latin hypercube {lhc:.5e}")
    assert adaptive < lhc
