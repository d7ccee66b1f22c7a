"""The host side of the posterior sample paths (andvaranaut_amd/paths.py; options 54 / 55 of mi_gp_set_option) on the CPU: the
spectral samplers against the oracle's kernels, the moments of the np.longdouble / NumPy restatement of the whole draw
(tests/paths_ref.py) against the oracle's posterior, the block helpers against the header's formulas, and the refusals that
need no device."""
import os
import re

import numpy as np
import pytest

import grad_refs as gr
import paths_ref as pr
from andvaranaut_amd import _lib, paths
from oracle import gp_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kernel", pr.SAMPLER_KERNELS)
def test_spectral_sampler_reproduces_the_kernel(kernel):
    """kd mean_i 2 cos(om_i . x + b_i) cos(om_i . x' + b_i) over F_total = 2^19 features, in 32 blocks of 2^14, against
    orc.kernel_matrix at 12 points of the cube: max |Phi Phi^T - K| <= 6 kd / sqrt(F_total), about 6 standard errors of an entry
    (an entry's summand 2 kd cos cos has a standard deviation of at most kd)."""
    kerns, ops = gr.split(kernel)
    d, blocks, Fb = 2, 32, 1 << 14
    theta = gr.well_conditioned_theta(kernel, d)
    ls, kv, al, _, _ = orc.split_theta(theta, d, len(kerns))
    X = np.random.default_rng(41).random((12, d))
    K = orc.kernel_matrix(X, X, kerns, ops, theta)
    acc = np.zeros((12, 12))
    for blk in range(blocks):
        rng = np.random.Generator(np.random.Philox(9000 + blk))
        om, kd = paths.spectral_frequencies(kerns, ops, ls, kv, al, Fb, rng)
        b = rng.random(Fb) * 2.0 * np.pi
        phi = np.cos(X @ om.T + b[None, :])
        acc += 2.0 * kd / Fb * (phi @ phi.T)
    assert om.shape == (Fb, d) and abs(kd - orc.kernel_diag(kerns, ops, theta, d)) <= 1e-15 * kd
    err = np.abs(acc / blocks - K).max() / (kd / np.sqrt(blocks * Fb))
    print(f"spectral sampler {kernel}: max |Phi Phi^T - K| = {err:.2f} kd / sqrt(F_total) (cap 6)")
    assert err <= 6.0


def test_the_same_seed_gives_the_same_block_and_the_draw_order_is_the_documented_one():
    kerns, ops = gr.split("Matern52+RBF")
    theta = gr.well_conditioned_theta("Matern52+RBF", 3)
    a = paths.draw_block_parts(kerns, ops, theta, 3, 10, 4, 32, 77)
    b = paths.draw_block_parts(kerns, ops, theta, 3, 10, 4, 32, 77)
    c = paths.draw_block_parts(kerns, ops, theta, 3, 10, 4, 32, 78)
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and not np.array_equal(a[0], c[0])
    # Omega, then b, W and E from the same generator
    rng = np.random.Generator(np.random.Philox(77))
    ls, kv, al, gv, jit = orc.split_theta(theta, 3, 2)
    om, kd = paths.spectral_frequencies(kerns, ops, ls, kv, al, 32, rng)
    assert np.array_equal(om, a[0]) and kd == a[4] == 2.0
    assert np.array_equal(rng.random(32) * (2.0 * np.pi), a[1])
    assert np.array_equal(np.sqrt(2.0 * kd / 32) * rng.standard_normal((32, 4)), a[2])
    assert np.array_equal(np.sqrt(np.full(10, gv + jit))[:, None] * rng.standard_normal((10, 4)), a[3])
    d = paths.draw_block_parts(kerns, ops, theta, 3, 10, 4, 32, 77, diag=np.arange(10.0))
    assert np.array_equal(d[2], a[2]) and np.allclose(d[3] / a[3], np.sqrt((gv + jit + np.arange(10.0)) / (gv + jit))[:, None])


def test_reference_moments_against_the_oracle_posterior():
    """paths_ref.path_reference at n = 40, d = 2, F = 4096, 32 draws of 128 paths (the seeds of the device's moment test): the
    path means lie within 5 standard errors of the oracle's posterior mean at 12 points and the variance ratios in
    [0.85, 1.15]."""
    X, y, theta, Xt, mu, var = pr.moment_problem()
    vals = np.vstack([pr.path_reference(X, y, pr.MOMENT_KERNEL, theta, seed, pr.MOMENT_S, pr.MOMENT_F, Xt, precise=False)["values"]
                      for seed in pr.MOMENT_SEEDS])
    assert vals.shape == (pr.MOMENT_S * pr.MOMENT_DRAWS, 12)
    z, lo, hi = pr.moment_margins(vals, mu, var)
    print(f"reference moments over {vals.shape[0]} paths: mean within {z:.2f} standard errors (cap 5), variance ratios "
          f"{lo:.3f} .. {hi:.3f} (caps 0.85, 1.15)")
    assert z <= 5.0 and 0.85 <= lo and hi <= 1.15


def test_precise_and_float64_references_agree_and_vanish_at_the_data():
    """One small draw both ways; and the update's defining identity in the reference itself: at the training points
    f_s(X) = y - E - D V with D = K_y - K_f, up to the solve's residual."""
    X, y = orc.synth_problem(30, 2, seed=3)
    theta = gr.well_conditioned_theta("Matern32", 2)
    a = pr.path_reference(X, y, "Matern32", theta, 5, 3, 64, X, precise=True)
    b = pr.path_reference(X, y, "Matern32", theta, 5, 3, 64, X, precise=False)
    assert np.abs(a["values"].astype(np.float64) - b["values"]).max() <= 1e-10
    D = pr.noise_part(X, "Matern32", theta)
    assert np.abs(D - np.diag(np.diag(D))).max() <= 64 * pr.EPS  # (off the diagonal: the two r2 forms' roundings)
    lhs = a["values"].T
    rhs = y[:, None].astype(pr.LD) - a["E"].astype(pr.LD) - D @ a["V"]
    assert np.abs(lhs - rhs).max() <= 1e-14 * max(1.0, float(np.abs(rhs).max()))


def test_block_helpers_follow_the_header_formulas():
    header = open(os.path.join(ROOT, "include", "mi_gp.h")).read()
    para = header[header.index("Option 54") :]
    assert "F * d + F + F * ldw" in para and "F * d + F" in para and "F * d" in para
    for F, d, ldw, n, S in ((16, 1, 2, 5, 1), (48, 5, 4, 63, 3), (1040, 32, 128, 130, 128), (64, 17, 18, 7, 17)):
        off = paths.block_offsets(F, d, ldw, n)
        assert (off["omega"], off["b"], off["W"], off["V"]) == pr.header_offsets(F, d, ldw)
        assert off["len"] == off["V"] + n * ldw
        rng = np.random.default_rng(F)
        om, b, W, V = rng.random((F, d)), rng.random(F), rng.random((F, S)), rng.random((n, S))
        blk = paths.pack_block(om, b, W, V, ldw)
        assert blk.shape == (off["len"],)
        assert np.array_equal(blk[off["W"] + 3 * ldw : off["W"] + 3 * ldw + S], W[3]) and blk[off["V"] + 2 * ldw] == V[2, 0]
        back = paths.unpack_block(blk, F, d, ldw, n, S)
        assert all(np.array_equal(x, y) for x, y in zip(back, (om, b, W, V)))
        pad = blk[off["W"] :].reshape(F + n, ldw)[:, S:]
        assert (pad == 0.0).all()
    assert [paths.block_ldw(s) for s in (1, 2, 3, 127, 128)] == [2, 2, 4, 128, 128]
    assert [paths.path_window(d) for d in (1, 4, 5, 16, 17, 32)] == [4, 4, 16, 16, 32, 32]
    assert [paths.path_tile(d, True) for d in (4, 16, 32)] == [8, 2, 1] and paths.path_tile(9, False) == 16
    # the kernel file states the same tiles
    src = open(os.path.join(ROOT, "andvaranaut_amd", "csrc", "paths_f64.hip")).read()
    assert re.search(r"return !grad \? PATH_TILE_VALUE : d <= 4 \? 8 : d <= 16 \? 2 : 1;", src)


def test_refusals_that_need_no_device():
    from andvaranaut_amd.backend import MiGP

    for bad in (0, 129, -1):
        with pytest.raises(ValueError, match="npaths"):
            paths.check_counts(bad, 64)
    for bad in (0, 8, 24, 65552, 1 << 17):
        with pytest.raises(ValueError, match="nfeatures"):
            paths.check_counts(4, bad)
    assert paths.check_counts(128, 65536) == (128, 65536)
    gp = object.__new__(MiGP)  # (no handle: every refusal below comes before the first device call)
    gp.d, gp.n, gp.Z_t = 33, 10, object()
    with pytest.raises(ValueError, match="d <= 32"):
        gp.draw_paths(np.ones(3), 4)
    gp.d = 2
    with pytest.raises(ValueError, match="npaths"):
        gp.draw_paths(np.ones(3), 200)
    gp.Z_t = None
    with pytest.raises(RuntimeError, match="need_grad=False"):
        gp.draw_paths(np.ones(3), 4)
    gp._trend = 1
    with pytest.raises(ValueError, match="has no form under a trend"):
        gp.draw_paths(np.ones(3), 4)
    gp._trend, gp.nout = 0, 2
    with pytest.raises(ValueError, match="has no form under several outputs"):
        gp.draw_paths(np.ones(3), 4)
    # the factorisation serial: every assignment of the factored flag and nothing else advances it
    gp.nout = 1
    s0 = gp._path_serial
    assert getattr(gp, "_factored_ok", False) is False and gp._path_serial == s0
    gp._factored_ok = True
    assert gp._factored_ok is True and gp._path_serial == s0 + 1
    gp._factored_ok = False
    assert gp._path_serial == s0 + 2
    # a PathDraw refuses a stale serial, a closed MiGP and its own close() before any device call
    gp.h = object()
    draw = paths.PathDraw(gp, object(), 4, 64, 4, 1, gp._path_serial)
    gp._factored_ok = True
    with pytest.raises(RuntimeError, match="draw again"):
        draw.evaluate(np.zeros((1, 2)))
    draw = paths.PathDraw(gp, object(), 4, 64, 4, 1, gp._path_serial)
    gp.h = None
    with pytest.raises(RuntimeError, match="closed"):
        draw.evaluate(np.zeros((1, 2)))
    gp.h = object()
    draw.close()
    with pytest.raises(RuntimeError, match="closed"):
        draw.evaluate(np.zeros((1, 2)))
    gp.h = None  # (nothing for __del__ to destroy)


def test_the_c_abi_still_exports_57_entry_points():
    assert len(_lib.EXPORTS) == 57
