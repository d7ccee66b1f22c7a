"""bench.py --dump-outputs: the last timed step's results land in DIR/<name>.npy as float64, identical from run to run
with the same arguments, and equal to the oracle at the same inputs (the dump is what the timed path computed)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

N, D, STEPS, WARMUP, GRAD_STEPS = 2048, 4, 3, 1, 2


def _bench(out):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--n", str(N), "--d", str(D),
                        "--steps", str(STEPS), "--warmup", str(WARMUP), "--grad-steps", str(GRAD_STEPS), "--chains-per-gpu", "0",
                        "--roofline-steps", "1", "--no-sharded", "--no-cpu-baseline", "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    return json.loads(lines[0])


def test_dump_outputs_are_reproducible_and_match_the_oracle(tmp_path):
    from bench import synth_problem, theta_sequence
    from oracle import gp_oracle as orc

    a, b = tmp_path / "a", tmp_path / "b"
    line = _bench(a)
    assert line["steps"] == STEPS and line["ms_per_step"] > 0
    _bench(b)
    names = sorted(os.listdir(a))
    assert names == ["lml.npy", "lml_grad_gradient.npy", "lml_grad_value.npy"]
    assert sorted(os.listdir(b)) == names
    out = {}
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype == np.float64 and np.all(np.isfinite(x))
        assert np.array_equal(x, y), n
        out[n[:-4]] = x

    X, y = synth_problem(N, D, seed=0)
    thetas = theta_sequence(D, WARMUP + STEPS, seed=0)
    ref = orc.lml(X, y, ["Matern52"], [], thetas[-1])
    assert abs(float(out["lml"]) - ref) <= 1e-10 * abs(ref), (float(out["lml"]), ref)
    vref, gref = orc.lml_grad(X, y, ["Matern52"], [], thetas[GRAD_STEPS - 1])
    assert abs(float(out["lml_grad_value"]) - vref) <= 1e-10 * abs(vref)
    assert out["lml_grad_gradient"].shape == gref.shape
    assert np.allclose(out["lml_grad_gradient"], gref, rtol=1e-7, atol=1e-7 * np.abs(gref).max())
