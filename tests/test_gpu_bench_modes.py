"""bench.py's two modes on one GPU: a plain run prints the headline alone (nothing after the timed steps but the line), and
--full adds every extra record -- LML + gradient rate, concurrent chains, the roofline pass, the sharded sub-record and the CPU
baseline with its parity record -- on the same headline fields."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SMALL = ["--gpus", "1", "--n", "2048", "--d", "4", "--steps", "3", "--warmup", "1"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
EXTRAS = ("lml_grad", "concurrent_chains", "roofline_pass", "assembly", "roofline", "sharded", "cpu_baseline")


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + args, env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    line = json.loads(lines[0])
    assert line["metric"] == "gp_lml_evals_per_s" and line["unit"] == "evals/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0 and abs(line["value"] - 1e3 / line["ms_per_step"]) <= 1e-9 * line["value"]
    return line


def test_plain_run_prints_the_headline_alone():
    line = _bench([])
    assert all(k in line for k in HEADLINE)
    assert not [k for k in EXTRAS if k in line], line


def test_full_run_adds_every_extra_record():
    line = _bench(["--full", "--grad-steps", "1", "--chains-per-gpu", "2", "--roofline-steps", "1", "--sharded-n", "3000",
                   "--sharded-d", "4", "--sharded-kernel", "Matern52", "--sharded-steps", "1", "--sharded-panel-tiles", "2"])
    assert line["lml_grad"]["steps"] == 1 and line["lml_grad"]["ms_per_eval"] > 0
    assert line["concurrent_chains"]["chains_per_gpu"] == 2 and line["concurrent_chains"]["evals_per_s"] > 0
    assert line["roofline_pass"]["steps"] == 1 and line["roofline"]["unit"] == "TFLOP/s" and line["assembly"]["ms"] > 0
    rec = line["sharded"]
    assert "error" not in rec and rec["finite"] and rec["scaling"] == "strong" and rec["collectives"] == "rccl"
    assert rec["rel_diff_vs_single_gpu_path"] <= 1e-10
    cpu = line["cpu_baseline"]
    assert cpu["measured_at_full_size"] and cpu["value"] > 0 and cpu["rel_diff_vs_gpu"] <= cpu["rtol_target"]
