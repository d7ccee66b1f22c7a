"""Ties the host-only launch traces (tests/sched_trace, tests/test_sched_trace_host.py) to the library on the device: the
GEMM launches and algorithmic flops that mi_gp_timers counts for an evaluation at profiling level 2 are the ones the trace of
the same configuration holds.  If the trace program's stand-ins, its handle or its options drifted from the real library's,
the schedules the host tests check would not be the schedules that run."""
import numpy as np
import pytest

import sched_check as C
import sched_trace_harness as H

pytestmark = pytest.mark.gpu

ORACLE_SIZES = (600, 3300)


@pytest.fixture(scope="module")
def prog():
    return H.build_trace_program()


@pytest.mark.parametrize("n", [600, 3300, 5100, 8900])
def test_gemm_launches_and_flops_of_the_device_run_are_the_trace_s(n, prog, tmp_path):
    import torch

    assert torch.cuda.is_available()
    from andvaranaut_amd import MiGP
    from oracle import gp_oracle as orc

    d = 3
    option_sets = ({}, {26: 0})
    lines = [H.config_line(None, e, options=dict(o, prof=2), n=n, d=d) for o in option_sets for e in ("lml", "lml_grad")]
    traces = iter(C.split_evaluations(H.run_traces(prog, lines, tmp_path)))
    X, y = orc.synth_problem(n, d, seed=n)
    theta = orc.synth_theta(d)
    if n in ORACLE_SIZES:
        ref, gref = orc.lml_grad(X, y, ["RBF"], [], theta)
    gp = MiGP(X, y, "RBF")
    gp.set_profiling(2)
    first = True
    for o in option_sets:
        gp.set_option(26, o.get(26, 2))
        for entry in ("lml", "lml_grad"):
            cfg, recs, end = next(traces)
            assert cfg["entry"] == entry and cfg["n"] == n and cfg["options"]["26"] == gp.get_option(26) == o.get(26, 2)
            if first:  # the trace program's handle has the device handle's value of every option
                assert {k: gp.get_option(int(k)) for k in cfg["options"]} == cfg["options"]
                first = False
            if entry == "lml":
                val, g = gp.lml(theta), None
            else:
                val, g = gp.lml_grad(theta)
            t = gp.timers()
            launches, flops = C.gemm_figures(recs)
            print(n, o, entry, "device:", t["gemm_launches"], t["gemm_flops"], "trace:", launches, flops)
            assert (end["n_gemm"], end["gemm_flops"]) == (launches, flops)  # (the library's own count under the stand-ins)
            assert t["gemm_launches"] == launches
            assert abs(t["gemm_flops"] - flops) <= 1e-12 * flops
            if n in ORACLE_SIZES:
                assert abs(val - ref) <= 1e-10 * abs(ref), (val, ref)
                if g is not None:
                    assert np.abs(g - gref).max() <= 1e-8 * np.abs(gref).max()
    gp.close()
