"""Time of mi_gp_lml_grad under option 48 = 1 with the fold size (option 49) at 1 (leave-one-out: the parent path), 8, 37 and 128
on ONE handle, interleaved, at N = 1024, 4096 and 16384 (d = 16, Matern52), median of --reps; option 48 = 0 rides along so that
the tails (objective minus evaluation) can be compared.  Then ONE kernel-trace run of a child of its own (rocprofv3
--kernel-trace -- python tools/bench_cv_objective.py --trace-child N) gives the per-launch times of each tail at N = --trace-n:
the launches between the tail's first kernel and its contraction kernel, summed by kernel.

    timeout -k 10 900 python tools/bench_cv_objective.py [--sizes 1024 4096 16384] [--reps 7] [--out profiles/cv_objective_bench.json]

--lib PATH runs the timing with another build of libmi_gp.so that has option 48 but not option 49 (the parent commit's): only the
block size 1 is timed there; --against PATH (a JSON written by such a run) adds its 49 = 1 time and the ratio to the output.
--no-trace skips the kernel-trace run."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from andvaranaut_amd import _lib  # noqa: E402
from oracle import gp_oracle as orc  # noqa: E402

BLOCKS = (1, 8, 37, 128)


def _ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def _problem(N, d):
    from andvaranaut_amd import MiGP

    X, y = orc.synth_problem(N, d, seed=1)
    return MiGP(X, y, "Matern52", device=0), orc.synth_theta(d, gv=1e-4)


def trace_child(N, d):
    """what the kernel trace records: warm-up, then ONE evaluation per block size in the order of BLOCKS"""
    gp, theta = _problem(N, d)
    gp.set_option(48, 1)
    for b in (1, 2):
        gp.set_option(49, b)
        gp.lml_grad(theta)
    for b in BLOCKS:
        gp.set_option(49, b)
        gp.lml_grad(theta)
    gp.close()


def _short(name):
    name = name.split("(")[0].split("<")[0]
    return name.split("::")[-1].split(" ")[-1]


def tails_from_trace(directory):
    """{block size: {kernel: [launches, total us]}} from the kernel trace of trace_child: the tail under 49 = 1 starts at the last
    loo_weights_kernel, the tails under 8, 37 and 128 at the first kfold_gather_kernel behind the tail before; each ends with its
    grad_contract kernel."""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), _short(r["Kernel_Name"])))
    rows.sort()
    names = [r[2] for r in rows]
    out = {}
    pos = max(i for i, nm in enumerate(names) if nm == "loo_weights_kernel")
    for b in BLOCKS:
        if b > 1:
            pos = next(i for i in range(pos, len(rows)) if names[i] == "kfold_gather_kernel")
        end = next(i for i in range(pos, len(rows)) if "grad_contract" in names[i])
        while end + 1 < len(rows) and "grad" in names[end + 1]:  # (the contraction's final reduction)
            end += 1
        agg = {}
        for s, e, nm in rows[pos : end + 1]:
            a = agg.setdefault(nm, [0, 0.0])
            a[0] += 1
            a[1] += (e - s) / 1e3
        out[b] = {"span_us": (rows[end][1] - rows[pos][0]) / 1e3, "kernels": {k: [v[0], round(v[1], 2)] for k, v in agg.items()}}
        pos = end + 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096, 16384])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--against", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-n", type=int, default=16384)
    ap.add_argument("--trace-child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cv_objective_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cv_objective.py needs the MI355X: nothing is measured without it")
    if a.trace_child:
        return trace_child(a.trace_child, a.d)
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    base = {}
    if a.against:
        with open(a.against) as f:
            base = {r["N"]: r for r in json.load(f)["sizes"]}
    res = {"d": a.d, "kernel": "Matern52", "device": torch.cuda.get_device_name(0), "reps": a.reps, "lib": a.lib or "this tree", "sizes": []}
    for N in a.sizes:
        gp, theta = _problem(N, a.d)
        blocks = BLOCKS if not a.lib else (1,)
        for b in blocks:  # warm-up (and the tail's scratch)
            gp.lml_grad(theta)
            gp.set_option(48, 1)
            if b > 1:
                gp.set_option(49, b)
            gp.lml_grad(theta)
            gp.set_option(48, 0)
        t = {b: [] for b in (0,) + tuple(blocks)}
        for _ in range(a.reps):  # interleaved: every block size sees the same clocks
            t[0].append(_ms(lambda: gp.lml_grad(theta)))
            gp.set_option(48, 1)
            for b in blocks:
                if not a.lib:
                    gp.set_option(49, b)
                t[b].append(_ms(lambda: gp.lml_grad(theta)))
            gp.set_option(48, 0)
        r = {"N": N, "lml_grad_ms": float(np.median(t[0]))}
        for b in blocks:
            r["cv_b%d_ms" % b] = float(np.median(t[b]))
            r["cv_b%d_all" % b] = [round(x, 4) for x in t[b]]
            r["tail_b%d_ms" % b] = r["cv_b%d_ms" % b] - r["lml_grad_ms"]
        for b in blocks[1:]:
            r["tail_b%d_over_b1" % b] = r["tail_b%d_ms" % b] / r["tail_b1_ms"]
            r["cv_b%d_over_b1" % b] = r["cv_b%d_ms" % b] / r["cv_b1_ms"]
        if N in base:
            r["cv_b1_ms_other_build"] = base[N]["cv_b1_ms"]
            r["cv_b1_over_other_build"] = r["cv_b1_ms"] / base[N]["cv_b1_ms"]
        res["sizes"].append(r)
        print(json.dumps({k: v for k, v in r.items() if not k.endswith("_all")}))
        gp.close()
    if not a.no_trace and not a.lib:
        prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
        tmp = tempfile.mkdtemp(prefix="cv_trace_")
        try:
            cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                   "--trace-child", str(a.trace_n), "--d", str(a.d)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit("the kernel-trace run failed:\n" + p.stdout[-2000:] + p.stderr[-2000:])
            res["trace"] = {"N": a.trace_n, "tails": tails_from_trace(tmp)}
            for b, tail in res["trace"]["tails"].items():
                print("N = %d, 49 = %d: tail %.1f us" % (a.trace_n, b, tail["span_us"]),
                      ", ".join("%s %d x %.1f" % (k, v[0], v[1]) for k, v in sorted(tail["kernels"].items(), key=lambda kv: -kv[1][1])))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
