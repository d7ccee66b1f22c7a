"""Time of mi_gp_lml_grad and of mi_gp_factor + mi_gp_predict under option 50 = 0 (no trend), 1 (constant) and 2 (linear) on ONE
handle, the three legs alternated evaluation by evaluation, at N = 4096 and 16384 (d = 16, Matern52).  The 0-leg is timed twice
per round (before and after the trend legs): the difference of the two medians is the spread the other legs are read against.

    timeout -k 10 900 python tools/bench_trend.py [--sizes 4096 16384] [--reps 20] [--out profiles/trend_bench.json]

--symm-only N: nothing but a warm-up and 20 evaluations under option 50 = 2 at that size, for a kernel trace of the symmetric
multiply (rocprofv3 --kernel-trace --stats -- python tools/bench_trend.py --symm-only 16384)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gp_oracle as orc  # noqa: E402

LEGS = (("none", 0), ("constant", 1), ("linear", 2))


def _ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def _stats(v):
    v = np.sort(np.asarray(v))
    return {"median_ms": float(np.median(v)), "min_ms": float(v[0]), "p90_ms": float(v[int(0.9 * (len(v) - 1))]), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--points", type=int, nargs="+", default=[256, 16384])
    ap.add_argument("--symm-only", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trend_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_trend.py needs the MI355X: nothing is measured without it")
    from andvaranaut_amd import MiGP

    if a.symm_only:
        X, y = orc.synth_problem(a.symm_only, a.d, seed=1)
        theta = orc.synth_theta(a.d, gv=1e-4)
        gp = MiGP(X, y, "Matern52", device=0)
        gp.set_trend("linear")
        for _ in range(2 + 20):
            gp.lml_grad(theta)
        gp.close()
        return
    res = {"d": a.d, "kernel": "Matern52", "device": torch.cuda.get_device_name(0), "reps": a.reps, "sizes": []}
    for N in a.sizes:
        X, y = orc.synth_problem(N, a.d, seed=1)
        theta = orc.synth_theta(a.d, gv=1e-4)
        gp = MiGP(X, y, "Matern52", device=0)
        for name, _ in LEGS + (("none", 0),):  # warm-up (and the trend's scratch)
            gp.set_trend(name)
            gp.lml_grad(theta)
        t = {"none": [], "constant": [], "linear": [], "none_again": []}
        for _ in range(a.reps):
            for key, name in (("none", "none"), ("constant", "constant"), ("linear", "linear"), ("none_again", "none")):
                gp.set_trend(name)
                t[key].append(_ms(lambda: gp.lml_grad(theta)))
        row = {"N": N, "lml_grad": {k: _stats(v) for k, v in t.items()}}
        row["lml_grad"]["spread_of_the_0_leg_ms"] = abs(row["lml_grad"]["none"]["median_ms"] - row["lml_grad"]["none_again"]["median_ms"])
        row["predict"] = []
        for m in a.points:
            Xn = np.random.default_rng(2).random((m, a.d)) * 1.5
            tp = {"none": [], "constant": [], "linear": []}
            for name in tp:  # warm-up (the work block)
                gp.set_trend(name)
                gp.predict(theta, Xn, via_inverse=False)
            for _ in range(max(3, a.reps // 4)):
                for name in tp:
                    gp.set_trend(name)  # (ends the factored state: every leg times factor + predict)
                    tp[name].append(_ms(lambda: gp.predict(theta, Xn, via_inverse=False)))
            row["predict"].append({"m": m, "factor_plus_predict": {k: _stats(v) for k, v in tp.items()}})
        gp.close()
        res["sizes"].append(row)
        print(json.dumps(row))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
