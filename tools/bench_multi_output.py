"""Time of mi_gp_lml_grad and of mi_gp_factor + a 256-point mi_gp_predict under option 51 = q (q outputs under one shared kernel)
for q in {2, 8, 128} at N = 1024, 4096 and 16384 (d = 16, Matern52), beside the single-output evaluation on the same handle, the
legs alternated evaluation by evaluation.  The single leg is timed twice per round (before and after the q legs): the difference
of the two medians is the spread the other legs are read against.  The baseline of q outputs without the option is q times the
single-output evaluation; --single-only times nothing else and uses only what every earlier build has, so the same file can time
another build of the package (--package-root: the directory that holds its andvaranaut_amd/).

    timeout -k 10 900 python tools/bench_multi_output.py [--sizes 1024 4096 16384] [--reps 20] [--out profiles/multi_output_bench.json]
    timeout -k 10 900 python tools/bench_multi_output.py --single-only --package-root /path/to/parent --out parent.json

--tail-only N Q: nothing but a warm-up and 20 evaluations of lml_grad and of factor + predict under option 51 = Q at that size, for
a kernel trace of the tail and of the moment kernel (rocprofv3 --kernel-trace --stats -- python tools/bench_multi_output.py
--tail-only 16384 8).  The split of the tail comes from that trace: the handle's profiling level 1 times the phases of the ordinary
evaluation and has no timers for the tails behind it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QS = (2, 8, 128)
POINTS = 256


def _ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def _stats(v):
    v = np.sort(np.asarray(v))
    return {"median_ms": float(np.median(v)), "min_ms": float(v[0]), "p90_ms": float(v[int(0.9 * (len(v) - 1))]), "n": len(v)}


def _outputs(X, y, q):
    rng = np.random.default_rng(5)
    cols = [y] + [np.sin(X @ rng.normal(size=X.shape[1]) + rng.uniform(0, 6)) + 0.1 * rng.normal(size=len(y)) for _ in range(q - 1)]
    return np.ascontiguousarray(np.column_stack(cols))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096, 16384])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--single-only", action="store_true")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--tail-only", type=int, nargs=2, default=None, metavar=("N", "Q"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_output_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_multi_output.py needs the MI355X: nothing is measured without it")
    sys.path.insert(0, os.path.abspath(a.package_root))
    if ROOT not in sys.path:
        sys.path.append(ROOT)
    from andvaranaut_amd import MiGP
    from oracle import gp_oracle as orc

    theta = orc.synth_theta(a.d, gv=1e-4)
    Xn = np.random.default_rng(2).random((POINTS, a.d))
    if a.tail_only:
        N, q = a.tail_only
        X, y = orc.synth_problem(N, a.d, seed=1)
        gp = MiGP(X, y, "Matern52", device=0)
        gp.set_outputs(_outputs(X, y, q))
        for _ in range(2 + 20):
            gp.lml_grad(theta)
            gp.predict(theta, Xn)
        gp.close()
        return
    res = {"d": a.d, "kernel": "Matern52", "device": torch.cuda.get_device_name(0), "reps": a.reps, "points": POINTS,
           "legs": "single only" if a.single_only else "single and q in %s" % (QS,), "sizes": []}
    for N in a.sizes:
        X, y = orc.synth_problem(N, a.d, seed=1)
        gp = MiGP(X, y, "Matern52", device=0)
        legs = [("single", 1)] + ([] if a.single_only else [("q%d" % q, q) for q in QS]) + [("single_again", 1)]
        Y = None if a.single_only else _outputs(X, y, max(QS))

        def select(q):
            if not a.single_only:
                gp.set_outputs(Y[:, :q])  # (rebinds the data: every leg starts without resident state)

        def predict():
            gp._factored_ok = False  # (every leg times factor + predict)
            gp.predict(theta, Xn, via_inverse=False)

        for _, q in legs:  # warm-up (the scratch, the work block)
            select(q)
            gp.lml_grad(theta)
            predict()
        t = {k: [] for k, _ in legs}
        tp = {k: [] for k, _ in legs}
        for _ in range(a.reps):
            for key, q in legs:
                select(q)
                t[key].append(_ms(lambda: gp.lml_grad(theta)))
                tp[key].append(_ms(predict))
        row = {"N": N, "lml_grad": {k: _stats(v) for k, v in t.items()}, "factor_plus_predict": {k: _stats(v) for k, v in tp.items()}}
        for part in ("lml_grad", "factor_plus_predict"):
            row[part]["spread_of_the_single_leg_ms"] = abs(row[part]["single"]["median_ms"] - row[part]["single_again"]["median_ms"])
        gp.close()
        res["sizes"].append(row)
        print(json.dumps(row))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
