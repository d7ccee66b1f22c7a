"""Posterior predictive over k hyper-parameter draws: (a) MiGP.predict_batch (mi_gp_factor_batch + mi_gp_predict_batch, one
lockstep batch) against (b) a Python loop of factor + predict over the same draws (the blocked triangular solve, i.e. the same
algebra one draw at a time), RBF, d = 8, at N in {512, 1024, 2048, 4096, 8192}, k in {8, 32}, M in {1000, 10000}.  Wall time
per call (median of --reps after one warm-up), the speed-up, and whether every row of (a) equals (b) bit for bit.  Writes JSON
to profiles/bench_predict_posterior.json (or --out).

  python tools/bench_predict_posterior.py [--sizes 512,1024] [--ks 8] [--ms 1000] [--reps 3] [--batched-only]

--batched-only times (a) alone (what a rocprofv3 --kernel-trace --stats run of one shape wants to see)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _theta(d, k, rng):
    out = []
    for _ in range(k):
        ls = np.full(d, 0.6) * rng.uniform(0.7, 1.5, d)
        out.append(np.concatenate([ls, [1.7 * rng.uniform(0.8, 1.3)], [1.0], [10.0 ** rng.uniform(-4.5, -2.5), 1e-6]]))
    return np.array(out)


def _median_time(fn, reps):
    fn()  # warm-up (buffers, code objects)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024,2048,4096,8192")
    ap.add_argument("--ks", default="8,32")
    ap.add_argument("--ms", default="1000,10000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--batched-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_predict_posterior.json"))
    a = ap.parse_args()
    import torch

    from andvaranaut_amd import MiGP

    rows = []
    for N in [int(v) for v in a.sizes.split(",")]:
        rng = np.random.default_rng(N)
        X = rng.random((N, a.d))
        y = np.sin(X.sum(axis=1)) + 0.1 * rng.standard_normal(N)
        gp = MiGP(X, y, "RBF", need_grad=False)
        for k in [int(v) for v in a.ks.split(",")]:
            th = _theta(a.d, k, rng)
            for M in [int(v) for v in a.ms.split(",")]:
                Xs = rng.random((M, a.d))

                def batched():
                    return gp.predict_batch(th, Xs, mixture=True)

                def loop():
                    mu, var = np.empty((k, M)), np.empty((k, M))
                    for p in range(k):
                        gp.factor(th[p])
                        mu[p], var[p] = gp.predict(th[p], Xs, via_inverse=False)
                    return mu, var

                tb, (bm, bv, _, _) = _median_time(batched, a.reps)
                row = {"N": N, "k": k, "M": M, "batched_ms": 1e3 * tb, "draws_per_s_batched": k / tb}
                if not a.batched_only:
                    tl, (lm, lv) = _median_time(loop, a.reps)
                    row.update({"loop_ms": 1e3 * tl, "speedup": tl / tb, "draws_per_s_loop": k / tl,
                                "bit_equal": bool(np.array_equal(bm, lm) and np.array_equal(bv, lv))})
                rows.append(row)
                print(json.dumps(row), flush=True)
        gp.close()
        torch.cuda.empty_cache()
    res = {"what": "predict_batch vs a loop of factor + predict over the same draws (RBF, d = %d, wall ms, median of %d)" % (a.d, a.reps),
           "device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
