"""Time of exact k-fold cross-validation from the resident K^-1 (MiGP.kfold: one lml_grad + the fold pass of mi_gp_kfold) against
a refit per fold (factor + predict on the complement of the fold), both on this library:

    N = 4096   32 folds of 128
    N = 16384  leave-one-out, and 128 folds of 128

The refit is timed on a sample of the folds (--refit-folds, the median per fold) and multiplied by the number of folds: the
16384 refits of leave-one-out at N = 16384 would run for minutes.  The sample's hold-out means are also compared with kfold's.
Writes <out>/kfold_<N>.json and prints one JSON line per workload.

    timeout -k 10 900 python tools/bench_kfold.py [--sizes 4096 16384] [--reps 5] [--refit-folds 8] [--out profiles]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from andvaranaut_amd import MiGP  # noqa: E402
from oracle import gp_oracle as orc  # noqa: E402

WORKLOADS = {4096: [("32x128", 128)], 16384: [("loo", 1), ("128x128", 128)]}


def _ms(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), [round(t, 4) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--refit-folds", type=int, default=8)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kfold.py needs the MI355X: nothing is measured without it")
    os.makedirs(a.out, exist_ok=True)
    for N in a.sizes:
        X, y = orc.synth_problem(N, a.d, seed=1)
        theta = orc.synth_theta(a.d, gv=1e-4)
        gp = MiGP(X, y, "Matern52", device=0)
        res = {"N": N, "d": a.d, "kernel": "Matern52", "device": torch.cuda.get_device_name(0), "reps": a.reps, "workloads": {}}
        gp.lml_grad(theta)  # warm-up
        res["lml_grad_ms"], res["lml_grad_all"] = _ms(lambda: gp.lml_grad(theta), a.reps)
        for name, size in WORKLOADS.get(N, [("%dx128" % (N // 128), 128)]):
            perm = np.random.default_rng(2).permutation(N)
            folds = np.arange(N).reshape(-1, 1) if size == 1 else perm.reshape(-1, size)  # (equal folds: the rows of one array)
            w = {"nfolds": len(folds), "fold_size": size}
            logp, mu, var, info = gp.kfold(theta, folds)  # warm-up (and the work block's allocation)
            assert not info.any() and np.isfinite(logp).all()
            w["kfold_ms"], w["kfold_all"] = _ms(lambda: gp.kfold(theta, folds), a.reps)
            w["fold_pass_ms"], w["fold_pass_all"] = _ms(lambda: gp.kfold(theta, folds, resident=True), a.reps)
            # the refit: one handle on N - size points, the complement of each sampled fold uploaded outside the timed window
            sample = list(range(0, len(folds), max(1, len(folds) // a.refit_folds)))[: a.refit_folds]
            J0 = np.setdiff1d(np.arange(N), folds[sample[0]])
            other = MiGP(X[J0], y[J0], "Matern52", device=0, need_grad=False)
            other.factor(theta)
            other.predict(theta, X[folds[sample[0]]], via_inverse=False)  # warm-up
            ts, err = [], 0.0
            for f in sample:
                J = np.setdiff1d(np.arange(N), folds[f])
                other.update_data(X[J], y[J])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                assert other.factor(theta) == 0
                m2, v2 = other.predict(theta, X[folds[f]], via_inverse=False)
                torch.cuda.synchronize()
                ts.append(1e3 * (time.perf_counter() - t0))
                err = max(err, float(np.max(np.abs(m2 - mu[f]))))
            other.close()
            w["refit_per_fold_ms"] = float(np.median(ts))
            w["refit_per_fold_all"] = [round(t, 4) for t in ts]
            w["refit_ms_extrapolated"] = w["refit_per_fold_ms"] * len(folds)
            w["refit_over_kfold"] = w["refit_ms_extrapolated"] / w["kfold_ms"]
            w["max_abs_mean_difference_on_the_sample"] = err
            res["workloads"][name] = w
            print(json.dumps({"N": N, "workload": name, **{k: v for k, v in w.items() if not k.endswith("_all")}}))
        gp.close()
        with open(os.path.join(a.out, f"kfold_{N}.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
