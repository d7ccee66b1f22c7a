"""Time of MiGP.append (mi_gp_append) for k = 1, 16, 128 new points against a refactorisation (mi_gp_factor, and the
factorisation plus U = L^-T that predict_u / predict_grad need) at N = 4096 and 16384.  Writes profiles/append_<N>.json.

    timeout -k 10 900 python tools/bench_append.py [--sizes 4096 16384] [--reps 5]
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
    ap.add_argument("--d", type=int, default=8)
    a = ap.parse_args()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    for N in a.sizes:
        X, y = orc.synth_problem(N + 128, a.d, seed=1)
        theta = orc.synth_theta(a.d, gv=1e-4)
        Xs = np.random.default_rng(0).random((4, a.d))
        gp = MiGP(X[:N], y[:N], "Matern52", device=0, capacity=N + 128)
        res = {"N": N, "d": a.d, "kernel": "Matern52", "device": torch.cuda.get_device_name(0), "reps": a.reps}
        gp.factor(theta)
        res["factor_ms"], res["factor_all"] = _ms(lambda: gp.factor(theta), a.reps)

        def factor_u():
            gp.factor(theta)
            gp.predict_grad(theta, Xs, refactor=False)  # forms U = L^-T (+ a 4-point prediction)

        res["factor_u_ms"], res["factor_u_all"] = _ms(factor_u, a.reps)
        for k in (1, 16, 128):
            for with_u in (False, True):
                key = f"append_k{k}{'_u' if with_u else ''}_ms"
                ts = []
                for _ in range(a.reps):  # every repetition appends to the same N-point factor
                    gp.factor(theta)
                    if with_u:
                        gp.predict_grad(theta, Xs, refactor=False)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    assert gp.append(X[N : N + k], y[N : N + k]) == 0
                    torch.cuda.synchronize()
                    ts.append(1e3 * (time.perf_counter() - t0))
                    assert gp.append_refactors == 0
                    gp.close()
                    gp = MiGP(X[:N], y[:N], "Matern52", device=0, capacity=N + 128)
                res[key] = float(np.median(ts))
                res[key.replace("_ms", "_all")] = [round(t, 4) for t in ts]
        gp.close()
        res["speedup_k1"] = res["factor_ms"] / res["append_k1_ms"]
        res["speedup_k1_u"] = res["factor_u_ms"] / res["append_k1_u_ms"]
        out = os.path.join(ROOT, "profiles", f"append_{N}.json")
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps({k: v for k, v in res.items() if not k.endswith("_all")}))


if __name__ == "__main__":
    main()
