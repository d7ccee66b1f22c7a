"""Times the gradient binding against the plain handle at equal N (profiles/NOTES_deriv.md): the assembly, the contraction (the
handle's own event timers, mi_gp_set_profiling(1)) and LML + gradient (wall clock, profiling off), for n runs in d dimensions
under the binding and N = n (1 + d) plain points in d dimensions, in the same process.

    python tools/bench_deriv.py [--shapes 512x16,964x16] [--reps 5] [--kernel Matern52]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def _timers(gp):
    out = (ctypes.c_double * 17)()
    gp.lib.mi_gp_timers(gp.h, out, 17)
    return {"assemble_ms": out[0], "contract_ms": out[9], "chol_ms": out[1], "trtri_ms": out[7], "lauum_ms": out[8]}


def _measure(gp, theta, reps):
    gp.lml_grad(theta)  # warm-up
    gp.lib.mi_gp_set_profiling(gp.h, 1)
    prof = []
    for _ in range(reps):
        gp.lml_grad(theta)
        prof.append(_timers(gp))
    gp.lib.mi_gp_set_profiling(gp.h, 0)
    gp.lml_grad(theta)
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        gp.lml_grad(theta)
        wall.append((time.perf_counter() - t0) * 1e3)
    res = {k: float(np.median([p[k] for p in prof])) for k in prof[0]}
    res["lml_grad_ms"] = float(np.median(wall))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="512x16,964x16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel", default="Matern52")
    args = ap.parse_args()
    from andvaranaut_amd import MiGP
    from andvaranaut_amd.deriv import MiDerivGP

    for shape in args.shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        N = n * (1 + d)
        rng = np.random.default_rng(n)
        X = rng.random((n, d))
        w = rng.standard_normal(d)
        y = np.sin(X @ w)
        dY = np.cos(X @ w)[:, None] * w[None, :]
        theta = np.concatenate([np.exp(np.linspace(np.log(0.4), np.log(1.5), d)), [1.7, 1.0, 1e-3, 1e-6]])
        gp = MiDerivGP(X, y, dY, args.kernel, grad_noise=1e-2)
        bound = _measure(gp, theta, args.reps)
        gp.close()
        Xp = rng.random((N, d))
        plain_gp = MiGP(Xp, np.sin(Xp @ w), args.kernel)
        plain = _measure(plain_gp, theta, args.reps)
        plain_gp.close()
        share = (bound["assemble_ms"] + bound["contract_ms"]) / bound["lml_grad_ms"]
        print(json.dumps({"n": n, "d": d, "N": N, "tile_columns": (N + 127) // 128, "kernel": args.kernel, "bound": bound, "plain": plain,
                          "new_kernels_share_of_evaluation": share}))


if __name__ == "__main__":
    main()
