"""Time of mi_gp_lml_grad under option 51 = q outputs with option 52 = 0 (independent outputs) and 52 = 1 (the between-output
covariance integrated out) for q in {8, 128} at N = 4096 and 16384 (d = 16, Matern52).  Three repeats per leg (--repeats), each
the median of --evals evaluations, the legs alternated repeat by repeat.  --shared-only times the 52 = 0 legs alone and uses only
what the build before the option has, so the same file can time that build (--package-root: the directory that holds its
andvaranaut_amd/): the 52 = 0 legs of the two builds must agree within the spread of their own repeats.

    timeout -k 10 600 python tools/bench_output_cov.py [--sizes 4096 16384] [--out profiles/output_cov_bench.json]
    timeout -k 10 600 python tools/bench_output_cov.py --shared-only --package-root /path/to/parent --out parent.json"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QS = (8, 128)
REPEATS = 3  # (--repeats: more of them narrow the comparison of two builds)


def _ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def _outputs(X, y, q):
    rng = np.random.default_rng(5)
    cols = [y] + [np.sin(X @ rng.normal(size=X.shape[1]) + rng.uniform(0, 6)) + 0.1 * rng.normal(size=len(y)) for _ in range(q - 1)]
    return np.ascontiguousarray(np.column_stack(cols))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--evals", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=REPEATS)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--shared-only", action="store_true")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "output_cov_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_output_cov.py needs the MI355X: nothing is measured without it")
    sys.path.insert(0, os.path.abspath(a.package_root))
    if ROOT not in sys.path:
        sys.path.append(ROOT)
    from andvaranaut_amd import MiGP
    from oracle import gp_oracle as orc

    theta = orc.synth_theta(a.d, gv=1e-4)
    covs = (0,) if a.shared_only else (0, 1)
    res = {"d": a.d, "kernel": "Matern52", "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "evals_per_repeat": a.evals,
           "legs": "option 52 = 0 only" if a.shared_only else "option 52 = 0 and 1", "sizes": []}
    for N in a.sizes:
        X, y = orc.synth_problem(N, a.d, seed=1)
        gp = MiGP(X, y, "Matern52", device=0)
        Y = _outputs(X, y, max(QS))
        legs = [(q, c) for q in QS for c in covs]

        def select(q, c):
            gp.set_outputs(Y[:, :q])  # (rebinds the data: every leg starts without resident state)
            if not a.shared_only:
                gp.set_output_cov("integrated" if c else "shared")

        for q, c in legs:  # warm-up (the scratch)
            select(q, c)
            gp.lml_grad(theta)
        t = {leg: [] for leg in legs}
        for _ in range(a.repeats):
            for leg in legs:
                select(*leg)
                t[leg].append(float(np.median([_ms(lambda: gp.lml_grad(theta)) for _ in range(a.evals)])))
        row = {"N": N, "lml_grad_ms": {"q%d_cov%d" % leg: {"repeats": v, "median": float(np.median(v)), "spread": max(v) - min(v)}
                                       for leg, v in t.items()}}
        gp.close()
        res["sizes"].append(row)
        print(json.dumps(row))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
