"""A/B of ONE inverse_opt potential evaluation (value + gradient, nobs = 1, d = 16, Matern-5/2): the refactorising path
(MiGP.update_data + lml_grad_data on the N + 1 rows) against MiGP.logpdf on the resident N-row factor, at N = 1024, 4096 and
16384 -- same process, warm, the two paths alternating, medians over --reps calls (host clock around calls that end in a
stream synchronisation).  Beside them the time of MiGP.predict_grad at one point on the same factor: the per-point passes over
U that a small-k route of mi_gp_logpdf would use.  Then the split of the new call by phase from the handle's HIP events
(profiling level 1, a run of its own: the events add to the call).  Prints one JSON line per size.

    timeout -k 10 900 python tools/ab_logpdf.py [--sizes 1024 4096 16384] [--reps 50] [--out profiles/logpdf_ab.jsonl]
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

HBM_BYTES_PER_S = 6.29e12  # measured copy bandwidth of the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096, 16384])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ab_logpdf.py measures on the GPU: none found")
    lines = []
    for N in a.sizes:
        X, y = orc.synth_problem(N + 1, a.d, seed=1)
        theta = orc.synth_theta(a.d, gv=0.0, jitter=0.0)  # (inverse_opt: the noise enters through the diagonal)
        diag = np.full(N + 1, np.sqrt(1e-4 + 1e-6))
        rng = np.random.default_rng(0)
        trial = rng.random((a.reps + 3, a.d))
        old = MiGP(X, y, "Matern52", device=0)
        old.set_diag(diag)
        new = MiGP(X[:N], y[:N], "Matern52", device=0)
        new.set_diag(diag[:N])
        assert new.factor(theta) == 0
        xaug = X.copy()

        def call_old(x):
            xaug[-1] = x
            old.update_data(X=xaug)
            val, _, _, gx = old.lml_grad_data(theta, want_x=True)
            return val, gx[-1]

        def call_new(x):
            val, gx, _ = new.logpdf(theta, x[None, :], y[N:], diag=diag[N:])
            return val, gx[0]

        logdet, quad = new.lml_parts()
        lml_n = -0.5 * N * np.log(2.0 * np.pi) - 0.5 * quad - logdet
        t_old, t_new, dv, dg = [], [], 0.0, 0.0
        for i, x in enumerate(trial):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vo, go = call_old(x)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            vn, gn = call_new(x)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if i >= 3:  # (warm: the first calls form U, size the work blocks and load the code objects)
                t_old.append(1e3 * (t1 - t0))
                t_new.append(1e3 * (t2 - t1))
            dv = max(dv, abs(lml_n + vn - vo) / max(abs(vo), 1.0))
            dg = max(dg, float(np.max(np.abs(gn - go)) / np.max(np.abs(go))))
        # yardstick for a per-point route: mi_gp_predict_grad at ONE point runs one trmv_upper_t and one trmv_upper pass over U
        # (the two products a k <= 16 route of mi_gp_logpdf would take instead of its two GEMMs) plus its own small kernels
        t_pg = []
        for x in trial:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            new.predict_grad(theta, x[None, :], refactor=False)
            torch.cuda.synchronize()
            t_pg.append(1e3 * (time.perf_counter() - t0))
        t_pg = t_pg[3:]
        # the new call by phase
        new.set_profiling(1)
        ph = []
        for x in trial[:20]:
            call_new(x)
            tm = new.timers()
            ph.append([tm["logpdf_block_ms"], tm["logpdf_weights_ms"], tm["logpdf_grad_ms"]])
        new.set_profiling(0)
        ph = np.median(np.array(ph), axis=0)
        npad = new.np_
        res = {"N": N, "d": a.d, "kernel": "Matern52", "nobs": 1, "reps": a.reps, "device": torch.cuda.get_device_name(0),
               "refactor_path_ms": float(np.median(t_old)), "refactor_path_min_max_ms": [min(t_old), max(t_old)],
               "logpdf_ms": float(np.median(t_new)), "logpdf_min_max_ms": [min(t_new), max(t_new)],
               "speedup": float(np.median(t_old) / np.median(t_new)),
               "predict_grad_one_point_ms": float(np.median(t_pg)),
               "phase_conditional_block_ms": float(ph[0]), "phase_weights_ms": float(ph[1]), "phase_grad_kernel_ms": float(ph[2]),
               # two passes over U (K21 U11 in the conditional block, L21 U11^T in the weights), n^2 * 8 B each
               "floor_two_passes_over_U_ms": 1e3 * 2.0 * npad * npad * 8.0 / HBM_BYTES_PER_S,
               "max_rel_value_diff": dv, "max_rel_grad_diff": dg}
        print(json.dumps(res), flush=True)
        lines.append(res)
        old.close()
        new.close()
        del old, new
        torch.cuda.empty_cache()
    if a.out:
        with open(os.path.join(ROOT, a.out), "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
