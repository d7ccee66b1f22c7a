"""Joint conditional and posterior draws: wall time of mi_gp_predict_cov (mean + Sigma at m points) and mi_gp_sample_cov
(L_Sigma + s draws) at the resident factor, RBF, d = 8, (N, m, s) in {(2048, 1024, 1), (4096, 4096, 16), (4096, 10000, 1)},
next to the same algebra in SciPy on the host (host_total_ms: cholesky of K, solve_triangular, Kss - A^T A, cholesky of Sigma,
mean + Z L^T; host_sample_ms: the last two).  Median of --reps
after one warm-up; flop counts N^2 m (solve), m^2 N (Sigma), m^3 / 3 (L_Sigma), m^2 s (draws).  Writes JSON to
profiles/bench_predict_joint.json (or --out).

  python tools/bench_predict_joint.py [--cases 2048:1024:1,4096:4096:16] [--reps 3] [--no-host]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_time(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def _rbf(A, B, ls, kv):
    Xa, Xb = A / ls, B / ls
    r2 = np.clip(-2.0 * Xa @ Xb.T + (np.sum(Xa ** 2, 1)[:, None] + np.sum(Xb ** 2, 1)[None, :]), 0.0, np.inf)
    return kv * np.exp(-0.5 * r2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="2048:1024:1,4096:4096:16,4096:10000:1")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_predict_joint.json"))
    a = ap.parse_args()
    import scipy.linalg as sla
    import torch

    from andvaranaut_amd import MiGP

    d, kv, gv, jit = 8, 1.7, 1e-3, 1e-6
    ls = np.full(d, 0.8)
    theta = np.concatenate([ls, [kv], [1.0], [gv, jit]])
    rng = np.random.default_rng(0)
    records = []
    for case in a.cases.split(","):
        N, m, s = (int(v) for v in case.split(":"))
        X = rng.random((N, d))
        y = np.sin(3.0 * X.sum(1))
        Xn = rng.random((m, d))
        gp = MiGP(X, y, "RBF", need_grad=False)
        assert gp.factor(theta) == 0
        mp = (m + 127) // 128 * 128
        need = int(gp.lib.mi_gp_sample_cov_work(m, s))
        with torch.cuda.device(gp.dev):
            work = torch.empty(need, dtype=torch.float64, device=gp.dev)
            draws = torch.empty((s, m), dtype=torch.float64, device=gp.dev)
        state = {}

        def dev_cov():
            state["mu"], state["cov"] = gp._joint_device(Xn, False)

        def dev_sample():
            dev_cov()  # (sample_cov overwrites Sigma: rebuild it, timed separately below)
            torch.cuda.synchronize(gp.dev)
            t0 = time.perf_counter()
            r = gp.lib.mi_gp_sample_cov(gp.h, state["cov"].data_ptr(), mp, m, state["mu"].data_ptr(), 0.0, s, 1, 0,
                                        draws.data_ptr(), m, work.data_ptr(), need)
            state["t"] = time.perf_counter() - t0
            assert r == 0, gp.last_error()

        t_cov = _median_time(dev_cov, a.reps)
        ts = []
        dev_sample()
        for _ in range(a.reps):
            dev_sample()
            ts.append(state["t"])
        t_smp = float(np.median(ts))
        rec = {"N": N, "m": m, "s": s, "predict_cov_ms": 1e3 * t_cov, "sample_cov_ms": 1e3 * t_smp,
               "predict_cov_gflops": (N * N * m + m * m * N) / t_cov / 1e9,
               "sample_cov_gflops": (m ** 3 / 3 + m * m * s) / t_smp / 1e9}
        if not a.no_host:
            K = _rbf(X, X, ls, kv) + (jit + gv) * np.eye(N)

            def host():
                L = sla.cholesky(K, lower=True)
                A = sla.solve_triangular(L, _rbf(X, Xn, ls, kv), lower=True)
                S = _rbf(Xn, Xn, ls, kv) - A.T @ A + jit * np.eye(m)
                mu = A.T @ sla.solve_triangular(L, y, lower=True)
                t0 = time.perf_counter()
                LS = sla.cholesky(S, lower=True)
                D = mu[None, :] + np.random.default_rng(1).standard_normal((s, m)) @ LS.T
                return time.perf_counter() - t0, D

            t0 = time.perf_counter()
            t_hs, _ = host()
            rec["host_total_ms"] = 1e3 * (time.perf_counter() - t0)
            rec["host_sample_ms"] = 1e3 * t_hs
            rec["host_threads"] = os.environ.get("OMP_NUM_THREADS")
        print(json.dumps(rec), flush=True)
        records.append(rec)
        gp.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
