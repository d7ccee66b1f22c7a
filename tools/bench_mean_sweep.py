"""Time of the matrix-free mean sweep (option 53 of mi_gp_set_option) against the routes it replaces, on ONE handle per size:

  * the sweep's mean against mi_gp_predict_u (MiGP.predict(via_inverse=True)'s call, in its chunks of 16384 points) at
    m = 4096, 65536 and 1e6 query points;
  * the sweep's mean + gradient against mi_gp_predict_grad (option 53 = 0) at m = 1024 (its per-point launches make a larger m
    pointless).

N in --sizes (default 1024 4096 16384), d = 2 and 16, Matern52 and the three-component RBF+Matern52*Matern32.  Every call is
the raw C call on device-resident buffers -- it returns with the stream synchronised -- inside a host clock; one warm-up per
shape, then --reps alternating repetitions of the two routes, the median of each.  Beside every measured ratio stands the
ratio of the flop counts below (counts from shapes, not measurements).  Each size runs in a child process under its own time
limit; the first child that fails ends the run.

    timeout -k 10 1100 python tools/bench_mean_sweep.py [--sizes 1024 4096 16384] [--reps 3] [--out profiles/mean_sweep_bench.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("Matern52", "RBF+Matern52*Matern32")
DIMS = (2, 16)
MEAN_POINTS = (4096, 65536, 1000000)
GRAD_POINTS = 1024
CHUNK = 16384          # MiGP.predict's chunk of points per mi_gp_predict_u call
COMP_FLOPS = 40        # value and derivative of one component at one pair: exp, root, polynomial (a count, ~ +-10)


def sweep_flops(n, d, nk, m, grad):
    """The sweep's arithmetic: per pair and component 3 operations per staged dimension for r2 (subtract, scale, multiply-add:
    the window is 4, 16 or 32 dimensions) and the component itself; with the gradient nk + 2 more per dimension."""
    w = 4 if d <= 4 else 16 if d <= 16 else 32
    per = nk * (3 * w + COMP_FLOPS) + 2 * nk
    if grad:
        per += (nk + 2) * w + 3 * nk
    return float(m) * n * per


def predict_u_flops(n, d, nk, m):
    """mi_gp_predict_u: the cross-covariance rows (expansion form: 2 d + the component per pair), the triangular-k GEMM K* U
    (n^2 / 2 multiply-adds per point: n^2 operations) and the reduction (4 n)."""
    return float(m) * (n * (nk * (2 * d + COMP_FLOPS)) + float(n) * n + 4.0 * n)


def predict_grad_flops(n, d, nk, m):
    """mi_gp_predict_grad at m > 16: the blocked solve (n^2), one trmv over U per point (n^2) and the scalar gradient kernel."""
    return float(m) * (2.0 * float(n) * n + n * (nk * (3 * d + COMP_FLOPS) + 4 * nk * d))


def _ms(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def child(N, reps):
    import torch

    from andvaranaut_amd import MiGP
    from oracle import gp_oracle as orc

    assert torch.cuda.is_available(), "bench_mean_sweep needs the MI355X"
    rows = []
    for d in DIMS:
        X, y = orc.synth_problem(N, d, seed=1)
        rng = np.random.default_rng(2)
        xq = torch.from_numpy(rng.random((max(MEAN_POINTS), d))).to("cuda:0")
        for kernel in KERNELS:
            nk = kernel.count("+") + kernel.count("*") + 1
            theta = orc.synth_theta(d, nkern=nk, gv=1e-4)
            gp = MiGP(X, y, kernel, device=0)
            lib, h = gp.lib, gp.h
            assert gp.factor(theta) == 0
            work = torch.empty((2 * CHUNK, gp.lda), dtype=torch.float64, device="cuda:0")
            mean = torch.empty(max(MEAN_POINTS), dtype=torch.float64, device="cuda:0")
            mean_u = torch.empty(max(MEAN_POINTS), dtype=torch.float64, device="cuda:0")
            var = torch.empty(max(MEAN_POINTS), dtype=torch.float64, device="cuda:0")
            dmean = torch.empty((GRAD_POINTS, d), dtype=torch.float64, device="cuda:0")
            dvar = torch.empty((GRAD_POINTS, d), dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()

            def sweep(m, grad):
                gp.set_option(53, 1)
                r = lib.mi_gp_predict_grad(h, xq.data_ptr(), m, None, 0, mean.data_ptr(), None, 0, dmean.data_ptr() if grad else None, None)
                gp.set_option(53, 0)
                assert r == 0, gp.last_error()

            def via_u(m):
                for s in range(0, m, CHUNK):
                    mc = min(CHUNK, m - s)
                    r = lib.mi_gp_predict_u(h, xq.data_ptr() + 8 * s * d, mc, work.data_ptr(), gp.lda, mean_u.data_ptr() + 8 * s,
                                            var.data_ptr() + 8 * s, 1)
                    assert r == 0, gp.last_error()

            def full_grad(m):
                r = lib.mi_gp_predict_grad(h, xq.data_ptr(), m, work.data_ptr(), gp.lda, mean_u.data_ptr(), var.data_ptr(), 1,
                                           dmean.data_ptr(), dvar.data_ptr())
                assert r == 0, gp.last_error()

            for m in MEAN_POINTS:
                sweep(min(m, 4096), False)  # warm-up (code objects; U and alpha resident)
                via_u(min(m, 4096))
                ts, tu = [], []
                for _ in range(reps):
                    ts.append(_ms(lambda: sweep(m, False)))
                    tu.append(_ms(lambda: via_u(m)))
                torch.cuda.synchronize()
                scale = float(np.abs(mean_u[:m].cpu().numpy()).max())
                diff = float(np.abs((mean[:m] - mean_u[:m]).cpu().numpy()).max())
                fs, fu = sweep_flops(N, d, nk, m, False), predict_u_flops(N, d, nk, m)
                rows.append(dict(N=N, d=d, kernel=kernel, m=m, what="mean", sweep_ms=float(np.median(ts)), parent_ms=float(np.median(tu)),
                                 parent="mi_gp_predict_u", sweep_ms_all=ts, parent_ms_all=tu, ratio=float(np.median(tu) / np.median(ts)),
                                 flop_ratio=fu / fs, sweep_gflops=fs / np.median(ts) * 1e-6, max_abs_diff=diff, max_abs_mean=scale))
                print(json.dumps(rows[-1]), flush=True)
            m = GRAD_POINTS
            sweep(m, True)
            full_grad(m)
            ts, tg = [], []
            for _ in range(reps):
                ts.append(_ms(lambda: sweep(m, True)))
                tg.append(_ms(lambda: full_grad(m)))
            fs, fg = sweep_flops(N, d, nk, m, True), predict_grad_flops(N, d, nk, m)
            rows.append(dict(N=N, d=d, kernel=kernel, m=m, what="mean+gradient", sweep_ms=float(np.median(ts)),
                             parent_ms=float(np.median(tg)), parent="mi_gp_predict_grad", sweep_ms_all=ts, parent_ms_all=tg,
                             ratio=float(np.median(tg) / np.median(ts)), flop_ratio=fg / fs, sweep_gflops=fs / np.median(ts) * 1e-6))
            print(json.dumps(rows[-1]), flush=True)
            gp.close()
            del work, mean, mean_u, var, dmean, dvar
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096, 16384])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mean_sweep_bench.json"))
    ap.add_argument("--limit", type=int, default=330, help="seconds per size")
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps)
        return
    rows = []
    for N in a.sizes:
        p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", str(N), "--reps",
                            str(a.reps)], stdout=subprocess.PIPE, text=True)
        rows += [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
        with open(a.out, "w") as f:
            json.dump({"rows": rows, "complete": False}, f, indent=1)
        if p.returncode != 0:
            print(f"N = {N}: the child ended with status {p.returncode}; nothing more is started", file=sys.stderr)
            sys.exit(p.returncode)
    with open(a.out, "w") as f:
        json.dump({"rows": rows, "complete": True}, f, indent=1)
    for r in rows:
        print(f"N={r['N']:6d} d={r['d']:2d} {r['kernel']:22s} m={r['m']:8d} {r['what']:14s} sweep {r['sweep_ms']:10.3f} ms  {r['parent']} "
              f"{r['parent_ms']:10.3f} ms  ratio {r['ratio']:8.2f}  flop ratio {r['flop_ratio']:8.2f}")


if __name__ == "__main__":
    main()
