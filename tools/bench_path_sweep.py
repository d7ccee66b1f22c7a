"""Time of the path sweep (options 54 / 55 of mi_gp_set_option) on ONE handle per size:

  (a) the value-only sweep of S = 16 and S = 128 paths, F = 4096 features, at m = 65536 and 1e6 query points against S times the
      mean sweep (option 53) at the same shape -- what S weight vectors cost without the path kernel; d = 2 and 16, Matern52;
  (b) the conditioning call of one draw of 128 paths (condition = 1, m = 0) beside one mi_gp_factor;
  (c) at N = 4096 only: one posterior draw at M = 8192 points through MiGP.draw_paths + evaluate and through
      MiGP.sample_posterior (the M x M route), both end to end from Python.

Every call of (a) and (b) is the raw C call on device-resident buffers -- it returns with the stream synchronised -- inside a
host clock; one warm-up per shape, then --reps alternating repetitions of the two routes, the median of each.  Each size runs
in a child process under its own time limit; the first child that fails ends the run.

    timeout -k 10 1100 python tools/bench_path_sweep.py [--sizes 1024 4096 16384] [--reps 3] [--out profiles/path_sweep_bench.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNEL = "Matern52"
DIMS = (2, 16)
POINTS = (65536, 1000000)
PATHS = (16, 128)
FEATURES = 4096
JOINT_N, JOINT_M = 4096, 8192


def _ms(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def child(N, reps):
    import torch

    from andvaranaut_amd import MiGP, paths
    from oracle import gp_oracle as orc

    assert torch.cuda.is_available(), "bench_path_sweep needs the MI355X"
    F = FEATURES
    for d in DIMS:
        X, y = orc.synth_problem(N, d, seed=1)
        rng = np.random.default_rng(2)
        xq = torch.from_numpy(rng.random((max(POINTS), d))).to("cuda:0")
        theta = orc.synth_theta(d, nkern=1, gv=1e-4)
        gp = MiGP(X, y, KERNEL, device=0)
        lib, h = gp.lib, gp.h
        t_factor = [_ms(lambda: gp.factor(theta)) for _ in range(reps + 1)][1:]
        out = torch.empty(max(PATHS) * max(POINTS), dtype=torch.float64, device="cuda:0")
        ls = theta[:d].reshape(1, d)
        omega, _ = paths.spectral_frequencies([KERNEL], [], ls, theta[d : d + 1], None, F, rng)
        b = rng.random(F) * 2.0 * np.pi
        torch.cuda.synchronize()

        def mean_sweep(m):
            gp.set_option(53, 1)
            r = lib.mi_gp_predict_grad(h, xq.data_ptr(), m, None, 0, out.data_ptr(), None, 0, None, None)
            gp.set_option(53, 0)
            assert r == 0, gp.last_error()

        for S in PATHS:
            ldw = paths.block_ldw(S)
            host = paths.pack_block(omega, b, rng.standard_normal((F, S)) * np.sqrt(2.0 / F), np.sqrt(1e-4) * rng.standard_normal((N, S)), ldw)
            blk = torch.from_numpy(host).to("cuda:0")
            gp.set_option(55, F)

            def path_call(m, condition):
                gp.set_option(54, S)
                r = lib.mi_gp_predict_grad(h, xq.data_ptr() if m else None, m, blk.data_ptr(), ldw, out.data_ptr() if m else None, None,
                                           condition, None, None)
                gp.set_option(54, 0)
                assert r == 0, gp.last_error()

            if S == max(PATHS):  # (b): every repetition conditions a fresh noise draw
                tc = []
                for _ in range(reps + 1):
                    blk.copy_(torch.from_numpy(host))
                    torch.cuda.synchronize()
                    tc.append(_ms(lambda: path_call(0, 1)))
                row = dict(N=N, d=d, kernel=KERNEL, what="conditioning", S=S, F=F, condition_ms=float(np.median(tc[1:])),
                           factor_ms=float(np.median(t_factor)), condition_ms_all=tc[1:], factor_ms_all=t_factor)
                print(json.dumps(row), flush=True)
            for m in POINTS:
                path_call(4096, 0)  # warm-up (code objects; U and alpha resident)
                mean_sweep(4096)
                tp, tm = [], []
                for _ in range(reps):
                    tp.append(_ms(lambda: path_call(m, 0)))
                    tm.append(_ms(lambda: mean_sweep(m)))
                row = dict(N=N, d=d, kernel=KERNEL, what="sweep", S=S, F=F, m=m, path_ms=float(np.median(tp)),
                           mean_sweep_ms=float(np.median(tm)), s_mean_sweeps_ms=float(S * np.median(tm)), path_ms_all=tp,
                           mean_sweep_ms_all=tm, ratio=float(S * np.median(tm) / np.median(tp)))
                print(json.dumps(row), flush=True)
            del blk
        if N == JOINT_N:  # (c)
            Xm = rng.random((JOINT_M, d))
            tj, tw = [], []
            for i in range(reps + 1):
                def pathwise():
                    draw = gp.draw_paths(theta, 1, F, seed=i)
                    draw.evaluate(Xm)
                    draw.close()

                tw.append(_ms(pathwise))
                tj.append(_ms(lambda: gp.sample_posterior(theta, Xm, 1, seed=i)))
            row = dict(N=N, d=d, kernel=KERNEL, what="one draw", M=JOINT_M, F=F, draw_paths_ms=float(np.median(tw[1:])),
                       sample_posterior_ms=float(np.median(tj[1:])), draw_paths_ms_all=tw[1:], sample_posterior_ms_all=tj[1:])
            print(json.dumps(row), flush=True)
        gp.close()
        del out, xq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096, 16384])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_sweep_bench.json"))
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
        if r["what"] == "sweep":
            print(f"N={r['N']:6d} d={r['d']:2d} S={r['S']:3d} m={r['m']:8d} path sweep {r['path_ms']:10.3f} ms  S mean sweeps "
                  f"{r['s_mean_sweeps_ms']:10.3f} ms  ratio {r['ratio']:6.2f}")
        elif r["what"] == "conditioning":
            print(f"N={r['N']:6d} d={r['d']:2d} conditioning of {r['S']} paths {r['condition_ms']:9.3f} ms  mi_gp_factor {r['factor_ms']:9.3f} ms")
        else:
            print(f"N={r['N']:6d} d={r['d']:2d} one draw at M={r['M']}: draw_paths + evaluate {r['draw_paths_ms']:9.3f} ms  sample_posterior "
                  f"{r['sample_posterior_ms']:9.3f} ms")


if __name__ == "__main__":
    main()
