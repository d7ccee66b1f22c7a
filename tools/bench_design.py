"""Times the design call (options 56 / 57 of mi_gp_set_option behind mi_gp_predict_cov) and the same selection built from the
calls that existed before it, in one run, and prints one JSON line per configuration.

  python tools/bench_design.py --n 4096 16384 --mc 8192 --mr 2048 --b 16 128 --d 16

What is measured directly: the whole call (host clock around the C entry point, buffers allocated before, best of --reps) for each
b, for Mr reference points and for Mr = 0; a device-to-device copy of Mc x Mr and of padded n x Mc doubles.  What is derived from
those: the step time (t[b_hi] - t[b_lo]) / (b_hi - b_lo), the setup t[b_lo] - b_lo * step, the candidate-column pass as the step of
the Mr = 0 call (column + the v update) and the fused pass as the difference of the two steps.  The existing route -- per round
mi_gp_predict for the candidates' and the references' rows of A, one GEMM G = K(C, R) - A_C A_R^T (mi_gp_gemm_f64), the scores in
NumPy, mi_gp_append of the chosen point -- runs --rounds rounds and is extrapolated linearly to b."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--mc", type=int, default=8192)
    ap.add_argument("--mr", type=int, default=2048)
    ap.add_argument("--b", type=int, nargs=2, default=[16, 128])
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch

    from andvaranaut_amd import MiGP

    d, Mc, Mr = args.d, args.mc, args.mr
    rng = np.random.default_rng(0)
    theta = np.concatenate([np.full(d, 0.4 * np.sqrt(d)), [1.3], [1.0], [1e-3, 1e-6]])
    C, R = rng.random((Mc, d)), rng.random((Mr, d))
    for n in args.n:
        X = rng.random((n, d))
        y = np.sin(X.sum(1))
        gp = MiGP(X, y, "Matern52", device=0, capacity=n + 128)
        assert gp.factor(theta) == 0
        dev = gp.dev
        mcp, mrp = gp._padded(Mc), gp._padded(Mr)
        xn = torch.from_numpy(np.concatenate([C, R])).to(dev)
        work = torch.empty((mcp + mrp, gp.lda), dtype=torch.float64, device=dev)
        G = torch.empty((mcp, mrp), dtype=torch.float64, device=dev)
        out = torch.empty(Mc + 2 * max(args.b) + 1, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)

        def call(b, mr):
            gp.set_option(57, mr)
            gp.set_option(56, b)
            try:
                best = np.inf
                for _ in range(args.reps + 1):  # (the first repetition allocates the handle's scratch)
                    t0 = time.perf_counter()
                    r = gp.lib.mi_gp_predict_cov(gp.h, xn.data_ptr(), Mc + mr, work.data_ptr(), gp.lda, out.data_ptr(),
                                                 G.data_ptr() if mr else None, mrp, 1)
                    dt = time.perf_counter() - t0
                    assert r == 0, gp.last_error()
                    best = min(best, dt)
                return best
            finally:
                gp.set_option(56, 0)

        def copy_rate(rows, cols):
            a = torch.empty((rows, cols), dtype=torch.float64, device=dev).normal_()
            bb = torch.empty_like(a)
            best = np.inf
            for _ in range(5):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                bb.copy_(a)
                torch.cuda.synchronize(dev)
                best = min(best, time.perf_counter() - t0)
            return 16.0 * rows * cols / best

        b_lo, b_hi = args.b
        t = {(b, mr): call(b, mr) for b in (b_lo, b_hi) for mr in (Mr, 0)}
        step = (t[b_hi, Mr] - t[b_lo, Mr]) / (b_hi - b_lo)
        step0 = (t[b_hi, 0] - t[b_lo, 0]) / (b_hi - b_lo)
        res = dict(n=n, Mc=Mc, Mr=Mr, d=d, kernel="Matern52",
                   call_s={f"b{b}": t[b, Mr] for b in (b_lo, b_hi)}, call_var_s={f"b{b}": t[b, 0] for b in (b_lo, b_hi)},
                   setup_s=t[b_lo, Mr] - b_lo * step, step_s=step, column_step_s=step0, fused_step_s=step - step0,
                   fused_GBps=16.0 * Mc * Mr / max(step - step0, 1e-12) / 1e9, column_GBps=8.0 * gp.np_ * Mc / max(step0, 1e-12) / 1e9,
                   copy_McxMr_GBps=copy_rate(Mc, Mr) / 1e9, copy_npxMc_GBps=copy_rate(gp.np_, Mc) / 1e9)

        # the existing route, a few rounds: A rows by mi_gp_predict, G by mi_gp_gemm_f64, scores in NumPy, mi_gp_append
        il = torch.from_numpy(1.0 / theta[:d]).to(dev)
        xc, xr = xn[:Mc] * il, xn[Mc:] * il
        r = torch.sqrt(torch.clamp(torch.cdist(xc, xr) ** 2, min=0) + 1e-12)
        Kcr = torch.zeros((mcp, mrp), dtype=torch.float64, device=dev)
        Kcr[:Mc, :Mr] = theta[d] * (1 + np.sqrt(5) * r + 5.0 / 3.0 * r * r) * torch.exp(-np.sqrt(5) * r)
        mu = torch.empty(max(Mc, Mr), dtype=torch.float64, device=dev)
        var = torch.empty(max(Mc, Mr), dtype=torch.float64, device=dev)
        work2 = torch.empty((mrp, gp.lda), dtype=torch.float64, device=dev)
        alive = np.ones(Mc, dtype=bool)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.rounds):
            lda, npad = gp.lda, gp.np_  # (append may move both)
            if work.shape[1] != lda:
                work = torch.empty((mcp + mrp, lda), dtype=torch.float64, device=dev)
                work2 = torch.empty((mrp, lda), dtype=torch.float64, device=dev)
            assert gp.lib.mi_gp_predict(gp.h, xn.data_ptr(), Mc, work.data_ptr(), lda, mu.data_ptr(), var.data_ptr(), 1) == 0
            v = var[:Mc].cpu().numpy()
            assert gp.lib.mi_gp_predict(gp.h, xn[Mc:].data_ptr(), Mr, work2.data_ptr(), lda, mu.data_ptr(), var.data_ptr(), 1) == 0
            G.copy_(Kcr)
            assert gp.lib.mi_gp_gemm_f64(0, 1, mcp, mrp, npad, -1.0, work.data_ptr(), lda, work2.data_ptr(), lda, 1.0, G.data_ptr(), mrp,
                                         0, 0, 1, 0, 0, 0, None) == 0
            torch.cuda.synchronize(dev)
            Gh = G[:Mc, :Mr].cpu().numpy()
            score = np.where(alive, np.einsum("ij,ij->i", Gh, Gh) / (Mr * v), -np.inf)
            p = int(np.argmax(score))
            alive[p] = False
            assert gp.append(C[p : p + 1], np.zeros(1)) == 0
        per_round = (time.perf_counter() - t0) / args.rounds
        res.update(existing_round_s=per_round, existing_rounds_timed=args.rounds,
                   existing_extrapolated_s={f"b{b}": b * per_round for b in (b_lo, b_hi)})
        print(json.dumps(res), flush=True)
        gp.close()
        del work, work2, G, Kcr


if __name__ == "__main__":
    main()
