"""Times of the sparse inducing-point bound (MiSparseGP: mi_gp_sparse_bound_grad) on one MI355X, one JSON line per (n, m):

  value_ms / grad_ms   the bound alone (pass 1 and the algebra of F) and the bound with its gradient, host clock around calls
                       that return synchronised, best and median of --reps
  exact_ms             MiGP.lml_grad on the same data in the same run (--exact; n up to 32768)
  phases (--phases)    one full chunk's launches in isolation through the block-level entry points with the shapes the object
                       uses -- the cross-assembly, the blocked solve, the Psi update (lower-trapezoid GEMM, transa = 1), the T rows
                       (chunk x m x m GEMM) -- by device events, times the number of chunks; what is left of value_ms is the m x m
                       algebra of F, what is left of grad_ms - value_ms the contraction plus the gradient's m x m algebra
  model                10 n m^2 flops per gradient evaluation at the Psi update's measured rate

The contraction kernel's own time comes from a kernel trace of `--once` runs (rocprofv3 --kernel-trace --stats, a run of its
own): sparse_contract_kernel against grad_contract_kernel of an exact evaluation with as many pairs, n m = N (N + 1) / 2."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def problem(n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.random((n, d))
    y = np.sin(3.0 * X.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    return X, (y - y.mean()) / y.std()


def theta_for(kernel, d):
    nk = len(kernel.replace("*", "+").split("+"))
    ls = np.linspace(0.4, 1.5, d) * np.sqrt(max(d, 2) / 2.0)
    return np.concatenate([np.tile(ls, nk), np.full(nk, 1.7), np.full(nk, 2.5), [1e-2, 1e-6]])


def timed(fn, reps):
    import torch

    fn()  # warm-up: code objects, allocations
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return min(out), float(np.median(out))


def chunk_phases(sp, theta, reps):
    """ms of one full chunk's launches in isolation: assembly, solve, Psi update, T rows"""
    import torch

    from andvaranaut_amd import _lib

    lib, dev = _lib.load(), sp.dev  # (the block-level entry points are libmi_gp.so's)
    mp, c, d = (sp.m + 127) // 128 * 128, sp.chunk, sp.d
    ntm = mp // 128
    st = torch.cuda.current_stream(dev).cuda_stream
    ids = (ctypes.c_int * 8)(*[_lib.KERNEL_IDS[k] for k in sp.kerns] + [0] * (8 - sp.nkern))
    ops = (ctypes.c_int * 8)(*[_lib.OP_IDS[o] for o in sp.ops] + [0] * (8 - len(sp.ops)))
    th = torch.from_numpy(theta).to(dev)
    W = torch.zeros((c, mp), dtype=torch.float64, device=dev)
    T = torch.zeros((c, mp), dtype=torch.float64, device=dev)
    Psi = torch.zeros((mp, mp), dtype=torch.float64, device=dev)
    L = torch.zeros((mp, mp), dtype=torch.float64, device=dev)
    dinv = torch.zeros(ntm * 128 * 128, dtype=torch.float64, device=dev)
    info = torch.zeros(4, dtype=torch.int32, device=dev)
    rows = min(c, sp.n)

    def assemble(out, X1, n1, n2, rp, cp, noise_form, row0):
        return lib.mi_gp_assemble_block(d, sp.nkern, ids, ops, th.data_ptr(), X1, n1, sp.Z_t.data_ptr(), n2, row0, 0, out.data_ptr(),
                                        mp, rp, cp, noise_form, st)

    # Kuu + its factor and leaf inverses, as the solve's operand
    assert assemble(L, sp.Z_t.data_ptr(), sp.m, sp.m, mp, mp, 4, 0) == 0
    assert lib.mi_gp_chol_panel(L.data_ptr(), mp, ntm, ntm, dinv.data_ptr(), info.data_ptr(), 0, st) == 0
    steps = {
        "assemble": lambda: assemble(W, sp.X_t.data_ptr(), rows, sp.m, c, mp, 0, 1 << 30),
        "solve": lambda: lib.mi_gp_trsm_block(L.data_ptr(), mp, dinv.data_ptr(), 0, ntm, W.data_ptr(), mp, c, st),
        "psi_gemm": lambda: lib.mi_gp_gemm_f64(1, 0, mp, mp, c, 1.0, W.data_ptr(), mp, W.data_ptr(), mp, 1.0, Psi.data_ptr(), mp, 1, 0, 1,
                                               0, 0, 0, st),
        "t_gemm": lambda: lib.mi_gp_gemm_f64(0, 0, c, mp, mp, 1.0, W.data_ptr(), mp, Psi.data_ptr(), mp, 0.0, T.data_ptr(), mp, 0, 0, 1,
                                             0, 0, 0, st),
    }
    out = {}
    for name, fn in steps.items():
        assert fn() == 0, (name, lib.mi_gp_last_global_error())
        torch.cuda.synchronize()
        best = np.inf
        for _ in range(reps):
            W.normal_() if name != "assemble" else None  # (a solve in place must not run away over repetitions)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1))
        out[name] = best
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[16384])
    ap.add_argument("--m", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--kernel", default="Matern52")
    ap.add_argument("--chunk", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--exact", action="store_true")
    ap.add_argument("--phases", action="store_true")
    ap.add_argument("--once", action="store_true", help="one warm-up and one gradient evaluation per (n, m): for a kernel trace")
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "bench_sparse needs the MI355X"
    from andvaranaut_amd import MiGP, MiSparseGP

    for n in a.n:
        X, y = problem(n, a.d, seed=n)
        theta = theta_for(a.kernel, a.d)
        exact = None
        if a.exact and n <= 32768:
            gp = MiGP(X, y, a.kernel, device=0)
            if a.once:
                gp.lml_grad(theta), gp.lml_grad(theta)
            else:
                exact = timed(lambda: gp.lml_grad(theta), a.reps)
            gp.close()
        for m in a.m:
            Z = X[np.sort(np.random.default_rng(m).choice(n, m, replace=False))].copy()
            sp = MiSparseGP(X, y, Z, a.kernel, device=0, chunk=a.chunk)
            F, g = sp.lml_grad(theta)
            rec = {"n": n, "m": m, "d": a.d, "kernel": a.kernel, "chunk": sp.chunk, "info": sp.info, "F": F}
            if a.once:
                sp.lml_grad(theta)
            else:
                rec["value_ms"], rec["value_median_ms"] = timed(lambda: sp.bound(theta), a.reps)
                rec["grad_ms"], rec["grad_median_ms"] = timed(lambda: sp.lml_grad(theta), a.reps)
                if exact is not None:
                    rec["exact_ms"], rec["exact_median_ms"] = exact
                if a.phases:
                    ph = chunk_phases(sp, theta, a.reps)
                    nch = -(-n // sp.chunk)
                    rec["chunks"] = nch
                    rec["chunk_phase_ms"] = ph
                    pass1 = nch * (ph["assemble"] + ph["solve"] + ph["psi_gemm"])
                    pass2 = nch * (ph["assemble"] + ph["solve"] + ph["t_gemm"])
                    rec["pass1_ms"], rec["pass2_without_contraction_ms"] = pass1, pass2
                    rec["value_rest_ms"] = rec["value_ms"] - pass1  # v and yy, both factorisations, LB^-T, c, the scalars
                    rec["grad_rest_ms"] = rec["grad_ms"] - rec["value_ms"] - pass2  # the contraction and the gradient's m x m algebra
                    mp = (m + 127) // 128 * 128
                    rate = (mp * (mp + 128)) * sp.chunk / (ph["psi_gemm"] * 1e-3)  # flops / s of the lower-trapezoid update
                    rec["psi_gemm_tflops"] = rate / 1e12
                    rec["model_10nm2_ms"] = 10.0 * n * m * m / rate * 1e3
            sp.close()
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
