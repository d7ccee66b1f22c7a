"""Times of the sparse bound's gradients by the data (MiSparseGP(data_grad=True): mi_gp_sparse_bound_grad behind
mi_gp_sparse_bind_data_grad) on one MI355X, one JSON line per (n, m), in the manner of tools/bench_sparse_zgrad.py.  All in the
same run, on the same data, host clock around calls that return synchronised, best and median of --reps:

  grad_ms     the bound with its theta gradient on an object without data_grad (libmi_gp_sparse.so: the path as it was)
  zgrad_ms    + dF/dZ on a z_grad object without data_grad
  ygrad_ms    + dF/dy alone (nothing but dF/dy bound: the X kernel does not run), the library call, the outputs left on the device
  xgrad_ms    + dF/dy + dF/dX, the library call
  data_ms     lml_grad_data(theta): the same call and the download of both outputs to the host (n (d + 1) doubles)
  slabs       the slabs per full chunk the library's rule gives dF/dX's kernel (--slabs caps them)

The kernels' own times come from a kernel trace of `--once` runs (rocprofv3 --kernel-trace --stats, a run of its own: one
evaluation with dF/dtheta, dF/dZ, dF/dy and dF/dX per (n, m)): sparse_xgrad_kernel beside sparse_zgrad_kernel and
sparse_contract_kernel on the same pairs in the same trace."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_sparse import problem, theta_for, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[16384, 262144, 1048576])
    ap.add_argument("--m", type=int, nargs="+", default=[1024, 256])
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--kernel", default="Matern52")
    ap.add_argument("--chunk", type=int, default=None)
    ap.add_argument("--slabs", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="one warm-up and one evaluation with every gradient per (n, m): for a kernel trace")
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "bench_sparse_data_grad needs the MI355X"
    from andvaranaut_amd import MiSparseGP

    for n in a.n:
        X, y = problem(n, a.d, seed=n)
        theta = theta_for(a.kernel, a.d)
        for m in a.m:
            Z = X[np.sort(np.random.default_rng(m).choice(n, m, replace=False))].copy()
            spd = MiSparseGP(X, y, Z, a.kernel, device=0, chunk=a.chunk, z_grad=a.once, data_grad=True, xgrad_slabs=a.slabs)
            out = spd.lml_grad_data(theta, want_z=a.once)
            F, g, gy, gx = out[:4]
            cnt, cap = min(spd.chunk, n), 1024 if a.slabs is None else a.slabs
            slabs = min(-(-m // 64), cap, -(-1024 // -(-cnt // 64)))  # (the 64 MB rule does not bind at these shapes)
            rec = {"n": n, "m": m, "d": a.d, "kernel": a.kernel, "chunk": spd.chunk, "slabs": slabs, "info": spd.info, "F": F,
                   "max_abs_dFdy": float(np.max(np.abs(gy))), "max_abs_dFdX": float(np.max(np.abs(gx)))}
            if a.once:
                spd.lml_grad_data(theta, want_z=True)
            else:
                sp = MiSparseGP(X, y, Z, a.kernel, device=0, chunk=a.chunk)
                spz = MiSparseGP(X, y, Z, a.kernel, device=0, chunk=a.chunk, z_grad=True)
                F0, g0 = sp.lml_grad(theta)
                assert F0 == F and np.array_equal(g0, g)
                rec["grad_ms"], rec["grad_median_ms"] = timed(lambda: sp.lml_grad(theta), a.reps)
                rec["zgrad_ms"], rec["zgrad_median_ms"] = timed(lambda: spz.lml_grad_z(theta), a.reps)
                spd._bind_data_grad(False)
                rec["ygrad_ms"], rec["ygrad_median_ms"] = timed(lambda: spd._bound_grad(theta), a.reps)
                spd._bind_data_grad(True)
                rec["xgrad_ms"], rec["xgrad_median_ms"] = timed(lambda: spd._bound_grad(theta), a.reps)
                rec["data_ms"], rec["data_median_ms"] = timed(lambda: spd.lml_grad_data(theta), a.reps)
                rec["xgrad_over_grad"] = rec["xgrad_ms"] / rec["grad_ms"]
                sp.close()
                spz.close()
            spd.close()
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
