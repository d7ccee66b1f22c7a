"""Times of the sparse bound's gradient by the inducing locations (MiSparseGP(z_grad=True): mi_gp_sparse_bound_grad with
zgrad_slabs >= 1) on one MI355X, one JSON line per (n, m), in the manner of tools/bench_sparse.py:

  grad_ms    the bound with its theta gradient on an object without the Z gradient (zgrad_slabs = 0: the path as it was)
  zgrad_ms   the bound with its theta gradient and dF/dZ, same data, same run; host clock around calls that return synchronised,
             best and median of --reps
  slabs      the slabs per full chunk the library's rule gives (--slabs caps them)

The new kernel's own time comes from a kernel trace of `--once` runs (rocprofv3 --kernel-trace --stats, a run of its own):
sparse_zgrad_kernel against sparse_contract_kernel on the same pairs, and grad_x_kernel on Kuu's m (m + 1) / 2 pairs.

--facade: the tutorial function of tests/test_gpu_sparse_zgrad.py (n = 600, d = 2, Matern52): the bound of a MAP fit on m fixed
k-means++ points, of the fit that goes on from there with optimize_inducing=True, and of fixed-Z fits at growing m, to read off
the m at which fixed points reach the optimised ones' bound."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_sparse import problem, theta_for, timed  # noqa: E402


def facade(m, more):
    import scipy.stats as st

    from andvaranaut_amd import GPMCMC, normal, uniform

    def fun(x):
        return np.array([x[0] ** 2 - x[0] - x[1] ** 2 * x[0] + x[1]])

    priors = [st.uniform(loc=0, scale=2), st.uniform(loc=1, scale=0.5)]
    g = GPMCMC(kernel="Matern52", noise=True, xconrevs=[uniform(priors[0]), normal(priors[1])], yconrevs=[None], nx=2, ny=1,
               priors=priors, target=fun, parallel=False, nproc=1, verbose=False)
    g.sample(nsamps=600, seed=1)

    def fit(mm, **kw):
        data = g.fit(method="map", inducing=mm, inducing_seed=3, return_data=True, **kw)
        return {"m": mm, "logp": data["logp"], "F": g.gp.bound(g._theta_from_hypers(g.hypers, 1e-6)), "nfev": data["nfev"]}

    fixed = fit(m)
    opt = fit(m, optimize_inducing=True, start=dict(g.hypers))
    print(json.dumps({"facade": "fixed", **fixed}), flush=True)
    print(json.dumps({"facade": "optimised", **opt}), flush=True)
    for mm in more:
        print(json.dumps({"facade": "fixed", **fit(mm)}), flush=True)
    g.change_model()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[16384])
    ap.add_argument("--m", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--kernel", default="Matern52")
    ap.add_argument("--chunk", type=int, default=None)
    ap.add_argument("--slabs", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="one warm-up and one evaluation with dF/dZ per (n, m): for a kernel trace")
    ap.add_argument("--facade", type=int, nargs="*", default=None, help="m of the facade problem, then the larger fixed m to try")
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "bench_sparse_zgrad needs the MI355X"
    from andvaranaut_amd import MiSparseGP

    if a.facade is not None:
        facade(a.facade[0] if a.facade else 20, a.facade[1:])
        return
    for n in a.n:
        X, y = problem(n, a.d, seed=n)
        theta = theta_for(a.kernel, a.d)
        for m in a.m:
            Z = X[np.sort(np.random.default_rng(m).choice(n, m, replace=False))].copy()
            spz = MiSparseGP(X, y, Z, a.kernel, device=0, chunk=a.chunk, z_grad=True, zgrad_slabs=a.slabs)
            F, g, gz = spz.lml_grad_z(theta)
            cnt, cap = min(spz.chunk, n), 1024 if a.slabs is None else a.slabs
            slabs = min(-(-cnt // 64), cap, -(-1024 // -(-m // 64)))  # (the 64 MB rule does not bind at these shapes)
            rec = {"n": n, "m": m, "d": a.d, "kernel": a.kernel, "chunk": spz.chunk, "slabs": slabs, "info": spz.info, "F": F,
                   "max_abs_dFdZ": float(np.max(np.abs(gz)))}
            if a.once:
                spz.lml_grad_z(theta)
            else:
                sp = MiSparseGP(X, y, Z, a.kernel, device=0, chunk=a.chunk)
                F0, g0 = sp.lml_grad(theta)
                assert F0 == F and np.array_equal(g0, g)
                rec["grad_ms"], rec["grad_median_ms"] = timed(lambda: sp.lml_grad(theta), a.reps)
                rec["zgrad_ms"], rec["zgrad_median_ms"] = timed(lambda: spz.lml_grad_z(theta), a.reps)
                rec["zgrad_over_grad"] = rec["zgrad_ms"] / rec["grad_ms"]
                sp.close()
            spz.close()
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
