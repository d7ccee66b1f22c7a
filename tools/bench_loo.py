"""Time of mi_gp_lml_grad under option 48 = 0 (log marginal likelihood) and 48 = 1 (leave-one-out objective: the same evaluation
plus the tail of csrc/api_loo.hip) on ONE handle, interleaved, at N = 1024, 4096 and 16384 (d = 16, Matern52), and of the tail's
GEMM alone (mi_gp_gemm_f64 with the tail's arguments on the handle's own buffers): its share of the tail.

    timeout -k 10 900 python tools/bench_loo.py [--sizes 1024 4096 16384] [--reps 7] [--out profiles/loo_bench.json]

--lib PATH times option 0 alone with another build of libmi_gp.so (the parent commit's, which has no option 48) in this process,
--lml-only does the same with this tree's (the two, alternated, are the A/B of option 0 against the parent: interleaved with the
tail's N^3 GEMM the evaluation runs on a warmer chip);
--against PATH (a JSON written by such a run) adds option 0's time there and the ratio to the output."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from andvaranaut_amd import _lib  # noqa: E402
from oracle import gp_oracle as orc  # noqa: E402


def _ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096, 16384])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--lml-only", action="store_true", help="time option 0 alone (no evaluation under option 1 in between)")
    ap.add_argument("--against", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loo_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loo.py needs the MI355X: nothing is measured without it")
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from andvaranaut_amd import MiGP

    base = {}
    if a.against:
        with open(a.against) as f:
            base = {r["N"]: r for r in json.load(f)["sizes"]}
    res = {"d": a.d, "kernel": "Matern52", "device": torch.cuda.get_device_name(0), "reps": a.reps, "lib": a.lib or "this tree", "sizes": []}
    for N in a.sizes:
        X, y = orc.synth_problem(N, a.d, seed=1)
        theta = orc.synth_theta(a.d, gv=1e-4)
        gp = MiGP(X, y, "Matern52", device=0)
        has_loo = gp.get_option(48) is not None and not a.lml_only
        for _ in range(2):  # warm-up (and the tail's vectors)
            gp.lml_grad(theta)
            if has_loo:
                gp.loo_grad(theta)
        t0, t1, tg = [], [], []
        for _ in range(a.reps):  # interleaved: both objectives see the same clocks
            t0.append(_ms(lambda: gp.lml_grad(theta)))
            if has_loo:
                gp.set_option(48, 1)
                t1.append(_ms(lambda: gp.lml_grad(theta)))
                gp.set_option(48, 0)
                # the tail's GEMM alone: G' += B B^T over the lower tiles, k = padded n (the operands' contents do not matter)
                np_, ld = gp.np_, gp.lda
                tg.append(_ms(lambda: gp.lib.mi_gp_gemm_f64(0, 1, np_, np_, np_, 1.0, gp.Z_t.data_ptr(), ld, gp.Z_t.data_ptr(), ld, 1.0,
                                                            gp.K_t.data_ptr(), ld, 1, 0, 1, 0, 0, 0, None)))
                gp.Z_t.zero_()  # (as the tail leaves it)
        r = {"N": N, "lml_grad_ms": float(np.median(t0)), "lml_grad_all": [round(t, 4) for t in t0]}
        if has_loo:
            r["loo_grad_ms"] = float(np.median(t1))
            r["loo_grad_all"] = [round(t, 4) for t in t1]
            r["tail_ms"] = r["loo_grad_ms"] - r["lml_grad_ms"]
            r["tail_over_lml_grad"] = r["tail_ms"] / r["lml_grad_ms"]
            r["tail_gemm_ms"] = float(np.median(tg))
            r["gemm_share_of_tail"] = r["tail_gemm_ms"] / r["tail_ms"]
        if N in base:
            r["lml_grad_ms_other_build"] = base[N]["lml_grad_ms"]
            r["lml_grad_over_other_build"] = r["lml_grad_ms"] / base[N]["lml_grad_ms"]
        res["sizes"].append(r)
        print(json.dumps({k: v for k, v in r.items() if not k.endswith("_all")}))
        gp.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
