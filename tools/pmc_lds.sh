#!/bin/bash
# LDS bank conflicts / LDS activity per kernel from one --pmc pass per counter over bench.py:   tools/pmc_lds.sh [<out dir>]
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(realpath -m "${1:-pmc_lds}")
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
for c in SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_LDS; do
  rocprofv3 --pmc $c --kernel-trace --output-format csv -d "$OUT/pmc_lds_$c" -- python3 $ROOT/bench.py --full --steps 1 --warmup 1 --roofline-steps 1 --no-lookahead --no-cpu-baseline --no-sharded --chains-per-gpu 0 --grad-steps 0 > "$OUT/pmc_lds_$c.log" 2>&1
  echo "$c exit $?"
done
python3 - "$OUT" <<'PY'
import csv, glob, collections, sys
out = sys.argv[1]
for c in ("SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE", "SQ_INSTS_LDS"):
    fs = glob.glob(f"{out}/pmc_lds_{c}/**/*counter_collection.csv", recursive=True)
    if not fs:
        print(c, "no file"); continue
    tot = collections.Counter(); n = collections.Counter()
    for r in csv.DictReader(open(fs[0])):
        k = r["Kernel_Name"].split("(")[0].replace("void migp::", "")[:44]
        tot[k] += float(r["Counter_Value"]); n[k] += 1
    for k in tot:
        if "gemm" in k or "strip" in k or "leaf" in k or "thin" in k:
            print(f"{c:24s} {k:42s} launches {n[k]:5d} total {tot[k]:.4g} per launch {tot[k]/n[k]:.4g}")
PY
