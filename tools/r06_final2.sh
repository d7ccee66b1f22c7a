#!/bin/bash
# round 6 final measurements, part 2: the suite, the bench line (with this round's PMC traffic record), chain stamps, full-size
# gradient parity, configs 3 and 5 through the host drivers, the sharded model
ROOT=${GRAFT_REPO_ROOT:-/root/repo}
OUT=$(realpath -m "${1:?usage: tools/r06_final2.sh <out dir>}")
mkdir -p "$OUT"
cd $ROOT
python -m pytest tests -m gpu -q > $OUT/r06_final_tests.txt 2>&1; echo "tests rc=$?"; tail -4 $OUT/r06_final_tests.txt
python bench.py --full > $OUT/r06_bench_stdout.txt 2> $OUT/r06_bench_stderr.txt; grep '"metric"' $OUT/r06_bench_stdout.txt > $OUT/r06_bench_line.json; cut -c1-200 $OUT/r06_bench_line.json
( cd /tmp && export TMPDIR=/tmp && MIGP_OPTS=0=0 rocprofv3 --kernel-trace --output-format csv -d $OUT/tr_cs -- python3 $ROOT/tools/trace_n.py 4096 8 lml > $OUT/tr_cs.log 2>&1 )
{ echo "N=4096 RBF d=8, ONE stream (MIGP_OPTS=0=0), rocprofv3 kernel trace, last evaluation (tools/column_times.py):"; python tools/column_times.py $OUT/tr_cs; } > $OUT/r06_chain_stamps.txt 2>&1
rm -rf $OUT/tr_cs; cat $OUT/r06_chain_stamps.txt
python tools/fullsize_parity.py c3grad --out $OUT/r06_fullsize_parity.json > $OUT/r06_fullsize.log 2>&1; tail -2 $OUT/r06_fullsize.log | cut -c1-300
python tools/run_configs.py > $OUT/r06_configs_3_5.txt 2>&1; tail -3 $OUT/r06_configs_3_5.txt | cut -c1-300
python tools/emulate_rank.py --curve --out $OUT/r06_sharded_model.json > $OUT/r06_emulate.log 2>&1; grep predicted_ms $OUT/r06_emulate.log | cut -c1-220 | tail -12
