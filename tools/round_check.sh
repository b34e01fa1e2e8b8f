#!/bin/bash
# Round evidence in one GPU call: parity tests, the full bench line (bench.py --full), the rocprofv3
# kernel-trace/stats of the same bench command, then the PMC traffic passes.
# Logs and results go to $OUT (default: bench_out/ in the repository root).
R=$GRAFT_REPO_ROOT
TAG=${1:-r01}
cd $R
OUT=${OUT:-$R/bench_out}
mkdir -p $OUT
timeout -k 10 600 python -m pytest tests/ -q -x -m gpu > $OUT/t_$TAG.log 2>&1; rc=$?
tail -3 $OUT/t_$TAG.log
[ $rc -ne 0 ] && { echo "TESTS FAILED rc=$rc"; exit $rc; }
timeout -k 10 400 python bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { echo BENCH FAILED; tail -20 $OUT/bench_$TAG.err; exit 1; }
cat $OUT/bench_$TAG.json
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o run -- python $R/bench.py --full > $OUT/prof_$TAG.log 2>&1 || { echo PROF FAILED; exit 1; }
echo PROF ok
bash $R/tools/pmc_traffic.sh
