#!/bin/bash
# the headline line at 40 steps, then tools/sweep.py's configurations; logs go to $OUT (default: bench_out/)
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 300 python bench.py --full --steps 40 --warmup 3 --no-cpu-baseline > $OUT/bench_head.log 2>&1
rc=$?; echo "bench rc=$rc"; tail -1 $OUT/bench_head.log
if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 1000 python -u tools/sweep.py $OUT/sweep.jsonl > $OUT/sweep.log 2>&1
rc=$?; cat $OUT/sweep.log | tail -25; exit $rc
