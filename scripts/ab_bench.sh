#!/bin/bash
# A/B of library variants (tools/ab_build.py -> ab/libswarm_<name>.so) on the headline bench:
# VARIANTS="base nt wt" bash scripts/ab_bench.sh; "base" = the in-tree library.  Each variant runs
# REPS times, interleaved, so drift hits all of them alike.  One JSON line per run, in $OUT/ab.jsonl
# (OUT defaults to bench_out/).
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p $OUT
REPS=${REPS:-3}
: > $OUT/ab.jsonl
for rep in $(seq $REPS); do
  for v in $VARIANTS; do
    if [ "$v" = base ]; then lib="$PWD/experiments-2025-acsos-marl-for-swarming-behaviors_amd/libswarm_hip.so"; else lib="$PWD/ab/libswarm_$v.so"; fi
    SWARM_LIB_PATH=$lib timeout -k 10 300 python bench.py --full --no-cpu-baseline $BENCH_ARGS > $OUT/ab_$v.log 2>&1
    rc=$?
    if [ $rc -ne 0 ]; then echo "variant $v rc=$rc"; tail -5 $OUT/ab_$v.log; exit $rc; fi
    python -c "import json,sys; d=json.loads(open('$OUT/ab_$v.log').read().strip().splitlines()[-1]); print(json.dumps({'variant':'$v','rep':$rep,'value':d['value'],'ms_per_step':d['ms_per_step'],'us_per_tick':d.get('us_per_tick'),'tick_us':d.get('tick_us'),'kernel_us':(d['roofline'] or {}).get('kernel_us')}))" >> $OUT/ab.jsonl
  done
done
cat $OUT/ab.jsonl
