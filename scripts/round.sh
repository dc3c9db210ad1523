#!/bin/bash
# One verification pass on the GPU box: gpu parity tests, smoke, the full bench line, the
# rocprofv3 --kernel-trace --stats profile of the same bench command (csv, so that
# tools/trace_split.py can split the tick by dispatch start stamps), and bench.py's own
# multi-rank launch (two gloo ranks sharing the one GPU, started by bench.py itself).
# Stops at the first failure.  Logs go to $OUT (default: bench_out/).
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p $OUT
if [ -z "$SKIP_TESTS" ]; then
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q -p no:cacheprovider --timeout 120 --timeout-method thread > $OUT/pytest_gpu.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -4 $OUT/pytest_gpu.log
if [ $rc -ne 0 ]; then grep -E "Error|assert|FAILED" $OUT/pytest_gpu.log | head -20; exit $rc; fi
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1
rc=$?; echo "smoke rc=$rc"; tail -3 $OUT/smoke.log
if [ $rc -ne 0 ]; then exit $rc; fi
fi
timeout -k 10 600 python bench.py --full > $OUT/bench_default.log 2>&1
rc=$?; echo "bench rc=$rc"; tail -1 $OUT/bench_default.log
if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/final_prof -o run --output-format csv -- python bench.py --full --no-cpu-baseline > $OUT/final_prof.log 2>&1
rc=$?; echo "prof rc=$rc"; tail -1 $OUT/final_prof.log
if [ $rc -ne 0 ]; then exit $rc; fi
python tools/trace_split.py $OUT/final_prof/run_kernel_trace.csv $OUT/trace_split.json > $OUT/trace_split.log 2>&1
echo "trace_split rc=$?"; cat $OUT/trace_split.log | head -40
timeout -k 10 300 python bench.py --gpus 2 --backend gloo --steps 2 > $OUT/bench_spawn2.log 2>&1
rc=$?; echo "bench --gpus 2 (self-spawned gloo ranks) rc=$rc"; tail -1 $OUT/bench_spawn2.log
exit $rc
