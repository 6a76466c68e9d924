#!/bin/bash
# One GPU session: parity tests, smoke, bench, rocprofv3 kernel trace.  Everything lands in $OUT.
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export TMPDIR=/tmp
OUT=${OUT:?set OUT to the directory for the results}
mkdir -p "$OUT"
rocminfo 2>/dev/null | grep -E "Marketing Name|gfx|Compute Unit" | head -8 > $OUT/rocminfo.txt
nproc > $OUT/nproc.txt; lscpu | grep -E "Model name|^CPU\(s\)" >> $OUT/nproc.txt
if [ "${SKIP_TESTS:-0}" != "1" ]; then
echo "== pytest -m gpu"
timeout ${TEST_TIMEOUT:-1500} python -m pytest tests -m gpu -x -q 2>&1 | tail -40 | tee $OUT/pytest_gpu.log
echo "== smoke"
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -5 | tee $OUT/smoke.log
fi
echo "== bench"
timeout 900 python bench.py --full --steps ${BENCH_STEPS:-200} --warmup 20 2>$OUT/bench.err | tail -1 | tee $OUT/bench.json
tail -5 $OUT/bench.err
if [ "${SKIP_PROF:-0}" != "1" ]; then
echo "== rocprof (one frame at a time, d2 + r1mix)"
for wl in d2 r1mix; do
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$wl -o bench -- python bench.py --full --workload $wl --steps 40 --warmup 5 --in-flight 1 --timed-only > $OUT/rocprof_$wl.log 2>&1
find $OUT/prof_$wl -name "*kernel_stats*" | head -1 | xargs -r -I{} cp {} $OUT/kernel_stats_serial_$wl.csv
head -16 $OUT/kernel_stats_serial_$wl.csv
rm -rf $OUT/prof_$wl
done
fi
