#!/bin/bash
# A/B of two builds of libhakai_hip.so on the same box: bench.py alternately with the current library
# and with hakai-fem_amd/lib/libhakai_hip_old.so swapped in, RUNS times each (default 2), then the
# current one is put back. Run from the repository root; the lines go to $OUT (default results/).
# BENCH_ARGS replaces the bench's extra arguments (default: --full --cpu-baseline 0).
export TMPDIR=/tmp
OUT=${OUT:-results}
RUNS=${RUNS:-2}
BENCH_ARGS=${BENCH_ARGS:---full --cpu-baseline 0}
mkdir -p "$OUT"
L=hakai-fem_amd/lib
cp $L/libhakai_hip.so /tmp/libhakai_hip_new.so
run() {
  # --full: the nodal/BC kernel times in kernel_ms_per_step come from the pass after the timed region
  timeout -k 10 300 python -u bench.py --steps 200 --warmup 20 $BENCH_ARGS > "$OUT/ab_$1.json" 2>/dev/null || { cp /tmp/libhakai_hip_new.so $L/libhakai_hip.so; exit 1; }
  python -c "import json; d=json.loads(open('$OUT/ab_$1.json').read().strip().splitlines()[-1]); print('$1', d['value'], d['ms_per_step'], d['roofline']['avg_launch_ms'], d['config'].get('kernel_ms_per_step'))"
}
for i in $(seq 1 "$RUNS"); do
  cp /tmp/libhakai_hip_new.so $L/libhakai_hip.so; run new$i
  cp $L/libhakai_hip_old.so $L/libhakai_hip.so; run old$i
done
cp /tmp/libhakai_hip_new.so $L/libhakai_hip.so
