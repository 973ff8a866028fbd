#!/bin/bash
# Bench lines for the SURVEY.md §8(d) configs other than C2 (one GPU), plus the C2 stress variant (5% FATPIPE,
# 10% bounded, penalties {1,2,4}), each with its CPU baseline (--full); each step under its own limit.
# Output: $BENCH_OUT (default bench_out/).
O=${BENCH_OUT:-bench_out}
mkdir -p "$O"
timeout -k 10 400 python bench.py --full --variant stress --steps 5 --warmup 1 --dropin-steps 0 --cpu-reps 3 \
  > "$O/bench_c2_stress.json" 2> "$O/bench_c2_stress.log"
rc=$?; echo "stress rc=$rc" >> "$O/bench_c2_stress.log"
if [ $rc -ne 0 ]; then echo "STOP stress rc=$rc"; tail -20 "$O/bench_c2_stress.log"; exit $rc; fi
cat "$O/bench_c2_stress.json"
for w in c3 c4 c5; do
  timeout -k 10 400 python bench.py --full --workload $w --steps 10 --warmup 2 > "$O/bench_$w.json" 2> "$O/bench_$w.log"
  rc=$?; echo "$w rc=$rc" >> "$O/bench_$w.log"
  if [ $rc -ne 0 ]; then echo "STOP $w rc=$rc"; tail -20 "$O/bench_$w.log"; exit $rc; fi
  cat "$O/bench_$w.json"
done
