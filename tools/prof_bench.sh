#!/bin/bash
# The reference bench command with every leg (--full), alone and under
# rocprofv3 --kernel-trace --stats (the summary behind the JSON line's kernel
# durations), then one FETCH_SIZE and one WRITE_SIZE pass
# (tools/pmc_traffic_json.py folds them).  Every GPU step under its own time
# limit; stop at the first failure.  Output goes to $OUT (default bench_out/).
cd "$(dirname "$0")/.."
OUT="${OUT:-bench_out}"
mkdir -p "$OUT"
CMD="bench.py --gpus 1 --steps 20 --warmup 5 --full"
timeout -k 10 400 python3 $CMD > "$OUT/bench_plain.log" 2>&1 || { echo "bench failed"; tail -20 "$OUT/bench_plain.log"; exit 1; }
grep '^{' "$OUT/bench_plain.log" | tail -1 > "$OUT/bench_plain.json"
timeout -k 10 500 rocprofv3 --kernel-trace --stats -T --output-format csv -d "$PWD/$OUT/prof_bench" -o bench -- python3 $CMD > "$OUT/bench_prof.log" 2>&1 || { echo "prof failed"; tail -20 "$OUT/bench_prof.log"; exit 1; }
grep '^{' "$OUT/bench_prof.log" | tail -1 > "$OUT/bench_prof.json"
python3 tools/u1_trace_summary.py "$OUT/prof_bench/bench_kernel_trace.csv" "$OUT/bench_prof.json" "$OUT/u1_timed_launches.json"
python3 tools/u4_trace_summary.py "$OUT/prof_bench/bench_kernel_trace.csv" "$OUT/bench_prof.json" "$OUT/u4_timed_launches.json"
python3 tools/kernel_phases.py "$OUT/prof_bench/bench_kernel_trace.csv" "$OUT/kernel_phases.json" > /dev/null 2>&1 || true
# the full trace (~1M rows at 1,024 frames per step) is not kept: its summaries above are
rm -f "$OUT/prof_bench/bench_kernel_trace.csv"
if [ -n "$PMC" ]; then
  for c in FETCH_SIZE WRITE_SIZE; do
    timeout -k 10 400 rocprofv3 --kernel-include-regex "k_vote|k_compact|k_fg_count|k_refine|k_hyp_gen|k_front" --pmc $c -T --output-format csv \
      -d "$PWD/$OUT/pmc_$c" -o b -- python3 bench.py --steps 5 --warmup 2 --full --skip-cpu --skip-e2e --skip-config3 --skip-u4 > "$OUT/pmc_$c.log" 2>&1 || { echo "pmc $c failed"; exit 1; }
    timeout -k 10 300 rocprofv3 --kernel-include-regex "k_vote_mfma|k_evd" --pmc $c -T --output-format csv \
      -d "$PWD/$OUT/pmcu4_$c" -o b -- python3 tools/u4_probe.py 10 > "$OUT/pmcu4_$c.log" 2>&1 || { echo "pmc u4 $c failed"; exit 1; }
  done
  python3 tools/pmc_traffic_json.py "$OUT/pmc_FETCH_SIZE" "$OUT/pmc_WRITE_SIZE" "$OUT/pmc_traffic.json" \
    "$OUT/pmcu4_FETCH_SIZE" "$OUT/pmcu4_WRITE_SIZE" > /dev/null
fi
echo ok
