#!/bin/bash
# A/B of library variants (variants/*.so) on the vote bench; each run time-limited.
# Logs go to $OUT (default bench_out/).
cd "$(dirname "$0")/.."
OUT="${OUT:-bench_out}"
mkdir -p "$OUT"
for rep in 1 2; do
  for v in "$@"; do
    PVVOTE_LIB=variants/$v.so timeout -k 10 200 python bench.py --steps 50 --warmup 10 --full --skip-cpu --skip-e2e --skip-u1 --skip-config3 --skip-u4 --skip-batched > "$OUT/ab_$v.$rep.log" 2>&1 || exit $?
    python - "$v" "$rep" "$OUT/ab_$v.$rep.log" <<'PY'
import json, sys
l = [x for x in open(sys.argv[3]) if x.startswith("{")][-1]
d = json.loads(l)
print(sys.argv[1], sys.argv[2], "img/s", d["value"], "vote_us", round(d["roofline_vote_count"]["avg_kernel_ms"] * 1000, 2), "lat_us", round(d["latency_ms_per_image"] * 1000, 1))
PY
  done
done
