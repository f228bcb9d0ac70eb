#!/bin/bash
# FETCH_SIZE and WRITE_SIZE of the pipeline's kernels over the bench with its
# roofline legs (--full), one counter pass each; output under $OUT (default bench_out/).
cd "$(dirname "$0")/.."
OUT="${OUT:-bench_out}"
mkdir -p "$OUT"
timeout -k 10 300 rocprofv3 --kernel-include-regex "k_vote|k_compact|k_fg_count|k_refine|k_prep|k_hyp_gen" --pmc FETCH_SIZE -T --output-format csv -d "$PWD/$OUT/tr_fetch" -o b -- python3 bench.py --full --skip-cpu --skip-e2e --steps 20 > /dev/null 2>&1 &&
timeout -k 10 300 rocprofv3 --kernel-include-regex "k_vote|k_compact|k_fg_count|k_refine|k_prep|k_hyp_gen" --pmc WRITE_SIZE -T --output-format csv -d "$PWD/$OUT/tr_write" -o b -- python3 bench.py --full --skip-cpu --skip-e2e --steps 20 > /dev/null 2>&1
