#!/bin/bash
export OUT_DIR=${OUT_DIR:-prof_out}; mkdir -p "$OUT_DIR"      # where the runs and profiles go (tools/pmc_round.py too)
export TMPDIR=/tmp
rm -rf $OUT_DIR/prof
rocprofv3 --kernel-trace --output-format csv -d $OUT_DIR/prof -- python3 bench.py --full --steps 24 --warmup 3 --no-cpu-baseline --no-parity --no-extras --no-repeats --no-kernel-events > $OUT_DIR/prof_run.log 2>&1
t=$(find $OUT_DIR/prof -name "*kernel_trace.csv" | head -1)
python3 tools/diag/overlap_stats.py "$t" 12
rm -rf $OUT_DIR/prof
