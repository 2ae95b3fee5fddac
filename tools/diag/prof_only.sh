export OUT_DIR=${OUT_DIR:-prof_out}; mkdir -p "$OUT_DIR"      # where the runs and profiles go (tools/pmc_round.py too)
tag=$1
export TMPDIR=/tmp
for b in 8 1; do
  rm -rf $OUT_DIR/prof
  rocprofv3 --kernel-trace --stats --output-format csv -d $OUT_DIR/prof -- python3 bench.py --full --batch $b --steps 10 --warmup 2 --no-cpu-baseline --no-parity --no-extras --no-repeats --streams 1 > $OUT_DIR/${tag}_prof_run_b$b.log 2>&1
  tail -1 $OUT_DIR/${tag}_prof_run_b$b.log | cut -c1-200
  f=$(find $OUT_DIR/prof -name '*kernel_stats.csv' | head -1)
  [ -n "$f" ] && cp "$f" $OUT_DIR/${tag}_b${b}_kernel_stats.csv
  t=$(find $OUT_DIR/prof -name '*kernel_trace.csv' | head -1)
  [ -n "$t" ] && python3 tools/per_dispatch_table.py "$t" 2 > $OUT_DIR/${tag}_b${b}_per_dispatch_table.txt && awk 'NR>2 && $NF+0 > 3*$(NF-2)+50' $OUT_DIR/${tag}_b${b}_per_dispatch_table.txt | head -12
  rm -rf $OUT_DIR/prof
done
