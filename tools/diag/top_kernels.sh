export OUT_DIR=${OUT_DIR:-prof_out}; mkdir -p "$OUT_DIR"      # where the runs and profiles go (tools/pmc_round.py too)
export TMPDIR=/tmp
rm -rf $OUT_DIR/prof
SCENEEGO_CONV1X1=1 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT_DIR/prof -- python3 bench.py --full --batch 8 --steps 10 --warmup 2 --no-cpu-baseline --no-parity --no-extras --no-repeats --streams 1 > $OUT_DIR/prof_run.log 2>&1
f=$(find $OUT_DIR/prof -name "*kernel_stats.csv" | head -1)
head -14 $f | cut -c1-200
rm -rf $OUT_DIR/prof
