#!/bin/bash
# rocprofv3 kernel trace of the --full bench (UBD_PROF_ARGS: extra bench flags, default --no-train); summary -> prof_out/kernel_stats.csv
cd "$(dirname "$0")/.."
ROOT=$PWD; OUT=$ROOT/prof_out; SCRATCH=$(mktemp -d)
mkdir -p $OUT
( cd $SCRATCH && rocprofv3 --kernel-trace --stats --output-format csv -d $SCRATCH/prof -- python3 $ROOT/bench.py --full --steps 200 --warmup 20 --no-cpu-baseline ${UBD_PROF_ARGS:---no-train} > $OUT/prof_bench.log 2>&1 )
f=$(find $SCRATCH/prof -name "*kernel_stats.csv" | head -1)
cp "$f" $OUT/kernel_stats.csv 2>/dev/null
cut -c1-200 $OUT/kernel_stats.csv | head -40
tail -1 $OUT/prof_bench.log | cut -c1-3000
