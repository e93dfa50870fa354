#!/bin/bash
# The committed profile set of a round, in one command on a GPU machine: bench lines (three --full runs + one with the driver's flags),
# rocprofv3 kernel stats of the --full bench (forward only, and with the train legs) with full-size averages, HBM traffic tables
# (separate --pmc passes).  Everything lands in prof_out/; copy to profiles/<round>_* with tools/collect_profiles.py <round>.
cd "$(dirname "$0")/.."
ROOT=$PWD; OUT=$ROOT/prof_out; SCRATCH=$(mktemp -d)
mkdir -p $OUT
for i in 1 2 3; do python3 bench.py --full > $OUT/bench_default_$i.json 2> $OUT/bench_default_$i.err; tail -c 300 $OUT/bench_default_$i.json; echo; done
python3 bench.py --gpus 1 --steps 20 --warmup 5 > $OUT/bench_driver_flags.json 2> $OUT/bench_driver_flags.err
( cd $SCRATCH && rocprofv3 --kernel-trace --stats --output-format csv -d $SCRATCH/prof -- python3 $ROOT/bench.py --full --steps 200 --warmup 20 --no-cpu-baseline --no-train > $OUT/prof_bench.log 2>&1 )
python3 tools/full_size_avg.py "$(find $SCRATCH/prof -name '*kernel_trace.csv' | head -1)" "$(find $SCRATCH/prof -name '*kernel_stats.csv' | head -1)" $OUT/bench_kernel_stats.csv
( cd $SCRATCH && rocprofv3 --kernel-trace --stats --output-format csv -d $SCRATCH/prof2 -- python3 $ROOT/bench.py --full --steps 200 --warmup 20 --no-cpu-baseline > $OUT/prof_bench_full.log 2>&1 )
python3 tools/full_size_avg.py "$(find $SCRATCH/prof2 -name '*kernel_trace.csv' | head -1)" "$(find $SCRATCH/prof2 -name '*kernel_stats.csv' | head -1)" $OUT/bench_full_kernel_stats.csv
UBD_PMC_DTYPE=float32 bash tools/gpu_pmc_traffic.sh > /dev/null 2>&1
UBD_PMC_DTYPE=float16 bash tools/gpu_pmc_traffic.sh > /dev/null 2>&1
UBD_PMC_DTYPE=bfloat16 UBD_PMC_TRAIN=1 bash tools/gpu_pmc_traffic.sh > /dev/null 2>&1
UBD_PMC_DTYPE=float32 UBD_PMC_TRAIN=1 bash tools/gpu_pmc_traffic.sh > /dev/null 2>&1
head -12 $OUT/bench_kernel_stats.csv | cut -c1-160
ls -la $OUT | tail -20
