#!/bin/bash
# End-of-round evidence (on the GPU box, from the repo root): the driver's bench command, the default bench.py under
# rocprofv3 --kernel-trace --stats, the PMC traffic pass over K1.  Usage: bash tools/r03_final_profile.sh OUTDIR
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$(realpath -m "${1:?usage: bash tools/r03_final_profile.sh OUTDIR}")
mkdir -p $OUT
cd $R && python3 bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/bench_driver_cmd.json 2> $OUT/bench_driver_cmd.err; echo "bench rc $?"
export TMPDIR=/tmp
(cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_bench -o b --output-format csv -- python3 $R/bench.py --full --no-cpu-baseline > $OUT/bench_default_under_rocprof.json 2> $OUT/bench_under_rocprof.err); echo "rocprof rc $?"
cp $(find $OUT/prof_bench -name "b_kernel_stats.csv" | head -1) $OUT/kernel_stats_bench_default.csv
head -12 $OUT/kernel_stats_bench_default.csv | cut -c1-160
cd $R && bash tools/pmc_k1.sh > $OUT/pmc_k1.txt 2>&1; tail -8 $OUT/pmc_k1.txt | cut -c1-200
