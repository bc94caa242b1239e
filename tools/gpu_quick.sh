#!/bin/bash
# Quick GPU check of a tree: the parity / config GPU tests, the --full bench line with its per-op profile, the 256x256 bench line.
# Usage: tools/gpu_quick.sh <outdir>
R=$PWD
O=${1:?usage: tools/gpu_quick.sh <outdir>}; case $O in /*) ;; *) O=$R/$O;; esac
mkdir -p $O
cd $R
timeout 1800 python -m pytest tests/test_gpu_parity.py tests/test_gpu_configs.py -m gpu -x -q > $O/quick_gpu_tests.log 2>&1
echo "tests rc=$?"; tail -5 $O/quick_gpu_tests.log
timeout 900 python bench.py --full --no-cpu-baseline --no-split --profile-out $O/quick_per_op_profile.json > $O/quick_bench_1gpu.json 2> $O/quick_bench_1gpu.err
echo "bench rc=$?"; cut -c1-300 $O/quick_bench_1gpu.json
timeout 300 python bench.py --full --no-cpu-baseline --no-split --workload 256 --steps 50 > $O/quick_bench_256.json 2>> $O/quick_bench_1gpu.err
cut -c1-200 $O/quick_bench_256.json
