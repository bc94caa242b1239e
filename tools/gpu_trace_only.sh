#!/bin/bash
# Serialised kernel trace of the bench forward (--lanes 0) + its summary.  Usage: tools/gpu_trace_only.sh <outdir>
R=$PWD
O=${1:?usage: tools/gpu_trace_only.sh <outdir>}; case $O in /*) ;; *) O=$R/$O;; esac
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rm -rf $O/rocprof
timeout 600 rocprofv3 --kernel-trace --stats -d $O/rocprof -o bench -- python $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-split --lanes 0 > $O/rocprof.log 2>&1
echo "kernel-trace rc=$?"
cd $R
python tools/rocprof_summary.py $(ls $O/rocprof/*/*results.db $O/rocprof/*results.db 2>/dev/null | head -1) --forwards 5 > $O/kernel_stats.md 2> $O/kernel_stats.err
echo "summary rc=$?"; head -8 $O/kernel_stats.md; cat $O/kernel_stats.err
rm -rf $O/rocprof
