#!/bin/bash
# end-of-round measurement at the final tree: the driver's command with --full, then one bench line per config
# (tools/gpu_configs_bench.sh) - files $OUT_DIR/<tag>_* (default bench_out/).  PROF=1 also runs the driver's
# command under rocprofv3 --kernel-trace --stats (its exit status is the call's; <tag>_bench_kernel_stats.csv).
set -o pipefail
T=${TAG:-final}
TAG=$T bash tools/gpu_full.sh || exit 1
bash tools/gpu_configs_bench.sh $T || exit 1
if [ -n "$PROF" ]; then
  R=$PWD
  O=$(realpath ${OUT_DIR:-bench_out})
  cd /tmp && export TMPDIR=/tmp
  timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/${T}_prof -o run -- python3 $R/bench.py --gpus 1 --steps 20 --warmup 5 --full > $O/${T}_prof.log 2>&1
  rc=$?; echo "rocprofv3 bench rc=$rc" | tee -a $O/${T}_prof.log
  cp $(find $O/${T}_prof -name "*kernel_stats.csv" | head -1) $O/${T}_bench_kernel_stats.csv
  rm -rf $O/${T}_prof
  exit $rc
fi
