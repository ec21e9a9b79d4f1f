#!/bin/bash
# rocprofv3 kernel-trace summaries of the c2 step per conv arithmetic (bench.py --full):
#   bash tools/prof_modes.sh OUTDIR f16x3 bf16x3   (OUTDIR relative to the repository root)
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
PM=${1:?usage: bash tools/prof_modes.sh OUTDIR MATH...}
shift
mkdir -p "$PM"
for m in "$@"; do
  timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $PM/prof_$m -o p -- python3 bench.py --math $m --no-cpu-baseline --no-modes --full --steps 20 --warmup 3 > $PM/bench_$m.json 2> $PM/bench_$m.err || exit 1
  python tools/rocpd_stats.py $PM/prof_$m/p_results.db > $PM/kernel_stats_$m.csv 2> $PM/span_$m.txt
  rm -rf $PM/prof_$m
  echo "prof $m done"
done
