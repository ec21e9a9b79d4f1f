#!/bin/bash
# Round evidence on the GPU box: per workload the two --pmc passes (HBM bytes per launch), the kernel-trace summary and
# the bench line (bench.py --full throughout).  Run as: bash tools/evidence.sh OUTDIR (relative to the repository
# root); then copy OUTDIR/r03_* into profiles/.
# The PMC passes run WITHOUT any trace domain beside the kernel trace (gpurun refuses other combinations).
set -e
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
EV=${1:?usage: bash tools/evidence.sh OUTDIR}
mkdir -p "$EV"
MATH=${MATH:-f16x3}
PMC_ARGS=""
for c in c2 c3 c5; do
  ARGS="--config $c --math $MATH --steps 2 --warmup 1 --no-graph --no-modes --no-cpu-baseline --full"
  timeout -k 10 400 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $EV/pmc_fetch_$c -o f -- python3 bench.py $ARGS > $EV/pmc_fetch_$c.json 2> $EV/pmc_fetch_$c.err
  timeout -k 10 400 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $EV/pmc_write_$c -o w -- python3 bench.py $ARGS > $EV/pmc_write_$c.json 2> $EV/pmc_write_$c.err
  PMC_ARGS="$PMC_ARGS $c $(find $EV/pmc_fetch_$c -name '*counter_collection.csv') $(find $EV/pmc_write_$c -name '*counter_collection.csv')"
  echo "pmc $c done"
done
python tools/pmc_summary.py $MATH $PMC_ARGS > $EV/r03_pmc_traffic.json 2> $EV/pmc_summary.log
cp $EV/r03_pmc_traffic.json profiles/r03_pmc_traffic.json
rm -rf $EV/pmc_fetch_c* $EV/pmc_write_c*
for c in c2 c3 c5; do
  S="--steps 20 --warmup 5"; [ $c != c2 ] && S="--steps 6 --warmup 3"
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $EV/prof_$c -o p -- python3 bench.py --config $c --no-cpu-baseline --no-modes --full $S > $EV/prof_$c.json 2> $EV/prof_$c.err
  python tools/rocpd_stats.py $EV/prof_$c/p_results.db > $EV/r03_${c}_kernel_stats.csv 2> $EV/prof_${c}_span.txt
  rm -rf $EV/prof_$c
  echo "prof $c done"
done
timeout -k 10 900 python bench.py --full > $EV/r03_bench_c2.json 2> $EV/bench_c2.err
echo "bench c2 done"
timeout -k 10 600 python bench.py --config c3 --no-modes --full > $EV/r03_bench_c3.json 2> $EV/bench_c3.err
echo "bench c3 done"
timeout -k 10 600 python bench.py --config c5 --no-modes --full > $EV/r03_bench_c5.json 2> $EV/bench_c5.err
echo "bench c5 done"
