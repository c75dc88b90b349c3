#!/bin/bash
# GPU box: everything the committed evidence under profiles/ is made from, in one call (about five minutes):
# the -m gpu tests, the rocprofv3 passes of all six kinds, and the bench lines of every BASELINE configuration.
#   usage: tools/round_end.sh <tag> [round prefix, default r6] [output dir, default round_out]     outputs under <output dir>/<tag>_*;
#          then on the build machine: cp <output dir>/<tag>_profiles/* profiles/ and the bench lines you want to keep
set -e
T=${1:?tag}; O=${3:-round_out}; mkdir -p $O
python -m pytest tests -m gpu -x -q > $O/${T}_tests.log 2>&1 || { tail -30 $O/${T}_tests.log; exit 1; }
tail -2 $O/${T}_tests.log
for k in gather flat point maze maze_mj flagrun; do
  n=4096; [ $k = maze ] && n=8192
  rm -rf $O/prof_${T}_$k
  bash tools/profile_round.sh $O/prof_${T}_$k $k $n > $O/prof_${T}_$k.log 2>&1 && echo profiled $k
done
# condense them where the bench runs, so that its line carries the counters of exactly these kernels; the files end up under the output dir
R=${2:-r6}
for k in gather flat point maze maze_mj flagrun; do
  n=4096; [ $k = maze ] && n=8192
  name=${R}_$k; [ $k = gather ] && name=${R}_final
  python tools/summarize_profile.py $O/prof_${T}_$k $name $k $n > /dev/null
done
mkdir -p $O/${T}_profiles && cp profiles/pmc_summary.json profiles/${R}_*_pmc.json profiles/${R}_*_kernel_stats.csv $O/${T}_profiles/
# the evidence lines carry roofline, solver rows (and, for the headline, cpu_baseline): --full
: > $O/${T}_other_kinds.txt
for k in flat maze point maze_mj flagrun mixed; do
  n=4096; [ $k = maze ] && n=8192
  python bench.py --full --kind $k --envs $n --steps 1000 --warmup 200 --no-cpu-baseline 2>/dev/null | tail -1 >> $O/${T}_other_kinds.txt
done
python bench.py --full --envs 32768 --steps 300 --warmup 100 --no-cpu-baseline 2>/dev/null | tail -1 >> $O/${T}_other_kinds.txt
python bench.py --full --steps 20 --warmup 5 > $O/${T}_bench_driverlike.json 2>/dev/null
python bench.py --full > $O/${T}_bench.json 2> $O/${T}_bench.err
tail -c 400 $O/${T}_bench.json
