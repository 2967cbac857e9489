#!/bin/bash
# A/B of the agent kernel's specialised instantiation by DIE_PIC_K1_GENERIC on ONE build: interleaved bench processes, the driver command,
# one rocprofv3 --kernel-trace --stats run per mode, the --pmc passes (runs of their own).  Stops at the first failing GPU step.
set -o pipefail
# usage: scratch/k1_specialised_ab.sh OUTPUT_DIR   (from the repository root)
R=$(pwd); O=${1:?output directory}; case $O in /*) ;; *) O=$R/$O ;; esac; mkdir -p $O
B="python $R/bench.py --gpus 1 --steps 100 --warmup 20 --no-cpu-baseline --no-extras"
one() {  # tag, generic flag
  DIE_PIC_K1_GENERIC=$2 timeout -k 10 150 $B > $O/$1.json 2> $O/$1.err || { echo "bench $1 failed rc=$?"; tail -5 $O/$1.err; exit 1; }
  echo "$1 $(tail -1 $O/$1.json | cut -c1-400)"
}
one a1_generic 1; one a1_special 0
one a2_special 0; one a2_generic 1
one a3_generic 1; one a3_special 0
one a4_special 0; one a4_generic 1
for m in 1 0; do
  DIE_PIC_K1_GENERIC=$m timeout -k 10 400 python $R/bench.py --gpus 1 --steps 20 --warmup 5 > $O/driver_generic$m.json 2> $O/driver_generic$m.err || { echo "driver cmd (generic=$m) failed rc=$?"; tail -5 $O/driver_generic$m.err; exit 1; }
  echo "driver generic=$m $(tail -1 $O/driver_generic$m.json | cut -c1-300)"
done
cd $O
for m in 1 0; do
  DIE_PIC_K1_GENERIC=$m timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats_generic$m -- $B > $O/stats_generic$m.log 2>&1 || { echo "stats run (generic=$m) failed rc=$?"; tail -5 $O/stats_generic$m.log; exit 1; }
  echo "== stats generic=$m"; tail -1 $O/stats_generic$m.log | cut -c1-300
  find $O/stats_generic$m -name '*kernel_stats.csv' | head -1 | xargs -r head -6
done
for m in 0 1; do
  i=0
  for set in "FETCH_SIZE" "WRITE_SIZE TCC_HIT_sum TCC_MISS_sum"; do
    d=$O/pmc_generic${m}_$i
    DIE_PIC_K1_GENERIC=$m timeout -k 10 200 rocprofv3 --pmc $set --output-format csv -d $d -- python3 $R/bench.py --steps 16 --warmup 8 --no-cpu-baseline --no-extras --kernel-reps 1 > $d.log 2>&1 || { echo "pmc pass $i (generic=$m) failed rc=$?"; tail -5 $d.log; exit 1; }
    i=$((i+1))
  done
  python3 $R/scratch/pmc_agg.py $O/pmc_generic${m}_* > $O/pmc_generic${m}_per_kernel_avg.json && echo "== pmc generic=$m" && grep -A6 "forward_move\|kernel_source_sha" $O/pmc_generic${m}_per_kernel_avg.json | head -24
done
# keep what travels back small: the aggregated files and the stats csv, not the raw counter dumps
find $O -name '*counter_collection.csv' -delete; find $O -name '*kernel_trace.csv' -delete; find $O -name '*.db' -delete
du -sh $O
