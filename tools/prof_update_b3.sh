#!/bin/bash
# k_update_b3 in the default bench (C2): kernel times from a kernel-trace run and counters from counters-only runs
# (one run per counter set: a pass holds 8 SQ counters), each run a process of its own.
# usage (GPU box, repository root): [PROF_OUT=<dir>] bash tools/prof_update_b3.sh <tag> [<library>]
#   -> <dir>/<tag>/kernel_stats.txt, <dir>/<tag>/pmc_update_b3.txt   (<dir>: prof_out under the repository by default)
set -u
TAG=${1:?tag}
R=$PWD
if [ -n "${2:-}" ]; then export GNNRAG_LIB=$(realpath "$2"); fi
OUT=$(realpath -m "${PROF_OUT:-$R/prof_out}")/$TAG
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/kt -o bench -- python $R/bench.py --gpus 1 > $OUT/kt.log 2>&1 || { echo "kernel-trace run failed"; tail -5 $OUT/kt.log; exit 1; }
( cd $R && python tools/rocpd_stats.py $(find $OUT/kt -name 'bench_results.db' | head -1) > $OUT/kernel_stats.txt 2>&1 )
SETS=(
 "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_VALU_MFMA_BUSY_CYCLES"
 "SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_BUSY_CU_CYCLES SQ_INSTS_SALU"
 "GRBM_GUI_ACTIVE GRBM_COUNT"
)
i=0
for C in "${SETS[@]}"; do
  i=$((i+1))
  timeout -k 10 300 rocprofv3 --pmc $C -f csv rocpd -d $OUT/pmc -o set$i -- python $R/bench.py --gpus 1 --steps 10 --warmup 10 > $OUT/pmc_set$i.log 2>&1 || { echo "counter run $i failed"; tail -5 $OUT/pmc_set$i.log; exit 1; }
done
( cd $R && python tools/rocpd_pmc.py $(find $OUT/pmc -name '*_results.db' | sort) > $OUT/pmc_all.txt 2>&1 )
awk '/^[^ ]/{p=/k_update_b3/} p' $OUT/pmc_all.txt > $OUT/pmc_update_b3.txt
for f in $(find $OUT/pmc -name '*counter_collection.csv'); do grep -E "Counter_Name|k_update_b3" $f | cut -c1-400 > $OUT/$(basename $f .csv)_update_b3.csv; done
find $OUT -name '*.db' -delete
find $OUT/pmc $OUT/kt -name '*.csv' -delete
grep -E "^kernel|k_update_b3" $OUT/kernel_stats.txt | cut -c1-60,92-150
cat $OUT/pmc_update_b3.txt | head -80
tail -1 $OUT/kt.log | cut -c1-300
