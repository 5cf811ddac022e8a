#!/bin/bash
# k_walk_slice in the default bench (C2): kernel times from a kernel-trace run and counters from a counters-only run
# (one pass of 8 SQ counters), each run a process of its own; the same for a second library when one is named, so that two
# builds are measured in one session.
# usage (GPU box, repository root): [PROF_OUT=<dir>] bash tools/prof_walk_slice.sh <tag> [<library>]
#   -> <dir>/<tag>/kernel_stats.txt, <dir>/<tag>/pmc_walk_slice.txt   (<dir>: prof_out under the repository by default)
set -u
TAG=${1:?tag}
R=$PWD
if [ -n "${2:-}" ]; then export GNNRAG_LIB=$(realpath "$2"); fi
OUT=$(realpath -m "${PROF_OUT:-$R/prof_out}")/$TAG
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/kt -o bench -- python $R/bench.py --gpus 1 > $OUT/kt.log 2>&1 || { echo "kernel-trace run failed"; tail -5 $OUT/kt.log; exit 1; }
( cd $R && python tools/rocpd_stats.py $(find $OUT/kt -name 'bench_results.db' | head -1) > $OUT/kernel_stats.txt 2>&1 )
C="SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAIT_ANY SQ_WAIT_INST_ANY"
timeout -k 10 300 rocprofv3 --pmc $C -f csv rocpd -d $OUT/pmc -o set1 -- python $R/bench.py --gpus 1 --steps 10 --warmup 10 > $OUT/pmc_set1.log 2>&1 || { echo "counter run failed"; tail -5 $OUT/pmc_set1.log; exit 1; }
( cd $R && python tools/rocpd_pmc.py $(find $OUT/pmc -name '*_results.db' | sort) > $OUT/pmc_all.txt 2>&1 )
awk '/^[^ ]/{p=/k_walk_slice/} p' $OUT/pmc_all.txt > $OUT/pmc_walk_slice.txt
find $OUT -name '*.db' -delete
find $OUT/pmc $OUT/kt -name '*.csv' -delete
grep -E "^kernel|k_walk_slice|k_update_b3|k_tables_vq" $OUT/kernel_stats.txt | cut -c1-60,92-150
head -40 $OUT/pmc_walk_slice.txt
tail -1 $OUT/kt.log | cut -c1-200
