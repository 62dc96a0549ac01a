#!/bin/bash
# Profiles `bench.py` on the GPU box: kernel trace + stats, then PMC passes (each in its own run;
# --pmc is never combined with other trace domains).  Output under gpurun_out/prof_<tag>/.
# Every run has its own time limit (PROF_STEP_LIMIT seconds, default 300) and the first one that fails or times out
# ends the script.  KMC_LIB_PATH selects the library (a variant of tools/build_variant.sh).  PROF_TRACE_ONLY=1: no PMC passes.
# usage: tools/profile_bench.sh <tag> [bench args...]
set -u
tag=$1; shift
root=${GRAFT_REPO_ROOT:-$(pwd)}
out=$root/gpurun_out/prof_$tag
mkdir -p $out
export TMPDIR=/tmp
args="--full --steps 5 --warmup 6 --no-cpu-baseline --no-cold $*"
limit=${PROF_STEP_LIMIT:-300}
cd $root
timeout -k 10 $limit rocprofv3 --kernel-trace --stats --output-format csv -d $out/trace -- python3 bench.py $args > $out/trace.log 2>&1
rc=$?
echo "trace rc=$rc"
[ $rc -ne 0 ] && exit $rc
[ -n "${PROF_TRACE_ONLY:-}" ] && exit 0   # (a step timeline needs the kernel trace alone: tools/step_timeline.py)
i=0
for ctrs in "FETCH_SIZE" "WRITE_SIZE" \
  "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT" \
  "SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_LDS SQ_INSTS_VMEM_RD SQ_LDS_IDX_ACTIVE SQ_WAVES SQ_INSTS_SMEM" \
  "GRBM_GUI_ACTIVE TCC_HIT_sum TCC_MISS_sum"; do
  i=$((i+1))
  timeout -k 10 $limit rocprofv3 --pmc $ctrs --output-format csv -d $out/pmc$i -- python3 bench.py $args > $out/pmc$i.log 2>&1
  rc=$?
  echo "pmc$i ($ctrs) rc=$rc"
  [ $rc -ne 0 ] && exit $rc
done
find $out -name "*.csv" | head -40
