#!/bin/bash
# Memory-side traffic + L2 hit rate of K5 in one bench regime: three rocprofv3 PMC passes (counters only) over
# `python3 tools/perf_k5.py pmc`, then tools/pmc_to_json.py (gfx950 FETCH_SIZE x2 correction, kernel-source sha stamp).
# usage: bash tools/pmc_traffic.sh <out-subdir-of-gpurun_out> <regime: r2|r1|locality|script> [fp8|pv]
#        bash tools/pmc_traffic.sh <out-subdir> <tools/perf_block64.py shape: hunyuan_r2|hunyuan_gilbert|...> "" b64
#        (64-token blocks: the launches of tools/perf_block64.py pmc instead of tools/perf_k5.py pmc)
# Every pass runs under a time limit of its own (RSA_PMC_TIMEOUT seconds, default 240); a pass that fails or runs into it ends
# the script: nothing more is started on the device and no JSON is written.
R=$PWD; OUT=$R/gpurun_out/$1; mkdir -p $OUT
export RSA_PERF_REGIME=$2 RSA_PERF_NODENSE=1
KERN=bsfwd
if [ "$3" = "fp8" ]; then export RSA_PERF_FP8=1; KERN=bsfwd_fp8; fi
if [ "$3" = "pv" ]; then export RSA_PERF_FP8=pv; KERN=bsfwd_fp8; fi
cd /tmp; export TMPDIR=/tmp
N=0
LIMIT="timeout -k 10 ${RSA_PMC_TIMEOUT:-240}"
for P in "TCC_HIT_sum TCC_MISS_sum GRBM_GUI_ACTIVE" "FETCH_SIZE" "WRITE_SIZE"; do
  N=$((N+1))
  if [ "$4" = "b64" ]; then
    RSA_PERF_SHAPES=$2 RSA_PERF_BLOCK=64 $LIMIT rocprofv3 --pmc $P --output-format csv -d $OUT/p$N -- python3 $R/tools/perf_block64.py pmc > $OUT/p$N.log 2>&1 || { echo "pass $N ($P) failed: $OUT/p$N.log"; tail -5 $OUT/p$N.log; exit 1; }
  else
    $LIMIT rocprofv3 --pmc $P --output-format csv -d $OUT/p$N -- python3 $R/tools/perf_k5.py pmc > $OUT/p$N.log 2>&1 || { echo "pass $N ($P) failed: $OUT/p$N.log"; tail -5 $OUT/p$N.log; exit 1; }
  fi
done
cd $R
python3 tools/pmc_to_json.py $OUT/traffic.json $KERN "$OUT/**/*counter_collection.csv"
