#!/bin/bash
# the checks of a finished tree on one GPU: full GPU suite, smoke, the full bench line (results under $OUT, default out/)
set -x
OUT=${OUT:-out}; mkdir -p $OUT
python -m pytest tests -x -q -m gpu 2>&1 | grep -v "^RCCL\|^HIP version\|^ROCm\|^Hostname\|^Librccl" | tail -6 > $OUT/suite_tests.txt
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1 > $OUT/suite_smoke.txt
python bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/suite_bench.json 2> $OUT/suite_bench.err
cat $OUT/suite_tests.txt $OUT/suite_smoke.txt; tail -c 400 $OUT/suite_bench.json; tail -3 $OUT/suite_bench.err
