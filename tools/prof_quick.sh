# usage: bash tools/prof_quick.sh <tag> <bench args...> : rocprofv3 kernel stats of a short full bench run, summary to stdout
# (trace and log under $OUT/<tag>, default out/)
TAG=$1; shift
R=$PWD; OUT=$(mkdir -p "${OUT:-out}" && cd "${OUT:-out}" && pwd); cd /tmp; export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$TAG -- python3 $R/bench.py --steps 5 --warmup 2 --full --no-cpu-baseline "$@" > $OUT/$TAG.log 2>&1
cd $R; python3 tools/summarize_prof.py $(find $OUT/$TAG -name "*kernel_stats.csv" | head -1) | cut -c1-140
