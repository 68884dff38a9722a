#!/bin/bash
# rocprofv3 kernel trace + stats of the C3 bench (no CPU baseline / outlier), then
# the per-superstep dispatch table; outputs under $OUT/${TAG}_prof*.
cd /tmp && export TMPDIR=/tmp
cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${OUT:-bench_out}   # a folder under the repository root
mkdir -p "$OUT"
TAG=${TAG:-prof}
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_prof -o run --output-format csv -- python3 bench.py --full --no-cpu-baseline --no-outlier ${BENCH_ARGS} > $OUT/${TAG}_prof.json 2> $OUT/${TAG}_prof.err
rc=$?
[ $rc -ne 0 ] && { tail -20 $OUT/${TAG}_prof.err; exit $rc; }
cat $OUT/${TAG}_prof.json
exit 0
