#!/bin/bash
# Bench sweep on one GPU: default bench (C3, N = 1, CPU baseline + outlier), then
# --config C2 / C5, then a rocprofv3 kernel-trace + stats pass of the default bench.
# Each GPU step has its own limit; the chain stops at the first failure.
# Every run is bench.py --full (the sweep is about the extra keys); outputs land in
# $OUT (a folder under the repository root, default bench_out).
cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
TAG=${TAG:-bench}
run() {  # name limit args...
  local n=$1 l=$2; shift 2
  timeout -k 10 $l python3 -u bench.py --full "$@" > $OUT/${TAG}_$n.json 2> $OUT/${TAG}_$n.err
  local rc=$?
  cat $OUT/${TAG}_$n.json
  [ $rc -ne 0 ] && { tail -20 $OUT/${TAG}_$n.err; exit $rc; }
  return 0
}
run c3 400 ${BENCH_ARGS}
[ -n "$ONLY_C3" ] && exit 0
run c2 200 --config C2 --no-cpu-baseline
run c5 400 --config C5 --no-cpu-baseline --no-outlier --steps 3
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_prof -o run --output-format csv -- python3 bench.py --full --no-cpu-baseline --no-outlier > $OUT/${TAG}_prof.json 2> $OUT/${TAG}_prof.err
rc=$?
[ $rc -ne 0 ] && { tail -20 $OUT/${TAG}_prof.err; exit $rc; }
cat $OUT/${TAG}_prof.json
exit 0
