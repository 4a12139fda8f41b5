#!/bin/bash
# GPU box, end of a round (or any full check): the whole GPU test suite, smoke(), the default bench
# line with every leg (bench.py --full), then the headline profile (tools/gpu_profile.sh: trace + stats,
# timeline, PMC traffic of the timed forwards, SQ counters).  Results go to $OUT (default: out/).
# Usage: [OUT=dir] bash tools/gpu_round.sh TAG [--no-tests] [--no-profile]
set -o pipefail
TAG=${1:-round}
shift
cd "${GRAFT_REPO_ROOT:-.}"
export TMPDIR=/tmp
export OUT=${OUT:-out}
mkdir -p "$OUT"
if [[ " $* " != *" --no-tests "* ]]; then
  timeout -k 10 1050 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread -p no:cacheprovider \
      > $OUT/gpu_tests_$TAG.log 2>&1; rc=$?
  tail -3 $OUT/gpu_tests_$TAG.log
  [ $rc -eq 0 ] || { grep -E "^E |FAILED|Error" $OUT/gpu_tests_$TAG.log | head -30; exit $rc; }
  timeout -k 10 150 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" \
      > $OUT/smoke_$TAG.log 2>&1 || { tail -5 $OUT/smoke_$TAG.log; exit 1; }
  tail -1 $OUT/smoke_$TAG.log
fi
timeout -k 10 300 python -u bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err \
    || { tail -5 $OUT/bench_$TAG.err; exit 1; }
cat $OUT/bench_$TAG.json
if [[ " $* " != *" --no-profile "* ]]; then
  bash tools/gpu_profile.sh $TAG || exit 1
  cat $OUT/timeline_$TAG.txt | tail -2
fi
