# headline bench with every leg (--full) + profile (trace, timeline, reconciled PMC traffic, SQ), then (TRAIN=1)
# the training configs: configs[2] (yolox_s fp32 bs 8) eager, configs[4] (yolox_x 1280 --fp16 bs 8) eager and
# captured.  Results go to $OUT (default: out/).
cd "${GRAFT_REPO_ROOT:-.}"
export TMPDIR=/tmp
export OUT=${OUT:-out}
mkdir -p "$OUT"
T=${TAG:-perf}
timeout -k 10 300 python -u bench.py --full > $OUT/bench_$T.json 2> $OUT/bench_$T.err || { tail -5 $OUT/bench_$T.err; exit 1; }
cat $OUT/bench_$T.json
bash tools/gpu_profile.sh $T || exit 1
tail -1 $OUT/timeline_$T.txt
if [ -n "$TRAIN" ]; then
  TAG=$T bash tools/gpu_train_bench.sh || exit 1
fi
