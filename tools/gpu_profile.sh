#!/bin/bash
# GPU box: evidence for one bench configuration -- bench (+ per-layer table, tune file, every leg of
# --full), rocprofv3 kernel trace + stats of the same bench, PMC HBM traffic (FETCH_SIZE / WRITE_SIZE in
# separate passes, MI355X_MICROARCH.md HBM section) and an SQ / GRBM pass for MFMA utilisation per kernel.
# Results go to $OUT (default: out/).
# Usage: [OUT=dir] [TRAFFIC_ARGS='yolox_l 16 640 fp16'] bash tools/gpu_profile.sh TAG [bench args...]
#        (e.g. --model yolox_l --batch 16 --dtype fp16; TRAFFIC_ARGS names the workload in the traffic JSON)
set -o pipefail
TAG=${1:-run}
shift
ARGS="$*"
cd "${GRAFT_REPO_ROOT:-.}"
export TMPDIR=/tmp
OUT=${OUT:-out}
mkdir -p "$OUT"
TUNE=$OUT/tune_$TAG.json
timeout -k 10 300 python bench.py $ARGS --full --layers --tune-file $TUNE > $OUT/bench_$TAG.json \
    2> $OUT/bench_$TAG.err || exit 1
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv \
    -- python bench.py $ARGS --steps 10 --warmup 3 --no-cpu-baseline --tune-file $TUNE \
    > $OUT/prof_$TAG.log 2>&1 || exit 1
for CNT in FETCH_SIZE WRITE_SIZE; do
  timeout -s KILL 120 rocprofv3 --pmc $CNT -d $OUT/pmc_${TAG}_$CNT -o run --output-format csv \
      -- python bench.py $ARGS --steps 4 --warmup 1 --no-cpu-baseline --tune-file $TUNE \
      > $OUT/pmc_${TAG}_$CNT.log 2>&1 || exit 1
done
timeout -s KILL 120 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_INSTS_MFMA SQ_INSTS_VALU SQ_WAVES GRBM_GUI_ACTIVE \
    -d $OUT/pmc_${TAG}_SQ -o run --output-format csv \
    -- python bench.py $ARGS --steps 4 --warmup 1 --no-cpu-baseline --tune-file $TUNE \
    > $OUT/pmc_${TAG}_SQ.log 2>&1 || exit 1
timeout -s KILL 120 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_LDS \
    SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT GRBM_GUI_ACTIVE \
    -d $OUT/pmc_${TAG}_SQ2 -o run --output-format csv \
    -- python bench.py $ARGS --steps 4 --warmup 1 --no-cpu-baseline --tune-file $TUNE \
    > $OUT/pmc_${TAG}_SQ2.log 2>&1 || exit 1
python tools/forward_timeline.py $OUT/prof_$TAG/run_kernel_trace.csv > $OUT/timeline_$TAG.txt || exit 1
# HBM bytes of exactly the 4 timed forwards of the PMC passes, launch list reconciled with the trace
python tools/traffic.py $OUT/pmc_$TAG $OUT/traffic_$TAG.json $TRAFFIC_ARGS --replays 4 \
    --timeline $OUT/timeline_$TAG.txt || exit 1
python tools/mfma_util.py $OUT/pmc_${TAG}_SQ/run_counter_collection.csv --last 3 \
    --stalls $OUT/pmc_${TAG}_SQ2/run_counter_collection.csv --json $OUT/mfma_util_$TAG.json \
    > $OUT/mfma_util_$TAG.txt || exit 1
echo "profile $TAG done"
