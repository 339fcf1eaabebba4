#!/bin/bash
# bench (--full: kernel table, roofline, secondary workloads, CPU baseline) + rocprofv3 kernel-trace stats; summaries land in $OUT_DIR
# (default bench_out/)
OUT_DIR=${OUT_DIR:-bench_out}
mkdir -p $OUT_DIR
TAG=${1:-r01}
STEPS=${2:-5}
MORIG_BENCH_DETAIL=$OUT_DIR/bench_detail_$TAG.json python bench.py --full --steps $STEPS --warmup ${3:-10} > $OUT_DIR/bench_$TAG.json 2> $OUT_DIR/bench_$TAG.err
tail -n 1 $OUT_DIR/bench_$TAG.json | head -c 4096; echo; echo "last-line bytes: $(tail -n 1 $OUT_DIR/bench_$TAG.json | wc -c)"
export TMPDIR=/tmp
( cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_$TAG -- python $GRAFT_REPO_ROOT/bench.py --steps 5 --warmup 2 --cpu-seconds 0 --secondary 0 --prof-steps 0 > /tmp/prof_$TAG.log 2>&1 )
f=$(find /tmp/prof_$TAG -name "*kernel_stats.csv" | head -1)
if [ -n "$f" ]; then head -40 "$f" > $OUT_DIR/rocprof_kernel_stats_$TAG.csv; else tail -20 /tmp/prof_$TAG.log > $OUT_DIR/rocprof_$TAG.err; fi
ls $OUT_DIR
