#!/bin/bash
# secondary configs (BASELINE.json configs[2], configs[3]) on one GPU, each with its --full record; output in $OUT_DIR (default bench_out/)
OUT_DIR=${OUT_DIR:-bench_out}
mkdir -p $OUT_DIR
TAG=${1:-r01}
python bench.py --full --workload mask_skin --steps 3 --warmup 1 > $OUT_DIR/bench_maskskin_$TAG.json 2> $OUT_DIR/bench_maskskin_$TAG.err
tail -c 2500 $OUT_DIR/bench_maskskin_$TAG.json
python bench.py --full --workload corrnet --steps 3 --warmup 1 > $OUT_DIR/bench_corrnet_$TAG.json 2> $OUT_DIR/bench_corrnet_$TAG.err
tail -c 2500 $OUT_DIR/bench_corrnet_$TAG.json; tail -3 $OUT_DIR/bench_corrnet_$TAG.err
python bench.py --full --workload deformnet --steps 3 --warmup 1 --cpu-seconds 0 > $OUT_DIR/bench_deformnet_$TAG.json 2> $OUT_DIR/bench_deformnet_$TAG.err
tail -c 1500 $OUT_DIR/bench_deformnet_$TAG.json; tail -3 $OUT_DIR/bench_deformnet_$TAG.err
