#!/bin/bash
# full validation of a build: every -m gpu test (as the driver runs them), smoke, the --full bench line; output in $OUT_DIR
# (default bench_out/)
OUT_DIR=${OUT_DIR:-bench_out}
mkdir -p $OUT_DIR
TAG=${1:-full}
timeout 2400 python -m pytest tests -q -m gpu --timeout=1200 2>&1 | tail -45 > $OUT_DIR/pytest_gpu_$TAG.txt; tail -45 $OUT_DIR/pytest_gpu_$TAG.txt
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -4
MORIG_BENCH_DETAIL=$OUT_DIR/bench_detail_$TAG.json python bench.py --full > $OUT_DIR/bench_$TAG.json 2> $OUT_DIR/bench_$TAG.err
python -c "
import json; r=json.loads(open('$OUT_DIR/bench_$TAG.json').read().strip().splitlines()[-1])
print(r['value'], r['ms_per_step'], r['ms_per_step_median']); s=r['secondary']
print({k: (v.get('value'), v.get('ms_per_step')) for k, v in s.items() if isinstance(v, dict) and 'value' in v}); print(json.dumps(s['small_batch'])); print(json.dumps(s['joint_extraction'])); print('last-line bytes', len(open('$OUT_DIR/bench_$TAG.json').read().strip().splitlines()[-1]))"; tail -3 $OUT_DIR/bench_$TAG.err
