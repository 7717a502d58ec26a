#!/bin/bash
# Round-end check on the GPU host (repo root): the GPU suite, smoke(), and one default bench.py --full
# line, logged under $RR_OUT (default out/).
set -e
OUT=${RR_OUT:-out}
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -q --timeout 240 --timeout-method thread > $OUT/final_tests.log 2>&1; grep -E "passed|failed" $OUT/final_tests.log | tail -3
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/final_smoke.log 2>&1; tail -1 $OUT/final_smoke.log
timeout -k 10 600 python -u bench.py --full --steps 20 --warmup 5 > $OUT/final_bench.log 2>&1; grep '^{' $OUT/final_bench.log | tail -1 | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['value'], d['ms_per_step'], d['roofline']['frac'], d['encode']['gib_s'])"
