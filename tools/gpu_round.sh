#!/bin/bash
# One GPU call of round 6 (GPU host, repo root): the GPU suite, the compat shim's call-pattern and
# latency benches, and the bench.py --full line, under $RR_OUT (default out/).  Each step under its
# own time limit; the first failure ends it.
# usage: tools/gpu_round.sh TAG [steps...]   steps: suite callpattern latency bench (default: all)
set -e
tag=$1; shift
steps=${*:-"suite callpattern latency bench"}
OUT=${RR_OUT:-out}
mkdir -p $OUT
for s in $steps; do
  case $s in
    suite) timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 240 --timeout-method thread \
             > $OUT/${tag}_suite.log 2>&1 || { tail -40 $OUT/${tag}_suite.log; exit 1; }
           tail -3 $OUT/${tag}_suite.log ;;
    callpattern) timeout -k 10 600 python tests/test_compat.py callpattern 4 > $OUT/${tag}_callpattern.txt 2>&1
           tail -c 3000 $OUT/${tag}_callpattern.txt ;;
    latency) for c in 4 1 3; do timeout -k 10 300 python tests/test_compat.py latency $c 2000; done \
             > $OUT/${tag}_latency.txt 2>&1; cat $OUT/${tag}_latency.txt ;;
    bench) timeout -k 10 600 python bench.py --full > $OUT/${tag}_bench.json 2> $OUT/${tag}_bench.err
           tail -c 2500 $OUT/${tag}_bench.json ;;
  esac
done
