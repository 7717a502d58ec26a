#!/bin/bash
# BASELINE.md's single-GPU rows (on the GPU host, repo root): one bench.py --full line per BASELINE
# config, each with its CPU baseline legs, into $RR_OUT/bl/ (default out/bl/).
# usage: tools/baseline_table.sh
OUT=${RR_OUT:-out}/bl
mkdir -p $OUT
run() {   # name args...
    local name=$1; shift
    timeout -k 10 400 python3 -u bench.py --full --no-split --no-snappy "$@" > $OUT/$name.log 2>&1
    local rc=$?
    grep '^{' $OUT/$name.log | tail -1 > $OUT/$name.json
    echo "$name rc=$rc"
    return $rc
}
run cfg1 --config 1 --n 100000 --no-host && \
run cfg2 --config 2 --no-host && \
run cfg3 --config 3 --no-host && \
run cfg4_10m --config 4 --n 10000000 --steps 10 --warmup 2 --no-host && \
run cfg5_shard7 --config 5 --steps 10 --warmup 2 --no-host
