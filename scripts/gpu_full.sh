#!/bin/bash
# Round check: every -m gpu test, then the default bench line (C4, --full).
# Outputs under $VBHEM_OUT/TAG (default bench_out/TAG).
set -o pipefail
TAG=${1:-full}; shift
OUT=${VBHEM_OUT:-bench_out}/$TAG; mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -x -q -m gpu --timeout 300 --timeout-method thread > $OUT/tests.log 2>&1
rc=$?; tail -3 $OUT/tests.log; [ $rc -ne 0 ] && exit $rc
timeout -k 10 600 python -u bench.py --full "$@" > $OUT/bench.json 2> $OUT/bench.err
rc=$?; tail -c 600 $OUT/bench.json; exit $rc
