#!/bin/bash
# The whole -m gpu suite, then the full bench line (bench.py --full: CPU baselines, drop-in
# stage wall time and config 5 included) into $O (default bench_out/full).
set -e
O=${O:-bench_out/full}
mkdir -p $O
timeout -k 10 500 python -u -m pytest tests -m gpu -v --timeout 120 --timeout-method thread > $O/gpu_tests.log 2>&1
timeout -k 10 400 python -u bench.py --full > $O/bench.log 2>&1
echo full-done
