#!/bin/bash
# Parity suite, then a short bench of the default build and (A/B) of an alternative build
# given as $1 (a .so under gnn-track-finding_amd/gtf/), into $O (default bench_out/chk).
set -e
O=${O:-bench_out/chk}
mkdir -p $O
timeout -k 10 400 python -u -m pytest tests -m gpu -v --timeout 120 --timeout-method thread > $O/gpu_tests.log 2>&1
timeout -k 10 200 python -u bench.py --full --no-cpu --no-c5 --no-dropin --steps 30 --warmup 3 > $O/bench.log 2>&1
if [ -n "$1" ]; then
  GTF_LIB=$PWD/gnn-track-finding_amd/gtf/$1 timeout -k 10 200 python -u bench.py --full --no-cpu --no-c5 --steps 30 --warmup 3 > $O/bench_alt.log 2>&1
fi
echo check-done
