#!/bin/bash
# The sharding tests, then a rehearsal of bench.py's N > 1 path with two ranks on one GPU
# over gloo (RCCL needs one GPU per rank), into $O (default bench_out/shard).
set -e
O=${O:-bench_out/shard}
mkdir -p $O
timeout -k 10 300 python -u -m pytest tests/test_shard.py -v --timeout 200 --timeout-method thread > $O/tests.log 2>&1
timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29517 \
  bench.py --gpus 2 --steps 10 --warmup 2 --backend gloo --full > $O/bench2.log 2>&1
echo shard-done
