#!/bin/bash
# round 5, session 1 (diagnostics): L2 weight-stream probe, where the ATen / copy
# launches come from, host profile, the
# forced-collective 1-rank bench WITH the bf16 leg
mkdir -p gpurun_out; export TMPDIR=/tmp
O=gpurun_out
timeout 200 python tools/probe/run_l2_weight_stream.py $O/r05_probe_l2_weight_stream.json > $O/r05s1_probe.log 2>&1; echo probe rc=$?
timeout 200 python tools/find_copies.py fp32 > $O/r05_find_copies_fp32.txt 2>&1; echo fc32 rc=$?
timeout 200 python tools/find_copies.py bf16 > $O/r05_find_copies_bf16.txt 2>&1; echo fcbf rc=$?
timeout 200 python tools/host_profile.py bf16 > $O/r05_host_profile_bf16.txt 2>&1; echo hp rc=$?
LD_FORCE_COLLECTIVES=1 timeout 500 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29517 bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline --no-graph > $O/r05_bench_torchrun_1rank_forced_collectives_bf16.json 2> $O/r05s1_bench_fc.err; echo bench rc=$?
cat $O/r05_bench_torchrun_1rank_forced_collectives_bf16.json | head -c 1500
tail -5 $O/r05s1_probe.log; head -30 $O/r05_find_copies_bf16.txt
