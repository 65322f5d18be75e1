#!/bin/bash
# round-3 profile set: everything lands in gpurun_out/r3prof/, the summaries judged are copied into profiles/ by hand
#   gpurun --timeout 1200 -- 'bash tools/gpu_r3_profiles.sh'
set -o pipefail
cd /root/repo
O=/root/repo/gpurun_out/r3prof; mkdir -p $O
export TMPDIR=/tmp
# the driver's line: bare bench.py = configs[3] as written, with its sub-records and the CPU baseline
timeout -k 10 600 python bench.py --steps 5 --warmup 2 --full > $O/bench_default.json 2> $O/bench_default.err; echo "default rc=$?"; cut -c1-300 $O/bench_default.json
timeout -k 10 300 python bench.py --config shard --steps 10 --warmup 3 --no-cpu-baseline --full > $O/bench_shard.json 2> $O/bench_shard.err; echo "shard rc=$?"; cut -c1-300 $O/bench_shard.json
timeout -k 10 300 python bench.py --config cqt --steps 5 --warmup 2 --full > $O/bench_cqt.json 2> $O/bench_cqt.err; echo "cqt rc=$?"
cd /tmp
# kernel trace of the default command (1 step): the Viterbi's average duration must agree with the line's kernel_ms
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/p_folder -o b -- python3 /root/repo/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-extras > $O/prof_folder.log 2>&1; echo "prof folder rc=$?"
find /tmp/p_folder -name "*kernel_stats.csv" -exec cp {} $O/kernel_stats_folder.csv \;
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/p_shard -o b -- python3 /root/repo/bench.py --config shard --steps 3 --warmup 1 --no-cpu-baseline --no-extras > $O/prof_shard.log 2>&1; echo "prof shard rc=$?"
find /tmp/p_shard -name "*kernel_stats.csv" -exec cp {} $O/kernel_stats_shard.csv \;
# HBM counters, separate passes; counter collection serialises kernels (no persistent launch could see its frame stage)
export AEGIS_VITERBI_PERSISTENT=0
for W in folder shard; do
  timeout -k 10 400 rocprofv3 --pmc FETCH_SIZE --output-format csv -d /tmp/p_fetch_$W -o f -- python3 /root/repo/bench.py --config $W --steps 1 --warmup 1 --no-cpu-baseline --no-extras > $O/pmc_fetch_$W.log 2>&1; echo "pmc fetch $W rc=$?"
  timeout -k 10 400 rocprofv3 --pmc WRITE_SIZE --output-format csv -d /tmp/p_write_$W -o w -- python3 /root/repo/bench.py --config $W --steps 1 --warmup 1 --no-cpu-baseline --no-extras > $O/pmc_write_$W.log 2>&1; echo "pmc write $W rc=$?"
  F=$(find /tmp/p_fetch_$W -name "*counter_collection.csv" | head -1); Wr=$(find /tmp/p_write_$W -name "*counter_collection.csv" | head -1)
  python3 /root/repo/tools/summarize_pmc.py "$F" "$Wr" 2 $O/pmc_hbm_$W.json > $O/pmc_summary_$W.log 2>&1; echo "pmc summary $W rc=$?"; tail -5 $O/pmc_summary_$W.log
done
unset AEGIS_VITERBI_PERSISTENT
cd /root/repo
timeout -k 10 300 python3 tools/bench_engine_e2e.py > $O/engine_e2e.json 2>&1; tail -c 700 $O/engine_e2e.json
timeout -k 10 300 python3 tools/bench_host_path.py > $O/host_path.json 2>&1; tail -c 400 $O/host_path.json
timeout -k 10 300 python3 tools/bench_v2_engine.py > $O/v2_engine.json 2>&1; tail -c 500 $O/v2_engine.json
timeout -k 10 200 python3 tools/bench_stream.py 4000 > $O/stream_latency.json 2>&1; tail -c 300 $O/stream_latency.json
ls -la $O
