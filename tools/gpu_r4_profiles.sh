#!/bin/bash
# round-4 profile set: everything lands in gpurun_out/r4prof/, the summaries judged are copied into profiles/ by hand
#   gpurun --timeout 1200 -- 'bash tools/gpu_r4_profiles.sh'
set -o pipefail
cd /root/repo
O=/root/repo/gpurun_out/r4prof; mkdir -p $O
export TMPDIR=/tmp
# the driver's line: bare bench.py = configs[3] as written, with its sub-records and the CPU baseline
timeout -k 10 700 python bench.py --steps 5 --warmup 2 --full > $O/bench_default.json 2> $O/bench_default.err; echo "default rc=$?"; cut -c1-300 $O/bench_default.json
cd /tmp
# kernel trace of the default command: the kernels' average durations must agree with the line's kernel_ms
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/p_folder -o b -- python3 /root/repo/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-extras > $O/prof_folder.log 2>&1; echo "prof folder rc=$?"
find /tmp/p_folder -name "*kernel_stats.csv" -exec cp {} $O/kernel_stats_folder.csv \;
# HBM and SQ counters, separate passes; counter collection serialises kernels
for C in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 400 rocprofv3 --pmc $C --output-format csv -d /tmp/p_$C -o f -- python3 /root/repo/bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-extras > $O/pmc_$C.log 2>&1; echo "pmc $C rc=$?"
done
F=$(find /tmp/p_FETCH_SIZE -name "*counter_collection.csv" | head -1); Wr=$(find /tmp/p_WRITE_SIZE -name "*counter_collection.csv" | head -1)
python3 /root/repo/tools/summarize_pmc.py "$F" "$Wr" 2 $O/pmc_hbm_folder.json > $O/pmc_summary_folder.log 2>&1; echo "pmc summary rc=$?"; tail -5 $O/pmc_summary_folder.log
timeout -k 10 400 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_SALU SQ_ACTIVE_INST_VALU --output-format csv -d /tmp/sq1 -o a -- python3 /root/repo/bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-extras > $O/sq1.log 2>&1; echo "sq pass1 rc=$?"
timeout -k 10 400 rocprofv3 --pmc SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_WAVE_CYCLES SQ_BUSY_CU_CYCLES --output-format csv -d /tmp/sq2 -o b -- python3 /root/repo/bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-extras > $O/sq2.log 2>&1; echo "sq pass2 rc=$?"
A=$(find /tmp/sq1 -name "*counter_collection.csv" | head -1); B=$(find /tmp/sq2 -name "*counter_collection.csv" | head -1)
python3 /root/repo/tools/summarize_sq.py 2 $O/sq_counters_folder.json "$A" "$B" > $O/sq_summary.log 2>&1; echo "sq summary rc=$?"; tail -3 $O/sq_summary.log
cd /root/repo
timeout -k 10 300 python bench.py --config shard --steps 10 --warmup 3 --no-cpu-baseline --full > $O/bench_shard.json 2> $O/bench_shard.err; echo "shard rc=$?"; cut -c1-200 $O/bench_shard.json
timeout -k 10 300 python bench.py --config cqt --steps 5 --warmup 2 --full > $O/bench_cqt.json 2> $O/bench_cqt.err; echo "cqt rc=$?"; cut -c1-200 $O/bench_cqt.json
# the time-split Viterbi: one clip, the tonal variant of a rank's shard, every rank's shard under the automatic rule
timeout -k 10 500 python tools/bench_split.py single rank8tonal ranks > $O/split_bench.log 2> $O/split_bench.err; echo "split rc=$?"; grep -c "^{" $O/split_bench.log
timeout -k 10 200 python tools/tube_survey.py 768 > $O/tube_survey.txt 2>&1; echo "tube survey rc=$?"; tail -1 $O/tube_survey.txt
timeout -k 10 300 python tools/bench_v2_engine.py > $O/v2_engine.json 2> $O/v2_engine.err; echo "v2 rc=$?"; tail -c 300 $O/v2_engine.json
AEGIS_HIP_LIB=/root/repo/_ablate/lib_abcqunc8.so timeout -k 10 200 python tools/cqt_cycles.py > $O/cqt_cycles.txt 2>&1; echo "cqt cycles rc=$?"
ls -la $O
