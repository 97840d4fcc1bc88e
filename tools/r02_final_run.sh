# Round-2 measurement set (run on the MI355X box): PMC traffic + utilisation, kernel stats, bench lines.
set -e
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${OUT:-prof_out}; mkdir -p $OUT
Q="--no-cpu-baseline --no-host-to-host --no-parity --pipelined-streams 0"
rm -rf $OUT/pmc_fetch $OUT/pmc_write $OUT/pmc_mfma $OUT/pmc_lds $OUT/prof_final
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/pmc_fetch -- python3 bench.py --size 256 --steps 1 --warmup 0 $Q > $OUT/pmc_fetch.log 2>&1
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/pmc_write -- python3 bench.py --size 256 --steps 1 --warmup 0 $Q > $OUT/pmc_write.log 2>&1
timeout -k 10 300 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --kernel-trace --output-format csv -d $OUT/pmc_mfma -- python3 bench.py --size 256 --steps 1 --warmup 0 $Q > $OUT/pmc_mfma.log 2>&1
timeout -k 10 300 rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE --kernel-trace --output-format csv -d $OUT/pmc_lds -- python3 bench.py --size 256 --steps 1 --warmup 0 $Q > $OUT/pmc_lds.log 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_final -- python3 bench.py $Q > $OUT/bench_prof_final.log 2>&1
python profiles/summarize.py stats $OUT/prof_final/*/*_kernel_stats.csv $OUT/r02_bench_fp16_1024_kernel_stats.txt > /dev/null
python profiles/summarize.py pmc $OUT/pmc_fetch/*/*_counter_collection.csv $OUT/pmc_write/*/*_counter_collection.csv $OUT/r02_pmc_hbm_fp16.json fp16 > /dev/null
python profiles/summarize.py util $OUT/pmc_mfma/*/*_counter_collection.csv $OUT/pmc_lds/*/*_counter_collection.csv $OUT/r02_pmc_util_fp16.json fp16 > $OUT/pmc_util.log 2>&1 || true
rm -rf $OUT/pmc_fetch $OUT/pmc_write $OUT/pmc_mfma $OUT/pmc_lds $OUT/prof_final
timeout -k 10 900 python bench.py --full > $OUT/r02_bench_default.log 2>&1; tail -1 $OUT/r02_bench_default.log > $OUT/r02_bench_default.json; cut -c1-300 $OUT/r02_bench_default.json
timeout -k 10 300 python bench.py --full --dtype bf16 --no-cpu-baseline --no-host-to-host > $OUT/r02_bench_bf16.log 2>&1; tail -1 $OUT/r02_bench_bf16.log > $OUT/r02_bench_bf16_1024.json; cut -c1-200 $OUT/r02_bench_bf16_1024.json
timeout -k 10 300 python bench.py --full --dtype fp32 --size 512 --batch 8 --no-cpu-baseline --no-host-to-host > $OUT/r02_bench_fp32.log 2>&1; tail -1 $OUT/r02_bench_fp32.log > $OUT/r02_bench_fp32_512.json; cut -c1-200 $OUT/r02_bench_fp32_512.json
python tools/layer_times.py --size 1024 > $OUT/r02_layer_times.txt 2>&1; cat $OUT/r02_layer_times.txt
