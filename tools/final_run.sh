# Round-end measurement set (run on the MI355X box): PMC traffic, kernel stats, bench lines.
set -e
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${OUT:-prof_out}; mkdir -p $OUT
rm -rf $OUT/pmc_fetch $OUT/pmc_write $OUT/prof_final
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/pmc_fetch -- python3 bench.py --size 256 --steps 1 --warmup 0 --no-cpu-baseline > $OUT/pmc_fetch.log 2>&1
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/pmc_write -- python3 bench.py --size 256 --steps 1 --warmup 0 --no-cpu-baseline > $OUT/pmc_write.log 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_final -- python3 bench.py --no-cpu-baseline > $OUT/bench_prof_final.log 2>&1
python profiles/summarize.py stats $OUT/prof_final/*/*_kernel_stats.csv $OUT/final_kernel_stats.txt > /dev/null
python profiles/summarize.py pmc $OUT/pmc_fetch/*/*_counter_collection.csv $OUT/pmc_write/*/*_counter_collection.csv $OUT/final_pmc_hbm_bf16.json bf16 > /dev/null
cp $OUT/final_pmc_hbm_bf16.json profiles/r01_pmc_hbm_bf16.json
timeout -k 10 600 python bench.py --full > $OUT/bench_default.log 2>&1; tail -1 $OUT/bench_default.log | cut -c1-200
timeout -k 10 300 python bench.py --full --dtype fp16 --no-cpu-baseline > $OUT/bench_fp16.log 2>&1; tail -1 $OUT/bench_fp16.log | cut -c1-200
timeout -k 10 300 python bench.py --full --dtype fp32 --size 512 --batch 8 --no-cpu-baseline > $OUT/bench_fp32.log 2>&1; tail -1 $OUT/bench_fp32.log | cut -c1-200
