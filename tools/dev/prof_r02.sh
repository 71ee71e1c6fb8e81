cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
OUT=${OUT:-prof_out}; mkdir -p "$OUT"      # where the passes and their summaries go
rocprofv3 -L > $OUT/rocprof_counters.txt 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/r02_movegen_kt -- python bench.py --full --steps 200 --warmup 20 --no-cpu-baseline --selfplay-plies 0 --no-whole-games --train-steps 0 --no-overlap > $OUT/r02_movegen_kt.log 2>&1 &&
rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVES GRBM_GUI_ACTIVE --output-format csv -d $OUT/r02_movegen_pmc_a -- python bench.py --full --steps 50 --warmup 5 --no-cpu-baseline --selfplay-plies 0 --no-whole-games --train-steps 0 --no-overlap > $OUT/r02_movegen_pmc_a.log 2>&1 &&
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/r02_selfplay_kt -- python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --selfplay-plies 3 --no-whole-games --train-steps 0 --no-overlap --no-cpu-baseline-selfplay > $OUT/r02_selfplay_kt.log 2>&1 &&
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $OUT/r02_net_pmc_a -- python tools/net_latency.py 1024 > $OUT/r02_net_pmc_a.log 2>&1 &&
rocprofv3 --pmc SQ_INSTS_LDS SQ_INSTS_VALU SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY --output-format csv -d $OUT/r02_net_pmc_b -- python tools/net_latency.py 1024 > $OUT/r02_net_pmc_b.log 2>&1 &&
rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum --output-format csv -d $OUT/r02_net_pmc_c -- python tools/net_latency.py 1024 > $OUT/r02_net_pmc_c.log 2>&1 &&
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/r02_train_kt -- python tools/train_prof.py > $OUT/r02_train_kt.log 2>&1
echo profiles rc=$?
for d in r02_movegen_kt r02_movegen_pmc_a r02_net_pmc_a r02_net_pmc_b r02_net_pmc_c; do python tools/prof_summary.py $OUT/$d hive > $OUT/$d.md 2>&1; done
python tools/prof_summary.py $OUT/r02_net_pmc_a conv > $OUT/r02_net_pmc_a_conv.md 2>&1
python tools/prof_summary.py $OUT/r02_net_pmc_b conv > $OUT/r02_net_pmc_b_conv.md 2>&1
python tools/prof_summary.py $OUT/r02_net_pmc_c conv > $OUT/r02_net_pmc_c_conv.md 2>&1
python tools/prof_summary.py $OUT/r02_net_pmc_a resblock > $OUT/r02_net_pmc_a_res.md 2>&1
python tools/prof_summary.py $OUT/r02_net_pmc_b resblock > $OUT/r02_net_pmc_b_res.md 2>&1
python tools/prof_summary.py $OUT/r02_net_pmc_c resblock > $OUT/r02_net_pmc_c_res.md 2>&1
python tools/top_kernels.py $OUT/r02_selfplay_kt 20 > $OUT/r02_selfplay_top.md 2>&1
python tools/top_kernels.py $OUT/r02_train_kt 25 > $OUT/r02_train_top.md 2>&1
find $OUT/r02_* -name "*.csv" -size +3M -delete
ls $OUT | tail -30
