cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
OUT=${OUT:-prof_out}; mkdir -p "$OUT"      # where the passes and their summaries go
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/r02_movegen_pmc_f -- python bench.py --full --steps 50 --warmup 5 --no-cpu-baseline --sat-boards 0 --selfplay-plies 0 --no-whole-games --train-steps 0 --no-overlap > $OUT/r02_movegen_pmc_f.log 2>&1 &&
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/r02_movegen_pmc_w -- python bench.py --full --steps 50 --warmup 5 --no-cpu-baseline --sat-boards 0 --selfplay-plies 0 --no-whole-games --train-steps 0 --no-overlap > $OUT/r02_movegen_pmc_w.log 2>&1
echo rc=$?
python tools/prof_summary.py $OUT/r02_movegen_pmc_f hive > $OUT/r02_movegen_pmc_f.md 2>&1
python tools/prof_summary.py $OUT/r02_movegen_pmc_w hive > $OUT/r02_movegen_pmc_w.md 2>&1
