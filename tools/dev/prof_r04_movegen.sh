# Round 4: kernel trace of the default bench command (the driver's flags), for profiles/r04_movegen_kernel_trace.md
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
OUT=${OUT:-prof_out}; mkdir -p "$OUT"      # where the passes and their summaries go
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/r04_mg_kt -- python3 bench.py --full --steps 200 --warmup 20 --windows 5 --no-cpu-baseline --no-overlap --selfplay-plies 0 --no-whole-games --train-steps 0 --encode-boards 0 > $OUT/r04_mg_kt.log 2>&1
echo rc=$?
python3 tools/prof_summary.py $OUT/r04_mg_kt hive > $OUT/r04_mg_kt.md; cat $OUT/r04_mg_kt.md | cut -c1-160 | head
find $OUT/r04_mg_kt -name "*.csv" -size +1M -delete
