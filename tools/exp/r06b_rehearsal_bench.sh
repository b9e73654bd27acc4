# second session, final sources: the configs[2] rehearsal of the C++ step under the executable again (the rebuild kernel changed: shard
# folders byte-identical to the round-1 scheme's, checksum = bench.py's), then the default bench line for profiles/r06_bench.json
OUT=${OUT:?set OUT to the folder the results go to}; mkdir -p "$OUT"
set -x
STEPS=2 WARMUP=2 bash tools/exp/r06_step_rehearsal.sh $OUT/r06c > $OUT/r06c_rehearsal.log 2>&1 || { tail -20 $OUT/r06c_rehearsal.log; exit 1; }
cat $OUT/r06c/summary.txt
timeout -k 10 600 python3 bench.py --full > $OUT/r06_bench_final.json 2> $OUT/r06_bench_final.err || { tail -5 $OUT/r06_bench_final.err; exit 1; }
echo bench done
