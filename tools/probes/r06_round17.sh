# round 6, seventeenth call: the whole -m gpu suite + smoke on the final tree; default bench line; Paraformer bench line
set -x
OUT=${OUT:-build/probes/r06q}
mkdir -p $OUT
python -m pytest tests -m gpu -q --durations=8 > $OUT/pytest_all.txt 2>&1
tail -14 $OUT/pytest_all.txt
python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.txt 2>&1; tail -2 $OUT/smoke.txt
python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err; tail -c 600 $OUT/bench_default.json
python bench.py --workload paraformer --steps 10 2>/dev/null | tail -1 > $OUT/bench_paraformer.json
