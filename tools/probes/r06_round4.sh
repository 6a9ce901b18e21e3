# round 6, fourth measurement: the block kernel with FFN-2 split over K (f16 partials exchanged, hid stays in LDS) against the round-4 form
set -x
OUT=${OUT:-build/probes/r06d}
mkdir -p $OUT
python -m pytest tests/test_sensevoice_gpu.py tests/test_paraformer_gpu.py tests/test_shim_gpu.py -m gpu -q -x --durations=5 > $OUT/pytest.txt 2>&1
tail -12 $OUT/pytest.txt
for k in 1 0 1 0; do
  ASR_SANM_BLOCK_FFNK=$k python bench.py --full --steps 100 --warmup 5 --no-cpu-baseline --no-extras > $OUT/bench_ffnk$k.json 2> $OUT/bench_ffnk$k.err
  python -c "
import json
d = json.loads(open('$OUT/bench_ffnk$k.json').read().strip().splitlines()[-1])
print('FFNK=$k', d['ms_per_step'], d['value'], d['roofline']['frac'], d['roofline'].get('avg_block_us'), d['kernels'].get('sanm_block'))
"
done
for k in 1 0; do echo "=== phase clock FFNK=$k, 64 windows"; ASR_SANM_BLOCK_FFNK=$k ASR_SANM_BLOCK_DBG=10 python tools/probes/sanm_block_clock.py 2>&1 | grep -v amdgpu.ids | tail -17; done > $OUT/phase_clock.txt 2>&1
cat $OUT/phase_clock.txt
for k in 1 0; do echo "=== phase clock FFNK=$k, one window (idle chip)"; CLOCK_B=1 ASR_SANM_BLOCK_MIN=1 ASR_SANM_BLOCK_FFNK=$k ASR_SANM_BLOCK_DBG=10 python tools/probes/sanm_block_clock.py 2>&1 | grep -v amdgpu.ids | tail -17; done > $OUT/phase_clock_b1.txt 2>&1
cat $OUT/phase_clock_b1.txt
