"""GPU: the streaming form of the device resampler (asr_op_resample_stream; csrc/resample.hip) against the offline launch, bit for bit, and against the float64
statement (tests/resample_ref.py, tests/resample_stream_ref.py).

Three streams over six steps with a staggered mode -- stream 0 in every step, stream 1 in every other one, stream 2 from step 2 on with a reset at step 4 -- so
one launch holds streams at different step counts. A reset starts a new stream: the table below lists the (stream, steps) runs that are each one signal.

1. frames_out is the statement's need(c), 0 for a stream that is not in a step;
2. every run's concatenated outputs equal engine.op_resample of its concatenated consumed frames, cut to C S, bit for bit;
3. ... and stay within (T + channels + 2) 2^-24 sum_k |c[p][k]| |x[.]| of the float64 statement (test_resample_gpu.py's bound, per output);
4. nothing past a row's first need(c) frames is read: NaN (int16: full scale) there changes no output;
5. impulses either side of a step boundary return the table's coefficients exactly."""
import numpy as np
import pytest

import resample_ref as R
import resample_stream_ref as RS
from conftest import sub

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
MODE = np.asarray([[1, 1, 0], [1, 0, 0], [1, 1, 1], [1, 0, 1], [1, 1, 2], [1, 0, 1]], dtype=np.int32)       # [step][stream]
RUNS = [(0, [0, 1, 2, 3, 4, 5]), (1, [0, 2, 4]), (2, [2, 3]), (2, [4, 5])]                                  # (stream, the steps of one signal)

# rate, dtype, channels, int16 scale flag, chunk. The first five are the grid; the sixth is an odd chunk while up-sampling, where outputs c S - 1 and c S share a
# centre frame and the first output of a step reads 2 W + 1 carried frames.
GRID = [(8000, np.float32, 1, False, 960), (44100, np.int16, 2, True, 960), (11025, np.float16, 3, False, 960), (48000, np.int16, 2, False, 960),
        (16000, np.float32, 2, False, 960), (8000, np.float32, 2, False, 961)]


def _signal(rng, n, channels, dtype):
    if dtype == np.int16:
        return rng.integers(-32768, 32768, size=(n, channels)).astype(np.int16)
    return rng.standard_normal((n, channels)).astype(dtype)


def _rows(signals, S, rate, channels, dtype, tail):
    """The op's audio [steps][streams][pitch][channels] from the runs' signals, every row's tail beyond need(c) (and every row that is not in a step) = tail."""
    P = RS.pitch(S, rate)
    audio = np.full(MODE.shape + (P, channels), tail, dtype=dtype)
    for (stream, steps), x in zip(RUNS, signals):
        for c, k in enumerate(steps):
            a0, a1 = RS.start(S, rate, c), RS.start(S, rate, c + 1)
            audio[k, stream, :a1 - a0] = x[a0:a1]
    return audio


@pytest.mark.parametrize("rate,dtype,channels,scale,S", GRID, ids=[f"{r}-{np.dtype(d).name}-c{c}{'-scaled' if s else ''}-S{S}" for r, d, c, s, S in GRID])
def test_staggered_streams_equal_the_offline_resampler_bit_for_bit(rate, dtype, channels, scale, S):
    eng = sub("engine")
    L, M, W, T, _ = R.design(rate)
    c64 = R.table(rate)
    rng = np.random.default_rng(rate + channels + S)
    signals = [_signal(rng, RS.start(S, rate, len(steps)), channels, dtype) for _, steps in RUNS]
    poison = np.nan if dtype != np.int16 else 32767
    out, frames, pitch = eng.op_resample_stream(_rows(signals, S, rate, channels, dtype, poison), MODE, rate, channels=channels, int16_scale=scale, chunk=S)
    assert pitch == RS.pitch(S, rate) and out.shape == MODE.shape + (S,) and out.dtype == np.float32
    # 1. the frame counts
    want_frames = np.zeros(MODE.shape, np.int32)
    for stream, steps in RUNS:
        for c, k in enumerate(steps):
            want_frames[k, stream] = RS.need(S, rate, c)
    assert np.array_equal(frames, want_frames), (frames, want_frames)
    assert np.all(out[MODE == 0] == 0)                                # rows of streams that are not in a step: untouched
    worst = 0.0
    for (stream, steps), x in zip(RUNS, signals):
        C = len(steps)
        got = np.concatenate([out[k, stream] for k in steps])
        assert np.isfinite(got).all() and np.count_nonzero(got) > got.size // 2
        # 2. the offline launch over the same frames
        whole, offs = eng.op_resample(x.reshape(-1), [0, x.shape[0]], rate, channels=channels, int16_scale=scale)
        assert offs[-1] >= C * S
        bad = np.flatnonzero(got.view(np.int32) != whole[:C * S].view(np.int32))
        assert bad.size == 0, (stream, steps, bad[:8], got[bad[:8]], whole[bad[:8]])
        # 3. the float64 statement
        y64, mag = R.resample(R.mono(x, scale and dtype == np.int16), rate, c64=c64)
        err, bound = np.abs(got.astype(np.float64) - y64[:C * S]), (T + channels + 2) * EPS * mag[:C * S]
        print(f"stream {stream} steps {steps}: worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.4f}")
        assert np.all(err <= bound), (stream, steps, np.flatnonzero(err > bound)[:8])
    # 4. another tail, the same bits
    again, frames2, _ = eng.op_resample_stream(_rows(signals, S, rate, channels, dtype, 0), MODE, rate, channels=channels, int16_scale=scale, chunk=S)
    assert np.array_equal(frames2, frames) and np.array_equal(again.view(np.int32), out.view(np.int32))


@pytest.mark.parametrize("rate", [8000, 44100, 48000])
def test_impulses_either_side_of_a_step_boundary_return_the_table_exactly(rate):
    """Stream 0: one frame of 1.0 at A(1) - 1, the last frame step 0 consumes (step 1 sees it among its carried frames). Stream 1: one at A(1), the first frame of
    step 1's row (step 0's last outputs do not reach it, step 1's first ones read it through their right halves). One product with 1.0 and zeros is exact in any order."""
    eng = sub("engine")
    S, C = 960, 3
    L, M, W, c32 = eng.resample_table(rate)
    T = 2 * W + 1
    P, a1 = RS.pitch(S, rate), RS.start(S, rate, 1)
    where = [a1 - 1, a1]
    audio = np.full((C, 2, P), np.nan, np.float32)
    for stream, i in enumerate(where):
        x = np.zeros(RS.start(S, rate, C), np.float32)
        x[i] = 1.0
        for c in range(C):
            audio[c, stream, :RS.need(S, rate, c)] = x[RS.start(S, rate, c):RS.start(S, rate, c + 1)]
    out, frames, _ = eng.op_resample_stream(audio, np.ones((C, 2), np.int32), rate, chunk=S)
    n = np.arange(C * S)
    for stream, i in enumerate(where):
        k = i - (n * M) // L + W
        ok = (k >= 0) & (k < T)
        want = np.where(ok, c32[(n * M) % L, np.clip(k, 0, T - 1)], np.float32(0))
        got = out[:, stream].reshape(-1)
        assert ok[:S].any() == (stream == 0) and ok[S:2 * S].any()       # step 1 reads both; step 0 reads its own last frame and never the next row's first
        assert np.count_nonzero(want[ok]) > ok.sum() // 2                # not vacuous: most outputs that see the impulse are non-zero
        assert np.array_equal(got, want), (rate, i, np.flatnonzero(got != want)[:8])
