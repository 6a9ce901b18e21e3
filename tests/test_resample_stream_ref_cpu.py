"""CPU: the arithmetic of the streaming input format (tests/resample_stream_ref.py) checked from itself and against the offline float64 statement, and the host
functions of input_format against it. Nothing here needs a GPU; test_resample_stream_gpu.py holds the kernels against this statement."""
import numpy as np
import pytest

import resample_ref as R
import resample_stream_ref as RS
from conftest import sub

RATES = (8000, 11025, 22050, 32000, 44100, 48000)
CHUNKS = (960, 8000)
STEPS = 400


@pytest.mark.parametrize("S", CHUNKS)
@pytest.mark.parametrize("rate", RATES)
def test_step_ranges_tile_the_stream_and_reach_back_two_half_widths_at_most(rate, S):
    L, M, W = R.design(rate)[:3]
    P = RS.pitch(S, rate)
    at = 0
    for c in range(STEPS):
        assert RS.start(S, rate, c) == at                           # no gap, no overlap
        n = RS.need(S, rate, c)
        assert 0 < n <= P
        assert RS.reach(S, rate, c) <= 2 * W
        at += n
        C = c + 1
        assert at == RS.start(S, rate, C)
        assert -((-at * L) // M) >= C * S                           # the offline resampler makes at least C S outputs of A(C) frames
    later = {RS.need(S, rate, c) for c in range(1, STEPS)}
    assert len(later) <= 2 and max(later) - min(later) <= 1
    assert abs(RS.need(S, rate, 0) - W - min(later)) <= M // L + 1     # the first step takes the look-ahead, W frames, on top (up to the rounding of one output)


def test_the_counts_of_the_contract():
    want = {48000: (24100, {24000}), 44100: (22142, {22050}), 11025: (5546, {5512, 5513}), 8000: (4034, {4000})}
    for rate, (first, later) in want.items():
        assert RS.need(8000, rate, 0) == first
        assert {RS.need(8000, rate, c) for c in range(1, STEPS)} == later


@pytest.mark.parametrize("S", CHUNKS)
@pytest.mark.parametrize("rate", RATES)
def test_chunk_by_chunk_float64_equals_the_offline_statement_exactly(rate, S):
    C = 5 if S == 960 else 2
    rng = np.random.default_rng(rate + S)
    x = rng.standard_normal(RS.start(S, rate, C))
    c64 = R.table(rate)
    whole, _ = R.resample(x, rate, c64=c64)
    got = RS.resample_chunks(x, S, rate, C, c64=c64)
    assert got.size == C * S and np.count_nonzero(got) > got.size // 2
    assert np.array_equal(got, whole[:C * S])


@pytest.mark.parametrize("S", CHUNKS + (961,))
@pytest.mark.parametrize("rate", RATES + (16000,))
def test_input_format_host_functions_are_the_reference(rate, S):
    fmt = sub("input_format")
    assert fmt.half_width(rate, 16000) == R.design(rate)[2]
    assert fmt.stream_pitch(S, rate, 16000) == RS.pitch(S, rate)
    for c in list(range(40)) + [STEPS - 1, 10 ** 6]:
        assert fmt.stream_frames(S, rate, 16000, c) == RS.need(S, rate, c)
        assert fmt.stream_start(S, rate, 16000, c) == RS.start(S, rate, c)
