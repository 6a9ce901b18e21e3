"""Host side of a session's input format (engine set_input_format: audio at another sample rate / with interleaved channels, resampled on the device).

The transcribers take `sample_rate=None, channels=1`: None is the default format and changes nothing; otherwise the session's format is set for the
call and restored behind it, clips are frames [n, channels] of int16, and the windowed loops cut their windows in input frames -- a window of `window`
model-rate samples is `window * M / L` frames (L / M the reduced rate ratio), which has to be an integer, so that every window comes out of the
resampler exactly `window` samples long. Seconds in results come from model-rate samples and rows and do not change.
"""
from __future__ import annotations

import math
from contextlib import contextmanager

import numpy as np


def ratio(sample_rate: int, model_rate: int) -> tuple[int, int]:
    """(L, M): rate_model / g, sample_rate / g."""
    g = math.gcd(int(sample_rate), int(model_rate))
    return int(model_rate) // g, int(sample_rate) // g


def model_samples(frames: int, sample_rate: int, model_rate: int) -> int:
    """ceil(frames * L / M): what the resampler makes of `frames` input frames."""
    L, M = ratio(sample_rate, model_rate)
    return -((-int(frames) * L) // M)


def input_frames(samples: int, sample_rate: int, model_rate: int, what: str = "window") -> int:
    """`samples` model-rate samples as input frames, samples * M / L; ValueError when that is no integer."""
    L, M = ratio(sample_rate, model_rate)
    if (int(samples) * M) % L:
        raise ValueError(f"{what} of {samples} samples at {model_rate} Hz is {samples * M / L:.3f} frames at {sample_rate} Hz: not an integer "
                         f"(choose a multiple of {L // math.gcd(L, M)})")
    return int(samples) * M // L


def half_width(sample_rate: int, model_rate: int) -> int:
    """W of the resampler's filter (asr_resample_table): ceil(32 / fc) input frames, fc = 0.945 min(1, L / M); 0 at equal rates (the pure down-mix)."""
    L, M = ratio(sample_rate, model_rate)
    if L == M:
        return 0
    return math.ceil(32.0 / (0.945 * min(1.0, L / M)))


def _stream_hi(chunk: int, L: int, M: int, W: int, step: int) -> int:
    return ((int(step) + 1) * int(chunk) - 1) * M // L + W


def stream_start(chunk: int, sample_rate: int, model_rate: int, step: int) -> int:
    """A(step): the first input frame the stream's step `step` (0, 1, .. since its reset) consumes. A(0) = 0, A(c) = hi(c - 1) + 1 with
    hi(c) = floor(((c + 1) chunk - 1) M / L) + W, the last frame the step's outputs [c chunk, (c + 1) chunk) read."""
    L, M = ratio(sample_rate, model_rate)
    return 0 if step <= 0 else _stream_hi(chunk, L, M, half_width(sample_rate, model_rate), step - 1) + 1


def stream_frames(chunk: int, sample_rate: int, model_rate: int, step: int) -> int:
    """need(step) = hi(step) + 1 - A(step): the frames a streaming session with this format reads from a stream's row at that step. The first step takes W
    frames more than the later ones (the look-ahead)."""
    L, M = ratio(sample_rate, model_rate)
    return _stream_hi(chunk, L, M, half_width(sample_rate, model_rate), step) + 1 - stream_start(chunk, sample_rate, model_rate, step)


def stream_pitch(chunk: int, sample_rate: int, model_rate: int) -> int:
    """Frames per row of a formatted step's audio: max(need(0), floor(chunk M / L) + 1), at least every step's need."""
    L, M = ratio(sample_rate, model_rate)
    return max(stream_frames(chunk, sample_rate, model_rate, 0), int(chunk) * M // L + 1)


def as_frames(audio_int16, channels: int) -> np.ndarray:
    """int16 frames [n, channels] of a clip given as [n, channels] or flat interleaved."""
    a = np.asarray(audio_int16, dtype=np.int16)
    if a.ndim == 2 and a.shape[1] == channels:
        return np.ascontiguousarray(a)
    if a.size % channels:
        raise ValueError(f"{a.size} samples are not frames of {channels} interleaved channels")
    return np.ascontiguousarray(a.reshape(-1, channels))


def cut_windows(frames: np.ndarray, window: int | None, stride: int, sample_rate: int, model_rate: int):
    """The windowed loop's cuts in input frames -> (window in model samples, [(start in model samples, frames of the window)]). window None: the whole clip
    as one window (a dynamic audio axis). Otherwise windows of `window` model samples every `stride`, the tail zero-padded, as the reference's loops pad
    (Inference_SenseVoice_ONNX.py:243-260); both must be whole numbers of input frames."""
    n = frames.shape[0]
    if window is None:
        return model_samples(n, sample_rate, model_rate), [(0, frames)]
    w_in, s_in = input_frames(window, sample_rate, model_rate, "a window"), input_frames(stride, sample_rate, model_rate, "a stride")
    n_win = 1 if n <= w_in else -(-(n - w_in) // s_in) + 1
    need = (n_win - 1) * s_in + w_in
    if need > n:
        frames = np.concatenate([frames, np.zeros((need - n, frames.shape[1]), dtype=frames.dtype)])
    return int(window), [(k * int(stride), frames[k * s_in:k * s_in + w_in]) for k in range(n_win)]


@contextmanager
def session_input_format(sess, sample_rate: int | None, channels: int = 1):
    """Set `sess`'s input format for one call and put back what was in force; sample_rate None: leave the session alone (yields False)."""
    if sample_rate is None:
        if channels != 1:
            raise ValueError("channels needs sample_rate: an input format is (sample rate, channels)")
        yield False
        return
    before = sess.input_format
    sess.set_input_format(int(sample_rate), int(channels))
    try:
        yield True
    finally:
        sess.set_input_format(*before)
