"""Pause-aware segmentation of long audio: the host side of the device VAD (engine.op_vad, csrc/vad.hip).

A file goes in as int16 frames at its own rate; `segment` asks the detector where the speech is, `pack` lays the kept frames out as one ragged batch, and
`plan_batches` groups the segments into session calls in file order. `run_long` is the loop the transcribers' `transcribe_long` share: segments in, one
result per segment out, every time in it shifted to seconds of the file. Nothing is resampled here: the detector works at the file's rate and a session
with an input format set resamples only what is kept.
"""
from __future__ import annotations

import numpy as np

from . import engine
from .input_format import as_frames, ratio


def limit_frames(max_model_samples: int, sample_rate: int, model_rate: int) -> int:
    """The longest run of input frames that the resampler turns into at most max_model_samples: floor(max * M / L)."""
    L, M = ratio(sample_rate, model_rate)
    return int(max_model_samples) * M // L


def segment(audio, rate: int, channels: int = 1, params: engine.VadParams | None = None, full_scale: float = 32768.0, max_input_frames: int | None = None):
    """One file -> (segments [S, 2] int64 input-frame offsets in file order, info). audio: frames [n, channels] (or flat interleaved) of int16 / float32 /
    float16. max_input_frames: no segment is longer (a transcriber's window); the parameters' own max_seconds also holds.
    info = {"audio_seconds", "speech_seconds", "floor", "peak", "thr"} (the three levels as asr_op_vad's stats)."""
    a = np.ascontiguousarray(audio)
    n = a.size // channels
    if a.size % channels:
        raise ValueError(f"{a.size} samples are not frames of {channels} interleaved channels")
    params = params if params is not None else engine.VadParams()
    H = engine.vad_hop(rate)
    pc = params.to_c(rate, full_scale, None if max_input_frames is None else max(2, int(max_input_frames) // H))
    seg, _, _, _, _, stats = engine.op_vad(a.reshape(-1), np.array([0, n], dtype=np.int64), rate=rate, channels=channels, params=pc, details=True)
    info = {"audio_seconds": n / rate, "speech_seconds": float((seg[:, 1] - seg[:, 0]).sum()) / rate,
            "floor": int(stats[0, 0]), "peak": int(stats[0, 1]), "thr": int(stats[0, 2])}
    return seg, info


def pack(audio, segments, channels: int = 1):
    """The frames of `segments` ([S, 2] frame offsets) of one file, back to back -> (packed flat samples, offsets [S + 1] in frames from 0)."""
    a = np.ascontiguousarray(audio).reshape(-1, channels)
    segments = np.asarray(segments, dtype=np.int64).reshape(-1, 2)
    offs = np.zeros(segments.shape[0] + 1, dtype=np.int64)
    offs[1:] = np.cumsum(segments[:, 1] - segments[:, 0])
    parts = [a[s:e].reshape(-1) for s, e in segments]
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=a.dtype)), offs


def plan_batches(segments, max_batch: int, max_frames_total: int):
    """Segments -> [(first, end)] index ranges, in file order: a batch holds at most max_batch segments and at most max_frames_total frames (a single longer
    segment is a batch of its own)."""
    if max_batch < 1 or max_frames_total < 1:
        raise ValueError("plan_batches: max_batch and max_frames_total are positive")
    segments = np.asarray(segments, dtype=np.int64).reshape(-1, 2)
    out, first, total = [], 0, 0
    for i, (s, e) in enumerate(segments):
        n = int(e - s)
        if i > first and (i - first == max_batch or total + n > max_frames_total):
            out.append((first, i))
            first, total = i, 0
        total += n
    if segments.shape[0] > first:
        out.append((first, segments.shape[0]))
    return out


_TIMED_LISTS = ("tokens", "segments", "words", "nbest")


def shift_times(result, by: float):
    """Every "start" / "end" and every "token_times" pair inside `result` (a per-call result: dicts and lists of dicts under tokens / segments / words /
    nbest) moved by `by` seconds, in place."""
    if isinstance(result, dict):
        for k in ("start", "end"):
            if isinstance(result.get(k), (int, float)) and not isinstance(result[k], bool):
                result[k] = by + result[k]
        if isinstance(result.get("token_times"), list):
            result["token_times"] = [(by + t0, by + t1) for t0, t1 in result["token_times"]]
        for k in _TIMED_LISTS:
            if isinstance(result.get(k), list):
                shift_times(result[k], by)
    elif isinstance(result, list):
        for r in result:
            if isinstance(r, (dict, list)):
                shift_times(r, by)
    return result


def run_long(audio_int16, vad, sample_rate: int | None, channels: int, model_rate: int, max_model_samples: int, prepare, run_batch, max_batch: int,
             max_frames_total: int | None = None):
    """The shared loop of transcribe_long. audio_int16: the file, frames [n, channels] (or flat) of int16 at sample_rate (None: the model's rate, mono).
    prepare(frames int16 [n, channels]) -> the same frames in the session's sample type; run_batch(prepared frames, segments [b, 2]) -> one result dict per
    segment with "token_ids" (and times in seconds from the segment's start). -> (segment records [{"start", "end", ...result}], info); no segment: no call."""
    rate = int(model_rate if sample_rate is None else sample_rate)
    frames = as_frames(audio_int16, channels)
    limit = limit_frames(max_model_samples, rate, model_rate)
    segs, info = segment(frames, rate, channels, vad, 32768.0, limit)
    records = []
    if segs.shape[0]:
        prepared = prepare(frames)
        for first, end in plan_batches(segs, max_batch, max_frames_total if max_frames_total is not None else max_batch * limit):
            for (s, e), res in zip(segs[first:end], run_batch(prepared, segs[first:end])):
                start = int(s) / rate
                records.append({"start": start, "end": int(e) / rate, **shift_times(res, start)})
    return records, info
