"""The energy VAD's statement (numpy only): what csrc/vad.hip computes, written from its definition. Energies are float64; everything after them is integer.

    H = max(1, (rate + 50) // 100) input frames per analysis frame;  F = ceil(n / H)
    e[f] = sum x[i]^2, i in [f H, min(n, f H + H)),  x = the widened channel mean
    q[f] = min(1023, (bits(max(float32(e[f]), 2^-40)) >> 20) - (bits(2^-40) >> 20))            8 steps per octave
    floor = the lowest level whose cumulative count reaches ceil(p_floor F);  peak = max q;  thr = max(abs_level, min(floor + margin, peak - peak_drop))
    m[f] = q[f] >= thr;  (a) speech runs < min_speech cleared  (b) pauses < min_pause between two speech runs set  (c) every run grows by pad, touching runs are one
    a run longer than max_frames: while end - start > max_frames, cut at the latest frame of lowest q in [start + max_frames // 2, start + max_frames]
    segments (start H, min(n, end H)) in input frames
"""
import math
from dataclasses import dataclass

import numpy as np

LEVELS = 1024
Q0 = (87 << 23) >> 20           # bits(2^-40) >> 20
MAX_F = 1 << 20


@dataclass
class Params:
    """asr_vad_params: analysis frames and level steps."""
    p_floor: float = 0.10
    margin: int = 24
    peak_drop: int = 16
    abs_level: int = 0
    min_speech: int = 10
    min_pause: int = 50
    pad: int = 10
    max_frames: int = 3000


def hop(rate):
    return max(1, (rate + 50) // 100)


def level(e):
    """float32 energies -> int levels (the bit rule; a NaN takes the floor)."""
    e = np.asarray(e, dtype=np.float32)
    m = np.where(e > np.float32(2.0 ** -40), e, np.float32(2.0 ** -40)).astype(np.float32)
    return np.minimum(LEVELS - 1, (m.view(np.uint32) >> 20).astype(np.int64) - Q0)


def default_params(rate, full_scale, max_frames=3000):
    a = hop(rate) * (float(np.float32(full_scale)) * 1e-3) ** 2          # H (full_scale 10^(-60/20))^2 in double, rounded once to f32, as the library
    return Params(abs_level=int(level(np.float32(a))), max_frames=max_frames)


def mono(frames):
    """[n, C] (or [n]) samples -> the float64 channel mean of the widened samples (no scale: full_scale says what the values mean)."""
    w = np.asarray(frames).astype(np.float64)
    return w if w.ndim == 1 else w.sum(axis=1) / w.shape[1]


def n_frames(n, H):
    return -(-int(n) // H)


def energies(x, H):
    """x float64 mono [n] -> (e [F] float64, mag [F] = the same sum: the scale of frame f's rounding error)."""
    x = np.asarray(x, dtype=np.float64)
    F = n_frames(x.size, H)
    xp = np.zeros(F * H)
    xp[:x.size] = x
    e = (xp * xp).reshape(F, H).sum(axis=1) if F else np.zeros(0)
    return e, e


def stats(q, p):
    """-> (floor, peak, thr); F == 0 gives floor = peak = 0."""
    q = np.asarray(q, dtype=np.int64)
    F = q.size
    if F == 0:
        floor = peak = 0
    else:
        need = min(F, max(1, math.ceil(float(np.float32(p.p_floor)) * F)))
        cum = np.cumsum(np.bincount(q, minlength=LEVELS))
        floor = int(np.argmax(cum >= need))
        peak = int(q.max())
    return floor, peak, max(p.abs_level, min(floor + p.margin, peak - p.peak_drop))


def runs_of(mask):
    """bool [F] -> [(start, end)] of its True runs."""
    m = np.concatenate([[0], np.asarray(mask, dtype=np.int8), [0]])
    d = np.diff(m)
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def padded_runs(q, thr, p):
    """Rules (a), (b), (c) on the mask q >= thr -> [(start, end)] in analysis frames, before any cut."""
    F = len(q)
    runs = [r for r in runs_of(np.asarray(q) >= thr) if r[1] - r[0] >= p.min_speech]                     # (a)
    merged = []
    for s, e in runs:                                                                                     # (b)
        if merged and s - merged[-1][1] < p.min_pause:
            merged[-1][1] = e
        else:
            merged.append([s, e])
    out = []
    for s, e in merged:                                                                                   # (c)
        s, e = max(0, s - p.pad), min(F, e + p.pad)
        if out and s <= out[-1][1]:
            out[-1][1] = e
        else:
            out.append([s, e])
    return [(s, e) for s, e in out]


def split_runs(runs, q, max_frames):
    q = np.asarray(q, dtype=np.int64)
    segs = []
    for s, e in runs:
        while e - s > max_frames:
            lo, hi = s + max_frames // 2, s + max_frames
            w = q[lo:hi + 1]
            c = lo + (w.size - 1 - int(np.argmin(w[::-1])))                                               # the latest minimum
            segs.append((s, c))
            s = c
        segs.append((s, e))
    return segs


def stage2(e32, n, H, p):
    """The integer half: float32 energies [F] of an utterance of n input frames -> (q, (floor, peak, thr), segments [S, 2] int64 in input frames)."""
    q = level(e32)
    st = stats(q, p)
    segs = split_runs(padded_runs(q, st[2], p), q, p.max_frames)
    out = np.array([(s * H, min(n, e * H)) for s, e in segs], dtype=np.int64).reshape(-1, 2)
    return q, st, out


def check_params(rate, channels, p):
    return rate >= 100 and 1 <= channels <= 8 and p.max_frames >= 2 and 0.0 < p.p_floor <= 1.0


def vad(frames, rate, p):
    """One utterance, float64 energies rounded once to float32 -> (e64, q, stats, segments)."""
    H = hop(rate)
    x = mono(frames)
    e64, _ = energies(x, H)
    q, st, segs = stage2(e64.astype(np.float32), x.size, H, p)
    return e64, q, st, segs
