"""Audio with a known answer for the VAD tests (CPU and GPU share it): planted sine bursts over noise, and clips whose frame levels follow a given pattern."""
import numpy as np

import vad_ref as V

RATE = 16000
NATURAL_CLIPS = ("zh_1", "shanghai8", "multitalk8")
PLANTED_F = 600
PLANTED_SPANS = [(40, 100), (200, 230), (400, 520)]          # analysis frames; the pauses between them are longer than min_pause + 2 pad


def planted_audio():
    """int16 mono at 16 kHz: 440 Hz bursts at -20 dBFS on analysis-frame boundaries over -72 dBFS Gaussian noise -> (audio, spans in analysis frames)."""
    H = V.hop(RATE)
    rng = np.random.default_rng(20240)
    x = rng.standard_normal(PLANTED_F * H) * (32768.0 * 10.0 ** (-72 / 20))
    t = np.arange(PLANTED_F * H) / RATE
    tone = 32768.0 * 10.0 ** (-20 / 20) * np.sin(2 * np.pi * 440.0 * t)
    for s, e in PLANTED_SPANS:
        x[s * H:e * H] += tone[s * H:e * H]
    return np.round(x).astype(np.int16), PLANTED_SPANS


def planted_expected(pad, n):
    H = V.hop(RATE)
    return np.array([((s - pad) * H, min(n, (e + pad) * H)) for s, e in PLANTED_SPANS], dtype=np.int64)


def clip_from_amplitudes(amp, H):
    """One int16 mono clip whose analysis frame f is the constant amp[f]: its energy is H amp^2 exactly (below 2^24 for the values used here)."""
    return np.repeat(np.asarray(amp, dtype=np.int16), H)


def pattern_amplitudes(runs, rng, speech=(2000, 2400, 2900, 3500), pause=(2, 3)):
    """[(is_speech, length)] -> per-frame amplitudes: speech frames draw from a few loud values (so a cut window has ties), pauses from quiet ones."""
    out = []
    for is_speech, n in runs:
        out.append(rng.choice(speech if is_speech else pause, size=n))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def natural_with_gaps():
    """The three committed speech clips (tests/golden/audio_natural.npz) as int16 with 2 s of sigma = 8 LSB Gaussian noise between them
    -> (audio int16, [(start, end)] of the clips in samples)."""
    from helpers import load_golden
    g = load_golden("audio_natural")
    rng = np.random.default_rng(7)
    parts, spans, pos = [], [], 0
    for i, k in enumerate(NATURAL_CLIPS):
        if i:
            gap = np.round(rng.standard_normal(2 * RATE) * 8.0).astype(np.int16)
            parts.append(gap)
            pos += gap.size
        c16 = np.ascontiguousarray(g[k], dtype=np.int16)
        parts.append(c16)
        spans.append((pos, pos + c16.size))
        pos += c16.size
    return np.concatenate(parts), spans
