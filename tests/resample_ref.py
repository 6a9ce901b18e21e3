"""The device resampler's statement in float64 (numpy only): the polyphase Kaiser-windowed sinc of csrc/resample.hip, written from its formula.

    g = gcd(rate_in, rate_model), L = rate_model / g, M = rate_in / g, fc = 0.945 min(1, L / M), W = ceil(32 / fc), T = 2 W + 1
    c[p][k] = fc sinc(t) I0(9 sqrt(1 - (t / 32)^2)) / I0(9),  t = ((k - W) - p / L) fc,  0 at |t| >= 32
    n_out = ceil(n_in L / M);  y[n] = sum_k c[(n M) mod L][k] x[floor(n M / L) - W + k],  x zero outside the utterance's own frames
    C channels: x[i] = (x[i][0] + ... + x[i][C - 1]) (1 / C)

rate_in == rate_model is the pure down-mix L = M = T = 1, W = 0, c = 1.
"""
import math

import numpy as np

RATES = (8000, 48000, 44100, 22050, 11025)
# rate_in -> (L, M, W, T) at a 16 kHz model
DESIGN = {8000: (2, 1, 34, 69), 48000: (1, 3, 102, 205), 44100: (160, 441, 94, 189), 22050: (320, 441, 47, 95), 11025: (640, 441, 34, 69)}


def bessel_i0(x):
    """I0 by its series sum_k ((x / 2)^k / k!)^2, elementwise."""
    x = np.asarray(x, dtype=np.float64)
    term, total = np.ones_like(x), np.ones_like(x)
    for k in range(1, 200):
        term = term * (0.5 * x) / k
        total = total + term * term
    return total


def design(rate_in, rate_model=16000):
    """-> (L, M, W, T, fc)"""
    if rate_in == rate_model:
        return 1, 1, 0, 1, 1.0
    g = math.gcd(rate_in, rate_model)
    L, M = rate_model // g, rate_in // g
    fc = 0.945 * min(1.0, L / M)
    W = math.ceil(32 / fc)
    return L, M, W, 2 * W + 1, fc


def table(rate_in, rate_model=16000):
    """c[L][T] float64"""
    L, M, W, T, fc = design(rate_in, rate_model)
    if T == 1:
        return np.ones((1, 1))
    k = np.arange(T, dtype=np.float64)[None, :]
    p = np.arange(L, dtype=np.float64)[:, None]
    t = ((k - W) - p / L) * fc
    inside = np.abs(t) < 32
    r = np.where(inside, t / 32, 0.0)
    c = fc * np.sinc(t) * bessel_i0(9 * np.sqrt(1 - r * r)) / bessel_i0(9.0)
    return np.where(inside, c, 0.0)


def n_out(n_in, rate_in, rate_model=16000):
    L, M = design(rate_in, rate_model)[:2]
    return -((-int(n_in) * L) // M)


def widen(x, int16_scale=False):
    """What Pcm<S>::widen makes of a sample, exactly: float32 of the value, int16 times 2^-15 where the flag says so."""
    x = np.asarray(x)
    w = x.astype(np.float64)
    return w * 2.0 ** -15 if (x.dtype == np.int16 and int16_scale) else w


def mono(frames, int16_scale=False):
    """[n, C] (or [n]) samples -> the float64 channel mean."""
    w = widen(frames, int16_scale)
    return w if w.ndim == 1 else w.sum(axis=1) / w.shape[1]


def resample(x, rate_in, rate_model=16000, c64=None):
    """One utterance: x float64 mono [n_in] -> (y [n_out], mag [n_out]) with mag[n] = sum_k |c[p][k]| |x[.]|, the scale of output n's rounding error."""
    L, M, W, T, _ = design(rate_in, rate_model)
    c = table(rate_in, rate_model) if c64 is None else c64
    x = np.asarray(x, dtype=np.float64)
    n = np.arange(n_out(x.size, rate_in, rate_model), dtype=np.int64)
    i0, p = (n * M) // L, (n * M) % L
    xp = np.concatenate([np.zeros(W), x, np.zeros(W + 1)])          # xp[i + W] = x[i]
    y, mag = np.zeros(n.size), np.zeros(n.size)
    for k in range(T):                                               # y[n] += c[p][k] x[i0 - W + k]   (i0 <= n_in - 1, so i0 + k stays inside xp)
        term = c[p, k] * xp[i0 + k]
        y += term
        mag += np.abs(term)
    return y, mag


def response_db(c, oversample=16):
    """The gain of the prototype filter the phases interleave to -> (f, dB): tap (p, k) sits at time (k - W) - p / L input frames, so the phases together are one
    FIR at L x rate_in with taps 1 / L apart and DC gain L. f is in units of the INPUT Nyquist and runs to L (the prototype's own Nyquist): an interpolator has to
    reject every image up to there. Evaluated by a zero-padded FFT, `oversample` points per tap-count bin."""
    L, T = c.shape
    W = (T - 1) // 2
    m = ((np.arange(T)[None, :] - W) * L - np.arange(L)[:, None]).reshape(-1)      # tap times in units of 1 / L input frames
    h = np.zeros(m.max() - m.min() + 1)
    h[m - m.min()] = c.reshape(-1)
    N = 1 << int(np.ceil(np.log2(h.size * oversample)))
    H = np.abs(np.fft.rfft(h, N)) / L
    f = 2.0 * L * np.arange(H.size) / N
    return f, 20 * np.log10(np.maximum(H, 1e-300))
