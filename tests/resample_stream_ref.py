"""The streaming input format's statement (numpy only; include/asr_mi355x.h), on top of the offline statement tests/resample_ref.py.

A stream's model-rate signal is resample_ref.resample of all its input frames. With chunk S and the design (L, M, W, T = 2 W + 1) of rate_in -> rate_model:

    hi(c)   = floor(((c + 1) S - 1) M / L) + W      the last input frame outputs [c S, (c + 1) S) read
    A(0)    = 0,  A(c) = hi(c - 1) + 1              step c consumes frames [A(c), A(c + 1))
    need(c) = hi(c) + 1 - A(c)
    pitch   = max(need(0), floor(S M / L) + 1)
    reach(c) = A(c) - (floor(c S M / L) - W)        frames in front of A(c) the step's first output reads (0 at c = 0: they are zeros)
"""
import numpy as np

import resample_ref as R


def hi(S, rate, c, model=16000):
    L, M, W = R.design(rate, model)[:3]
    return ((c + 1) * S - 1) * M // L + W


def start(S, rate, c, model=16000):
    return 0 if c == 0 else hi(S, rate, c - 1, model) + 1


def need(S, rate, c, model=16000):
    return hi(S, rate, c, model) + 1 - start(S, rate, c, model)


def pitch(S, rate, model=16000):
    L, M = R.design(rate, model)[:2]
    return max(need(S, rate, 0, model), S * M // L + 1)


def reach(S, rate, c, model=16000):
    L, M, W = R.design(rate, model)[:3]
    return 0 if c == 0 else start(S, rate, c, model) - (c * S * M // L - W)


def resample_chunks(x, S, rate, C, model=16000, c64=None):
    """x float64 mono of A(C) frames -> the C S outputs computed step by step from (the last 2 W frames carried | the step's own frames), float64, terms added in
    tap order as resample_ref.resample adds them."""
    L, M, W, T, _ = R.design(rate, model)
    c = R.table(rate, model) if c64 is None else c64
    x = np.asarray(x, dtype=np.float64)
    assert x.size == start(S, rate, C, model)
    carried, out = np.zeros(2 * W), []
    for step in range(C):
        a0, a1 = start(S, rate, step, model), start(S, rate, step + 1, model)
        buf = np.concatenate([carried, x[a0:a1]])                  # buf[0] is the stream's frame a0 - 2 W
        n = np.arange(step * S, (step + 1) * S, dtype=np.int64)
        i0, p = (n * M) // L - W - (a0 - 2 * W), (n * M) % L
        assert i0.min() >= 0 and i0.max() + T - 1 < buf.size
        y = np.zeros(n.size)
        for k in range(T):
            y += c[p, k] * buf[i0 + k]
        out.append(y)
        carried = buf[buf.size - 2 * W:] if W else buf[:0]
    return np.concatenate(out)
