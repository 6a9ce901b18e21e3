"""CPU: the float64 statement of the device resampler (tests/resample_ref.py) checked from itself -- the filter's dimensions, its frequency response, the
output-count rule and a sine through it. Nothing here needs the library; the GPU tests (test_resample_gpu.py) hold the kernel against this statement."""
import numpy as np
import pytest

import resample_ref as R


@pytest.mark.parametrize("rate", R.RATES)
def test_design_dimensions(rate):
    L, M, W, T, _ = R.design(rate)
    assert (L, M, W, T) == R.DESIGN[rate]
    assert R.table(rate).shape == (L, T)


@pytest.mark.parametrize("rate", R.RATES + (16000,))
def test_library_table_is_this_design(rate):
    """The table is host code (double, rounded once), so the library's own copy can be held against the statement without a device: the dimensions, and every
    entry within one rounding to float32 (2^-24 relative) plus the difference between two double-precision sines (1e-12)."""
    from conftest import sub
    L, M, W, coeffs = sub("engine").resample_table(rate)
    assert (L, M, W) == R.design(rate)[:3]
    c64 = R.table(rate)
    assert coeffs.dtype == np.float32 and coeffs.shape == c64.shape
    assert np.all(np.abs(coeffs.astype(np.float64) - c64) <= 2.0 ** -24 * np.abs(c64) + 1e-12)


@pytest.mark.parametrize("rate", R.RATES)
def test_frequency_response_and_phase_sums(rate):
    """Conditions on the design (the design's own figures: 0.0002 dB, -92.3 dB or lower, 6.5e-6)."""
    L, M, _, _, _ = R.design(rate)
    c = R.table(rate)
    f, db = R.response_db(c)
    narrow = min(1.0, L / M)                                 # the narrower Nyquist in units of the input's
    passband, stopband = np.abs(db[f <= 0.85 * narrow]).max(), db[f >= 1.06 * narrow].max()
    sums = np.abs(c.sum(axis=1) - 1.0).max()
    print(f"{rate} Hz: passband {passband:.6f} dB, stopband {stopband:.2f} dB, phase sums within {sums:.2e}")
    assert passband <= 0.001
    assert stopband <= -90.0
    assert sums <= 1e-5


@pytest.mark.parametrize("rate", R.RATES + (16000,))
def test_output_count_rule(rate):
    L, M = R.design(rate)[:2]
    for n_in in (0, 1, M - 1, M, M + 1):
        want = int(np.ceil(n_in * L / M))
        assert R.n_out(n_in, rate) == want
        y, mag = R.resample(np.ones(n_in), rate)
        assert y.size == want and mag.size == want


def test_equal_rates_are_the_identity_and_stereo_is_the_mean():
    x = np.random.default_rng(0).standard_normal((37, 2))
    y, _ = R.resample(R.mono(x), 16000)
    assert np.array_equal(y, (x[:, 0] + x[:, 1]) / 2)
    pcm = np.array([[-32768, 32767], [100, -100]], dtype=np.int16)
    assert np.array_equal(R.mono(pcm, int16_scale=True), np.array([-0.5 / 32768, 0.0]))
    assert np.array_equal(R.mono(pcm), np.array([-0.5, 0.0]))


def test_impulse_returns_the_table():
    """x = 1 at frame i: output n is c[(n M) mod L][i - floor(n M / L) + W] where that tap exists, zero elsewhere."""
    for rate in (8000, 48000, 44100):
        L, M, W, T, _ = R.design(rate)
        c = R.table(rate)
        x = np.zeros(500)
        x[123] = 1.0
        y, _ = R.resample(x, rate)
        n = np.arange(y.size)
        k = 123 - (n * M) // L + W
        ok = (k >= 0) & (k < T)
        want = np.where(ok, c[(n * M) % L, np.clip(k, 0, T - 1)], 0.0)
        assert np.array_equal(y, want)


def test_sine_at_48k_comes_out_as_the_sine_at_16k():
    """1 kHz is far inside the passband. The reference gives 3.75e-6 (the passband ripple of a beta-9 Kaiser window); the bound is twice that."""
    W = R.design(48000)[2]
    x = np.sin(2 * np.pi * 1000 * np.arange(12000) / 48000)
    y, _ = R.resample(x, 48000)
    assert y.size == 4000
    err = np.abs(y - np.sin(2 * np.pi * 1000 * np.arange(4000) / 16000))[W:-W].max()
    print(f"sine: max error away from the edges {err:.3e}")
    assert err <= 7.5e-6
