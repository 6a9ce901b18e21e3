"""GPU, op level: the CTC head with frame log-probabilities (asr_probe_ctc_head: arg-max GEMM epilogue with the sum-of-exponentials partial + row reduce)
against the float64 statement of the bf16-rounded operands (tests/ctc_timing_ref.py), on each kernel form the dispatcher can pick for the head, at the
smallest shapes its own rules send there (K = 512):
  pp_amax     M >= 1024, ceil(M / 256) * (N / 256) >= 0.8 * 256 tiles, M >= 0.9 * the padded rows  ->  M = 1160 (5 row tiles, the last 136 rows), N = 10496
  t288w_amax  ASR_GEMM_AMAX_PP=0, M >= 2304, ceil(M / 288) * (N / 256) >= 1024 tiles                ->  M = 4610 (17 row tiles, the last 2 rows), N = 15616
  pipe        variant 2 (128 x 128 tiles), any M                                                    ->  M = 130, N = 640
The float64 reference is evaluated on a subset of the rows of the two large forms (every row kind, the first tile, the last rows); ids are compared on
all rows with asr_probe_gemm's arg-max of the same operands. The budget is ctc_timing_ref.budget: derived, not tuned."""
import functools

import numpy as np
import pytest

import ctc_timing_ref as R
from conftest import sub

pytestmark = pytest.mark.gpu

FORMS = {"pp_amax": (1160, 10496, -1, None), "t288w_amax": (4610, 15616, -1, "0"), "pipe": (130, 640, 2, None)}
# n_valid: a multiple of 64 with two wholly invalid slabs behind it; 64 k + 1 with a wholly invalid slab behind the one-column slab; the usual ragged tail
TAILS = {"mult64": lambda N: N - 128, "64k+1": lambda N: N - 127, "ragged": lambda N: N - 33}


@functools.lru_cache(maxsize=2)
def _case(form, tail):
    M, N, variant, env = FORMS[form]
    n_valid = TAILS[tail](N)
    a, w, bias, kinds = R.head_operands(len(form) * 7 + len(tail), M, N, n_valid)
    rows = np.arange(M) if M <= 512 else np.unique(np.concatenate([np.arange(128), np.arange(M - 64, M), np.arange(0, M, 37)]))
    return a, w, bias, kinds, n_valid, rows, R.head_reference(a, w, bias, n_valid, rows)


@pytest.mark.parametrize("tail", sorted(TAILS))
@pytest.mark.parametrize("form", sorted(FORMS))
def test_frame_logprob_within_budget(form, tail, monkeypatch):
    probe = sub("_probe")
    M, N, variant, env = FORMS[form]
    if env is not None:
        monkeypatch.setenv("ASR_GEMM_AMAX_PP", env)
    a, w, bias, kinds, n_valid, rows, (ref_ids, ref_lp, spread, abs_dot, vmax) = _case(form, tail)
    assert (n_valid % 64 == 0) == (tail == "mult64") and (n_valid % 64 == 1) == (tail == "64k+1") and (N - n_valid >= 64) == (tail != "ragged")
    ids, lp, stray, kern = probe.ctc_head(a, w, bias, n_valid=n_valid, variant=variant)
    assert kern == form, kern
    assert M % {"pp_amax": 256, "t288w_amax": 288, "pipe": 128}[form] != 0
    assert stray == 0, f"{stray} words written in rows past M"
    plain, kern2 = probe.gemm(a, w, bias, argmax=True, n_valid=n_valid, variant=variant)
    assert kern2 == form and np.array_equal(ids, plain["ids"])             # the (max, index) partials and their tie rule are untouched
    assert np.isfinite(lp).all() and (lp <= 0).all()
    b = R.budget(n_valid, ref_lp, spread, R.HEAD_K, abs_dot, vmax)
    err = np.abs(lp[rows].astype(np.float64) - ref_lp)
    worst = int(np.argmax(err / b))
    print(f"ctc_head {form} {tail}: max err/budget {float((err / b).max()):.3f} (row {rows[worst]} {kinds[rows[worst]]}, err {err[worst]:.2e}, budget {b[worst]:.2e}); max budget {b.max():.2e}")
    assert b.max() < 1e-3
    assert (err <= b).all(), (rows[worst], kinds[rows[worst]], err[worst], b[worst])
    # the float64 arg-max agrees wherever its margin clears the logits' own error; the planted rows' arg-max is one of the two peaks
    for r, m in enumerate(rows):
        kind = kinds[m]
        if kind == "equal":
            assert ids[m] == 0 and abs(lp[m] + np.log(n_valid)) <= b[r]
        elif kind == "dominant":
            assert ids[m] == R.COL_TOP and -1e-6 < lp[m] <= 0
        elif kind.startswith("plant_"):
            assert ids[m] in (R.COL_TOP, R.COL_SLAB0, R.COL_RIGHT, n_valid - 1)
