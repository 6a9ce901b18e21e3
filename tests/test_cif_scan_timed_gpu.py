"""GPU, operator level: the timed CIF scan (csrc/kernels.hip cif_scan_kernel<true>) through asr_op_cif_scan_timed on host arrays -- the fire rows and the
counts equal the rule's statement (paraformer_timing_ref.fire_frames) exactly, slots outside the contract keep the caller's fill."""
import numpy as np
import pytest

import paraformer_timing_ref as R
from conftest import sub

pytestmark = pytest.mark.gpu

FILL = -7
TAIL = 0.45


def _enc(seed, T, d):
    return np.random.default_rng(seed).standard_normal((T, d)).astype(np.float32)


def _check(fire, num, refs, max_tokens):
    for b, ref in enumerate(refs):
        n = min(len(ref), max_tokens)
        assert int(num[b]) == len(ref), (b, int(num[b]), len(ref))          # the full count, whatever max_tokens is
        assert np.array_equal(fire[b, :n], ref[:n]), (b, fire[b, :n], ref[:n])
        assert (fire[b, n:] == FILL).all(), b                               # nothing behind the tokens is written


@pytest.mark.parametrize("d", [1, 80, 512])
def test_hand_cases(d):
    """Every hand case as its own utterance of one ragged batch (T = 1 .. 8), for a one-column, a sub-wave-multiple and a wide embedding."""
    eng = sub("engine")
    names = sorted(R.FIRE_CASES)
    for tail in sorted({R.FIRE_CASES[n][1] for n in names}):
        group = [n for n in names if R.FIRE_CASES[n][1] == tail]
        alphas = [np.asarray(R.FIRE_CASES[n][0], np.float32) for n in group]
        lens = [a.size for a in alphas]
        enc = _enc(11 + d, sum(lens), d)
        ac, fire, num = eng.op_cif_scan_timed(np.concatenate(alphas), enc, lens, tail, fill=FILL)
        refs = [R.fire_frames(a, tail) for a in alphas]
        for n, ref in zip(group, refs):
            assert ref.tolist() == R.FIRE_CASES[n][2], n
        _check(fire, num, refs, max(lens) + 1)
        ac2, fire2, num2 = eng.op_cif_scan_timed(np.concatenate(alphas), enc, lens, tail, fill=FILL)
        assert np.array_equal(ac.view(np.uint32), ac2.view(np.uint32)) and np.array_equal(fire, fire2) and np.array_equal(num, num2)
        r = 0
        for n, a, ref in zip(group, alphas, refs):
            rows = ac[r:r + a.size]
            assert (rows[min(len(ref), a.size):] == 0).all(), n             # token rows first, zeros behind them
            if n == "ones":                                                 # alpha = 1: every row is its own token
                assert np.allclose(rows, enc[r:r + a.size], atol=1e-5)
            r += a.size


def test_ragged_batch_long_utterance_and_a_single_row():
    """T = 1 beside T = 700 (44 row tiles, several passes of the workgroup over d = 80): 343 tokens, the last fired by the tail threshold on row T;
    the one-row utterance fires on its tail row; then max_tokens below the count, and a zero-token utterance in the same batch."""
    eng = sub("engine")
    long_a = R.ragged_alphas()
    alphas = [np.asarray([0.6], np.float32), long_a, np.asarray([0.2, 0.1, 0.1], np.float32)]
    lens = [a.size for a in alphas]
    refs = [R.fire_frames(a, TAIL) for a in alphas]
    assert refs[0].tolist() == [1] and len(refs[1]) == 343 and refs[1][-1] == 700 and len(refs[2]) == 0
    enc = _enc(5, sum(lens), 80)
    ac, fire, num = eng.op_cif_scan_timed(np.concatenate(alphas), enc, lens, TAIL, fill=FILL)
    assert fire.shape == (3, 701)
    _check(fire, num, refs, 701)
    assert (np.diff(fire[1, :343]) > 0).all() and fire[1, 0] >= 0
    assert (ac[1 + 343:1 + 700] == 0).all() and np.abs(ac[1:1 + 343]).max() > 0 and (ac[701:] == 0).all()
    ac_b, fire_b, num_b = eng.op_cif_scan_timed(np.concatenate(alphas), enc, lens, TAIL, max_tokens=100, fill=FILL)
    _check(fire_b, num_b, refs, 100)
    assert np.array_equal(ac.view(np.uint32), ac_b.view(np.uint32))       # the embeddings do not depend on max_tokens
    ac_c, fire_c, num_c = eng.op_cif_scan_timed(np.concatenate(alphas), enc, lens, TAIL, max_tokens=1, fill=FILL)
    _check(fire_c, num_c, refs, 1)
