"""The beam-search self-attention form ("self_beam" of launch_decode_attention: hypothesis rows with per-row extents read through an
ancestry table) against the float64 statement in tests/decode_attn_ref.py, through the probe library.

Every case draws a random ancestry table inside each utterance, puts NaN in every slot past the current position (a kernel that reads one
fails), checks the new K / V row landed in the row's own slot and that no other slot changed, and asserts the form that ran."""
import numpy as np
import pytest

import decode_attn_ref as R
from conftest import sub

pytestmark = pytest.mark.gpu

HISTS = [4, 5, 15, 16, 17, 63, 64, 65, 130]


def _case(rng, U, beam, H, p0, hist, bf16):
    rows, S = U * beam, hist + 3
    ext = rng.standard_normal((rows, 2, H, S, 64)).astype(np.float32)
    ext[:, :, :, hist + 1:] = np.nan                                 # never read
    ext[:, :, :, hist] = 7.0                                         # overwritten by the call
    src = np.zeros((rows, max(hist - p0, 1)), np.int32)
    for r in range(rows):
        b = r // beam
        src[r, :hist - p0] = b * beam + rng.integers(0, beam, hist - p0)
    q = (rng.standard_normal((rows, H * 64)) * 0.25).astype(np.float32)
    kv_new = rng.standard_normal((rows, 2 * H * 64)).astype(np.float32)
    if hist > p0:                                                    # row 0, head 0: its best key sits in an ancestor's extent, last generated slot
        a = src[0, hist - p0 - 1]
        qh = q[0, :64]
        ext[a, 0, 0, hist - 1] = qh * (12.0 / float(qh @ qh))
    cast = R.bf16_round if bf16 else (lambda x: np.ascontiguousarray(x, np.float32))
    return cast(q), cast(kv_new), np.where(np.isnan(ext), ext, cast(ext)), src


def _reference(q, kv_new, ext, src, p0, hist):
    rows, _, H = ext.shape[:3]
    k_hist = np.zeros((rows, H, hist, 64), np.float64)
    v_hist = np.zeros_like(k_hist)
    for r in range(rows):
        for s in range(hist):
            owner = r if s < p0 else int(src[r, s - p0])
            k_hist[r, :, s], v_hist[r, :, s] = ext[owner, 0, :, s], ext[owner, 1, :, s]
    return R.self_attention(q, kv_new, k_hist, v_hist, 1)


@pytest.mark.parametrize("hist", HISTS)
@pytest.mark.parametrize("U,beam,H,p0", [(2, 3, 6, 4), (8, 5, 20, 4), (3, 8, 4, 1), (4, 1, 6, 3)])
@pytest.mark.parametrize("bf16", [True, False])
def test_self_beam_follows_the_ancestry(bf16, U, beam, H, p0, hist):
    rng = np.random.default_rng(1000 * U + 100 * beam + hist + (7 if bf16 else 0))
    q, kv_new, ext, src = _case(rng, U, beam, H, p0, hist, bf16)
    out, after, stray, kernel = sub("_probe").decode_attention_beam(q, kv_new, ext, src, beam, p0, hist, bf16=bf16, hist_dev=hist % 2 == 1)
    assert kernel == "self_beam"
    ref, vmax, amax = _reference(q, kv_new, ext, src, p0, hist)
    tol = R.budget(ref, vmax, amax, bf16, fast_exp=True)
    err = np.abs(out - ref)
    assert np.isfinite(out).all() and (err <= tol).all(), float((err - tol).max())
    rows = U * beam
    kn = kv_new[:, :H * 64].reshape(rows, H, 64)
    vn = kv_new[:, H * 64:].reshape(rows, H, 64)
    assert np.array_equal(after[:, 0, :, hist], kn) and np.array_equal(after[:, 1, :, hist], vn)   # the new row: the row's own slot `hist`
    assert stray == 0                                                                             # nothing else written
