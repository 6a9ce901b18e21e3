"""Left-padded prompts at kernel level, through the probe library, against the float64 statement in tests/decode_attn_ref.py:
the prompt-attention kernel (launch_prompt_attention, csrc/prompt_attn.hip: prefills of more than 8 ids or of ragged lengths) and the
single-token self-attention forms with DecAttnArgs::key_start ("self_wave", "general_n1", "self_beam").

Everything a real row must not read holds NaN: the pad rows of q and kv_new, the cache (empty before a prompt prefill), the cached rows
below key_start. Budgets come from the arithmetic (decode_attn_ref.budget plus the term derived in _budget), not from observed errors."""
import numpy as np
import pytest

import decode_attn_ref as R
from conftest import sub

pytestmark = pytest.mark.gpu

H, B = 2, 3
MAX_POS = 448
PROMPT_N = [9, 16, 17, 64, 65, 232]              # padded lengths: around the 16- and 64-row tiles and the 64-key blocks, and a full-size prompt
KS_HISTS = [8, 63, 64, 130]


def _rnd(rng, shape, scale=1.0):
    return rng.standard_normal(shape).astype(np.float32) * np.float32(scale)


def _as_type(x, bf16):
    return np.where(np.isnan(x), x, R.bf16_round(np.nan_to_num(x))) if bf16 else np.ascontiguousarray(x, np.float32)


def _budget(ref, vmax, amax, bf16, prompt):
    """decode_attn_ref.budget (the hardware-exp class: these kernels run v_exp_f32) -- unchanged for f32. The bf16 prompt kernel feeds the
    probabilities to the PV product as bf16: every weight p_j carries a relative error <= 2^-9 (round to nearest, 8 significant bits), in the
    numerator sum_j p_j v_j and -- the kernel sums the rounded values -- in the normaliser sum_j p_j alike. The quotient moves by at most
    2^-9 max|v| through the numerator and 2^-9 |out| <= 2^-9 max|v| through the normaliser: 2^-8 max|v| in all."""
    tol = R.budget(ref, vmax, amax, bf16, fast_exp=True)
    if bf16 and prompt:
        tol = tol + np.repeat(2.0 ** -8 * vmax, 64, axis=1).reshape(tol.shape)
    return tol


def _assert_rows(out, ref, tol, rows, what):
    o, r, t = out[rows], ref[rows], tol[rows]
    err = np.abs(o - r)
    i = int(np.argmax(err - t))
    assert np.isfinite(o).all() and (err <= t).all(), f"{what}: |out - ref| = {err.flat[i]:.3g} > budget {t.flat[i]:.3g} at {np.unravel_index(i, err.shape)}"


def _lens(n):
    return (n, max(n // 2, 1), 1)


def _cache_kwargs(rng, layout):
    if layout == "contig":
        return dict(max_pos=MAX_POS)
    pps = MAX_POS // R.PAGE
    n_pages = B * pps + 5
    return dict(page_table=rng.permutation(n_pages)[:B * pps].reshape(B, pps), n_pages=n_pages)      # pages of every sequence scattered over the pool


def _toward(qh, score):
    return (qh * (score / float(qh @ qh))).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- prompt kernel, self
@pytest.mark.parametrize("layout", ["contig", "paged"])
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("n", PROMPT_N)
def test_prompt_self(n, bf16, layout):
    rng = np.random.default_rng(n * 4 + 2 * bf16 + (layout == "paged"))
    pad = np.array([n - L for L in _lens(n)], np.int32)
    q = _rnd(rng, (B * n, H * 64), 0.25)
    kv_new = _rnd(rng, (B * n, 2 * H * 64))
    for h in range(H):                           # sequence 0, last row: its best key is its own slot (the running max moves in the last key block)
        kv_new[n - 1, h * 64:(h + 1) * 64] = _toward(q[n - 1, h * 64:(h + 1) * 64], 12.0)
    for b in range(B):
        q[b * n:b * n + pad[b]] = np.nan
        kv_new[b * n:b * n + pad[b]] = np.nan
    q, kv_new = _as_type(q, bf16), _as_type(kv_new, bf16)
    empty = np.zeros((B, H, 0, 64), np.float32)
    out, (ka, va, stray), kernel = sub("_probe").decode_attention(q, bf16=bf16, n=n, kv_new=kv_new, k_hist=empty, v_hist=empty, key_start=pad,
                                                                 prompt=True, **_cache_kwargs(rng, layout))
    assert kernel == "prompt_self"
    ref = np.zeros((B * n, H * 64))
    vmax, amax = np.zeros((B * n, H)), np.ones((B * n, H))
    real = np.zeros(B * n, bool)
    for b in range(B):                           # the reference over the real slots alone: L rows, causal
        L, r0 = n - pad[b], b * n + pad[b]
        ref[r0:r0 + L], vmax[r0:r0 + L], amax[r0:r0 + L] = R.self_attention(q[r0:r0 + L], kv_new[r0:r0 + L], empty[:1], empty[:1], L)
        real[r0:r0 + L] = True
    _assert_rows(out, ref, _budget(ref, vmax, amax, bf16, True), real, kernel)
    assert not out[~real].any(), "pad query rows must be exactly 0"
    # the cache after the call: the new K / V of all n slots (pad slots as given), nothing else written
    assert np.array_equal(ka, kv_new[:, :H * 64].reshape(B, n, H, 64).transpose(0, 2, 1, 3), equal_nan=True)
    assert np.array_equal(va, kv_new[:, H * 64:].reshape(B, n, H, 64).transpose(0, 2, 1, 3), equal_nan=True)
    assert stray == 0, f"{stray} cache elements outside the sequences' slots changed"


# ---------------------------------------------------------------------------------------------------------------- prompt kernel, cross
def _plan(extents):
    row_off, r = [], 0
    for i, L in enumerate(extents):
        r += 16 * (i % 3)
        row_off.append(r)
        r = (r + L + 15) // 16 * 16
    return np.array(row_off, np.int32), np.array(extents, np.int32), r + 16


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("n,extents", [(9, (1, 65, 400)), (65, (1, 65, 400)), (232, (1, 65, 400)), (17, (1500, 63, 64))])
def test_prompt_cross(n, extents, bf16):
    rng = np.random.default_rng(n + 7 * bf16 + extents[0])
    row_off, n_lfr, rows = _plan(extents)
    k_slab = np.full((H, rows, 64), np.nan, np.float32)      # rows outside every extent are NaN: reading one shows
    v_slab = np.full((H, rows, 64), np.nan, np.float32)
    for b in range(B):
        r = slice(row_off[b], row_off[b] + n_lfr[b])
        k_slab[:, r], v_slab[:, r] = _rnd(rng, (H, n_lfr[b], 64)), _rnd(rng, (H, n_lfr[b], 64))
    pad = np.array([n - L for L in _lens(n)], np.int32)
    q = _rnd(rng, (B * n, H * 64), 0.25)
    for h in range(H):                           # sequence 0, last query: the best key is the extent's last row
        k_slab[h, row_off[0] + n_lfr[0] - 1] = _toward(q[n - 1, h * 64:(h + 1) * 64], 12.0)
    real = np.ones(B * n, bool)
    for b in range(B):
        q[b * n:b * n + pad[b]] = np.nan
        real[b * n:b * n + pad[b]] = False
    q, k_slab, v_slab = _as_type(q, bf16), _as_type(k_slab, bf16), _as_type(v_slab, bf16)
    out, _, kernel = sub("_probe").decode_attention(q, bf16=bf16, n=n, k_slab=k_slab, v_slab=v_slab, row_off=row_off, n_lfr=n_lfr, key_start=pad,
                                                    prompt=True)
    assert kernel == "prompt_cross"
    ref, vmax, amax = R.cross_attention(np.nan_to_num(q), k_slab, v_slab, row_off, n_lfr, n)
    _assert_rows(out, ref, _budget(ref, vmax, amax, bf16, True), real, kernel)
    assert not out[~real].any(), "pad query rows must be exactly 0"


# ---------------------------------------------------------------------------------------------------------------- key_start forms
def _ks_operands(rng, hist, bf16):
    ks = np.array([0, 5, hist - 1], np.int32)
    q = _rnd(rng, (B, H * 64), 0.25)
    kv_new = _rnd(rng, (B, 2 * H * 64))
    k_hist, v_hist = _rnd(rng, (B, H, hist, 64)), _rnd(rng, (B, H, hist, 64))
    for h in range(H):                           # sequence 1: the best key is the last cached row
        k_hist[1, h, hist - 1] = _toward(q[1, h * 64:(h + 1) * 64], 12.0)
    for b in range(B):
        k_hist[b, :, :ks[b]] = np.nan
        v_hist[b, :, :ks[b]] = np.nan
    return ks, [_as_type(x, bf16) for x in (q, kv_new, k_hist, v_hist)]


@pytest.mark.parametrize("layout", ["contig", "paged"])
@pytest.mark.parametrize("hist", KS_HISTS)
@pytest.mark.parametrize("form", ["self_wave", "general_bf16", "general_f32"])
def test_key_start_single_token(form, hist, layout, monkeypatch):
    if form == "general_bf16":
        monkeypatch.setenv("ASR_DECODE_ATTN_WAVE", "0")
    bf16 = form != "general_f32"
    rng = np.random.default_rng(hist * 3 + len(form))
    ks, (q, kv_new, k_hist, v_hist) = _ks_operands(rng, hist, bf16)
    kw = _cache_kwargs(rng, layout)
    out, (ka, va, stray), kernel = sub("_probe").decode_attention(q, bf16=bf16, kv_new=kv_new, k_hist=k_hist, v_hist=v_hist, key_start=ks, **kw)
    assert kernel == ("self_wave_ks" if form == "self_wave" else "general_n1_ks")
    for b in range(B):                           # the reference restricted to the visible keys
        ref, vmax, amax = R.self_attention(q[b:b + 1], kv_new[b:b + 1], k_hist[b:b + 1, :, ks[b]:], v_hist[b:b + 1, :, ks[b]:], 1)
        _assert_rows(out[b:b + 1], ref, _budget(ref, vmax, amax, bf16, False), slice(None), f"{kernel} sequence {b}")
    assert np.array_equal(ka[:, :, :hist], k_hist, equal_nan=True) and np.array_equal(va[:, :, :hist], v_hist, equal_nan=True)
    assert np.array_equal(ka[:, :, hist], kv_new[:, :H * 64].reshape(B, H, 64)) and np.array_equal(va[:, :, hist], kv_new[:, H * 64:].reshape(B, H, 64))
    assert stray == 0
    # key_start null: the entry's output equals the existing probe entry's bit for bit; so does a key_start of zeros (same keys, same order)
    k_full, v_full = np.nan_to_num(k_hist), np.nan_to_num(v_hist)
    plain, _, kernel0 = sub("_probe").decode_attention(q, bf16=bf16, kv_new=kv_new, k_hist=k_full, v_hist=v_full, **kw)
    null, _, kernel1 = sub("_probe").decode_attention(q, bf16=bf16, kv_new=kv_new, k_hist=k_full, v_hist=v_full, ks_entry=True, **kw)
    zeros, _, _ = sub("_probe").decode_attention(q, bf16=bf16, kv_new=kv_new, k_hist=k_full, v_hist=v_full, key_start=np.zeros(B, np.int32), **kw)
    assert kernel0 == kernel1 == ("self_wave" if form == "self_wave" else "general_n1")
    assert np.array_equal(plain.view(np.uint32), null.view(np.uint32)) and np.array_equal(plain.view(np.uint32), zeros.view(np.uint32))


@pytest.mark.parametrize("hist", KS_HISTS)
@pytest.mark.parametrize("bf16", [True, False])
def test_key_start_beam(bf16, hist):
    U, beam, p0 = 3, 2, 7
    rows, S = U * beam, hist + 3
    rng = np.random.default_rng(hist + 50 * bf16)
    ks = np.array([0, 5, hist - 1], np.int32)
    ext = rng.standard_normal((rows, 2, H, S, 64)).astype(np.float32)
    ext[:, :, :, hist + 1:] = np.nan
    ext[:, :, :, hist] = 7.0
    src = np.zeros((rows, hist - p0), np.int32)
    for r in range(rows):
        src[r] = (r // beam) * beam + rng.integers(0, beam, hist - p0)
        ext[r, :, :, :ks[r // beam]] = np.nan                        # below the utterance's start: never read
    q = (rng.standard_normal((rows, H * 64)) * 0.25).astype(np.float32)
    kv_new = rng.standard_normal((rows, 2 * H * 64)).astype(np.float32)
    q, kv_new, ext = _as_type(q, bf16), _as_type(kv_new, bf16), _as_type(ext, bf16)
    out, after, stray, kernel = sub("_probe").decode_attention_beam(q, kv_new, ext, src, beam, p0, hist, bf16=bf16, key_start=ks)
    assert kernel == "self_beam_ks"
    for r in range(rows):
        k0 = int(ks[r // beam])
        k_hist = np.zeros((1, H, hist - k0, 64))
        v_hist = np.zeros_like(k_hist)
        for s in range(k0, hist):
            owner = r if s < p0 else int(src[r, s - p0])
            k_hist[0, :, s - k0], v_hist[0, :, s - k0] = ext[owner, 0, :, s], ext[owner, 1, :, s]
        ref, vmax, amax = R.self_attention(q[r:r + 1], kv_new[r:r + 1], k_hist, v_hist, 1)
        _assert_rows(out[r:r + 1], ref, _budget(ref, vmax, amax, bf16, False), slice(None), f"{kernel} row {r}")
    assert np.array_equal(after[:, 0, :, hist], kv_new[:, :H * 64].reshape(rows, H, 64)) and np.array_equal(after[:, 1, :, hist], kv_new[:, H * 64:].reshape(rows, H, 64))
    assert stray == 0
    # key_start of zeros == the plain beam entry, bit for bit
    full = np.nan_to_num(ext)
    full[:, :, :, hist + 1:] = np.nan
    plain, _, _, kernel0 = sub("_probe").decode_attention_beam(q, kv_new, full, src, beam, p0, hist, bf16=bf16)
    zeros, _, _, _ = sub("_probe").decode_attention_beam(q, kv_new, full, src, beam, p0, hist, bf16=bf16, key_start=np.zeros(U, np.int32))
    assert kernel0 == "self_beam" and np.array_equal(plain.view(np.uint32), zeros.view(np.uint32))
