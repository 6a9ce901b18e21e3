"""Whisper decoder attention (launch_decode_attention: the single-token wave kernel, the one-pass cross-attention kernel and the general
two-pass kernel, bf16 / f32 / FP8 slabs) against the float64 statement in tests/decode_attn_ref.py, through the probe library.

Every case asserts which form the dispatcher ran, so a later change of the selection rule cannot turn a case into a test of another
kernel. Budgets come from the arithmetic (decode_attn_ref.budget), not from observed errors."""
import numpy as np
import pytest

import decode_attn_ref as R
from conftest import sub

pytestmark = pytest.mark.gpu

MAX_POS = 448                                    # max_target_positions: the self cache extent of every Whisper size
HISTS = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 447]
EXTENTS = [1, 7, 8, 31, 32, 33, 127, 128, 129, 255, 256, 257, 513, 1000]


def _rnd(rng, shape, scale=1.0):
    return rng.standard_normal(shape).astype(np.float32) * np.float32(scale)


def _as_type(x, bf16):
    return R.bf16_round(x) if bf16 else np.ascontiguousarray(x, np.float32)


def _toward(qh, score):
    """A key row whose dot product with the query head qh is `score`."""
    return (qh * (score / float(qh @ qh))).astype(np.float32)


def _assert_within(out, ref, vmax, amax, bf16, kernel, rows=None):
    tol = R.budget(ref, vmax, amax, bf16, fast_exp=kernel in ("self_wave", "cross_1pass", "cross_1pass_fp8"))
    if rows is not None:
        out, ref, tol = out[rows], ref[rows], tol[rows]
    err = np.abs(out - ref)
    i = int(np.argmax(err - tol))
    assert np.isfinite(out).all() and (err <= tol).all(), f"{kernel}: |out - ref| = {err.flat[i]:.3g} > budget {tol.flat[i]:.3g} at {np.unravel_index(i, err.shape)}"


# ---------------------------------------------------------------------------------------------------------------- self-attention
def _self_operands(rng, B, H, hist, n, bf16):
    q = _rnd(rng, (B * n, H * 64), 0.25)         # scores q . k ~ N(0, 2^2)
    kv_new = _rnd(rng, (B * n, 2 * H * 64))
    k_hist, v_hist = _rnd(rng, (B, H, hist, 64)), _rnd(rng, (B, H, hist, 64))
    for h in range(H):
        qh = q[0, h * 64:(h + 1) * 64]
        if hist:                                 # sequence 0: the best key is the last cached row (the running max moves in the last block)
            k_hist[0, h, hist - 1] = _toward(qh, 12.0)
        if n > 1:                                # ... and its query 0 has a future key scoring 130: only the -128 mask (not -inf, not 0) leaves it its weight
            kv_new[n - 1, h * 64:(h + 1) * 64] = _toward(qh, 130.0)
    return [_as_type(x, bf16) for x in (q, kv_new, k_hist, v_hist)]


def _cache_kwargs(rng, layout, B):
    if layout == "contig":
        return dict(max_pos=MAX_POS)
    pps = MAX_POS // R.PAGE
    n_pages = B * pps + 5
    pt = rng.permutation(n_pages)[:B * pps].reshape(B, pps)      # pages of every sequence scattered over the pool
    return dict(page_table=pt, n_pages=n_pages, hist_dev=layout.endswith("hist_dev"))


def _run_self(B, H, hist, n, bf16, layout, expect, seed):
    rng = np.random.default_rng(seed)
    q, kv_new, k_hist, v_hist = _self_operands(rng, B, H, hist, n, bf16)
    out, (ka, va, stray), kernel = sub("_probe").decode_attention(q, bf16=bf16, n=n, kv_new=kv_new, k_hist=k_hist, v_hist=v_hist,
                                                                 **_cache_kwargs(rng, layout, B))
    assert kernel == expect
    ref, vmax, amax = R.self_attention(q, kv_new, k_hist, v_hist, n)
    _assert_within(out, ref, vmax, amax, bf16, kernel)
    # the cache after the call: the cached rows untouched, the new rows at positions hist .. hist + n - 1 (in the page the table names), nothing else written
    assert np.array_equal(ka[:, :, :hist], k_hist) and np.array_equal(va[:, :, :hist], v_hist)
    assert np.array_equal(ka[:, :, hist:], kv_new[:, :H * 64].reshape(B, n, H, 64).transpose(0, 2, 1, 3))
    assert np.array_equal(va[:, :, hist:], kv_new[:, H * 64:].reshape(B, n, H, 64).transpose(0, 2, 1, 3))
    assert stray == 0, f"{stray} cache elements outside the sequences' positions changed"


@pytest.mark.parametrize("layout", ["contig", "paged", "paged_hist_dev"])
@pytest.mark.parametrize("H", [6, 20])
@pytest.mark.parametrize("hist", HISTS)
@pytest.mark.parametrize("form", ["self_wave", "general_bf16", "general_f32"])
def test_self_single_token(form, hist, H, layout, monkeypatch):
    if form == "general_bf16":
        monkeypatch.setenv("ASR_DECODE_ATTN_WAVE", "0")
    _run_self(3, H, hist, 1, form != "general_f32", layout, "self_wave" if form == "self_wave" else "general_n1", seed=hist * 7 + H)


@pytest.mark.parametrize("layout", ["contig", "paged"])
@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("hist", [0, 5, 60])
@pytest.mark.parametrize("n", [2, 4, 8])
def test_self_prefill_causal(n, hist, bf16, layout):
    _run_self(2, 6, hist, n, bf16, layout, "general_n8", seed=100 + n * 10 + hist)


# ---------------------------------------------------------------------------------------------------------------- cross-attention
def _plan(extents):
    """row_off with gaps between the extents (as Mpad leaves them), every offset a multiple of 16."""
    row_off, r = [], 0
    for i, L in enumerate(extents):
        r += 16 * (i % 3)
        row_off.append(r)
        r = (r + L + 15) // 16 * 16
    return np.array(row_off, np.int32), np.array(extents, np.int32), r + 16


def _cross_operands(rng, extents, H, n, bf16, ld_q=None, q_col0=0, specials=True):
    row_off, n_lfr, rows = _plan(extents)
    B = len(extents)
    k_slab = np.full((H, rows, 64), np.nan, np.float32)    # rows outside every extent are NaN: reading one shows
    v_slab = np.full((H, rows, 64), np.nan, np.float32)
    for b in range(B):
        r = slice(row_off[b], row_off[b] + n_lfr[b])
        k_slab[:, r], v_slab[:, r] = _rnd(rng, (H, n_lfr[b], 64)), _rnd(rng, (H, n_lfr[b], 64))
    ld_q = ld_q or H * 64
    q = _rnd(rng, (B * n, ld_q), 0.25)
    if specials:
        for b, L in enumerate(extents):
            r0, qb = row_off[b], q[b * n, q_col0:q_col0 + H * 64].reshape(H, 64)
            for h in range(H):
                if L in (129, 257, 1000, 1500):          # the best key is the last row: rescale in the final trip / last group
                    k_slab[h, r0 + L - 1] = _toward(qb[h], 12.0)
                elif L == 513:                           # every score equal: the context is the mean of the rows
                    k_slab[h, r0:r0 + L] = 0.0
                elif L == 255:                           # |scores| 60 .. 80: the exp range and the cross-wave merge
                    s = rng.uniform(60.0, 80.0, L) * rng.choice([-1.0, 1.0], L)
                    k_slab[h, r0:r0 + L] = qb[h][None, :] * (s / float(qb[h] @ qb[h]))[:, None]
    return _as_type(q, bf16), _as_type(k_slab, bf16), _as_type(v_slab, bf16), row_off, n_lfr


def _q_view(q, q_col0, H):
    return q[:, q_col0:q_col0 + H * 64]


@pytest.mark.parametrize("route", ["default", "max_keys_1001", "online_off", "ld_q_odd"])
@pytest.mark.parametrize("bf16", [True, False])
def test_cross_single_token(bf16, route, monkeypatch):
    H = 6
    rng = np.random.default_rng(7 + bf16)
    ld_q, q_col0 = (H * 64 + 12, 4) if route == "ld_q_odd" else (None, 0)
    q, k_slab, v_slab, row_off, n_lfr = _cross_operands(rng, EXTENTS, H, 1, bf16, ld_q, q_col0)
    if route == "online_off":
        monkeypatch.setenv("ASR_DECODE_ATTN_ONLINE", "0")
    out, _, kernel = sub("_probe").decode_attention(q, bf16=bf16, q_col0=q_col0, k_slab=k_slab, v_slab=v_slab, row_off=row_off, n_lfr=n_lfr,
                                                    max_keys=1001 if route == "max_keys_1001" else 0)
    assert kernel == ("cross_1pass" if route == "default" else "general_n1")
    ref, vmax, amax = R.cross_attention(_q_view(q, q_col0, H), k_slab, v_slab, row_off, n_lfr, 1)
    _assert_within(out, ref, vmax, amax, bf16, kernel)
    # the all-equal sequence: its context is the plain mean of its value rows
    b = EXTENTS.index(513)
    mean = v_slab[:, row_off[b]:row_off[b] + 513].astype(np.float64).mean(axis=1).reshape(-1)
    assert np.abs(out[b] - mean).max() <= (2.0 ** -8 * np.abs(mean) + 1e-5 * np.abs(v_slab[:, row_off[b]:row_off[b] + 513]).max()).max()


@pytest.mark.parametrize("n,prec", [(4, "bf16"), (8, "f32"), (4, "fp8"), (8, "fp8"), (8, "bf16")])
def test_cross_prefill(n, prec):
    H, extents = 6, [1, 40, 257, 130]
    rng = np.random.default_rng(n + len(prec))
    bf16 = prec != "f32"
    q, k_slab, v_slab, row_off, n_lfr = _cross_operands(rng, extents, H, n, bf16)
    out, after, kernel = sub("_probe").decode_attention(q, bf16=bf16, n=n, k_slab=k_slab, v_slab=v_slab, row_off=row_off, n_lfr=n_lfr,
                                                        fp8=prec == "fp8")
    assert kernel == ("general_n8_fp8" if prec == "fp8" else "general_n8")
    if prec == "fp8":
        kv8, sc8 = after
        t = sub("_probe").e4m3_table()
        ref, vmax, amax = R.cross_attention(q, t[kv8[0]], t[kv8[1]], row_off, n_lfr, n, sc8[0], sc8[1])
    else:
        ref, vmax, amax = R.cross_attention(q, k_slab, v_slab, row_off, n_lfr, n)
    _assert_within(out, ref, vmax, amax, bf16, kernel)


# ---------------------------------------------------------------------------------------------------------------- FP8 slabs
def _check_quantiser(k_slab, v_slab, row_off, n_lfr, kv8, sc8):
    """Power-of-two scale per (K | V, head, sequence) with amax / scale in (224, 448]; bytes within half an e4m3 step of the bf16 value."""
    t = sub("_probe").e4m3_table()
    for kv, slab in enumerate((k_slab, v_slab)):
        for h in range(slab.shape[0]):
            for b in range(len(n_lfr)):
                r = slice(row_off[b], row_off[b] + n_lfr[b])
                x, s = slab[h, r].astype(np.float64), float(sc8[kv, h, b])
                assert np.frexp(s)[0] == 0.5, s
                amax = np.abs(x).max()
                assert 224.0 < amax / s <= 448.0, (kv, h, b, amax, s)
                deq = t[kv8[kv, h, r]] * s
                assert (np.abs(deq - x) <= 2.0 ** -4 * np.abs(x) + 2.0 ** -10 * s).all()


@pytest.mark.parametrize("sub_batch", [False, True])
@pytest.mark.parametrize("online", [True, False])
def test_cross_fp8_slabs(online, sub_batch, monkeypatch):
    H, extents = 6, [1, 33, 129, 257, 1000, 1500]
    B = len(extents)
    rng = np.random.default_rng(31 + 2 * online + sub_batch)
    q, k_slab, v_slab, row_off, n_lfr = _cross_operands(rng, extents, H, 1, True)
    for b in range(B):                                   # per-(head, sequence) slab magnitudes 2^-1 .. 2^1: a wrong scale index cannot pass
        r = slice(row_off[b], row_off[b] + n_lfr[b])
        for h in range(H):
            k_slab[h, r] *= np.float32(2.0 ** ((h + 2 * b) % 3 - 1))
            v_slab[h, r] *= np.float32(2.0 ** ((2 * h + b) % 3 - 1))
    if not online:
        monkeypatch.setenv("ASR_DECODE_ATTN_ONLINE", "0")
    b0, nb = (2, 3) if sub_batch else (0, 0)
    out, (kv8, sc8), kernel = sub("_probe").decode_attention(q, bf16=True, B=B, b0=b0, nb=nb, k_slab=k_slab, v_slab=v_slab, row_off=row_off,
                                                             n_lfr=n_lfr, fp8=True)
    assert kernel == ("cross_1pass_fp8" if online else "general_n1_fp8")
    _check_quantiser(k_slab, v_slab, row_off, n_lfr, kv8, sc8)
    launched = np.arange(b0, b0 + (nb or B))
    assert all(len(np.unique(sc8[kv][:, launched])) > 1 for kv in (0, 1))
    t = sub("_probe").e4m3_table()
    ref, vmax, amax = R.cross_attention(q, t[kv8[0]], t[kv8[1]], row_off, n_lfr, 1, sc8[0], sc8[1])
    _assert_within(out, ref, vmax, amax, True, kernel, rows=launched)
    outside = np.setdiff1d(np.arange(B), launched)
    assert not out[outside].any(), "rows of sequences outside the launch were written"


# ---------------------------------------------------------------------------------------------------------------- batch composition
def test_cross_30s_neighbour_and_alone():
    """H = 20, a 50-key sequence next to a 1500-key one: the bf16 batch takes the two-pass kernel (max_keys > 1000), the same sequence
    alone the one-pass kernel. Both must be within budget of the reference; they need not agree bit for bit (the kernel choice follows
    the batch's longest extent)."""
    H = 20
    rng = np.random.default_rng(30)
    q, k_slab, v_slab, row_off, n_lfr = _cross_operands(rng, [1500, 50], H, 1, True)
    p = sub("_probe")
    out, _, kernel = p.decode_attention(q, bf16=True, k_slab=k_slab, v_slab=v_slab, row_off=row_off, n_lfr=n_lfr)
    assert kernel == "general_n1"
    ref, vmax, amax = R.cross_attention(q, k_slab, v_slab, row_off, n_lfr, 1)
    _assert_within(out, ref, vmax, amax, True, kernel)
    out1, _, kernel1 = p.decode_attention(q[1:2], bf16=True, k_slab=k_slab, v_slab=v_slab, row_off=row_off[1:], n_lfr=n_lfr[1:])
    assert kernel1 == "cross_1pass"
    _assert_within(out1, ref[1:2], vmax[1:2], amax[1:2], True, kernel1)
