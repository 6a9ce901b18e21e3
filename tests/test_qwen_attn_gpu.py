"""The Qwen3 decoder's attention kernels (qw_qk_rope_kernel, qw_attn_kernel, qw_decode_attn_kernel with and without BEAM, and the MFMA prefill
kernel with its causal / GQA arguments) against the float64 statement in tests/qwen_attn_ref.py, through the session's own launcher
(launch_qwen_attention) in the probe library.

Every case asserts the form the launcher reports, so a later change of the selection rule cannot turn a case into a test of another kernel.
Budgets come from the arithmetic (qwen_attn_ref.budget), not from observed errors. The reference masks with the additive -128 of the original
graphs, the kernels mask strictly: every case asserts that the largest weight the -128 leaves a masked key is below a tenth of its smallest
budget, i.e. that it sits where the two agree ("Causal masking of the Qwen3 decoder").

Keys are planted, because random normed rows give near-uniform attention in which a dropped key or a wrong merge maximum moves nothing:
a planted key is a pre-norm row chosen so that its normed, rotated key is a positive multiple of one query head's rotated query
(qwen_attn_ref.key_for) -- the largest score a normed row can reach -- and the case checks that the reference gives it a weight above 0.9."""
import numpy as np
import pytest

import qwen_attn_ref as R
from conftest import sub

pytestmark = pytest.mark.gpu

EPS = 1e-6
HD = R.HD
S_SMALL, S_BIG = 1024, 4224                       # max_seq_len of the two session geometries (4224 / 16 = 264 table entries > the 256 kept in LDS)
RATIOS = {}                                       # form -> largest err / budget seen (reported at the end of the module; nothing reads it)


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    for k in sorted(RATIOS):
        print(f"\n[qwen_attn] largest err / budget, {k}: {RATIOS[k]:.3f}")


def _rope(n, f16=False, _cache={}):
    if (n, f16) not in _cache:
        _cache[(n, f16)] = R.rope_table(n, f16=f16)
    return _cache[(n, f16)]


def _norm_weights(rng, scale=0.36):
    """Folded q_norm / k_norm weights: about 1.2 x those of the synthetic checkpoints (128^-1/4 (1 + 0.1 N)), so that a planted key scores ~ 16 against
    random keys' ~ N(0, 1.5^2) and wins even among 4000 of them."""
    return [(scale * (1.0 + 0.1 * rng.standard_normal(HD))).astype(np.float32) for _ in range(2)]


def _elem(x, bf16):
    x = np.asarray(x, np.float32)
    return R.bf16_round(x) if bf16 else x


def _hist_rows(rng, KV, n, kn, rope, bf16):
    """n cached positions of one sequence: keys as a session would have cached them (normed, rotated random rows), values N(0, 1); [KV][n][128] each."""
    x = rng.standard_normal((n, KV, HD))
    k = R.rotate(R.rms_norm(x, kn, EPS), rope[:n][:, None, :]).transpose(1, 0, 2)
    v = rng.standard_normal((KV, n, HD))
    return _elem(k, bf16), _elem(v, bf16)


def _planted_hist_key(q_post, kn, rope, pos, bf16, sign=1.0):
    x, c = R.key_for(q_post, kn, rope[pos], EPS, sign)
    return _elem(R.rotate(R.rms_norm(x.astype(np.float64), kn, EPS), rope[pos]), bf16)


def _layout(rng, layout, n_pos, S_max):
    """Cache layout arguments for sequences holding n_pos[b] positions after the call. Pages: page 0 is the scratch page every unowned table entry names."""
    if layout == "extents":
        return {}
    pps = S_max // R.PAGE
    need = [(int(n) + R.PAGE - 1) // R.PAGE for n in n_pos]
    n_pages = sum(need) + 4
    ids = 1 + (rng.permutation(n_pages - 1) if layout == "pages_shuffled" else np.arange(n_pages - 1))
    table, at = np.zeros((len(n_pos), pps), np.int32), 0
    for b, m in enumerate(need):
        table[b, :m] = ids[at:at + m]
        at += m
    return dict(table=table, n_pages=n_pages)


def _check_ctx(out, ref, st, form, bf16, rows):
    tol = R.budget(ref, st, form, bf16)
    got, ref, tol = out["ctx"][rows].astype(np.float64), ref[rows], tol[rows]
    worst_masked = float(np.nanmax(st["masked_weight"][rows]))
    assert worst_masked < 0.1 * tol.min(), f"the reference's -128 leaves a masked key the weight {worst_masked:.3g}: the case is outside the range where strict masking agrees"
    err = np.abs(got - ref)
    assert np.isfinite(got).all(), f"{out['kernel']}: {np.count_nonzero(~np.isfinite(got))} non-finite context elements"
    key = f"{form} {'bf16' if bf16 else 'f32'}"
    RATIOS[key] = max(RATIOS.get(key, 0.0), float((err / tol).max()))
    i = int(np.argmax(err - tol))
    assert (err <= tol).all(), f"{out['kernel']}: |ctx - ref| = {err.flat[i]:.3g} > budget {tol.flat[i]:.3g} at {np.unravel_index(i, err.shape)}"


def _check_new_rows(got_k, got_v, k_ref, v_ref, bf16, what):
    """Cached rows of the positions a call wrote: k within the f32 bound (f32) or one bf16 ulp (bf16) of float64, v exact."""
    bound = R.norm_rope_f32_bound(k_ref) + (R.bf16_ulp(k_ref) if bf16 else 0.0)
    err = np.abs(got_k.astype(np.float64) - k_ref)
    assert (err <= bound).all(), f"{what}: cached k off by {err.max():.3g} (bound {bound.flat[int(np.argmax(err - bound))]:.3g})"
    key = f"norm+rope {'bf16' if bf16 else 'f32'}"
    RATIOS[key] = max(RATIOS.get(key, 0.0), float((err / bound).max()))
    assert np.array_equal(got_v, v_ref.astype(np.float32)), f"{what}: cached v is not the input row"


# ---------------------------------------------------------------------------------------------------------------- one decode step
def _step_case(seed, G, KV, hists, bf16, layout, S_max, plant, no_fuse=False, f16_rope=False, w_scale=0.36):
    rng = np.random.default_rng(seed)
    H, B = G * KV, len(hists)
    hists = np.asarray(hists, np.int32)
    rope = _rope(S_max, f16_rope)
    qn, kn = _norm_weights(rng, w_scale)
    qkv = rng.standard_normal((B, (H + 2 * KV) * HD)).astype(np.float32)
    hist_kv = [_hist_rows(rng, KV, int(h), kn, rope, bf16) for h in hists]
    k_hist, v_hist = [k for k, _ in hist_kv], [v for _, v in hist_kv]
    # planted keys on sequence 0, kv head 0: q head g gets the key at position where[g]
    h0 = int(hists[0])
    q_post = R.new_rows(qkv, H, KV, qn, kn, rope, EPS, hists)[0]
    where = {}
    if plant == "last":                                  # the running maximum moves in the final block
        where = {0: h0 - 1}
    elif plant == "block_first":                         # first rows of the last 64-key block
        where = {g: (h0 - 1) // 64 * 64 + g for g in range(G)}
    elif plant == "new":                                 # the new key itself (held in LDS) beats everything cached
        where = {0: h0}
    elif plant == "spread":                              # the group's q heads find their maximum in different lane groups (key s belongs to group s % 16)
        where = dict(zip(range(G), [h0 - 1, 5, h0 // 2 + 3, 26]))
        assert len({p % 16 for p in where.values()}) == len(where)
    elif plant == "merge":                               # head 0: every key of lane group 0 (position 0 and the new key) points AWAY from the query, key 7 at it
        where = {0: 7}
        k_hist[0][0, 0] = _planted_hist_key(q_post[0, 0], kn, rope, 0, bf16, sign=-1.0)
        qkv[0, H * HD:(H + 1) * HD] = R.key_for(q_post[0, 0], kn, rope[h0], EPS, sign=-1.0)[0]
    where = {g: p for g, p in where.items() if 0 <= p <= h0}
    assert len(set(where.values())) == len(where)
    for g, p in where.items():
        if p == h0:
            qkv[0, H * HD:(H + 1) * HD] = R.key_for(q_post[0, g], kn, rope[p], EPS)[0]
        else:
            k_hist[0][0, p] = _planted_hist_key(q_post[0, g], kn, rope, p, bf16)
    T = np.ones(B, np.int32)
    q, k, v = R.new_rows(qkv, H, KV, qn, kn, rope, EPS, hists, bf16)
    ref, st = R.attention(q, k, v, k_hist, v_hist, hists, T, np.arange(B), G)
    for g in where:
        assert st["win"][0, g] > 0.9, f"planted key of head {g} only has weight {st['win'][0, g]:.3f}"
    hmax = int(hists.max())
    pack = lambda rows: np.stack([np.pad(r, ((0, 0), (0, hmax - r.shape[1]), (0, 0))) for r in rows])
    out = sub("_probe").qwen_attention(qkv, H, KV, qn, kn, rope, EPS, hists, T, S_max, bf16=bf16, step=True, no_fuse=no_fuse, k_hist=pack(k_hist),
                                       v_hist=pack(v_hist), **_layout(rng, layout, hists + 1, S_max))
    return dict(out=out, ref=ref, st=st, k=k, v=v, k_hist=k_hist, v_hist=v_hist, hists=hists, B=B)


def _check_step(c, form, kernel, bf16):
    out = c["out"]
    assert out["kernel"] == kernel
    _check_ctx(out, c["ref"], c["st"], form, bf16, slice(None))
    for b in range(c["B"]):
        h = int(c["hists"][b])
        assert np.array_equal(out["k_after"][b, :, :h], c["k_hist"][b]) and np.array_equal(out["v_after"][b, :, :h], c["v_hist"][b])
        _check_new_rows(out["k_after"][b, :, h], out["v_after"][b, :, h], c["k"][b], c["v"][b], bf16, f"sequence {b}")
    assert out["stray"] == 0, f"{out['stray']} cache elements outside the new positions changed"


def _hists3(hist, S_max):
    return [hist, hist // 2, min(hist + 7, S_max - 1)]


@pytest.mark.parametrize("layout", ["extents", "pages", "pages_shuffled"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("hist", [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 511])
def test_fused_step(hist, G, bf16, layout):
    c = _step_case(1000 * G + hist, G, 2, _hists3(hist, S_SMALL), bf16, layout, S_SMALL, "last")
    _check_step(c, "fused", f"fused_g{G}", bf16)


@pytest.mark.parametrize("layout", ["pages", "pages_shuffled"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("hist", [4095, 4096, 4097, 4130])
def test_fused_step_table_past_lds(hist, G, bf16, layout):
    """Positions >= 4096: their block-table entries are read from global memory, not from the 256 entries copied to LDS. The planted key of sequence 0
    is its last cached row (page index >= 255), sequence 2 is longer still."""
    c = _step_case(77 * G + hist, G, 1, _hists3(hist, S_BIG), bf16, layout, S_BIG, "last")
    _check_step(c, "fused", f"fused_g{G}", bf16)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("hist", [65, 129, 511])
@pytest.mark.parametrize("plant", ["block_first", "new", "spread"])
def test_fused_step_planted(plant, hist, G, bf16):
    c = _step_case(31 * G + hist, G, 2, _hists3(hist, S_SMALL), bf16, "pages_shuffled", S_SMALL, plant, f16_rope=plant == "new")
    _check_step(c, "fused", f"fused_g{G}", bf16)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("G", [1, 2, 4])
def test_fused_step_merge_maximum(G, bf16):
    """The 16-way merge must rescale by the maximum over ALL lane groups. The soft-max does not care which common offset is subtracted until exp overflows,
    so the case needs partial maxima more than 88.7 apart: norm weights of 0.62 (1.7 x the usual) put a planted key at +49 in lane group 7 while lane group
    0 (key 0 and the new key, 15 positions cached) only holds keys at -49. Rescaling by group 0's maximum would compute exp(98) = inf and return NaN."""
    c = _step_case(600 + G, G, 2, [15, 40, 3], bf16, "pages", S_SMALL, "merge", w_scale=0.62)
    assert c["st"]["smax"][0, 0] > 45.0
    _check_step(c, "fused", f"fused_g{G}", bf16)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("G", [1, 4])
def test_fused_step_planted_past_lds(G, bf16):
    c = _step_case(5 + G, G, 1, _hists3(4130, S_BIG), bf16, "pages_shuffled", S_BIG, "spread")
    _check_step(c, "fused", f"fused_g{G}", bf16)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("G", [1, 2, 4])
def test_forms_agree(G, bf16):
    """The fused step and the unfused one (RoPE kernel + scalar attention, ASR_QWEN_NO_FUSE) on the same operands: each within its own budget of float64,
    and the rows they cache are the same."""
    a = _step_case(900 + G, G, 2, [129, 16, 40], bf16, "pages", S_SMALL, "spread")
    b = _step_case(900 + G, G, 2, [129, 16, 40], bf16, "pages", S_SMALL, "spread", no_fuse=True)
    _check_step(a, "fused", f"fused_g{G}", bf16)
    _check_step(b, "scalar", "rope_scalar", bf16)
    assert np.array_equal(a["out"]["k_after"], b["out"]["k_after"], equal_nan=True) and np.array_equal(a["out"]["v_after"], b["out"]["v_after"], equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------- beam step
@pytest.mark.parametrize("layout", ["extents", "pages_shuffled"])
@pytest.mark.parametrize("n_utt,KV", [(4, 2), (3, 1)], ids=["units8", "units3"])         # B * KV / beam a multiple of 8 (XCD-aware workgroup order) and not
@pytest.mark.parametrize("beam", [2, 5, 8])
@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("gen", [0, 1, 16, 33, 47])
def test_beam_step(gen, G, beam, n_utt, KV, layout):
    bf16 = (gen + beam) % 2 == 0                                 # both element types over the grid
    rng = np.random.default_rng(gen * 100 + G * 10 + beam)
    S_hyp, S_max = 48, S_SMALL
    H, B = G * KV, n_utt * beam
    rope = _rope(S_max)
    qn, kn = _norm_weights(rng)
    p0_utt = [37, 128, 5, 64][:n_utt]
    p0 = np.repeat(p0_utt, beam).astype(np.int32)
    hists = p0 + gen
    qkv = rng.standard_normal((B, (H + 2 * KV) * HD)).astype(np.float32)
    prompt = [_hist_rows(rng, KV, p, kn, rope, bf16) for p in p0_utt]
    # ancestry: at every generated slot the rows of an utterance take new parents -- a permutation at even slots, a random (non-injective) choice at odd ones
    src = np.zeros((B, S_hyp), np.int32)
    for u in range(n_utt):
        for j in range(gen):
            src[u * beam:(u + 1) * beam, j] = u * beam + (rng.permutation(beam) if j % 2 == 0 else rng.integers(0, beam, beam))
    # extents: only slots on some row's ancestry hold rows, everything else is NaN
    ext_k, ext_v = np.full((B, KV, S_hyp, HD), np.nan, np.float32), np.full((B, KV, S_hyp, HD), np.nan, np.float32)
    for j in range(gen):
        for r in np.unique(src[:, j]):
            x = rng.standard_normal((KV, HD))
            pos = int(p0[r]) + j
            ext_k[r, :, j] = _elem(R.rotate(R.rms_norm(x, kn, EPS), rope[pos]), bf16)
            ext_v[r, :, j] = _elem(rng.standard_normal((KV, HD)), bf16)
    q_post = R.new_rows(qkv, H, KV, qn, kn, rope, EPS, hists)[0]
    planted = {}
    if gen > 0:                                                  # row 0, head 0: the last generated slot, wherever the ancestry keeps it
        ext_k[src[0, gen - 1], 0, gen - 1] = _planted_hist_key(q_post[0, 0], kn, rope, int(p0[0]) + gen - 1, bf16)
        planted[0] = True
    g_p = 1 if (gen > 0 and G > 1) else (0 if gen == 0 else None)    # the prompt's last row: head 1, or head 0 at the first step
    if g_p is not None:
        prompt[0][0][0, p0_utt[0] - 1] = _planted_hist_key(q_post[0, g_p], kn, rope, p0_utt[0] - 1, bf16)
        planted[g_p] = True
    k_hist = [R.beam_keys(prompt[b // beam][0], ext_k, src[b], int(p0[b]), gen) for b in range(B)]
    v_hist = [R.beam_keys(prompt[b // beam][1], ext_v, src[b], int(p0[b]), gen) for b in range(B)]
    assert all(np.isfinite(k).all() for k in k_hist)
    T = np.ones(B, np.int32)
    q, k, v = R.new_rows(qkv, H, KV, qn, kn, rope, EPS, hists, bf16)
    ref, st = R.attention(q, k, v, k_hist, v_hist, hists, T, np.arange(B), G)
    for g in planted:
        assert st["win"][0, g] > 0.9
    pmax = max(p0_utt)
    pack = lambda rows: np.stack([np.pad(r, ((0, 0), (0, pmax - r.shape[1]), (0, 0))) for r in rows])
    out = sub("_probe").qwen_attention(qkv, H, KV, qn, kn, rope, EPS, hists, T, S_max, bf16=bf16, step=True, k_hist=pack([p[0] for p in prompt]),
                                       v_hist=pack([p[1] for p in prompt]), beam=beam, src=src, p0=p0, ext_k=ext_k, ext_v=ext_v,
                                       **_layout(rng, layout, p0_utt, S_max))
    assert out["kernel"] == f"beam_g{G}"
    _check_ctx(out, ref, st, "beam", bf16, slice(None))
    for b in range(B):
        _check_new_rows(out["ext_k"][b, :, gen], out["ext_v"][b, :, gen], k[b], v[b], bf16, f"row {b}")
    assert out["stray"] == 0, f"{out['stray']} elements outside the rows' new slot changed"


# ---------------------------------------------------------------------------------------------------------------- prefill forms
def _prefill_case(seed, G, KV, hists, Ts, bf16, layout, S_max, no_fuse, step=False, f16_rope=False, rope_rows=None, garbage_gaps=False, tail_rows=0):
    """A ragged batch of sequences with T new positions each. Planted on the first sequence with T >= 2 (head 0 of kv head 0): a FUTURE key for query 0 (the
    key at t = 1 points at query 0: it would take nearly all the weight if visited); on the longest sequence: the key at position 0 points at its last query,
    and the key of query t = T // 2 points at that query itself (the diagonal)."""
    rng = np.random.default_rng(seed)
    H, B = G * KV, len(Ts)
    hists, Ts = np.asarray(hists, np.int32), np.asarray(Ts, np.int32)
    rope = _rope(rope_rows or S_max, f16_rope)
    qn, kn = _norm_weights(rng)
    row_off = np.arange(B) if step else np.concatenate([[0], np.cumsum((Ts + 15) // 16 * 16)[:-1]]).astype(np.int64)
    if step:
        rows = B
    elif tail_rows:                                              # (a session's row count is a multiple of 16; the kernels do not need it)
        rows = int(row_off[-1] + Ts[-1] + tail_rows)
    else:
        rows = int(row_off[-1] + (Ts[-1] + 15) // 16 * 16)
    live = np.zeros(rows, bool)
    pos = np.zeros(rows, np.int64)
    for b in range(B):
        live[row_off[b]:row_off[b] + Ts[b]] = True
        pos[row_off[b]:row_off[b] + Ts[b]] = hists[b] + np.arange(Ts[b])
    qkv = rng.standard_normal((rows, (H + 2 * KV) * HD)).astype(np.float32)
    if not garbage_gaps:
        qkv[~live] = 0.0                                         # a session's gap rows are zero rows
    hist_kv = [_hist_rows(rng, KV, int(h), kn, rope, bf16) for h in hists]
    k_hist, v_hist = [k for k, _ in hist_kv], [v for _, v in hist_kv]
    q_post = R.new_rows(qkv, H, KV, qn, kn, rope, EPS, pos)[0]
    kcol = slice(H * HD, (H + 1) * HD)
    expect_win = []
    two = [b for b in range(B) if Ts[b] >= 2]
    if two:
        r = int(row_off[two[0]])
        qkv[r + 1, kcol] = R.key_for(q_post[r, 0], kn, rope[pos[r + 1]], EPS)[0]
    bl = int(np.argmax(Ts))
    if Ts[bl] >= 8 and hists[bl] == 0:
        r, last, mid = int(row_off[bl]), int(row_off[bl] + Ts[bl] - 1), int(row_off[bl] + Ts[bl] // 2)
        qkv[mid, kcol] = R.key_for(q_post[mid, 0], kn, rope[pos[mid]], EPS)[0]
        expect_win.append((mid, 0))
        if G > 1:                                                # position 0 for head 1 of the last query (head 0's key row 0 must stay what it is for query 0's own soft-max)
            qkv[r, kcol] = R.key_for(q_post[last, 1], kn, rope[pos[r]], EPS)[0]
            expect_win.append((last, 1))
    q, k, v = R.new_rows(qkv, H, KV, qn, kn, rope, EPS, pos, bf16)
    ref, st = R.attention(q, k, v, k_hist, v_hist, hists, Ts, row_off, G)
    for r, g in expect_win:
        assert st["win"][r, g] > 0.9, f"planted key of row {r}, head {g} only has weight {st['win'][r, g]:.3f}"
    if two:
        assert st["masked_weight"][int(row_off[two[0]]), 0] > 0.0
    hmax = max(int(hists.max()), 1)
    pack = lambda rws: np.stack([np.pad(r, ((0, 0), (0, hmax - r.shape[1]), (0, 0))) for r in rws])
    out = sub("_probe").qwen_attention(qkv, H, KV, qn, kn, rope, EPS, hists, Ts, S_max, bf16=bf16, step=step, no_fuse=no_fuse, row_off=row_off,
                                       k_hist=pack(k_hist), v_hist=pack(v_hist), **_layout(rng, layout, hists + Ts, S_max))
    return dict(out=out, ref=ref, st=st, q=q, k=k, v=v, k_hist=k_hist, v_hist=v_hist, hists=hists, Ts=Ts, row_off=row_off, live=live, B=B, H=H, KV=KV)


def _check_prefill(c, form, kernel, bf16):
    out, live = c["out"], c["live"]
    assert out["kernel"] == kernel
    _check_ctx(out, c["ref"], c["st"], form, bf16, live)
    # operand rows: q of live rows against float64, nothing written for gap rows
    q_ref = c["q"].reshape(len(live), -1, HD)[live]
    q_got = out["q"].reshape(len(live), -1, HD)
    bound = R.norm_rope_f32_bound(q_ref) + (R.bf16_ulp(q_ref) if bf16 else 0.0)
    assert (np.abs(q_got[live].astype(np.float64) - q_ref) <= bound).all()
    assert np.isnan(q_got[~live]).all(), "a gap row's q was written"
    for b in range(c["B"]):
        h, T, r0 = int(c["hists"][b]), int(c["Ts"][b]), int(c["row_off"][b])
        assert np.array_equal(out["k_after"][b, :, :h], c["k_hist"][b]) and np.array_equal(out["v_after"][b, :, :h], c["v_hist"][b])
        _check_new_rows(out["k_after"][b, :, h:h + T], out["v_after"][b, :, h:h + T], c["k"][r0:r0 + T].transpose(1, 0, 2), c["v"][r0:r0 + T].transpose(1, 0, 2),
                        bf16, f"sequence {b}")
        if kernel == "rope_mfma":                                # the row-major key copy the MFMA kernel reads is the cached key, bit for bit
            kr = out["k_rows"].reshape(len(live), c["KV"], HD)[r0:r0 + T].transpose(1, 0, 2)
            assert np.array_equal(kr, out["k_after"][b, :, h:h + T])
    if kernel == "rope_mfma":
        assert np.isnan(out["k_rows"].reshape(len(live), -1)[~live]).all(), "a gap row's key copy was written"
    assert out["stray"] == 0, f"{out['stray']} cache elements outside the new positions changed"


SCALAR_SHAPES = {
    "prefill": dict(hists=[0, 0, 0, 0, 0], Ts=[17, 1, 2, 129, 300]),
    "mid_history": dict(hists=[5, 60, 5, 60], Ts=[2, 2, 17, 17]),
}


@pytest.mark.parametrize("layout", ["extents", "pages_shuffled"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("shape", list(SCALAR_SHAPES))
def test_scalar_prefill(shape, G, bf16, layout):
    c = _prefill_case(11 * G + len(shape), G, 2, bf16=bf16, layout=layout, S_max=S_SMALL, no_fuse=bf16, garbage_gaps=True, f16_rope=shape == "mid_history",
                      **SCALAR_SHAPES[shape])
    _check_prefill(c, "scalar", "rope_scalar", bf16)


@pytest.mark.parametrize("layout", ["extents", "pages_shuffled"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("G", [1, 2, 4])
def test_scalar_no_fuse_step(G, bf16, layout):
    """The unfused decode step: T = 1 with every history length in one launch (B * (H + 2 KV) units: the RoPE kernel's last wave is partly dead for G = 1, 2)."""
    hists = [1, 15, 16, 17, 127, 128, 129, 511, 3]
    c = _prefill_case(300 + G, G, 1, hists, [1] * len(hists), bf16, layout, S_SMALL, no_fuse=True, step=True)
    assert (len(hists) * (G + 2)) % 16 != 0
    _check_prefill(c, "scalar", "rope_scalar", bf16)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("f16_rope", [False, True], ids=["rope_f32", "rope_f16"])
def test_rope_table_end_and_dead_lanes(bf16, f16_rope):
    """Norm + RoPE + cache write at the edges: the last sequence ends on the last row of the rope table and of its extent, the row count leaves the
    last wave of the RoPE kernel partly dead (23 rows x 3 heads = 69 units of 16 lanes), and the gap rows hold garbage that must go nowhere."""
    S = 96
    c = _prefill_case(4242, 1, 2, [0, S - 5], [3, 5], bf16, "extents", S, no_fuse=bf16, f16_rope=f16_rope, rope_rows=S, garbage_gaps=True)
    c2 = _prefill_case(4243, 1, 1, [0, S - 5], [3, 5], bf16, "pages", S, no_fuse=bf16, f16_rope=f16_rope, rope_rows=S, garbage_gaps=True, tail_rows=2)
    assert (c2["live"].size * 3) % 16 != 0
    for x in (c, c2):
        _check_prefill(x, "scalar", "rope_scalar", bf16)


MFMA_BATCHES = {                                                # lengths -> (qt, whole utterance in one 256-key chunk)
    "to128": ([1, 15, 16, 17, 31, 32, 33, 127, 128], 1, True),
    "to256": ([129, 255, 17, 256, 1], 2, True),
    "to300": ([257, 33, 300], 2, False),
    "to511": ([129, 511, 16, 300], 2, False),
    "1_and_511": ([1, 511], 2, False),
}


@pytest.mark.parametrize("layout", ["extents", "pages_shuffled"])
@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("batch", list(MFMA_BATCHES))
def test_mfma_prefill(batch, G, layout):
    Ts, qt, big = MFMA_BATCHES[batch]
    c = _prefill_case(17 * G + len(batch), G, 2, [0] * len(Ts), Ts, True, layout, S_SMALL, no_fuse=False)
    assert c["out"]["qt"] == qt and (max(Ts) <= 256) == big
    _check_prefill(c, "mfma", "rope_mfma", True)
