"""The float64 statement of the Qwen3 decoder attention (tests/qwen_attn_ref.py) against two independent statements of the op: a dense torch
float64 restatement (rotate-half RoPE, repeat-interleaved kv heads, an explicit mask tensor built element by element) and QwenAsrOracle.decoder
itself on one layer of the synthetic qwen_asr_mid checkpoint. Cache layouts and the beam ancestry read are checked against element-by-element
loops; the bound on what the reference's additive -128 leaves a masked key is pinned and shown to be attained. Runs without a GPU, so the
reference the GPU parity tests lean on can be trusted on its own."""
import math

import numpy as np
import torch

import qwen_attn_ref as R
from conftest import sub

EPS = 1e-6
HD = R.HD


def _weights(rng, scale=0.36):
    return [(scale * (1.0 + 0.1 * rng.standard_normal(HD))).astype(np.float32) for _ in range(2)]


def _torch_layer(qkv, H, KV, qn, kn, rope, pos, k_hist, v_hist, hist):
    """One sequence, dense: qkv [T][(H + 2 KV) 128] at positions pos, history [KV][hist][128] -> (ctx [T][H 128], k [KV][hist + T][128])."""
    T, G = len(pos), H // KV
    x = torch.from_numpy(np.asarray(qkv, np.float64)).reshape(T, H + 2 * KV, HD)
    rms = lambda z: z * torch.rsqrt(z.pow(2).mean(-1, keepdim=True) + EPS)
    r = torch.from_numpy(np.asarray(rope, np.float64))[torch.as_tensor(pos)]
    cos, sin = torch.cat([r[:, :64]] * 2, -1)[:, None], torch.cat([r[:, 64:]] * 2, -1)[:, None]
    rot = lambda z: torch.cat([-z[..., 64:], z[..., :64]], -1)
    q = rms(x[:, :H]) * torch.from_numpy(qn.astype(np.float64))
    k = rms(x[:, H:H + KV]) * torch.from_numpy(kn.astype(np.float64))
    q, k = q * cos + rot(q) * sin, k * cos + rot(k) * sin
    k_all = torch.cat([torch.from_numpy(np.asarray(k_hist, np.float64)), k.transpose(0, 1)], 1)            # [KV][S][128]
    v_all = torch.cat([torch.from_numpy(np.asarray(v_hist, np.float64)), x[:, H + KV:].transpose(0, 1)], 1)
    S = hist + T
    mask = torch.zeros((T, S), dtype=torch.float64)
    for i in range(T):
        for j in range(S):
            if j > hist + i:
                mask[i, j] = -128.0
    kk, vv = k_all.repeat_interleave(G, dim=0), v_all.repeat_interleave(G, dim=0)                          # q head h reads kv head h // G
    s = q.transpose(0, 1) @ kk.transpose(-1, -2) + mask[None]
    ctx = torch.softmax(s, dim=-1) @ vv                                                                    # [H][T][128]
    return ctx.transpose(0, 1).reshape(T, H * HD).numpy(), k_all.numpy()


def test_reference_against_dense_torch():
    rng = np.random.default_rng(0)
    G, KV = 4, 2
    H = G * KV
    hists, Ts = [0, 37, 5], [21, 1, 17]
    rope = R.rope_table(64, f16=True)                    # the aligner's f16-rounded table: rows are not exact rotations, both statements must still agree
    qn, kn = _weights(rng)
    row_off = [0, 32, 48]
    rows = 80
    qkv = rng.standard_normal((rows, (H + 2 * KV) * HD))
    pos = np.zeros(rows, np.int64)
    for b in range(3):
        pos[row_off[b]:row_off[b] + Ts[b]] = hists[b] + np.arange(Ts[b])
    k_hist = [rng.standard_normal((KV, h, HD)) * 0.4 for h in hists]
    v_hist = [rng.standard_normal((KV, h, HD)) for h in hists]
    # a future key of sequence 0's query 0 that only the -128 (not -inf) leaves any weight
    q_post = R.new_rows(qkv, H, KV, qn, kn, rope, EPS, pos)[0]
    qkv[1, H * HD:(H + 1) * HD] = R.key_for(q_post[0, 0], kn, rope[1], EPS)[0]
    q, k, v = R.new_rows(qkv, H, KV, qn, kn, rope, EPS, pos)
    ctx, st = R.attention(q, k, v, k_hist, v_hist, hists, Ts, row_off, G)
    for b in range(3):
        r = slice(row_off[b], row_off[b] + Ts[b])
        ref, k_all = _torch_layer(qkv[r], H, KV, qn, kn, rope, pos[r], k_hist[b], v_hist[b], hists[b])
        assert np.abs(ctx[r] - ref).max() < 1e-12
        assert np.abs(k_all[:, hists[b]:] - k[r].transpose(1, 0, 2)).max() < 1e-13
    assert np.isnan(ctx[21:32]).all() and np.isnan(ctx[65:]).all()                      # gap rows
    assert st["n"][0, 0] == 1 and st["n"][32, 0] == 38 and st["n"][48 + 16, 0] == 22
    # the planted future key: masked, so its weight is exp(s - 128 - ...) > 0 and tiny; the statistic reports it
    assert 0.0 < st["masked_weight"][0, 0] < 1e-40 and st["masked_weight"][32].max() == 0.0
    tol = R.budget(ctx, st, "mfma", True)
    live = ~np.isnan(ctx[:, 0])
    assert tol.shape == ctx.shape and (tol[live] >= R.UBF * np.abs(ctx[live])).all()
    assert (R.budget(ctx, st, "fused", False)[live] < R.budget(ctx, st, "fused", True)[live]).all()


def test_key_for_reaches_the_query():
    rng = np.random.default_rng(1)
    qn, kn = _weights(rng)
    for f16 in (False, True):
        rope = R.rope_table(200, f16=f16)
        qp = R.rotate(R.rms_norm(rng.standard_normal(HD), qn, EPS), rope[150])
        for pos, sign in ((0, 1.0), (77, 1.0), (199, -1.0)):
            x, c = R.key_for(qp, kn, rope[pos], EPS, sign)
            key = R.rotate(R.rms_norm(x.astype(np.float64), kn, EPS), rope[pos])
            assert c > 0 and np.abs(key - sign * c * qp).max() < 1e-6 * np.abs(qp).max()


def test_reference_against_the_oracle_decoder(monkeypatch):
    """QwenAsrOracle.decoder on one layer: its soft-max output (tapped) times its own new_v is the attention context; its new_k the cached keys."""
    from oracle.qwen_asr_oracle import QwenAsrOracle
    cfg = sub("config").qwen_asr_mid()
    ck = sub("checkpoints").synth_qwen_asr_checkpoint(cfg, 3)
    orc = QwenAsrOracle(cfg, ck, [1], [2], [3])
    orc.dec = orc.dec[:1]
    L = orc.dec[0]
    H, KV, G = cfg.n_heads, cfg.n_kv_heads, cfg.n_heads // cfg.n_kv_heads
    taps = []
    real = torch.softmax

    def tapped(x, dim):
        taps.append(real(x, dim=dim))
        return taps[-1]
    monkeypatch.setattr(torch, "softmax", tapped)
    rng = np.random.default_rng(4)
    ang = torch.arange(64, dtype=torch.float32)[:, None] * orc.inv_freq[None, :]       # the oracle's own angles: the table is an input of the op, not part of it
    rope = torch.cat([torch.cos(ang), torch.sin(ang)], 1).numpy()
    assert np.abs(rope - R.rope_table(64, theta=cfg.rope_theta)).max() < 1e-5
    qn, kn = L["qn"].numpy(), L["kn"].numpy()
    keys = vals = None
    hist = 0
    for n in (20, 3, 1):                                                 # a prefill, then two appends over the oracle's own cache
        x = torch.from_numpy(rng.standard_normal((n, cfg.d_model)).astype(np.float32))
        with torch.inference_mode():
            _, new_k, new_v = orc.decoder(x, hist, keys, vals)
            qkv = (orc._rms(x, cfg.rms_eps) @ L["wqkv"].t()).numpy()
        p = taps.pop().numpy().astype(np.float64)                        # (KV, G, n, hist + n)
        assert not taps
        o_ctx = (p @ new_v[0].numpy().astype(np.float64)[:, None]).transpose(2, 0, 1, 3).reshape(n, H * HD)
        pos = hist + np.arange(n)
        q, k, v = R.new_rows(qkv, H, KV, qn, kn, rope, cfg.rms_eps, pos)
        k_hist = [keys[0].numpy() if keys is not None else np.zeros((KV, 0, HD))]
        v_hist = [vals[0].numpy() if vals is not None else np.zeros((KV, 0, HD))]
        ctx, st = R.attention(q, k, v, k_hist, v_hist, [hist], [n], [0], G)
        # the oracle is an f32 evaluation of the same expression: it owes the reference what an f32 kernel owes it
        assert (np.abs(o_ctx - ctx) <= R.budget(ctx, st, "scalar", False)).all()
        o_k = new_k[0].numpy()[:, hist:].transpose(1, 0, 2)
        assert (np.abs(o_k - k) <= R.norm_rope_f32_bound(k)).all()
        assert np.array_equal(new_v[0].numpy()[:, hist:].transpose(1, 0, 2), v.astype(np.float32))
        keys, vals, hist = new_k, new_v, hist + n


def test_cache_layouts_round_trip():
    rng = np.random.default_rng(5)
    KV, lens = 3, [1, 16, 17, 40]
    rows = [rng.standard_normal((KV, n, HD)) for n in lens]
    ext = R.scatter_extents(rows, 48)
    for b, n in enumerate(lens):
        assert np.array_equal(R.gather_extents(ext, b, n), rows[b]) and np.isnan(ext[b, :, n:]).all()
    pps, n_pages = 3, 20
    table = 1 + rng.permutation(n_pages - 1)[:len(lens) * pps].reshape(len(lens), pps)
    pool = R.scatter_pages(rows, table, n_pages, n_layers=2, layer=1)
    assert np.isnan(pool[:, 0]).all() and np.isnan(pool[0]).all()
    placed = 0
    for b, n in enumerate(lens):
        assert np.array_equal(R.gather_pages(pool, table, b, n, layer=1), rows[b])
        for s in range(n):                               # element by element, the layout [page][layer][kv head][16][128]
            for kv in range(KV):
                assert np.array_equal(pool[table[b][s // 16], 1, kv, s % 16], rows[b][kv, s])
                placed += HD
    assert np.count_nonzero(~np.isnan(pool)) == placed


def test_beam_ancestry_read():
    rng = np.random.default_rng(6)
    B, beam, KV, S, p0, gen = 6, 3, 2, 8, 5, 7
    prompt = rng.standard_normal((KV, 9, HD))
    ext = rng.standard_normal((B, KV, S, HD))
    src = np.stack([(b // beam) * beam + rng.integers(0, beam, S) for b in range(B)])
    for b in (0, 4):
        got = R.beam_keys(prompt, ext, src[b], p0, gen)
        assert got.shape == (KV, p0 + gen, HD)
        for kv in range(KV):
            for s in range(p0 + gen):
                want = prompt[kv, s] if s < p0 else ext[src[b][s - p0], kv, s - p0]
                assert np.array_equal(got[kv, s], want)
    assert R.beam_keys(prompt, ext, src[0], p0, 0).shape == (KV, p0, HD)


def test_masked_weight_bound_holds_and_is_attained():
    """Under the reference's additive -128 no masked key gets more than exp(2 c - 128), c = 128 max|qn| max|kn|: random operands stay below it, and
    operands built for it reach it -- constant weights a, one visible key pointing away from the query (score -c), one masked key pointing at it (+c)."""
    rng = np.random.default_rng(7)
    rope = R.rope_table(8)
    H, KV = 1, 1
    for scale in (0.3, 0.5, 0.7):
        qn, kn = _weights(rng, scale)
        c, bound = R.masked_weight_bound(qn, kn, rope)
        qkv = rng.standard_normal((6, 3 * HD))
        q, k, v = R.new_rows(qkv, H, KV, qn, kn, rope, 0.0, np.arange(6))
        assert np.abs(q[:, 0] @ k[:, 0].T).max() <= c
        _, st = R.attention(q, k, v, [np.zeros((1, 0, HD))], [np.zeros((1, 0, HD))], [0], [6], [0], 1)
        assert st["masked_weight"].max() <= bound
    for a in (0.25, 0.5, 0.68):
        qn = kn = np.full(HD, a, np.float32)
        c, bound = R.masked_weight_bound(qn, kn, rope)
        assert math.isclose(c, 128 * float(np.float32(a)) ** 2, rel_tol=1e-6)          # (the f32 table's rows are rotations to 2^-23)
        qkv = rng.standard_normal((2, 3 * HD))                          # any query row: with constant weights only its direction matters
        q0 = R.new_rows(qkv, H, KV, qn, kn, rope, 0.0, np.arange(2))[0][0, 0]
        qkv[0, HD:2 * HD] = R.key_for(q0, kn, rope[0], 0.0, sign=-1.0)[0]   # the query's own key: the only visible one
        qkv[1, HD:2 * HD] = R.key_for(q0, kn, rope[1], 0.0, sign=+1.0)[0]   # the next position's key: masked
        q, k, v = R.new_rows(qkv, H, KV, qn, kn, rope, 0.0, np.arange(2))
        assert abs(q[0, 0] @ k[0, 0] + c) < 1e-4 * c and abs(q[0, 0] @ k[1, 0] - c) < 1e-4 * c
        _, st = R.attention(q, k, v, [np.zeros((1, 0, HD))], [np.zeros((1, 0, HD))], [0], [2], [0], 1)
        w = st["masked_weight"][0, 0]
        assert w <= bound * (1 + 1e-9) and w >= 0.5 * bound * math.exp(-1e-3 * c), (w, bound)
    # the synthetic checkpoints of this tree: 128^-1/4 (1 + 0.1 N) folded weights
    cfg = sub("config").qwen_asr_mid()
    ck = sub("checkpoints").synth_qwen_asr_checkpoint(cfg, 0)
    sc = cfg.d_head ** -0.25
    worst = max(R.masked_weight_bound(ck[f"thinker.model.layers.{i}.self_attn.q_norm.weight"] * sc, ck[f"thinker.model.layers.{i}.self_attn.k_norm.weight"] * sc)[1]
                for i in range(cfg.n_layers))
    assert worst < 1e-30


def test_bf16_helpers():
    x = np.random.default_rng(8).standard_normal(4096).astype(np.float32) * 50
    assert np.array_equal(R.bf16_round(x), torch.from_numpy(x).to(torch.bfloat16).float().numpy())
    assert R.bf16_ulp(1.0) == 2.0 ** -7 and R.bf16_ulp(1.99) == 2.0 ** -7 and R.bf16_ulp(-2.0) == 2.0 ** -6
    assert (np.abs(R.bf16_round(x).astype(np.float64) - x) <= R.UBF * np.abs(x)).all()
