"""The float64 decoder-attention reference (tests/decode_attn_ref.py) against an independent statement of the op: dense padded
tensors, torch.softmax in float64 and an explicit mask tensor. Runs without a GPU, so the reference the GPU parity tests lean on
can be trusted on its own."""
import numpy as np
import torch

import decode_attn_ref as R


def _torch_attention(q, k, v, mask):
    """q [B][H][n][64], k / v [B][H][S][64], mask [B][n][S] additive (-inf = key absent)."""
    s = q @ k.transpose(-1, -2) + mask[:, None]
    return torch.softmax(s, dim=-1) @ v


def test_self_reference_paged_causal():
    rng = np.random.default_rng(0)
    B, H, hist, n = 3, 5, 37, 4
    S = hist + n
    q = rng.standard_normal((B * n, H * 64))
    kv_new = rng.standard_normal((B * n, 2 * H * 64))
    k_hist = rng.standard_normal((B, H, hist, 64)) * 0.3
    v_hist = rng.standard_normal((B, H, hist, 64))
    kv_new[n - 1, :64] = q[0, :64] * 130.0 / (q[0, :64] @ q[0, :64])   # a future key of query 0 scoring 130: visible through -128 only
    # the cached rows travel through a permuted paged pool and back
    pps, n_pages = (S + 15) // 16, 3 * ((S + 15) // 16) + 2
    pt = rng.permutation(n_pages)[:B * pps].reshape(B, pps)
    pool = R.scatter_pages(k_hist, pt, n_pages)
    assert np.array_equal(R.gather_pages(pool, pt, hist), k_hist)
    out, vmax, amax = R.self_attention(q, kv_new, R.gather_pages(pool, pt, hist), v_hist, n)

    # independent: keys read straight from the pool by (page, slot) per position, mask built element by element
    P = torch.from_numpy(pool)
    kc = torch.stack([torch.stack([P[pt[b][s // 16], 0, :, s % 16] for s in range(hist)], dim=1) for b in range(B)])   # [B][H][hist][64]
    kn = torch.from_numpy(kv_new[:, :H * 64]).reshape(B, n, H, 64).permute(0, 2, 1, 3)
    vn = torch.from_numpy(kv_new[:, H * 64:]).reshape(B, n, H, 64).permute(0, 2, 1, 3)
    k = torch.cat([kc, kn], dim=2)
    v = torch.cat([torch.from_numpy(v_hist), vn], dim=2)
    mask = torch.zeros((B, n, S), dtype=torch.float64)
    for i in range(n):
        for j in range(S):
            if j > hist + i:
                mask[:, i, j] = -128.0
    qt = torch.from_numpy(q).reshape(B, n, H, 64).permute(0, 2, 1, 3)
    ref = _torch_attention(qt, k, v, mask).permute(0, 2, 1, 3).reshape(B * n, H * 64).numpy()
    assert np.abs(out - ref).max() < 1e-12
    # the -128 (not -inf) semantics matter here: with -inf the masked key would have no weight at all
    inf_mask = torch.where(mask < 0, torch.tensor(-np.inf, dtype=torch.float64), mask)
    ref_inf = _torch_attention(qt, k, v, inf_mask).permute(0, 2, 1, 3).reshape(B * n, H * 64).numpy()
    assert np.abs(out[0, :64] - ref_inf[0, :64]).max() > 1e-3
    assert vmax.shape == amax.shape == (B * n, H) and (amax > 0).all()
    # the budget: f32 term + one bf16 rounding
    tol = R.budget(out, vmax, amax, bf16=True, fast_exp=False)
    assert tol.shape == out.shape and (tol >= 2.0 ** -8 * np.abs(out)).all()


def test_cross_reference_ragged_scaled():
    rng = np.random.default_rng(1)
    H, n = 3, 2
    n_lfr = np.array([1, 17, 130, 64])
    row_off = np.array([0, 16, 48, 192])                # gaps between the extents
    rows = 272
    B = len(n_lfr)
    k_slab = rng.standard_normal((H, rows, 64)) * 0.2
    v_slab = rng.standard_normal((H, rows, 64))
    k_scale = 2.0 ** rng.integers(-3, 3, size=(H, B))
    v_scale = 2.0 ** rng.integers(-3, 3, size=(H, B))
    q = rng.standard_normal((B * n, H * 64))
    out, _, _ = R.cross_attention(q, k_slab, v_slab, row_off, n_lfr, n, k_scale, v_scale)

    # independent: every sequence padded to the longest extent, absent keys masked with -inf
    Smax = int(n_lfr.max())
    k = torch.zeros((B, H, Smax, 64), dtype=torch.float64)
    v = torch.zeros_like(k)
    mask = torch.full((B, n, Smax), -np.inf, dtype=torch.float64)
    for b in range(B):
        L, r0 = int(n_lfr[b]), int(row_off[b])
        k[b, :, :L] = torch.from_numpy(k_slab[:, r0:r0 + L]) * torch.from_numpy(k_scale[:, b])[:, None, None]
        v[b, :, :L] = torch.from_numpy(v_slab[:, r0:r0 + L]) * torch.from_numpy(v_scale[:, b])[:, None, None]
        mask[b, :, :L] = 0.0
    qt = torch.from_numpy(q).reshape(B, n, H, 64).permute(0, 2, 1, 3)
    ref = _torch_attention(qt, k, v, mask).permute(0, 2, 1, 3).reshape(B * n, H * 64).numpy()
    assert np.abs(out - ref).max() < 1e-12
    # a single key: the context is that key's value row
    assert np.abs(out[:n].reshape(n, H, 64) - (v_slab[:, 0] * v_scale[:, 0, None])[None]).max() < 1e-12


def test_bf16_round_matches_torch():
    x = np.random.default_rng(2).standard_normal(4096).astype(np.float32) * 100
    x[:4] = [1.00390625, 1.01171875, -3.0e38, 0.0]      # ties to even either way
    assert np.array_equal(R.bf16_round(x), torch.from_numpy(x).to(torch.bfloat16).float().numpy())
