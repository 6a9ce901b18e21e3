"""Float64 statement of the Whisper decoder attention (launch_decode_attention, head_dim 64) and its error budget.

Scores are q . k with no extra scaling (the q projection carries it); the soft-max runs over the sequence's keys; a prefill's
causal mask is the reference's additive -128 (Export_Whisper.py:472), not -inf. The caller passes the operand values the kernel
saw: bf16-rounded inputs, or dequantised e4m3 bytes times their slab scale."""
import numpy as np

CAUSAL_MASK = -128.0
PAGE = 16
U32 = 2.0 ** -24


def bf16_round(x):
    """f32 -> nearest bf16 (ties to even), as f32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF) << 16).astype(np.uint32).view(np.float32)


def _attend(q, k, v, mask):
    """q [n][64], k / v [S][64], mask [n][S] additive -> (context [n][64], max |v| per query, max sum_i |q_i k_i| per query)."""
    q, k, v = (np.asarray(t, np.float64) for t in (q, k, v))
    s = q @ k.T + mask
    p = np.exp(s - s.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    n = q.shape[0]
    return p @ v, np.full(n, np.abs(v).max()), (np.abs(q) @ np.abs(k).T).max(axis=1)


def causal_mask(n, hist):
    """[n][hist + n]: query i (position hist + i) sees keys 0 .. hist + i; later keys get the additive -128."""
    j = np.arange(hist + n)[None, :]
    i = np.arange(n)[:, None]
    return np.where(j > hist + i, CAUSAL_MASK, 0.0)


def self_attention(q, kv_new, k_hist, v_hist, n, causal=True):
    """q [B n][H 64], kv_new [B n][2 H 64] (k columns, then v), k_hist / v_hist [B][H][hist][64].
    Returns (out [B n][H 64], vmax [B n][H], amax [B n][H])."""
    B, H, hist, _ = k_hist.shape
    qh = np.asarray(q, np.float64).reshape(B, n, H, 64)
    kn = np.asarray(kv_new, np.float64)[:, :H * 64].reshape(B, n, H, 64)
    vn = np.asarray(kv_new, np.float64)[:, H * 64:].reshape(B, n, H, 64)
    mask = causal_mask(n, hist) if causal else np.zeros((n, hist + n))
    out = np.zeros((B, n, H, 64))
    vmax, amax = np.zeros((B, n, H)), np.zeros((B, n, H))
    for b in range(B):
        for h in range(H):
            k = np.concatenate([k_hist[b, h], kn[b, :, h]], axis=0)
            v = np.concatenate([v_hist[b, h], vn[b, :, h]], axis=0)
            out[b, :, h], vmax[b, :, h], amax[b, :, h] = _attend(qh[b, :, h], k, v, mask)
    return out.reshape(B * n, H * 64), vmax.reshape(B * n, H), amax.reshape(B * n, H)


def cross_attention(q, k_slab, v_slab, row_off, n_lfr, n, k_scale=None, v_scale=None):
    """q [B n][H 64], slabs [H][rows][64]: sequence b attends rows row_off[b] .. row_off[b] + n_lfr[b] of every head, unmasked.
    k_scale / v_scale [H][B] multiply the slab rows (FP8 slabs: pass the e4m3 values). Returns (out, vmax, amax) as self_attention."""
    H = k_slab.shape[0]
    B = len(n_lfr)
    qh = np.asarray(q, np.float64).reshape(B, n, H, 64)
    out = np.zeros((B, n, H, 64))
    vmax, amax = np.zeros((B, n, H)), np.zeros((B, n, H))
    for b in range(B):
        r = slice(int(row_off[b]), int(row_off[b]) + int(n_lfr[b]))
        for h in range(H):
            k = np.asarray(k_slab[h, r], np.float64) * (1.0 if k_scale is None else float(k_scale[h, b]))
            v = np.asarray(v_slab[h, r], np.float64) * (1.0 if v_scale is None else float(v_scale[h, b]))
            out[b, :, h], vmax[b, :, h], amax[b, :, h] = _attend(qh[b, :, h], k, v, np.zeros((n, int(n_lfr[b]))))
    return out.reshape(B * n, H * 64), vmax.reshape(B * n, H), amax.reshape(B * n, H)


def budget(ref, vmax, amax, bf16, fast_exp):
    """Per-element error bound of a kernel that computes in f32 and stores `bf16` or f32.
    f32 part: a score error of <= 16 roundings of sum |q_i k_i| moves a soft-max weight by twice that (relative); exp, the
    normaliser and the context sums (<= ~60 dependent f32 additions) add 1e-5 of max |v| (2e-5 for the hardware __expf forms).
    bf16 output: one round-to-nearest of the result, 2^-8 |ref|."""
    H = vmax.shape[1]
    f32 = vmax * ((2e-5 if fast_exp else 1e-5) + 32 * U32 * amax)
    tol = np.repeat(f32, 64, axis=1).reshape(-1, H * 64)
    return tol + (2.0 ** -8 * np.abs(ref) if bf16 else 0.0)


def scatter_pages(rows, page_table, n_pages):
    """[B][H][S][64] rows -> a pool [n_pages][2][H][PAGE][64] (K half only) laid out as whisper.hip's paged cache:
    position s of (b, h) sits in page page_table[b][s // 16] at [h][s % 16]. Unused slots are NaN."""
    B, H, S, _ = rows.shape
    pool = np.full((n_pages, 2, H, PAGE, 64), np.nan)
    for b in range(B):
        for s in range(S):
            pool[page_table[b][s // PAGE], 0, :, s % PAGE] = rows[b, :, s]
    return pool


def gather_pages(pool, page_table, S):
    """Inverse of scatter_pages: [B][H][S][64] from the K half of the pool."""
    pt = np.asarray(page_table)
    s = np.arange(S)
    return pool[pt[:, s // PAGE], 0, :, s % PAGE].transpose(0, 2, 1, 3)
