"""Float64 statement of the attention stage of a Qwen3 decoder layer (head_dim 128) and its error budget.

Written from the reference's semantics (Export_Qwen_ASR.py DECODER_MAIN.forward, ROTARY_MASK_PREFILL / _DECODE), not from the kernels:
per-head RMSNorm of q and k over the 128 elements times the folded weights qn / kn (d_head^-1/4 inside, so scores carry no extra scale),
RoPE in the half-split convention from a table row [cos 0..63 | sin 0..63] at position hist + t, v cached unchanged, grouped-query
attention (q head h reads kv head h // G), soft-max over the sequence's keys with the reference's causal mask: an ADDITIVE -128 on the
keys past the query, not -inf. The HIP kernels mask strictly; `masked_weight` is the largest weight the reference's mask leaves a
masked key, i.e. how far the two can be apart ("Causal masking of the Qwen3 decoder")."""
import math

import numpy as np

HD = 128
HALF = 64
PAGE = 16
CAUSAL_MASK = -128.0
U32 = 2.0 ** -24            # unit roundoff of f32
UBF = 2.0 ** -8             # unit roundoff of bf16 (8 significant bits): round-to-nearest moves x by at most UBF |x|
ROPE_F32_UNITS = 18         # see norm_rope_f32_bound


def bf16_round(x):
    """f32 -> nearest bf16 (ties to even), as f32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF) << 16).astype(np.uint32).view(np.float32)


def bf16_ulp(x):
    """Spacing of bf16 numbers at |x| (x != 0): 2^(floor(log2 |x|) - 7)."""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126))) - 7)


def rope_table(n_pos, theta=1e6, f16=False):
    """[n_pos][cos 0..63 | sin 0..63] in f32, as the weight arena stores it; f16 = True: rounded through float16 (the forced aligner's table)."""
    inv_freq = (1.0 / (np.float32(theta) ** (np.arange(0, HD, 2, dtype=np.float32) / HD))).astype(np.float32)
    ang = np.arange(n_pos, dtype=np.float32)[:, None] * inv_freq[None, :]
    t = np.concatenate([np.cos(ang), np.sin(ang)], 1).astype(np.float32)
    return t.astype(np.float16).astype(np.float32) if f16 else t


def rms_norm(x, w, eps):
    x = np.asarray(x, np.float64)
    return x / np.sqrt((x * x).mean(axis=-1, keepdims=True) + eps) * np.asarray(w, np.float64)


def rotate(y, row):
    """Half-split RoPE of y [..., 128] by table row(s) [..., 128]: (y0, y1) -> (y0 c - y1 s, y1 c + y0 s)."""
    y, row = np.asarray(y, np.float64), np.asarray(row, np.float64)
    c, s = row[..., :HALF], row[..., HALF:]
    y0, y1 = y[..., :HALF], y[..., HALF:]
    return np.concatenate([y0 * c - y1 * s, y1 * c + y0 * s], -1)


def unrotate(y, row):
    """Inverse of rotate() when the row is an exact rotation; in general the solution z of rotate(z, row) = y."""
    y, row = np.asarray(y, np.float64), np.asarray(row, np.float64)
    c, s = row[..., :HALF], row[..., HALF:]
    det = c * c + s * s
    y0, y1 = y[..., :HALF], y[..., HALF:]
    return np.concatenate([(y0 * c + y1 * s) / det, (y1 * c - y0 * s) / det], -1)


def new_rows(qkv, H, KV, qn, kn, rope, eps, pos, bf16=False):
    """qkv [rows][(H + 2 KV) 128] at positions pos [rows] -> q [rows][H][128], k [rows][KV][128], v [rows][KV][128] in float64.
    q and k are NOT rounded to the session's element type (budget() accounts for that rounding); v is: a bf16 session caches bf16(v)."""
    x = np.asarray(qkv, np.float64).reshape(len(pos), H + 2 * KV, HD)
    r = np.asarray(rope, np.float64)[np.asarray(pos)][:, None, :]
    q = rotate(rms_norm(x[:, :H], qn, eps), r)
    k = rotate(rms_norm(x[:, H:H + KV], kn, eps), r)
    v = x[:, H + KV:]
    if bf16:
        v = bf16_round(v.astype(np.float32)).astype(np.float64)
    return q, k, v


def key_for(q_post, kn, rope_row, eps, sign=1.0):
    """The pre-norm key row x whose normed, rotated key at table row `rope_row` is sign * c * q_post with the one c > 0 a normed row can reach
    (kn * x / rms(x) has a fixed size). Returns (x in f32, c)."""
    z = unrotate(np.asarray(q_post, np.float64), rope_row) / np.asarray(kn, np.float64)
    c = 1.0 / math.sqrt(float((z * z).mean()))
    return (sign * c * z).astype(np.float32), c


def attend(q, k, v, qpos):
    """q [n][128] at positions qpos [n], k / v [S][128] (key j at position j) -> context [n][128] under the additive -128 mask, and per query:
    vmax (largest |v| among its visible keys), amax (largest sum_i |q_i k_i| among them), a1 (max |q| * largest 1-norm of a visible key + 1-norm
    of q * largest |k|), smax (largest |score|), n (visible keys), masked_weight (largest soft-max weight of a masked key, 0 if none)."""
    q, k, v = (np.asarray(t, np.float64) for t in (q, k, v))
    qpos = np.asarray(qpos)
    vis = np.arange(k.shape[0])[None, :] <= qpos[:, None]
    s = q @ k.T
    sm = s + np.where(vis, 0.0, CAUSAL_MASK)
    p = np.exp(sm - sm.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    absqk = np.abs(q) @ np.abs(k).T
    k1, kinf, vinf = np.abs(k).sum(axis=1), np.abs(k).max(axis=1), np.abs(v).max(axis=1)
    ninf = -np.inf
    st = dict(vmax=np.where(vis, vinf[None, :], ninf).max(axis=1), amax=np.where(vis, absqk, ninf).max(axis=1),
              a1=np.abs(q).max(axis=1) * np.where(vis, k1[None, :], ninf).max(axis=1) + np.abs(q).sum(axis=1) * np.where(vis, kinf[None, :], ninf).max(axis=1),
              smax=np.where(vis, np.abs(s), ninf).max(axis=1), n=vis.sum(axis=1).astype(np.float64),
              masked_weight=np.where(vis, 0.0, p).max(axis=1), win=np.where(vis, p, 0.0).max(axis=1))
    return p @ v, st


STAT_KEYS = ("vmax", "amax", "a1", "smax", "n", "masked_weight", "win")


def attention(q, k_new, v_new, k_hist, v_hist, hist, T, row_off, G):
    """The layer's attention over packed rows. q [rows][H][128], k_new / v_new [rows][KV][128] (new_rows), k_hist[b] / v_hist[b] [KV][>= hist[b]][128]
    (the sequence's cached rows, already gathered from wherever they live), sequence b = rows row_off[b] .. + T[b] at positions hist[b] ...
    Returns (ctx [rows][H 128], rows gap rows NaN; stats {name: [rows][H]})."""
    rows, H, _ = q.shape
    ctx = np.full((rows, H, HD), np.nan)
    st = {k: np.full((rows, H), np.nan) for k in STAT_KEYS}
    for b in range(len(T)):
        r = slice(int(row_off[b]), int(row_off[b]) + int(T[b]))
        h0 = int(hist[b])
        for h in range(H):
            kv = h // G
            k = np.concatenate([np.asarray(k_hist[b][kv][:h0], np.float64).reshape(h0, HD), k_new[r, kv]], 0)
            v = np.concatenate([np.asarray(v_hist[b][kv][:h0], np.float64).reshape(h0, HD), v_new[r, kv]], 0)
            ctx[r, h], s1 = attend(q[r, h], k, v, h0 + np.arange(int(T[b])))
            for key in STAT_KEYS:
                st[key][r, h] = s1[key]
    return ctx.reshape(rows, H * HD), st


def masked_weight_bound(qn, kn, rope=None):
    """No masked key's weight under the additive -128 exceeds exp(2 c - 128), c = 128 max|qn| max|kn| rho (folded weights): a normed row x / rms(x) has
    2-norm sqrt(128), so |q| <= sqrt(128) max|qn|, |k| <= sqrt(128) max|kn| before RoPE; a table row stretches a pair by sqrt(cos^2 + sin^2), which is 1
    for an exact rotation and up to sqrt(rho), rho = max (cos^2 + sin^2) over the table, for a rounded one (1 + 2^-23 in f32, 1 + 2^-10 for the aligner's
    f16 table); so every |score| <= c, and a masked key's weight is at most exp(s_masked - 128) / exp(s_visible) <= exp(c - 128 + c).
    (With the unfolded q_norm / k_norm weights w: 128 max|qn| max|kn| = sqrt(128) max|w_q| max|w_k|.) Returns (c, the bound)."""
    rho = 1.0 if rope is None else float((np.asarray(rope, np.float64)[:, :HALF] ** 2 + np.asarray(rope, np.float64)[:, HALF:] ** 2).max())
    c = HD * float(np.abs(qn).max()) * float(np.abs(kn).max()) * max(rho, 1.0)
    return c, math.exp(2.0 * c + CAUSAL_MASK)


def norm_rope_f32_bound(row):
    """Bound on |kernel - float64| per element of a normed, rotated row [..., 128] computed in f32: ROPE_F32_UNITS * 2^-24 * max|row| (u = 2^-24).
    Sum of 128 squares: one product rounding, then additions in a tree of depth <= 7 (lane-local, then shuffles) over positive terms: relative
    error <= 8 u. / 128 is exact, + eps one rounding: 9 u. rsqrtf is within 2 ulp = 4 u of 1 / sqrt, which halves the relative error of its
    argument: 4.5 u + 4 u = 8.5 u. Two multiplies (x * r * w): a0, a1 carry 10.5 u. y0 = a0 c - a1 s, y1 = a1 c + a0 s: two products and an
    addition (or a product and an fma) add 2 u on |a0 c| + |a1 s| <= sqrt(a0^2 + a1^2) (c^2 + s^2 = 1, to 2^-11 for the f16-rounded table):
    12.5 u times the pair's norm. The rotation keeps the pair's norm, sqrt(y0^2 + y1^2) <= sqrt(2) max|row|: 17.7 u max|row| -> 18."""
    return ROPE_F32_UNITS * U32 * np.abs(np.asarray(row, np.float64)).max(axis=-1, keepdims=True)


def budget(ref, st, form, bf16):
    """Per-element bound on |kernel - ref| for context rows ref [rows][H 128] with the stats of attention(); form in "fused", "beam", "scalar", "mfma".
    Every kernel computes in f32 (u = 2^-24) from operands of the session's element type. Per (row, head), with n visible keys:

    scores  q . k as 128 f32 fmas in any order: (128 + 1) u sum|q_i k_i| <= 129 u amax.
            The operands: in an f32 session q and the keys written by this call carry norm_rope_f32_bound (18 u max|.| per element), which
            moves a score by at most 18 u (max|q| |k|_1 + |q|_1 max|k|) = 18 u a1. In a bf16 session the kernel rounds q and the new k to bf16 AFTER
            RoPE; the reference does not round them, so each differs from the reference's by <= UBF |.| (+ the f32 error, which can also flip the
            rounding -- that is inside UBF |.| because round-to-nearest of a value e away lands within UBF |x| + e): 2 UBF amax (history keys are
            exact, the bound charges them too). d_score = 129 u amax + 18 u a1 [+ 2 UBF amax].
    weights a score error d moves the soft-max weights by at most expm1(2 d) in 1-norm.
    exp     weight j is a product of exponentials whose arguments (all <= 0) sum to s_j - max: exp(s_j - m_block), one rescale per block of
            the online soft-max, one factor in the 16-way merge. __expf(x) = exp2(x log2 e) and expf are within 2 u relative plus u |x| from rounding
            the argument; every factor costs one more multiply. With F factors: relative error <= (3 F + (max - s_j)) u, and sum_j w_j (max - s_j)
            <= ln n. Fused / beam: F = ceil(n / 64) + 2 (blocks of 4 x 16 keys per lane group -- beam: 2 x 16, F = ceil(n / 32) + 2 --, new key,
            merge); scalar (expf, two-pass): F = 1. Numerator and normaliser both: 2 (3 F + ln n) u.
            MFMA: p = exp2(fma(s, log2 e, -m log2 e)): the argument's error is relative to |s| + |m| <= 2 smax, not to s - m, and the running
            rescale exp2((m_old - m_new) log2 e) likewise; F = ceil(n / 32) + 1 sub-tiles: 2 F (3 + 4 smax) u.
            MFMA only: the probabilities are packed to bf16 as the B operand of O^T = V^T P^T while the normaliser sums them in f32 (kernels.hip,
            `pf.w[..] = pack_bf16x2(p..)` against `l_run = fma(l_run, alpha, ps)`): UBF on every weight of the numerator.
    sums    sum_j p_j v_j and sum_j p_j in f32: A u each, A additions on the longest chain: n + 2 (scalar: sequential; MFMA: order unspecified),
            ceil(n / 16) + 19 (fused / beam: one lane group's keys, then the merge of 16).
    divide  2 u.
    All of the above times vmax (the largest |v| the row can see). Output: a bf16 session stores bf16: UBF |ref|."""
    n, amax, a1, smax, vmax = st["n"], st["amax"], st["a1"], st["smax"], st["vmax"]
    d_score = 129 * U32 * amax + ROPE_F32_UNITS * U32 * a1 + (2 * UBF * amax if bf16 else 0.0)
    ln_n = np.log(np.maximum(n, 1.0))
    if form in ("fused", "beam"):
        F = np.ceil(n / (64 if form == "fused" else 32)) + 2
        w_exp, p_round, A = 2 * (3 * F + ln_n) * U32, 0.0, np.ceil(n / 16) + 19
    elif form == "scalar":
        w_exp, p_round, A = 2 * (3 + ln_n) * U32, 0.0, n + 2
    elif form == "mfma":
        F = np.ceil(n / 32) + 1
        w_exp, p_round, A = 2 * F * (3 + 4 * smax) * U32, UBF, n + 2
    else:
        raise ValueError(form)
    rel = np.expm1(2 * d_score) + w_exp + p_round + 2 * A * U32 + 2 * U32
    tol = np.repeat(vmax * rel, HD, axis=1)
    return tol + (UBF * np.abs(ref) if bf16 else 0.0)


# ---- cache layouts
def scatter_extents(rows, S_max):
    """rows[b] [KV][n_b][128] -> [B][KV][S_max][128], NaN past a sequence's rows."""
    KV = rows[0].shape[0]
    ext = np.full((len(rows), KV, S_max, HD), np.nan)
    for b, r in enumerate(rows):
        ext[b, :, :r.shape[1]] = r
    return ext


def gather_extents(ext, b, n):
    return ext[b, :, :n]


def scatter_pages(rows, table, n_pages, n_layers=1, layer=0):
    """rows[b] [KV][n_b][128] -> the pool [n_pages][n_layers][KV][16][128]: position s of sequence b sits in page table[b][s // 16], slot s % 16 of `layer`.
    Everything else is NaN."""
    KV = rows[0].shape[0]
    pool = np.full((n_pages, n_layers, KV, PAGE, HD), np.nan)
    for b, r in enumerate(rows):
        for s in range(r.shape[1]):
            pool[table[b][s // PAGE], layer, :, s % PAGE] = r[:, s]
    return pool


def gather_pages(pool, table, b, n, layer=0):
    """Inverse of scatter_pages for sequence b: [KV][n][128]."""
    s = np.arange(n)
    return pool[np.asarray(table)[b, s // PAGE], layer, :, s % PAGE].transpose(1, 0, 2)


def beam_keys(prompt, ext, src_row, p0, gen):
    """What hypothesis row b reads at positions [0, p0 + gen): prompt [KV][>= p0][128] (its utterance's prefill cache) for s < p0, then generated
    position p0 + j from slot j of row src_row[j] of the extents ext [B][KV][S][128]. -> [KV][p0 + gen][128]."""
    j = np.arange(gen)
    return np.concatenate([np.asarray(prompt)[:, :p0], ext[np.asarray(src_row)[:gen], :, j].transpose(1, 0, 2)], axis=1)
