"""Float64 statements of the decode GEMM (csrc/decode_gemm.hip) and of the low-bit kernels around it, their float32 evaluations in the kernels' own summation
orders (they exist ONLY to measure E_round = stat(exact - rounded)), the codecs of the byte and nibble formats, and planted faults that prove the comparison.

decode_gemm_ref(a, w, ...) is gemm_ref.gemm_ref restricted to what DecGemmArgs has: operands rounded to bf16, the optional LayerNorm fold over ALL K columns,
+ bias + add, activation 0..3, outputs "f32" and "lo". Low-bit weights enter as their dequantised copy (exact in bf16); w_scale (W8) only places the per-column
scale where the kernel has it in the float32 evaluation: after the K sum, before mean * colsum and the bias.

The float32 orders of a case: "seq", "lib" and the kernel's K partition (decode_partition): steps of 32 go into `splits` workgroup shares and then eight wave
shares, a wave sums its steps in order (a 32-long dot product enters the accumulator as one rounded term), the waves of a workgroup are added 0..7 (wave w of
column granule x holds share (w + x) & 7: `rot`), then the splits in order. The fold statistics follow the same partition in the one-pass form.
"""
import numpy as np
import torch

import gemm_ref as R
from gemm_ref import F32, F64, MARGIN, bf16, e_round, stat, within  # noqa: F401

DW = 8
E2M1_LEVELS = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
SENTINEL = 0xA5


# ---- the K partition ---------------------------------------------------------------------------------------------------------------------------------------
def decode_partition(K, splits):
    """[split][wave share 0..7] -> (k_lo, k_hi) in elements, as decode_gemm_kernel computes wg_lo, wg_n, w_lo, w_hi; empty shares included."""
    steps = K >> 5
    parts = []
    for ks in range(splits):
        wg_lo = steps * ks // splits
        wg_n = steps * (ks + 1) // splits - wg_lo
        parts.append([(32 * (wg_lo + wg_n * kw // DW), 32 * (wg_lo + wg_n * (kw + 1) // DW)) for kw in range(DW)])
    return parts


def mm32_parts(a, w, parts, rot=0):
    """gemm_ref.mm32 with a boundary list as the order: a [M][K] x w [N][K]^T in float32, every share a running sum of 32-long dot products, the shares of a
    split added in wave order (wave i holds share (i + rot) & 7), the splits added in order."""
    assert a.dtype == F32 and w.dtype == F32
    a64, w64 = a.to(F64), w.to(F64)
    tot = None
    for wg in parts:
        wsum = None
        for i in range(len(wg)):
            lo, hi = wg[(i + rot) % len(wg)]
            acc = torch.zeros(a.shape[0], w.shape[0], dtype=F32)
            for k in range(lo, hi, 32):
                acc += (a64[:, k:k + 32] @ w64[:, k:k + 32].t()).to(F32)
            wsum = acc if wsum is None else wsum + acc
        tot = wsum if tot is None else tot + wsum
    return tot


def _mm(a, w, order):
    if isinstance(order, tuple) and order and order[0] == "parts":
        return mm32_parts(a, w, order[1], order[2])
    return R.mm32(a, w, order)


def decode_orders(K, splits):
    """The float32 orders of one case: sequential, the library's, and the kernel's partition as column granules 0, 3 and 5 see it."""
    parts = decode_partition(K, splits)
    return ["seq", "lib"] + [("parts", parts, rot) for rot in (0, 3, 5)]


# ---- the decode GEMM ---------------------------------------------------------------------------------------------------------------------------------------
def decode_gemm_ref(a, w, bias=None, add=None, act=0, fold=False, ln_eps=1e-5, w_scale=None, rounded=None, order="seq", mut=None, splits=1, block_rows=0,
                    one_pass=True):
    """-> {"f32", "lo"} float64 arrays [M][N]. rounded=None: the float64 statement ("lo" unrounded, two-pass variance); "f32": float32 in `order`, one-pass
    variance summed in the same order (one_pass=False: the two-pass variance in float32, which no kernel computes -- test_lowbit_ref_cpu.py measures
    against it where the one-pass form stops working), stores rounded. mut (test_lowbit_ref_cpu.py): "drop_split" the partial of split 1 of `splits` left out,
    "stats_first_split" fold statistics of split 0 only, "w8_scale_late" the W8 scale applied after the mean * colsum term, "row_block" rows
    block_rows .. 2 block_rows - 1 computed from A rows 0 .., "act_before_add", "nibble_swap" the two elements of every weight byte exchanged."""
    assert rounded in (None, "f32")
    dt = F64 if rounded is None else F32
    with torch.inference_mode():
        A, W = bf16(R._t(a, F64)), bf16(R._t(w, F64))
        M, K = A.shape
        N = W.shape[0]
        parts = decode_partition(K, splits)
        Wm = W
        if mut == "nibble_swap":
            Wm = W.reshape(N, K // 2, 2).flip(2).reshape(N, K)
        Am = A.clone()
        if mut == "drop_split":
            Am[:, parts[1][0][0]:parts[1][-1][1]] = 0.0
        if mut == "row_block":
            n_blk = min(block_rows, M - block_rows)
            Am[block_rows:block_rows + n_blk] = A[:n_blk]
        sc = None if w_scale is None else R._t(w_scale, F64)
        Wk = Wm if sc is None else Wm / sc[:, None]                  # the bytes as the matrix pipe sees them (power-of-two scales: exact)
        c = Am @ Wk.t() if rounded is None else _mm(Am.to(F32), Wk.to(F32), order)
        scale_late = sc is not None and mut == "w8_scale_late"
        if sc is not None and not scale_late:
            c = c * sc.to(dt)[None, :]
        if fold:
            xs = A if mut != "stats_first_split" else A[:, parts[0][0][0]:parts[0][-1][1]]
            if rounded is None:
                mean = xs.sum(1, keepdim=True) / K
                var = ((xs - mean) ** 2).sum(1, keepdim=True) / K if mut != "stats_first_split" else ((xs * xs).sum(1, keepdim=True) / K - mean * mean).clamp(min=0.0)
            else:
                one = torch.ones(1, xs.shape[1], dtype=F32)
                if isinstance(order, tuple) and mut != "stats_first_split":
                    s1 = mm32_parts(xs.to(F32), one, order[1], order[2])
                    s2 = _diag_sq_parts(xs, order[1], order[2])
                else:
                    o = order if not isinstance(order, tuple) else "seq"
                    s1 = R.mm32(xs.to(F32), one, o)
                    s2 = R.mm32((xs * xs).to(F32), one, o)          # (the squares of bf16 values are exact in f32)
                inv_k = torch.tensor(1.0 / K, dtype=F32)
                mean = s1 * inv_k
                var = (s2 * inv_k - mean * mean).clamp(min=0.0)
                if not one_pass:
                    dev = xs.to(F32) - mean
                    var = R.mm32(dev * dev, one, "seq" if isinstance(order, tuple) else order) * inv_k
            colsum = W.sum(1).to(dt)                                 # the f32 table is the float64 sum of the dequantised weights rounded once
            c = (c - mean.to(dt) * colsum.unsqueeze(0)) * torch.rsqrt(var.to(dt) + ln_eps)
        if scale_late:
            c = c * sc.to(dt)[None, :]
        if bias is not None:
            c = c + R._t(bias, dt)
        if add is not None and mut != "act_before_add":
            c = c + R._t(add, dt)
        v = R._act(c, act, "lib", None)
        if add is not None and mut == "act_before_add":
            v = v + R._t(add, dt)
        lo = v if rounded is None else bf16(v)
        return {"f32": v.to(F64).numpy(), "lo": lo.to(F64).numpy()}


def _diag_sq_parts(x, parts, rot):
    """sum_k x^2 in the partition's order: per 32-step the exact sum of squares enters the accumulator as one rounded term (the diagonal of A A^T)."""
    sq = (x * x).to(F64)
    tot = None
    for wg in parts:
        wsum = None
        for i in range(len(wg)):
            lo, hi = wg[(i + rot) % len(wg)]
            acc = torch.zeros(x.shape[0], 1, dtype=F32)
            for k in range(lo, hi, 32):
                acc += sq[:, k:k + 32].sum(1, keepdim=True).to(F32)
            wsum = acc if wsum is None else wsum + acc
        tot = wsum if tot is None else tot + wsum
    return tot


def decode_forms(a, w, splits=1, **spec):
    """(the float64 statement, its float32 evaluations in decode_orders(K, splits))."""
    exact = decode_gemm_ref(a, w, **spec)
    K = np.asarray(a).shape[1]
    return exact, [decode_gemm_ref(a, w, rounded="f32", order=o, **spec) for o in decode_orders(K, splits)]


def np_bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def quantise_weights(w, wkind):
    """The weight operands of one case as decode_gemm_desc takes them: wkind 0 bf16, 1 e4m3 rows, 2 MXFP4 blocks; "w" is the dequantised copy (exact in bf16)."""
    wb = np_bf16(w)
    if wkind == 0:
        return dict(w=wb)
    if wkind == 1:
        q, s, dq = fp8_rows_reference(wb)
        return dict(w=dq.astype(np.float32), wq=q, w_scale=s)
    codes, sb, dq = mxfp4_reference(wb)
    return dict(w=dq.astype(np.float32), wq=mxfp4_pack(codes), w_scale8=sb)


def fold_inputs(M, N, K, seed, offset):
    """gemm_ref.inputs with every row's mean moved to `offset` standard deviations of that row (the residual stream of a pre-LN decoder is not centred)."""
    a, w, bias, add, _, s = R.inputs(M, N, K, seed)
    a = a.astype(np.float64)
    a = a - a.mean(1, keepdims=True)
    a = a + offset * a.std(1, keepdims=True)
    return a.astype(np.float32), w, bias, add, s


def decode_inputs(M, N, K, seed, fold=False, offset=0.0, wkind=0):
    """The operands of one decode GEMM case: (a, weight operands of quantise_weights, bias, add, the scale every row is judged at). Without the fold
    gemm_ref.inputs (rows at scales 0.1 .. 10, judged at their scale); with it fold_inputs (the normalised rows are all of order 1: judged as they are)."""
    if fold:
        a, w, bias, add, s = fold_inputs(M, N, K, seed, offset)
        s = np.ones(M)
    else:
        a, w, bias, add, _, s = R.inputs(M, N, K, seed)
    return a, quantise_weights(w, wkind), bias, add, s


def judge(got, exact, rounded, key, scale):
    """gemm_ref.judge: within() at margin 3 with every row divided by its scale -> (ok, (rms ratio, max ratio))."""
    return R.judge(got, exact, rounded, key, scale)


# ---- codecs ------------------------------------------------------------------------------------------------------------------------------------------------
def _e4m3_values():
    t = np.zeros(256, np.float64)
    for v in range(256):
        s, e, m = v >> 7, (v >> 3) & 15, v & 7
        x = (m / 8.0) * 2.0 ** -6 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7)
        if e == 15 and m == 7:
            x = np.nan
        t[v] = -x if s else x
    return t


E4M3 = _e4m3_values()


def e4m3_decode(b):
    return E4M3[np.asarray(b, np.uint8)]


def e4m3_encode(x):
    """OCP e4m3fn, round to nearest, ties to the even code, saturating at +-448; NaN -> 0x7f."""
    x = np.asarray(x, np.float64)
    pos = E4M3[:0x7F]                                                # 0 .. 448, ascending
    v = np.minimum(np.abs(np.nan_to_num(x)), 448.0)
    hi = np.clip(np.searchsorted(pos, v, side="left"), 0, 0x7E)
    lo = np.maximum(hi - 1, 0)
    d_lo, d_hi = v - pos[lo], pos[hi] - v
    code = np.where((d_hi < d_lo) | ((d_hi == d_lo) & (hi % 2 == 0)), hi, lo)
    code = np.where(pos[hi] == v, hi, code)
    code = code | (np.signbit(x).astype(np.int64) << 7)
    return np.where(np.isnan(x), 0x7F, code).astype(np.uint8)


def e4m3_ulp(y):
    """Spacing of the e4m3 grid in the binade of |y| (|y| clamped to 448; 2^-9 below 2^-6)."""
    v = np.minimum(np.abs(np.asarray(y, np.float64)), 448.0)
    e = np.floor(np.log2(np.maximum(v, 2.0 ** -6)))
    return 2.0 ** (e - 3)


def e2m1_decode(code):
    code = np.asarray(code, np.uint8)
    return np.where(code & 8, -1.0, 1.0) * E2M1_LEVELS[code & 7]


def e2m1_encode(x):
    """e2m1 code (sign in bit 3) of x: nearest level, ties to the even code, |x| >= 6 saturates."""
    x = np.asarray(x, np.float64)
    v = np.abs(x)
    code = np.zeros(v.shape, np.int64)
    for lo, hi, c_lo in ((0.0, 0.5, 0), (0.5, 1.0, 1), (1.0, 1.5, 2), (1.5, 2.0, 3), (2.0, 3.0, 4), (3.0, 4.0, 5), (4.0, 6.0, 6)):
        mid = 0.5 * (lo + hi)
        up = (v > mid) | ((v == mid) & (c_lo % 2 == 1))                       # a tie goes to the even code
        code = np.where((v >= lo) & up, c_lo + 1, code)
        code = np.where((v >= lo) & (v < hi) & ~up, c_lo, code)
    code = np.where(v >= 6.0, 7, code)
    return (code | (np.signbit(x).astype(np.int64) << 3)).astype(np.uint8)


def e8m0_decode(b):
    return 2.0 ** (np.asarray(b, np.float64) - 127.0)


# ---- row / block quantisers --------------------------------------------------------------------------------------------------------------------------------
def pow2_scale(amax):
    """The smallest power of two s with amax / s <= 448 (amax / s in (224, 448]); 1 for a zero row."""
    amax = np.asarray(amax)
    s = np.ones_like(amax, dtype=np.float32)
    nz = amax > 0
    m, e = np.frexp(amax[nz].astype(np.float32) / np.float32(448.0))
    s[nz] = np.ldexp(np.float32(1.0), np.where(m == 0.5, e - 1, e)).astype(np.float32)
    return s


def fp8_rows_reference(wb):
    """Row quantiser of the FP8 mode over bf16-exact values [N][K]: (bytes, scale [N] f32, dequantised f64)."""
    wb = np.asarray(wb, np.float64)
    s = pow2_scale(np.abs(wb).max(axis=1)).astype(np.float64)
    q = e4m3_encode(wb / s[:, None])
    return q, s.astype(np.float32), e4m3_decode(q) * s[:, None]


def mxfp4_reference(wb):
    """OCP MX v1.0, e2m1 + e8m0 over blocks of 32 along the last axis: (codes [N][K] uint8 incl. the sign bit, scale bytes [N][K / 32], dequantised f64)."""
    N, K = wb.shape
    blk = wb.reshape(N, K // 32, 32).astype(np.float64)
    amax = np.abs(blk).max(axis=2)
    e = np.where(amax > 0, np.floor(np.log2(np.where(amax > 0, amax, 1.0))) - 2, 0.0)
    sb = np.clip(e + 127, 1, 254).astype(np.int64)
    scale = 2.0 ** (sb - 127.0)
    code = e2m1_encode(blk / scale[..., None])
    dq = e2m1_decode(code) * scale[..., None]
    return code.reshape(N, K).astype(np.uint8), sb.astype(np.uint8), dq.reshape(N, K)


def mxfp4_pack(codes):
    """codes [N][K] -> bytes [N][K / 2]: element 2 i in the low nibble of byte i."""
    c = np.asarray(codes, np.uint8)
    return (c[:, 0::2] | (c[:, 1::2] << 4)).astype(np.uint8)


def mxfp4_dequant(packed, scale8, mut=None):
    """bytes [N][K / 2] + e8m0 [N][K / 32] -> values [N][K]. mut: "nibble_swap" the high nibble first, "scale_neighbour" block j scaled by block j + 1's byte
    (the last by its predecessor's)."""
    p = np.asarray(packed, np.uint8)
    lo, hi = p & 15, p >> 4
    if mut == "nibble_swap":
        lo, hi = hi, lo
    codes = np.stack([lo, hi], axis=2).reshape(p.shape[0], -1)
    sc = np.asarray(scale8, np.uint8)
    if mut == "scale_neighbour":
        sc = np.concatenate([sc[:, 1:], sc[:, -2:-1]], axis=1)
    return e2m1_decode(codes) * np.repeat(e8m0_decode(sc), 32, axis=1)


# ---- the FP8 cross-K/V cache -------------------------------------------------------------------------------------------------------------------------------
def crosskv_slabs(seed=0):
    """3 slabs of 240 rows; sequences of 0, 1, 17 and 144 rows on 16-row boundaries with gaps between them (rows 17 .. 47, 65 .. 79 and the tail behind 224),
    every sequence at a level of its own so that its scale is its own."""
    rng = np.random.default_rng(seed)
    row_off, n_lfr = [0, 16, 48, 80], [0, 1, 17, 144]
    x = np_bf16(rng.standard_normal((3, 240, 64)) * np.exp(rng.uniform(-3, 3, (3, 240, 1))))
    for b, (r0, n) in enumerate(zip(row_off, n_lfr)):
        x[:, r0:r0 + n] *= np.float32(4.0 ** b)
    return x, row_off, n_lfr


def crosskv_ref(slabs, row_off, n_lfr, dq_in_place=False, mut=None):
    """launch_quantize_crosskv_fp8: slabs [S][rows][64] (bf16-exact), sequence b at rows [row_off[b], row_off[b] + n_lfr[b]) -> (bytes [S][rows][64] with SENTINEL
    where no sequence lies, scale [S][B] f32 -- one per (slab, sequence) over the sequence's rows x 64 --, the slabs afterwards: their dequantisation with
    dq_in_place, unchanged otherwise). mut "scale_over_slab": one scale per slab, over all its sequences."""
    x = np.asarray(slabs, np.float64)
    S = x.shape[0]
    q = np.full(x.shape, SENTINEL, np.uint8)
    sc = np.ones((S, len(row_off)), np.float32)
    after = x.copy()
    for s in range(S):
        for b, (r0, n) in enumerate(zip(row_off, n_lfr)):
            reg = x[s, r0:r0 + n]
            amax = np.abs(reg).max() if n else 0.0
            if mut == "scale_over_slab":
                amax = max([np.abs(x[s, r:r + m]).max() for r, m in zip(row_off, n_lfr) if m] + [0.0])
            sc[s, b] = pow2_scale(np.array([amax]))[0]
            q[s, r0:r0 + n] = e4m3_encode(reg / np.float64(sc[s, b]))
            if dq_in_place:
                after[s, r0:r0 + n] = e4m3_decode(q[s, r0:r0 + n]) * np.float64(sc[s, b])
    return q, sc, after


# ---- LayerNorm -> e4m3 operand rows ------------------------------------------------------------------------------------------------------------------------
LN_ORDERS = ("lib", "seq", "lane")


# rows x inv_scale per D as the issue lists them. A normalised value cannot exceed sqrt(D - 1), so inv_scale = 2^4 can only saturate (|y| > 448) at D = 2048; the
# two 2^6 cases make the rows of D = 256 and 512 saturate as well.
LN_CASES = [(D, rows, inv) for D in (256, 512, 2048) for rows, inv in ((1, 1.0), (5, 2.0 ** -3), (9, 2.0 ** 4))] + [(256, 5, 2.0 ** 6), (512, 5, 2.0 ** 6)]


def ln_saturates(D, inv):
    return inv >= 64.0 or (inv >= 16.0 and D == 2048)


def ln_input(rows, D, ld_x, seed):
    """Rows with a mean of 0.5 .. 2 standard deviations at levels 0.1 .. 10, one element of row 0 at 60 standard deviations (normalised: about 15 at D = 256,
    21 at 512, 36 at 2048); the columns past D hold what must not be read (1e30)."""
    rng = np.random.default_rng([rows, D, seed])
    lvl = 10.0 ** rng.uniform(-1, 1, (rows, 1))
    x = np.full((rows, ld_x), 1e30, np.float32)
    v = rng.standard_normal((rows, D))
    v[0, 7] = 60.0
    x[:, :D] = ((v + rng.uniform(0.5, 2.0, (rows, 1))) * lvl).astype(np.float32)
    return x


def _sum32(v, order):
    """Row sums of a float32 array [rows][D] (D % 256 == 0): numpy's pairwise sum, one running sum, or the kernel's shape (per lane 4 + 4 + .. then a butterfly)."""
    if order == "lib":
        return v.sum(axis=1, dtype=np.float32)
    if order == "seq":
        return np.cumsum(v, axis=1, dtype=np.float32)[:, -1]
    q = v.reshape(v.shape[0], -1, 64, 4)
    lane = np.zeros((v.shape[0], 64), np.float32)
    for k in range(q.shape[1]):
        lane = lane + ((q[:, k, :, 0] + q[:, k, :, 1]) + (q[:, k, :, 2] + q[:, k, :, 3]))
    while lane.shape[1] > 1:
        lane = lane[:, 0::2] + lane[:, 1::2]
    return lane[:, 0]


def layernorm_fp8_ref(x, D, eps, inv_scale, rounded=None, order="lib", mut=None):
    """y = (x - mean) rstd inv_scale over the first D columns, BEFORE the clamp to +-448 and the e4m3 rounding: float64 [rows][D] (rounded="f32": float32 with
    two-pass statistics summed in `order`). mut "no_mean": the mean left at 0 in both places."""
    if rounded is None:
        v = np.asarray(x, np.float64)[:, :D]
        mean = v.mean(axis=1, keepdims=True) if mut != "no_mean" else 0.0
        var = ((v - mean) ** 2).mean(axis=1, keepdims=True)
        return (v - mean) / np.sqrt(var + eps) * inv_scale
    v = np.ascontiguousarray(np.asarray(x, np.float32)[:, :D])
    mean = (_sum32(v, order) / np.float32(D))[:, None] if mut != "no_mean" else np.float32(0.0)
    c = v - mean
    rstd = (np.float32(1.0) / np.sqrt(_sum32(c * c, order) / np.float32(D) + np.float32(eps))).astype(np.float32) * np.float32(inv_scale)
    return (c * rstd[:, None]).astype(np.float64)


def fp8_store_bound(y_exact, y_rounded_forms):
    """Per-element bound on |decode(byte) - clamp(y)|: half an e4m3 ulp at y + 3 x E_round, E_round = the worst |exact - rounded| of the element's ROW over the
    float32 forms (a row shares its mean and rstd, so its elements share their error). The ulp is taken at |y| + 3 E_round: a value that close under a binade
    edge may be rounded in the coarser binade above."""
    e = np.zeros(y_exact.shape[0])
    for r in y_rounded_forms:
        e = np.maximum(e, np.abs(y_exact - r).max(axis=1))
    e = MARGIN * e[:, None]
    return 0.5 * e4m3_ulp(np.abs(y_exact) + e) + e


def clamp448(y):
    return np.clip(y, -448.0, 448.0)


# ---- the FP8 matrix-pipe GEMM ------------------------------------------------------------------------------------------------------------------------------
FP8_ORDERS = ("seq", "lib", (128, 1), (128, 2))


def gemm_fp8_ref(a8, w8, w_scale, a_scale, bias, add=None, act=0, out_inv_scale=1.0, rounded=None, order="seq", gelu="lib"):
    """Fp8GemmArgs over the decoded bytes: v = (A W^T) a_scale w_scale[n] + bias; with `add` -> {"f32": v + add}; else t = act(v) out_inv_scale ->
    {"y": t before the clamp, "sat": the number of elements with |t| > 448 or NaN}. rounded="f32": float32, the product summed in `order`; gelu="fast": the
    erf-GELU by the formula of gemm_dev.h (gemm_ref.fast_gelu32), one more float32 form of that activation."""
    dt = F64 if rounded is None else F32
    with torch.inference_mode():
        A, W = torch.from_numpy(e4m3_decode(a8)), torch.from_numpy(e4m3_decode(w8))
        c = A @ W.t() if rounded is None else R.mm32(A.to(F32), W.to(F32), order)
        if c is None:
            return None
        v = c * (R._t(w_scale, dt) * torch.tensor(a_scale, dtype=dt))[None, :] + R._t(bias, dt)
        if add is not None:
            return {"f32": (v + R._t(add, dt)).to(F64).numpy()}
        t = (R._act(v, act, gelu, None) * torch.tensor(out_inv_scale, dtype=dt)).to(F64).numpy()
        return {"y": t, "sat": int(((np.abs(t) > 448.0) | np.isnan(t)).sum())}
