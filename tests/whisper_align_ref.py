"""Float64 statement of Whisper's token timestamps (OpenAI Whisper, timing.py: find_alignment / median_filter / dtw_cpu / backtrace) as the engine runs
them (csrc/whisper_align.hip), and the error budgets of its kernels, derived from the operands.

    scores  [P][N][M]   raw cross-attention scores q . k of P (layer, head) pairs, N token rows, M frames (cropped to the frames that hold audio)
    1. soft-max over frames            2. standardise over the token axis (population variance; a column whose rows are all equal -> 0, where OpenAI
    divides by zero; and the rows are the aligned rows only, where OpenAI's statistics also see the prompt rows and the eot input row: the two deviations)          3. median of `width` reflect-padded neighbours along frames (none when M <= width // 2)
    4. mean over pairs, negated -> cost [N][M]           5. DTW, OpenAI's recurrence and tie rule, -> per row the first frame on the path.
"""
import numpy as np

U = 2.0 ** -24                  # unit roundoff of f32
PRECISION = 0.02                # seconds per encoder frame


# ------------------------------------------------------------------------------------------------- steps 1-4
def softmax(scores):
    x = np.asarray(scores, np.float64)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def standardise(w):
    """[P][N][M] -> (z, mean [P][M], std [P][M], flat [P][M]): over the token axis, std_mean(dim=-2, unbiased=False); flat columns (all rows equal) give 0."""
    w = np.asarray(w, np.float64)
    flat = w.max(axis=1) == w.min(axis=1)
    mean = w.mean(axis=1)
    std = np.sqrt(((w - mean[:, None, :]) ** 2).mean(axis=1))
    safe = np.where(flat | (std == 0), 1.0, std)
    z = np.where((flat | (std == 0))[:, None, :], 0.0, (w - mean[:, None, :]) / safe[:, None, :])
    return z, mean, std, flat | (std == 0)


def reflect_index(M, width):
    """[M][width] source columns of the reflect-padded windows."""
    pad = width // 2
    c = np.arange(M)[:, None] + np.arange(width)[None, :] - pad
    c = np.where(c < 0, -c, c)
    return np.where(c >= M, 2 * (M - 1) - c, c)


def median_filter(x, width):
    """Along the last axis; OpenAI / HF: the input comes back unchanged when it is no longer than the pad."""
    x = np.asarray(x)
    M, pad = x.shape[-1], width // 2
    if M <= pad:
        return x
    return np.sort(x[..., reflect_index(M, width)], axis=-1)[..., pad]


def cost_matrix(scores, width, from_weights=False):
    """scores [P][N][M] (already cropped) -> cost [N][M] float64. from_weights: `scores` are soft-max weights already."""
    w = np.asarray(scores, np.float64) if from_weights else softmax(scores)
    z = standardise(w)[0]
    return -median_filter(z, width).mean(axis=0)


# ------------------------------------------------------------------------------------------------- step 5
def dtw(cost, dtype=np.float64):
    """OpenAI's dtw_cpu + backtrace -> (rows, frames) of the path from (0, 0) to (N - 1, M - 1). Ties: diagonal if c0 < c1 and c0 < c2, else vertical if
    c1 < c0 and c1 < c2, else horizontal. float64 runs on Python floats (the same arithmetic, fast enough for 448 x 1500); dtype float32 rounds every sum."""
    x = np.asarray(cost, dtype)
    N, M = x.shape
    inf = float("inf")
    rnd = (lambda v: v) if np.dtype(dtype) == np.float64 else (lambda v: float(np.float32(v)))
    xs = x.astype(np.float64).tolist()
    D = [[inf] * (M + 1) for _ in range(N + 1)]
    T = [[-1] * (M + 1) for _ in range(N + 1)]
    D[0][0] = 0.0
    for j in range(1, M + 1):
        for i in range(1, N + 1):
            c0, c1, c2 = D[i - 1][j - 1], D[i - 1][j], D[i][j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            D[i][j] = rnd(xs[i - 1][j - 1] + c)
            T[i][j] = t
    T[0] = [2] * (M + 1)
    for row in T:
        row[0] = 1
    i, j, rows, frames = N, M, [], []
    while i > 0 or j > 0:
        rows.append(i - 1); frames.append(j - 1)
        if T[i][j] == 0:
            i -= 1; j -= 1
        elif T[i][j] == 1:
            i -= 1
        else:
            j -= 1
    return np.asarray(rows[::-1]), np.asarray(frames[::-1])


def jump_frames(rows, frames):
    """OpenAI's jump_times before the division by 50: the frame at which the path enters each row."""
    rows, frames = np.asarray(rows), np.asarray(frames)
    jumps = np.pad(np.diff(rows), (1, 0), constant_values=1).astype(bool)
    return frames[jumps]


def path_cost(cost, rows, frames):
    return float(np.asarray(cost, np.float64)[np.asarray(rows), np.asarray(frames)].sum())


def is_monotone_path(rows, frames, N, M):
    rows, frames = np.asarray(rows), np.asarray(frames)
    if len(rows) == 0 or (rows[0], frames[0]) != (0, 0) or (rows[-1], frames[-1]) != (N - 1, M - 1):
        return False
    dr, df = np.diff(rows), np.diff(frames)
    return bool(((dr >= 0) & (df >= 0) & (dr <= 1) & (df <= 1) & (dr + df >= 1)).all())


def brute_force_optimum(cost):
    """The least cost over ALL monotone paths (steps right, down, diagonal), by enumeration."""
    x = np.asarray(cost, np.float64)
    N, M = x.shape

    def go(i, j):
        if i == N - 1 and j == M - 1:
            return x[i, j]
        best = np.inf
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < N and j + dj < M:
                best = min(best, go(i + di, j + dj))
        return x[i, j] + best
    return float(go(0, 0))


def token_times(frames, window_offset_s=0.0, window_end_s=None):
    """whisper.token_times restated: row r starts at its frame and ends where row r + 1 starts; the last row is eot's and only closes the last token,
    unless the ids were cut off (window_end_s given): then every row is a token and the last one ends with the window."""
    f = [window_offset_s + int(v) * PRECISION for v in frames]
    if window_end_s is not None:
        f.append(max(window_end_s, f[-1]) if f else window_end_s)
    return list(zip(f[:-1], f[1:]))


# ------------------------------------------------------------------------------------------------- budgets
def scores_budget(q, k):
    """|f32 q . k - exact| for the values the kernel saw (q [64], k [M][64]): the f32 dot-product part of decode_attn_ref.budget, 32 * 2^-24 * sum |q_i k_i|."""
    return 32 * U * (np.abs(np.asarray(q, np.float64))[None, :] * np.abs(np.asarray(k, np.float64))).sum(axis=1)


def softmax_budget(scores):
    """Relative error of an f32 soft-max weight [P][N][1]: the exponent's argument carries one rounding of |x - max| <= R, expf two units, the normaliser
    M / 256 strided additions per thread + 10 reduction levels, one reciprocal and one product."""
    x = np.asarray(scores, np.float64)
    R = (x.max(axis=-1, keepdims=True) - x.min(axis=-1, keepdims=True))
    return U * (2 * R + 8 + x.shape[-1] / 256 + 14)


def cost_budget(scores, width, from_weights=False):
    """Bound [N][M] on |f32 cost - float64 cost| for a kernel chain fed the same f32 scores (from_weights: fed the same f32 soft-max weights, so the soft-max
    adds nothing). Per pair and column, with w the weights, N rows, std the column's deviation and zmax = max |w - mean| / std:
      the weight and the mean are off by at most e = (2 rel + N u) max|w|  (rel: soft-max, N u: the N f32 additions of the mean),
      the deviation, relatively, by e (1 + u) / std + (N / 2 + 5) u         (N fused additions of the squares, division, square root, reciprocal),
      so a standardised value moves by at most (e / std) (1 + zmax) + zmax (N / 2 + 5) u.
    The median is a selection (1-Lipschitz in the largest error of its window: it adds nothing); the mean over P pairs adds P + 1 roundings of the mean
    magnitude. Flat columns are exact zeros on both sides."""
    w = np.asarray(scores, np.float64) if from_weights else softmax(scores)
    P, N, M = w.shape
    rel = 0.0 if from_weights else softmax_budget(scores).max(axis=1)          # [P][1]
    z, mean, std, flat = standardise(w)
    safe = np.where(flat, 1.0, std)
    e = (2 * rel + N * U) * np.abs(w).max(axis=1)                                # [P][M]
    zmax = np.abs(z).max(axis=1)
    bz = np.where(flat, 0.0, (e / safe) * (1 + zmax) + zmax * (N / 2 + 5) * U)   # [P][M]
    if M > width // 2:
        bz = bz[:, reflect_index(M, width)].max(axis=-1)
    med = np.abs(median_filter(z, width))                                        # [P][N][M]
    return bz.mean(axis=0)[None, :] + (P + 1) * U * med.mean(axis=0)


def path_slack(cost, budget):
    """How much more than the float64 optimum the GPU's path may cost on the float64 matrix: it is optimal, up to its f32 accumulation, on a matrix within
    `budget` of this one. (N + M) cells at most, each off by the budget on either path; each of the (N + M) f32 additions of a running cost of at most
    (N + M) max|cost| rounds once, again on either path."""
    c = np.asarray(cost, np.float64)
    N, M = c.shape
    acc = 2 * U * (N + M) * np.abs(c).max()
    return (N + M) * (2 * float(np.max(budget)) + acc)


# ------------------------------------------------------------------------------------------------- the decoder's cross-attention, teacher-forced
def cross_attention_probs(oracle, ids, cross_k, cross_v):
    """The cross-attention probabilities of every (layer, head) of oracle/whisper_oracle.WhisperOracle's decoder (its layer loop, Export_Whisper.py:614-667,
    restated in the oracle's dtype -- build it with dtype=torch.float64) for ONE utterance, teacher-forced on `ids` (prompt + generated ids, all positions
    in one causal pass: the additive -128 mask of the reference's prefill). cross_k / cross_v: (Ld, H, T, hd) from oracle.encode. -> [Ld][H][len(ids)][T]."""
    import torch
    F = torch.nn.functional
    c, ck, o = oracle.cfg, oracle.ck, oracle
    ids = torch.as_tensor(np.asarray(ids), dtype=torch.long)
    n, d, H, hd = ids.shape[0], c.d_model, c.n_heads, c.d_head
    h = o._c(ck["model.decoder.embed_tokens.weight"])[ids] + o._c(ck["model.decoder.embed_positions.weight"][:n])
    mask = torch.triu(torch.full((n, n), -128.0, dtype=o.dtype), diagonal=1)
    gelu = (lambda x: F.gelu(x, approximate="tanh")) if o.gelu == "tanh" else F.gelu
    probs = []
    for li, L in enumerate(o.dec):
        qkv = F.layer_norm(h, (d,)) @ o._c(L["wqkv"]).t() + o._c(L["bqkv"])
        q, k, v = [z.reshape(n, H, hd).transpose(0, 1) for z in qkv.split(d, dim=-1)]
        a = (torch.softmax(q @ k.transpose(1, 2) + mask, dim=-1) @ v).transpose(0, 1).reshape(n, d)
        h = a @ o._c(L["wo"]).t() + o._c(L["bo"]) + h
        cq = (F.layer_norm(h, (d,)) @ o._c(L["wcq"]).t() + o._c(L["bcq"])).reshape(n, H, hd).transpose(0, 1)
        p = torch.softmax(cq @ o._c(cross_k[li]).transpose(1, 2), dim=-1)              # (H, n, T)
        probs.append(p)
        a = (p @ o._c(cross_v[li])).transpose(0, 1).reshape(n, d)
        h = a @ o._c(L["wco"]).t() + o._c(L["bco"]) + h
        h = h + gelu(F.layer_norm(h, (d,)) @ o._c(L["w1"]).t() + o._c(L["b1"])) @ o._c(L["w2"]).t() + o._c(L["b2"])
    return torch.stack(probs).numpy()
