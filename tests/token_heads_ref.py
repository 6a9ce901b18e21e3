"""Numpy statement of the six token-selection heads of csrc/kernels.hip (launch_argmax_rows, launch_beam_topk, launch_apply_penalty,
launch_append_ids, launch_sample_topk_topp, launch_no_speech_prob), their decision margins and their error budgets.

Elementwise steps the reference graphs perform in f32 (adding `extra` / `bias`, the penalty multiplications, the 1 / temperature scaling)
are done in np.float32 and are therefore bit-defined; everything with a transcendental or a sum (log-soft-max, the sampler's soft-max and
cumulative sum, the Gumbel scores, the no-speech probability) is float64. Selections are ordered value descending, then index ascending,
by a stable sort. The sampler's counter-based generator (splitmix64, top 24 bits) is restated with Python integers.

The seeded inputs the GPU tests use are built here too, so tests/test_token_heads_ref_cpu.py can check their margins without a GPU."""
import math

import numpy as np

U32 = 2.0 ** -24                       # half an f32 ulp, relative
GRID = 2.0 ** -10
BEAM_MAX = 8
F32 = np.float32
MASK64 = (1 << 64) - 1

WIDTHS = [1, 3, 4, 5, 127, 128, 129, 4095, 4096, 4097, 4100, 8191, 8192, 8193, 12289, 51866, 151936]
WIDE = 12289                           # widths above this appear in one parametrisation per head
LOOP_WIDTHS = [5, 129, 4097, 51866]    # the heads that loop per column (sampler, no-speech)
SKIP_CAP = 0.02                        # largest share of a case's rows a margin may leave undecided


def grid_logits(seed, rows, n):
    """N(0, 3^2) rounded to multiples of 2^-10: distinct values stay distinct under a monotone f32 scaling, planted ties are exact."""
    rng = np.random.default_rng(seed)
    return (np.round(rng.normal(0.0, 3.0, (rows, n)) / GRID) * GRID).astype(F32)


def order(v):
    """Indices of v by value descending, then index ascending."""
    return np.argsort(-np.asarray(v), kind="stable")


def _gap(a, b):
    return 0.0 if a == b else float(a) - float(b)          # (-inf, -inf) is a tie, not NaN


# ------------------------------------------------------------------------------------------------ arg-max
def argmax_rows(logits, extra=None):
    """ids [rows] of the first maximum of logits + extra (f32 sum), and the gap to the runner-up (inf for a single column)."""
    v = np.asarray(logits, F32) if extra is None else (np.asarray(logits, F32) + np.asarray(extra, F32)[None, :]).astype(F32)
    ids, margin = np.zeros(len(v), np.int32), np.full(len(v), np.inf)
    for r, row in enumerate(v):
        o = order(row)
        ids[r] = o[0]
        if len(o) > 1:
            margin[r] = _gap(row[o[0]], row[o[1]])
    return ids, margin


# ------------------------------------------------------------------------------------------------ beam top-k
def beam_topk(logits, K, bias=None):
    """(topv [rows][K] float64 log-probabilities, topi [rows][K], lse [rows], margin [rows]) of logits + bias (f32 sum). A -inf column has zero
    weight and is no candidate; ranks past the last candidate come back as (-inf, 0). margin: the smallest gap between consecutive ranks
    1 .. K + 1 (0 on a tie, which the index decides)."""
    x = np.asarray(logits, F32) if bias is None else (np.asarray(logits, F32) + np.asarray(bias, F32)[None, :]).astype(F32)
    rows = len(x)
    topv, topi = np.full((rows, K), -np.inf), np.zeros((rows, K), np.int32)
    lse, margin = np.zeros(rows), np.full(rows, np.inf)
    for r in range(rows):
        x64 = x[r].astype(np.float64)
        M = x64.max()
        with np.errstate(invalid="ignore", divide="ignore"):
            lse[r] = M + math.log(np.exp(x64 - M).sum()) if M > -np.inf else np.nan
        o = order(x[r])[:K + 1]
        for k, i in enumerate(o[:K]):
            if x64[i] > -np.inf:
                topv[r, k], topi[r, k] = x64[i] - lse[r], i
        for a, b in zip(o[:-1], o[1:]):
            margin[r] = min(margin[r], _gap(x[r, a], x[r, b]))
    return topv, topi, lse, margin


def beam_topv_budget(n_valid, row_max, lse, topv):
    """Bound on |topv_gpu - topv| for beam_topk_kernel: topv = x - (M + logf(S)), S = sum exp(x - M) in f32.
    1. relative error of S, which is the absolute error of log S: the hardware __expf (2e-5, as decode_attn_ref.budget counts it) plus the depth of the
       f32 addition chain -- ceil(n_valid / 4096) * 4 terms per thread, 6 lane merges, 16 wave merges -- at 2^-24 each;
    2. logf: one ulp of log S = lse - M;
    3. two roundings, M + logf(S) at |lse| and x - lse at |topv|, 2^-24 relative each."""
    depth = -(-n_valid // 4096) * 4 + 6 + 16
    return (2e-5 + depth * U32) + 2 * U32 * np.abs(lse - row_max) + U32 * np.abs(lse) + U32 * np.abs(topv)


# ------------------------------------------------------------------------------------------------ penalty window, history
def apply_penalty(logits, save_ids, n_saved, range_, value, partial):
    """APPLY_PENALTY: the logits of the last `range_` saved ids times `value` (f32), every id scaled once however often it repeats (all
    originals are gathered before the first write). Whisper (partial = 0): nothing until `range_` ids are saved. Qwen3 (partial = 1): the
    window is save_ids[:, -range_:] of whatever exists."""
    logits = np.asarray(logits, F32)
    out = logits.copy()
    n = int(n_saved)
    if n < range_:
        if not partial or n == 0:
            return out
        range_ = n
    for r in range(len(out)):
        ids = np.asarray(save_ids[r][n - range_:n])
        out[r, ids] = logits[r, ids] * F32(value)
    return out


def append_ids(save_ids, next_ids, n_saved):
    """save_ids[r][n_saved] = next_ids[r]; a full table is left alone."""
    out = np.array(save_ids, np.int32, copy=True)
    if n_saved < out.shape[1]:
        out[:, n_saved] = next_ids
    return out


# ------------------------------------------------------------------------------------------------ sampler
def uniform_from_counter(seed, step, row, j):
    """splitmix64 of the counter (step, row, j) keyed by seed; the top 24 bits as a uniform in [0, 1). step is the device counter as uint32."""
    ctr = ((step & 0xFFFFFFFF) * 0x100000001B3 + (row << 8) + j + 1) & MASK64
    z = (seed + 0x9E3779B97F4A7C15 * ctr) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return F32((z >> 40) / 16777216.0)                       # 24 bits: exact in f32


def penalise_history(row, ids, rp):
    """Repetition penalty on the saved ids (f32): negative logits times rp, the others times float32(1 / rp); every id once."""
    out = np.asarray(row, F32).copy()
    if len(ids):
        ids = np.asarray(ids)
        pv = out[ids].copy()
        out[ids] = np.where(pv < 0, pv * F32(rp), pv * (F32(1.0) / F32(rp))).astype(F32)
    return out


def sample_topk_topp(logits, save_ids, n_saved, temperature, top_k, top_p, rp, extra=None, noise=None, seed=0):
    """TOPK_TOPP_SAMPLING. Returns (next [rows], margin [rows][3], logits after the call).
    The history is the first min(n_saved, ld_save) saved ids; the generator step (noise is None) is n_saved itself, unclamped.
    margin columns: the Gumbel-score gap between the winner and the best other kept rank; the smallest distance of an exclusive cumulative
    sum (ranks 2 .. k; rank 1's is exactly 0) from top_p; the gap between rank top_k and rank top_k + 1 (0 on a tie, which the index decides)."""
    logits = np.asarray(logits, F32)
    rows, n = logits.shape
    n_prev = min(int(n_saved), np.asarray(save_ids).shape[1])
    after = logits.copy()
    inv_t = F32(1.0) / F32(temperature)
    nxt, margin = np.zeros(rows, np.int32), np.full((rows, 3), np.inf)
    lo, hi = F32(1.0e-7), F32(1.0) - F32(1.0e-7)
    for r in range(rows):
        after[r] = penalise_history(logits[r], save_ids[r][:n_prev], rp)
        v = ((after[r] if extra is None else (after[r] + np.asarray(extra, F32)).astype(F32)) * inv_t).astype(F32)
        o = order(v)[:top_k + 1]
        vals = v[o[:top_k]].astype(np.float64)
        p = np.exp(vals - vals[0])
        p /= p.sum()
        excl = np.concatenate([[0.0], np.cumsum(p)[:-1]])
        keep = excl <= float(F32(top_p))
        u = np.asarray(noise[r], F32) if noise is not None else np.array([uniform_from_counter(seed, int(n_saved), r, k) for k in range(top_k)], F32)
        u = np.clip(u, lo, hi).astype(np.float64)
        sc = np.where(keep, vals - np.log(-np.log(u)), -np.inf)
        win = int(np.argmax(sc))                             # first maximum
        nxt[r] = o[win]
        others = np.delete(sc, win)
        if len(others) and others.max() > -np.inf:
            margin[r, 0] = sc[win] - others.max()
        if top_k > 1:
            margin[r, 1] = np.abs(excl[1:] - float(F32(top_p))).min()
        if len(o) > top_k:
            margin[r, 2] = _gap(v[o[top_k - 1]], v[o[top_k]])
    return nxt, margin, after


def sampler_budget(top_k, vmax=64.0):
    """(Gumbel-gap budget, top-p distance budget) of sample_topk_topp_kernel's step 3, which runs in f32 on bit-defined scores |v| <= vmax.
    Gumbel score v - logf(-logf(u)): logf(u) is good to an ulp (2^-23 relative), which is an absolute 2^-23 on the outer logarithm; the outer logf adds an
    ulp of its result, at most |log(-log(1e-7))| < 16.2 in magnitude; the subtraction rounds at |score| <= vmax + 16.2. Two scores are compared: twice that.
    Exclusive cumulative sum <= 1: each p = expf(v_k - v_1) / sum carries the rounding of its argument (weighted by p |v_k - v_1| <= 1 / e), two ulps of expf,
    the relative error of the sum (k additions) and the division -- (5 + k) 2^-24 in all -- and the running sum adds k roundings more.
    The rank gap needs no budget: the scores are bit-defined, so a tie is decided by the index."""
    gumbel = 2.0 * (2 * U32 + 2 * U32 * 16.2 + U32 * (vmax + 16.2))
    topp = (5 + 2 * top_k) * U32
    return gumbel, topp


def sampler_decided(margin, top_k, vmax=64.0):
    g, p = sampler_budget(top_k, vmax)
    return (margin[:, 0] > g) & (margin[:, 1] > p)


# ------------------------------------------------------------------------------------------------ the head over several steps
def head_steps(logits, steps, ld_save, range_, value, partial, bias=None, track_history=False, sampler=None, noise=None, change=None):
    """The sessions' head sequence (csrc/decode_head.h: TokenHead) on the same logits rows at every step, from an empty history: apply_penalty (decode
    steps only, not under the sampler), then the sampler or the arg-max, then append_ids and counter + 1 when the head is penalised, samples or
    tracks its history. Step 0 is the prefill: `bias` is added, nothing is penalised. sampler: (temperature, top_k, top_p, repetition_penalty, seed);
    noise: caller uniforms for step 0 only; change: (step, value, range) takes effect before that step.
    Returns (picks [steps][rows], save_ids [rows][ld_save], n_saved, decided [steps][rows]: the sampler's margins decide that pick -- all True for arg-max)."""
    logits = np.asarray(logits, F32)
    rows = len(logits)
    save, n = np.zeros((rows, ld_save), np.int32), 0
    picks, decided = np.zeros((steps, rows), np.int32), np.ones((steps, rows), bool)
    for t in range(steps):
        if change is not None and t == change[0]:
            value, range_ = change[1], change[2]
        penalised = value != 1.0 and sampler is None
        x = apply_penalty(logits, save, n, range_, value, partial) if penalised and t > 0 else logits
        if sampler is not None:
            temperature, top_k, top_p, rp, seed = sampler
            picks[t], margin, _ = sample_topk_topp(x, save, n, temperature, top_k, top_p, rp, extra=bias if t == 0 else None,
                                                   noise=noise if t == 0 else None, seed=seed)
            decided[t] = sampler_decided(margin, top_k)
        else:
            picks[t], _ = argmax_rows(x, bias if t == 0 else None)
        if penalised or sampler is not None or track_history:
            save = append_ids(save, picks[t], n)
            n += 1
    return picks, save, n, decided


# ------------------------------------------------------------------------------------------------ no-speech
def no_speech_prob(logits, penalty, no_speech_id):
    """NO_SPEECH_DETECTION: soft-max(logits - penalty)[no_speech_id]; the subtraction in f32, the soft-max in float64.
    Returns (prob [rows], d [rows] = the exponent y[id] - max y of the numerator)."""
    y = (np.asarray(logits, F32) - np.asarray(penalty, F32)[None, :]).astype(F32).astype(np.float64)
    mx = y.max(axis=1, keepdims=True)
    e = np.exp(y - mx)
    return e[:, no_speech_id] / e.sum(axis=1), y[:, no_speech_id] - mx[:, 0]


def no_speech_budget(n_valid, prob, d):
    """Bound on |prob_gpu - prob|, relative to prob, for no_speech_prob_kernel: expf(y_id - mx) / sum expf(y - mx) in f32. Built as beam_topv_budget:
    expf counted as decode_attn_ref.budget counts the library exponential (1e-5); the depth of the f32 addition chain -- ceil(n_valid / 1024) terms per
    thread, 6 lane merges, 16 wave merges -- at 2^-24 each; the rounding of the numerator's argument, 2^-24 |d|, which is relative in the result; the
    division and the final store, 2^-24 each."""
    depth = -(-n_valid // 1024) + 6 + 16
    return prob * (1e-5 + depth * U32 + U32 * np.abs(d) + 2 * U32)


# ------------------------------------------------------------------------------------------------ seeded inputs of the GPU tests
NO_SPEECH_ROWS = 3


def no_speech_inputs(n_valid, no_speech_id, target):
    """(logits carrying the suppress penalty, penalty [n_valid] with -128 on a suppressed set that includes no_speech_id, the set): grid logits whose
    no-speech column is placed so that the probability is ~ target (1.0: 16 above the log-sum-exp of the others)."""
    y = grid_logits([n_valid, no_speech_id, 3], NO_SPEECH_ROWS, n_valid).astype(np.float64)
    rng = np.random.default_rng([n_valid, 11])
    sup = np.union1d(rng.choice(n_valid, size=max(1, n_valid // 20), replace=False), [no_speech_id])
    others = np.delete(y, no_speech_id, axis=1)
    m = others.max(axis=1)
    lse = m + np.log(np.exp(others - m[:, None]).sum(axis=1))
    y[:, no_speech_id] = np.round((lse + (16.0 if target >= 1.0 else math.log(target / (1.0 - target)))) / GRID) * GRID
    pen = np.zeros(n_valid, F32)
    pen[sup] = -128.0
    x = (y.astype(F32) + pen[None, :]).astype(F32)             # exact: |y| < 64 on the 2^-10 grid, minus 128, fits 24 bits
    assert np.array_equal((x - pen[None, :]).astype(F32), y.astype(F32))
    return x, pen, sup


def history(seed, rows, n_valid, n_ids, ld_save):
    """A save_ids table [rows][ld_save] whose first n_ids entries are drawn from a handful of ids, so they repeat; the rest is a filler id."""
    rng = np.random.default_rng([seed, n_ids, n_valid])
    pool = rng.choice(n_valid, size=min(n_valid, 7), replace=False)
    tab = np.zeros((rows, ld_save), np.int32)
    tab[:, :n_ids] = pool[rng.integers(0, len(pool), (rows, n_ids))]
    return tab


SAMPLER_ROWS = 4
SAMPLER_LD_SAVE = 1024
HISTORIES = [0, 1, 255, 256, 257, 1024]      # the four-per-thread gather boundaries of the 256-thread workgroup


def sampler_noise_cases():
    """(n_valid, history, top_k, temperature, top_p, repetition_penalty): every value of every parameter, every history at every width. top_p = 1 is paired
    with top_k <= 10 -- with 64 ranks the last probabilities are below f32 resolution of the cumulative sum, and no margin could decide them."""
    ks, ts, ps, rps = [1, 2, 10, 64], [0.5, 0.7, 1.3], [0.3, 0.95, 1.0], [1.0, 1.3]
    cases = []
    for i, n in enumerate(LOOP_WIDTHS):
        for j, h in enumerate(HISTORIES):
            q = i + j
            k = ks[q % 4]
            if k > n:
                k = ks[q % 2]
            p = ps[(q + i) % 3]
            if k == 64 and p == 1.0:
                p = 0.95
            cases.append((n, h, k, ts[(q // 2 + j) % 3], p, rps[(q + 1) % 2]))
    return cases


def sampler_noise_inputs(case):
    n, h, k = case[:3]
    rng = np.random.default_rng([n, h, k, 17])
    logits = grid_logits([n, h, k, 1], SAMPLER_ROWS, n)
    save = history(3, SAMPLER_ROWS, n, h, SAMPLER_LD_SAVE)
    noise = rng.uniform(0.0, 1.0, (SAMPLER_ROWS, k)).astype(F32)
    return logits, save, noise


SEEDED_LD_SAVE = 16
SEEDED = dict(n_valid=4097, rows=5, top_k=10, temperature=0.7, top_p=0.95, rp=1.3)


def sampler_seeded_cases():
    """(seed, n_saved): two seeds; an empty history, a partial one, and a counter past the table (history clamped, generator step not)."""
    return [(s, n) for s in (1234567, 0xDEADBEEFCAFEF00D) for n in (0, 7, SEEDED_LD_SAVE + 3)]


def sampler_seeded_inputs(case):
    seed, n_saved = case
    c = SEEDED
    logits = grid_logits([c["n_valid"], n_saved, 5], c["rows"], c["n_valid"])
    save = history(9, c["rows"], c["n_valid"], min(n_saved, SEEDED_LD_SAVE), SEEDED_LD_SAVE)
    return logits, save


EXTRA = dict(n_valid=4097, rows=4, n_saved=300, temperature=0.7, top_p=0.95, rp=1.3)


def sampler_extra_inputs(top_k):
    """(logits, history, extra, noise): BEGIN_SUPPRESS as `extra` takes every row's best column out; top_k = 1 runs on constant noise."""
    c = EXTRA
    x = grid_logits([c["n_valid"], 12], c["rows"], c["n_valid"])
    save = history(5, c["rows"], c["n_valid"], c["n_saved"], SAMPLER_LD_SAVE)
    extra = np.zeros(c["n_valid"], F32)
    extra[[int(order(x[r])[0]) for r in range(c["rows"])]] = -np.inf
    noise = np.full((c["rows"], 1), 0.5, F32) if top_k == 1 else np.random.default_rng(3).uniform(0, 1, (c["rows"], top_k)).astype(F32)
    return x, save, extra, noise


UNIFORM = dict(n_valid=129, rows=4096, ids=[3, 64, 65, 128], n_saved=2, seed=20240607, checked=64)


HEAD_STEPS = dict(rows=3, n_valid=257, ld_save=16, steps=9, range_=4, value=0.5, sampler=(0.7, 10, 0.95, 1.3, 20240913))


def head_steps_inputs():
    """(logits, bias, noise): grid logits fed unchanged at every step, so an unpenalised head returns one id for ever; a step-0 bias that is -inf on each
    row's raw arg-max (BEGIN_SUPPRESS); caller uniforms for the sampler's step 0."""
    c = HEAD_STEPS
    x = grid_logits([c["n_valid"], 21], c["rows"], c["n_valid"])
    bias = np.zeros(c["n_valid"], F32)
    bias[argmax_rows(x)[0]] = -np.inf
    noise = np.random.default_rng(23).uniform(0.0, 1.0, (c["rows"], c["sampler"][1])).astype(F32)
    return x, bias, noise


def head_steps_cases():
    """name -> keyword arguments of head_steps (and of the probe's head_steps) beyond the logits and the shape of HEAD_STEPS."""
    c = HEAD_STEPS
    _, bias, noise = head_steps_inputs()
    base = dict(range_=c["range_"], value=c["value"])
    return {
        "partial 0, step-0 bias": dict(base, partial=0, bias=bias),
        "partial 1": dict(base, partial=1),
        "value 1.0, history tracked": dict(base, value=1.0, partial=0, track_history=True),
        "sampler, noise on step 0": dict(base, partial=1, bias=bias, sampler=c["sampler"], noise=noise),
        "penalty changed after step 4": dict(base, partial=1, change=(5, 0.25, 2)),
    }


def sampler_uniform_inputs():
    """4096 equal rows with four equal top logits (20.0), a two-id history that the penalty 1.0 leaves alone."""
    c = UNIFORM
    x = np.tile(grid_logits([c["n_valid"], 15], 1, c["n_valid"]), (c["rows"], 1))
    x[:, c["ids"]] = F32(20.0)
    return x, np.zeros((c["rows"], 4), np.int32)
