"""Float64 statement of the token scores (csrc/kernels.h: launch_argmax_logprob_rows, launch_logprob_at_rows; csrc/decode_head.h: TokenHead in scores
mode), the error budgets of the two kernels, a numpy f32 restatement of their online reduction in the kernels' own order, and the seeded rows the GPU tests use.

The score of a pick is the natural-log soft-max, at the picked id, of v = logits + extra over the first n_valid columns. The addition of `extra` is an
elementwise f32 step and therefore bit-defined (token_heads_ref.py's convention); everything after it is float64 here. A -inf column has zero weight; a
row without a column above -inf picks id 0 and scores -inf; a pick whose own column is -inf, or an id outside the row, scores -inf. No NaN.

Column ownership the rows rely on (logprob_rows_kernel = argmax_rows_kernel's): thread t (lane t % 64 of wave t / 64, 16 waves) reads columns 4 t .. 4 t + 3 of
every 4096-column stripe, two stripes per trip of the loop."""
import math

import numpy as np

import token_heads_ref as thr
from token_heads_ref import F32, GRID, U32, grid_logits

EXPF = 2e-5                            # the hardware __expf, relative, as token_heads_ref.beam_topv_budget counts it
NAN_FILL = np.float32(np.nan)          # what the tests put into every output slot before a call


def seen(logits, extra=None):
    """The f32 row the selection sees: logits + extra (f32 sum)."""
    x = np.asarray(logits, F32)
    return x if extra is None else (x + np.asarray(extra, F32)[None, :]).astype(F32)


def log_softmax(v):
    """float64 log-soft-max of the f32 rows v, -inf columns at zero weight; (lsm [rows][n], row max [rows], lse [rows]). A row without a finite column:
    lsm -inf everywhere, max and lse -inf."""
    v64 = np.asarray(v, F32).astype(np.float64)
    M = v64.max(axis=1)
    lse = np.full(len(v64), -np.inf)
    out = np.full(v64.shape, -np.inf)
    for r in range(len(v64)):
        if M[r] > -np.inf:
            lse[r] = M[r] + math.log(np.exp(v64[r] - M[r]).sum())
            fin = v64[r] > -np.inf
            out[r, fin] = v64[r, fin] - lse[r]
    return out, M, lse


def scores_at(logits, ids, extra=None):
    """(score [rows], row max, lse) of the picks `ids`; an id outside [0, n) scores -inf."""
    v = seen(logits, extra)
    lsm, M, lse = log_softmax(v)
    n = v.shape[1]
    s = np.array([lsm[r, i] if 0 <= i < n else -np.inf for r, i in enumerate(np.asarray(ids).tolist())])
    return s, M, lse


def argmax_scores(logits, extra=None):
    """(ids, score, row max, lse) of the greedy pick: token_heads_ref.argmax_rows' id (first maximum; 0 for an empty row) and its score."""
    ids, _ = thr.argmax_rows(logits, extra)
    s, M, lse = scores_at(logits, ids, extra)
    return ids, s, M, lse


# ------------------------------------------------------------------------------------------------ budgets
def s_budget(n_valid):
    """Relative error of S = sum exp(v - M) as logprob_rows_kernel forms it, which is the absolute error of log S. Per term, worst case:
    1. its own __expf: EXPF (this covers the rounding of the argument v - m and of v * log2(e) inside the instruction: both are 2^-24 |v - m| relative
       to the term, and a term weighs exp(-|v - m|) in S, so their sum over the row stays below 2^-23 / e);
    2. the rescales of the online form: a thread multiplies its sum by __expf(old max - new max) when a 16-byte load moves its maximum, at most once per
       load after the term's own -- trips - 1 times, trips = ceil(n_valid / 4096); six lane merges and one wave merge multiply by such a factor once
       more each: (trips + 6) factors, each EXPF for the factor and 2^-24 for the product;
    3. the f32 additions: 4 trips per thread, 6 lane merges, 16 wave partials, 2^-24 each."""
    trips = -(-n_valid // 4096)
    return EXPF * (1 + trips + 6) + U32 * ((trips + 6) + 4 * trips + 6 + 16)


def fused_budget(n_valid, row_max, lse):
    """Bound on |score_gpu - score| of launch_argmax_logprob_rows: score = -logf(S). s_budget, plus logf at one ulp of log S = lse - M."""
    lse, row_max = np.asarray(lse, np.float64), np.asarray(row_max, np.float64)
    with np.errstate(invalid="ignore"):
        return s_budget(n_valid) + 2 * U32 * np.where(np.isfinite(lse), np.abs(lse - row_max), 0.0)      # (an empty row scores -inf exactly: no budget)


def at_id_budget(n_valid, row_max, lse, score):
    """Bound on |score_gpu - score| of launch_logprob_at_rows: score = v[id] - (M + logf(S)), v bit-defined. fused_budget, plus two roundings: M + logf(S)
    at |lse| and the subtraction at |score|."""
    return fused_budget(n_valid, row_max, lse) + U32 * np.where(np.isfinite(lse), np.abs(lse), 0.0) + U32 * np.where(np.isfinite(score), np.abs(score), 0.0)


def over_budget(got, want, budget):
    """max |got - want| / budget over the finite wants (0.0 when there is none); -inf wants must be met exactly and nothing may be NaN."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert not np.isnan(got).any(), got
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin]), (got, want)
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin] - want[fin]) / np.broadcast_to(budget, want.shape)[fin]).max())


# ------------------------------------------------------------------------------------------------ the kernels' reduction in f32, in their order
def online_f32(v):
    """One row v [n] (f32, what the kernel's loads return after `extra` is added) through logprob_rows_kernel's reduction with np.float32 arithmetic:
    1024 threads, thread t takes its 16-byte groups in ascending order, rescales its sum when a group moves its maximum, adds the group's four terms one
    after the other; xor-butterfly over the 64 lanes of a wave (offsets 32 .. 1), then the 16 wave partials in order. -> (M, S) as f32. numpy's f32 exp
    stands in for __expf; the budget counts the instruction's own error on top."""
    v = np.asarray(v, F32)
    n = len(v)
    trips = -(-n // 4096)
    pad = np.full(trips * 4096, -np.inf, F32)
    pad[:n] = v
    g = pad.reshape(trips, 1024, 4)
    best, total = np.full(1024, -np.inf, F32), np.zeros(1024, F32)
    ninf = F32(-np.inf)

    def scale(m, M):
        with np.errstate(invalid="ignore"):
            return np.where(m == ninf, F32(0.0), np.exp((m - M).astype(F32))).astype(F32)

    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(trips):
            a = g[j]
            m4 = a.max(axis=1)
            moved = m4 > best
            total = np.where(moved, total * np.exp(np.where(moved, best - m4, F32(0.0)).astype(F32)), total).astype(F32)
            best = np.maximum(best, m4)
            mm = np.where(best == ninf, F32(0.0), best).astype(F32)
            for e in range(4):
                total = (total + np.exp((a[:, e] - mm).astype(F32))).astype(F32)
        lane = np.arange(1024)
        for o in (32, 16, 8, 4, 2, 1):
            ob, ot = best[lane ^ o], total[lane ^ o]
            M = np.maximum(best, ob)
            total = ((total * scale(best, M)).astype(F32) + (ot * scale(ob, M)).astype(F32)).astype(F32)
            best = M
        wb, wt = best[::64], total[::64]
        M = wb.max()
        S = F32(0.0)
        for w in range(16):
            S = F32(S + F32(wt[w] * scale(wb[w:w + 1], M)[0]))
    return F32(M), F32(S)


def online_scores(logits, ids=None, extra=None):
    """The f32 restatement's scores: fused (-log S at the arg-max) when ids is None, else v[id] - (M + log S), every step rounded to f32."""
    v = seen(logits, extra)
    out = np.zeros(len(v), np.float64)
    for r in range(len(v)):
        M, S = online_f32(v[r])
        if M == -np.inf:
            out[r] = -np.inf
        elif ids is None:
            out[r] = -F32(np.log(S))
        else:
            i = int(ids[r])
            x = v[r, i] if 0 <= i < v.shape[1] else F32(-np.inf)
            out[r] = -np.inf if x == -np.inf else F32(x - F32(M + F32(np.log(S))))
    return out


# ------------------------------------------------------------------------------------------------ seeded rows of the GPU tests
TOP = F32(20.0)                        # above every N(0, 3^2) draw used here
LOW = F32(-30.0)
LD_SAVE, COLUMN = 6, 2                 # the kernels' history table in the tests and the column the counter addresses
KERNEL_WIDTHS = [n for n in thr.WIDTHS if n <= thr.WIDE]
WIDE_WIDTHS = [n for n in thr.WIDTHS if n > thr.WIDE]
# pairs of columns whose partial sums meet at one level of the merges (module docstring): a lost partial moves the score by log 2
SPLITS = {"two lanes of a wave": (9, 101), "two waves": (8, 300), "two loads of a trip": (11, 4104), "two trips": (8, 8200), "first and last": (0, -1)}
SPOTS = [0, 4095, 4096, 8191, 8192]
TIES = {"one float4": (8, 10), "two lanes of a wave": (9, 101), "two waves": (8, 300), "two loads of a trip": (11, 4104), "later wave, lower id": (300, 4106),
        "two trips": (8, 8200), "two trips, other thread": (4100, 8461)}


def _three_to_five(rows):
    rows = list(rows)
    while len(rows) < 3:
        rows.append(rows[0].copy())
    return np.stack(rows[:5]).astype(F32)


def planted_rows(n):
    """Chunks of 3 to 5 grid rows: random ones, the maximum planted at each boundary column, equal maxima in pairs (the lower id wins)."""
    base = grid_logits([n, 41], 3, n)
    rows = [base[i].copy() for i in range(3)]
    for p in sorted({s for s in SPOTS if s < n} | {n - 1}):
        x = base[p % 3].copy()
        x[p] = TOP
        rows.append(x)
    for a, b in TIES.values():
        if b < n:
            x = base[a % 3].copy()
            x[[a, b]] = TOP
            rows.append(x)
    return [_three_to_five(rows[i:i + 5]) for i in range(0, len(rows), 5)]


def score_cases(n):
    """name -> (logits [3..5][n], extra [n] or None): the rows whose scores the GPU tests check within budget."""
    rnd = grid_logits([n, 43], 4, n)
    cases = {"random": (rnd, None)}
    split = []
    for a, b in SPLITS.values():
        b = n - 1 if b < 0 else b
        if b < n and a < n:
            x = np.full(n, LOW, F32) + grid_logits([n, a, b], 1, n)[0] * F32(0.125)      # the rest of the row weighs ~ n e^-40 beside the pair
            x[[a, b]] = F32(10.0)
            split.append(x)
    cases["half each on two columns"] = (_three_to_five(split or [rnd[0]]), None)
    cases["shifted by +-90"] = (np.stack([rnd[0] + F32(90.0), rnd[1] + F32(90.0), rnd[2] - F32(90.0), rnd[3] - F32(90.0)]).astype(F32), None)
    equal = np.full(n, F32(1.5), F32)
    dominant = rnd[0].copy()
    dominant[n // 2] = F32(60.0)
    last_only = np.full(n, -np.inf, F32)
    last_only[n - 1] = F32(-3.25)
    cases["equal, dominant, last column only, all -inf"] = (np.stack([equal, dominant, last_only, np.full(n, -np.inf, F32)]), None)
    holes = grid_logits([n, 47], 4, n)
    rng = np.random.default_rng([n, 53])
    holes[rng.uniform(size=holes.shape) < 0.3] = -np.inf
    holes[0, 0] = F32(0.5)                                      # (every row of this case keeps a finite column: n = 1 included)
    holes[1:, n - 1] = F32(-0.25)
    extra = grid_logits([n, 59], 1, n)[0]
    extra[rng.uniform(size=n) < 0.2] = -np.inf
    extra[n - 1] = F32(0.0)
    extra[0] = F32(0.0) if n == 1 else extra[0]
    cases["-inf columns, -inf extra"] = (holes, extra)
    suppress = np.zeros(n, F32)
    suppress[thr.argmax_rows(rnd[:3])[0]] = -np.inf             # BEGIN_SUPPRESS on the rows' raw arg-max
    if n > 3:
        cases["extra takes the arg-max out"] = (rnd[:3].copy(), suppress)
    return cases


def ids_for(logits, extra, kind):
    """The ids the at-id kernel is given: the maximum, a mid-rank column, a -inf column (the first one; the maximum where the row has none), column n - 1."""
    v = seen(logits, extra)
    rows, n = v.shape
    ids = np.zeros(rows, np.int32)
    for r in range(rows):
        o = thr.order(v[r])
        if kind == "maximum":
            ids[r] = o[0]
        elif kind == "mid-rank":
            ids[r] = o[min(n - 1, max(1, n // 3))]
        elif kind == "-inf column":
            inf = np.nonzero(v[r] == -np.inf)[0]
            ids[r] = inf[0] if len(inf) else o[0]
        else:
            ids[r] = n - 1
    return ids


ID_KINDS = ["maximum", "mid-rank", "-inf column", "last column"]


# ------------------------------------------------------------------------------------------------ the head over several steps, with scores
def head_steps(logits, steps, ld_save, range_, value, partial, bias=None, track_history=False, sampler=None, noise=None, change=None, timestamps=None):
    """token_heads_ref.head_steps (whisper_timestamps_ref.head_steps with timestamps) in scores mode: every pick joins the history whatever the head, and
    the score of step t's pick is the log-soft-max of step t's edited row -- after the penalty, the timestamp rules and the sampler's in-place repetition
    penalty, plus the bias on step 0 -- at the pick. -> (picks [steps][rows], save_ids, n_saved, decided [steps][rows], scores [steps][rows],
    budgets [steps][rows]: fused for the arg-max heads, at-id for the sampler)."""
    logits = np.asarray(logits, F32)
    rows, n_valid = logits.shape
    save, n = np.zeros((rows, ld_save), np.int32), 0
    picks, decided = np.zeros((steps, rows), np.int32), np.ones((steps, rows), bool)
    scores, budgets = np.zeros((steps, rows)), np.zeros((steps, rows))
    for t in range(steps):
        if change is not None and t == change[0]:
            value, range_ = change[1], change[2]
        penalised = value != 1.0 and sampler is None
        x = thr.apply_penalty(logits, save, n, range_, value, partial) if penalised and t > 0 else logits
        if timestamps is not None:
            import whisper_timestamps_ref as wtr
            x, margins, tb = wtr.apply(x, [save[r, :min(n, ld_save)].tolist() for r in range(rows)], timestamps)
            decided[t] &= np.asarray(margins) >= np.asarray(tb)
        b = bias if t == 0 else None
        if sampler is not None:
            temperature, top_k, top_p, rp, seed = sampler
            picks[t], margin, x = thr.sample_topk_topp(x, save, n, temperature, top_k, top_p, rp, extra=b, noise=noise if t == 0 else None, seed=seed)
            decided[t] &= thr.sampler_decided(margin, top_k)
            scores[t], M, lse = scores_at(x, picks[t], b)
            budgets[t] = at_id_budget(n_valid, M, lse, scores[t])
        else:
            picks[t], scores[t], M, lse = argmax_scores(x, b)
            budgets[t] = fused_budget(n_valid, M, lse)
        save = thr.append_ids(save, picks[t], n)
        n += 1
    return picks, save, n, decided, scores, budgets
