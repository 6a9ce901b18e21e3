"""Float64 statement of Whisper's timestamp rules (csrc/kernels.h: launch_timestamp_rules, the build's own mode: the reference always decodes behind
<|notimestamps|>), twice over:

  rules_openai()   a literal transcription of OpenAI Whisper's ApplyTimestampRules, log_softmax included;
  rules_reduced()  the form the kernel computes: contiguous masked ranges, and the comparison of the timestamps' log-sum-exp L with the best text
                   logit T on raw logits (the soft-max normaliser is common to both sides).

Masking is exact (-inf or the f32 input unchanged), so the only place where f32 arithmetic can decide differently from float64 is L > T. budget() bounds
the kernel's error on L; every case the generators hand out keeps |L - T| at least MARGIN_FACTOR budgets wide (asserted here, on the float64 side), so a
GPU test compares every row of every case bit for bit. The expectations of whisper.split_segments and the inputs of the GPU tests live here too, so
tests/test_whisper_timestamps_ref_cpu.py checks them without a GPU."""
import math

import numpy as np

import token_heads_ref as thr
from token_heads_ref import F32, GRID, U32, grid_logits

MARGIN_FACTOR = 64
NEG = F32(-np.inf)


# ------------------------------------------------------------------------------------------------ the rule, twice
def rules_openai(row, hist, ts_begin, no_ts, eot, max_initial):
    """ApplyTimestampRules.apply on one row (sample_begin = 0: `hist` holds the ids generated since the prefill). max_initial < 0: no limit."""
    x = np.asarray(row, F32).copy()
    seq = [int(t) for t in hist]
    x[no_ts] = NEG                                                     # suppress <|notimestamps|>, which is handled by without_timestamps
    last_was_timestamp = len(seq) >= 1 and seq[-1] >= ts_begin
    penultimate_was_timestamp = len(seq) < 2 or seq[-2] >= ts_begin
    if last_was_timestamp:
        if penultimate_was_timestamp:                                  # has to be non-timestamp
            x[ts_begin:] = NEG
        else:                                                          # cannot be normal text tokens
            x[:eot] = NEG
    timestamps = [t for t in seq if t >= ts_begin]
    if timestamps:
        # timestamps shouldn't decrease; forbid timestamp tokens smaller than the last; also force each segment to have a nonzero length
        timestamp_last = timestamps[-1] if last_was_timestamp and not penultimate_was_timestamp else timestamps[-1] + 1
        x[ts_begin:timestamp_last] = NEG
    if len(seq) == 0:
        x[:ts_begin] = NEG                                             # suppress generating non-timestamp tokens at the beginning
        if max_initial >= 0:                                           # apply the max_initial_timestamp option
            x[ts_begin + max_initial + 1:] = NEG
    x64 = x.astype(np.float64)
    mx = x64.max()
    if mx > -np.inf:                                                   # (a row with nothing left has no distribution; nothing more to mask either)
        logprobs = x64 - (mx + math.log(np.exp(x64 - mx).sum()))
        tsl = logprobs[ts_begin:]
        timestamp_logprob = tsl.max() + math.log(np.exp(tsl - tsl.max()).sum()) if tsl.max() > -np.inf else -np.inf
        max_text_token_logprob = logprobs[:ts_begin].max()
        if timestamp_logprob > max_text_token_logprob:
            x[:ts_begin] = NEG
    return x


def ranges(hist, n_valid, ts_begin, eot, max_initial):
    """(text_lo, ts_lo, ts_hi, closing, first): steps 1-4 leave text [text_lo, ts_begin) less no_timestamps_id and timestamps [ts_lo, ts_hi) unmasked.
    m is the LARGEST timestamp of the history (the latest one in every stream the rules produce)."""
    h = len(hist)
    last_ts = h >= 1 and hist[-1] >= ts_begin
    penult_ts = h < 2 or hist[-2] >= ts_begin
    closing, first = last_ts and not penult_ts, h == 0
    ts_lo = n_valid if (last_ts and penult_ts) else ts_begin
    stamps = [int(t) for t in hist if t >= ts_begin]
    if stamps:
        m = min(max(stamps), n_valid - 1)
        ts_lo = max(ts_lo, m if closing else m + 1)
    ts_hi = min(n_valid, ts_begin + max_initial + 1) if (first and max_initial >= 0) else n_valid
    text_lo = ts_begin if first else (eot if closing else 0)
    return text_lo, ts_lo, ts_hi, closing, first


def lse_and_max(row, hist, ts_begin, no_ts, eot, max_initial):
    """float64 (L, T, M, n_ts, arg): L the log-sum-exp and M the maximum of the unmasked timestamp columns, T the maximum of the unmasked columns below
    ts_begin, n_ts the width of the timestamp range, arg = sum |x - M| exp(x - M) / sum exp(x - M) (how far a rounding of x - M moves L)."""
    x = np.asarray(row, F32).astype(np.float64)
    text_lo, ts_lo, ts_hi, _, _ = ranges(hist, len(x), ts_begin, eot, max_initial)
    text = x[text_lo:ts_begin].copy()
    if text_lo <= no_ts:
        text[no_ts - text_lo] = -np.inf
    T = text.max() if len(text) else -np.inf
    ts = x[ts_lo:ts_hi]
    M = ts.max() if len(ts) else -np.inf
    if M == -np.inf:
        return -np.inf, T, M, len(ts), 0.0
    d = ts[ts > -np.inf] - M
    S = np.exp(d).sum()
    return M + math.log(S), T, M, len(ts), float((np.abs(d) * np.exp(d)).sum() / S)


def rules_reduced(row, hist, ts_begin, no_ts, eot, max_initial):
    """The kernel's form. Returns (masked row f32, |L - T| in float64 -- inf when a side is empty)."""
    x = np.asarray(row, F32).copy()
    n = len(x)
    text_lo, ts_lo, ts_hi, closing, first = ranges(hist, n, ts_begin, eot, max_initial)
    L, T, _, _, _ = lse_and_max(row, hist, ts_begin, no_ts, eot, max_initial)
    x[no_ts] = NEG
    x[ts_begin:ts_lo] = NEG
    x[ts_hi:n] = NEG
    x[:text_lo] = NEG
    if L > T:
        x[:ts_begin] = NEG
    return x, (np.inf if (L == -np.inf or T == -np.inf) else abs(L - T))


def budget(row, hist, ts_begin, no_ts, eot, max_initial):
    """Bound on |L_gpu - L| for timestamp_rules_kernel: L = M + logf(S), S = sum __expf(x - M) in f32 over the unmasked timestamp columns, M their exact maximum.
    1. relative error of S, which is the absolute error of log S: the hardware __expf (2e-5, as token_heads_ref.beam_topv_budget counts it); the rounding of
       every x - M, 2^-24 |x - M| relative in its term -- `arg`, weighted; the depth of the f32 addition chain -- ceil((n_ts + 3) / 4096) * 4 terms per thread
       (the stripes start at a multiple of four columns), 6 lane merges, 16 wave merges -- at 2^-24 each;
    2. logf: one ulp of log S = L - M;
    3. the rounding of M + logf(S), 2^-24 |L|.
    T and the comparison are exact. 0 when a side is empty (nothing is compared)."""
    L, T, M, n_ts, arg = lse_and_max(row, hist, ts_begin, no_ts, eot, max_initial)
    if L == -np.inf or T == -np.inf:
        return 0.0
    depth = -(-(n_ts + 3) // 4096) * 4 + 6 + 16
    return 2e-5 + U32 * arg + depth * U32 + 2 * U32 * abs(L - M) + U32 * abs(L)


def apply(logits, hists, params, openai=False):
    """Rows through rules_reduced (or rules_openai): (masked [rows][n] f32, margins [rows], budgets [rows])."""
    fn = rules_openai if openai else rules_reduced
    out, margins, budgets = [], [], []
    for row, hist in zip(np.asarray(logits, F32), hists):
        if openai:
            out.append(fn(row, hist, *params))
        else:
            y, mg = fn(row, hist, *params)
            out.append(y); margins.append(mg); budgets.append(budget(row, hist, *params))
    return np.stack(out), np.asarray(margins), np.asarray(budgets)


def grammatical(ids, ts_begin, no_ts, eot):
    """A stream the rules produce when the specials (eot, ts_begin) are suppressed, stated without the rules: every id is text (< eot) or a timestamp; the
    first id is a timestamp and text follows it; timestamps never decrease and come alone (closing a segment) or in pairs (closing one, opening the next),
    never three in a row; text appears only inside an open segment."""
    ids = [int(t) for t in ids]
    if any(eot <= t < ts_begin for t in ids):
        return False
    stamps = [t for t in ids if t >= ts_begin]
    if any(b < a for a, b in zip(stamps, stamps[1:])):
        return False
    is_open = False
    for i, t in enumerate(ids):
        prev_ts = i >= 1 and ids[i - 1] >= ts_begin
        if t >= ts_begin:
            if not prev_ts:
                is_open = i == 0                  # the stream's first id opens; a timestamp after text closes
            elif i == 1 or ids[i - 2] >= ts_begin:
                return False                      # a second timestamp right at the start, or a third in a row
            else:
                is_open = True                    # the second of a pair opens the next segment
        elif not is_open:
            return False                          # text before any timestamp, or right after a closing one
    return True


# ------------------------------------------------------------------------------------------------ inputs of the kernel tests
GEOMETRIES = [(129, 90, 100), (600, 499, 565), (4100, 4000, 4096), (8200, 4090, 4095), (51866, 50257, 50365)]     # (n_valid, eot, ts_begin)
LD_SAVE = 448                                                                                                      # Whisper's max_target_positions
MAX_INITIALS = [-1, 0, 50, 10 ** 6]


def params(geom, max_initial=-1):
    n_valid, eot, ts_begin = geom
    return ts_begin, ts_begin - 1, eot, max_initial


def history(kind, length, geom, rng, stamp=None):
    """A stream of `length` ids ending in `kind`: "empty"; "ts" [ts]; "text" [ts, text ...]; "closing" [ts, text ..., ts']; "pair" [ts, text ..., ts', ts''].
    stamp: the last timestamp id (default: a random one that leaves later ones free where the geometry has them)."""
    n_valid, eot, ts_begin = geom
    n_ts = n_valid - ts_begin
    if kind == "empty":
        return []
    last = int(stamp) if stamp is not None else ts_begin + int(rng.integers(1, max(2, n_ts // 2)))
    lo = ts_begin + (last - ts_begin) // 3
    tail = {"ts": [last], "text": [], "closing": [last], "pair": [max(lo, last - 1), last]}[kind]
    if kind == "ts":
        assert length == 1
        return tail
    head = [last if kind == "text" else lo]
    n_text = length - len(head) - len(tail)
    assert n_text >= 1
    return head + rng.integers(0, eot, n_text).tolist() + tail


def plant(logits, hists, geom, max_initial, above):
    """Rows whose best unmasked text logit sits MARGIN_FACTOR budgets (rounded up to the 2^-10 grid, plus one grid step) below (above[r]) or above the
    timestamps' log-sum-exp; every other unmasked text column is at least 0.5 lower. Rows with an empty side are left as they are."""
    p = params(geom, max_initial)
    ts_begin, no_ts, eot, _ = p
    x = np.asarray(logits, F32).copy()
    for r, hist in enumerate(hists):
        text_lo, _, _, _, _ = ranges(hist, x.shape[1], ts_begin, eot, max_initial)
        L, T, _, _, _ = lse_and_max(x[r], hist, *p)
        if L == -np.inf or T == -np.inf:
            continue
        cols = [c for c in range(text_lo, ts_begin) if c != no_ts]
        j = cols[(7 * r + 3) % len(cols)]
        for _ in range(2):                                       # the budget depends on L alone, not on the text side: one pass settles it
            gap = math.ceil(MARGIN_FACTOR * budget(x[r], hist, *p) / GRID + 1) * GRID
            t = (math.floor((L - gap) / GRID) if above[r] else math.ceil((L + gap) / GRID)) * GRID
            x[r, cols] = np.minimum(x[r, cols], F32(t - 0.5))
            x[r, j] = F32(t)
        assert float(x[r, j]) == t
    return x


def check_decided(logits, hists, p):
    """The generator's own assertion: every row that compares L with T does so MARGIN_FACTOR budgets away from a flip."""
    _, margins, budgets = apply(logits, hists, p)
    assert np.all(margins >= MARGIN_FACTOR * budgets), (margins, budgets)
    return margins, budgets


def _table(hists, rows, geom, seed):
    """save_ids [rows][LD_SAVE]: the histories, then valid filler ids the kernel must not read (timestamps, so a read past the counter shows)."""
    n_valid = geom[0]
    tab = np.full((rows, LD_SAVE), n_valid - 1, np.int32)
    for r, h in enumerate(hists):
        tab[r, :len(h)] = h
    return tab


def kernel_cases(geom):
    """name -> dict(logits, hists, save_ids, n_saved (int: the shared counter; array: per-row counters), params): 3 to 5 rows each."""
    n_valid, eot, ts_begin = geom
    last_id = n_valid - 1
    cases = {}

    def add(name, hists, max_initial=-1, above=None, shared=True, openai=True, logits=None):
        rows = len(hists)
        seed = [n_valid, len(cases), 41]
        x = grid_logits(seed, rows, n_valid) if logits is None else logits
        x = plant(x, hists, geom, max_initial, above if above is not None else [r % 2 == 0 for r in range(rows)])
        p = params(geom, max_initial)
        check_decided(x, hists, p)
        lens = [len(h) for h in hists]
        assert not shared or len(set(lens)) == 1
        cases[name] = dict(logits=x, hists=hists, save_ids=_table(hists, rows, geom, seed), n_saved=lens[0] if shared else np.asarray(lens, np.int32),
                           params=p, openai=openai)

    rng = np.random.default_rng([n_valid, 43])
    for mi in MAX_INITIALS:
        add(f"empty, max_initial {mi}", [[], [], []], max_initial=mi)
    add("[ts]", [history("ts", 1, geom, rng), history("ts", 1, geom, rng, stamp=ts_begin), history("ts", 1, geom, rng, stamp=last_id)])
    add("[ts, text]", [history("text", 2, geom, rng), history("text", 2, geom, rng), history("text", 2, geom, rng, stamp=ts_begin),
                       history("text", 2, geom, rng, stamp=last_id - 1), history("text", 2, geom, rng, stamp=last_id)])
    add("[ts, text, ts]", [history("closing", 3, geom, rng), history("closing", 3, geom, rng), history("closing", 3, geom, rng, stamp=last_id),
                           history("closing", 3, geom, rng, stamp=ts_begin + 1)])
    add("[.., ts, ts]", [history("pair", 4, geom, rng), history("pair", 4, geom, rng, stamp=last_id), history("pair", 4, geom, rng)])
    for n in (255, 256, 257, LD_SAVE - 1):
        add(f"shared counter {n}", [history("text", n, geom, rng), history("text", n, geom, rng), history("closing", n, geom, rng),
                                    history("pair", n, geom, rng)][:4 if n != 256 else 3], above=[True, False, True, False])
    add("per-row counters, short", [[], history("ts", 1, geom, rng), history("text", 2, geom, rng), history("closing", 3, geom, rng),
                                    history("pair", 4, geom, rng)], shared=False, above=[True, True, False, False, True])
    add("per-row counters, long", [history("closing", 255, geom, rng), history("text", 256, geom, rng), history("text", 257, geom, rng),
                                   history("closing", LD_SAVE - 1, geom, rng), history("text", 9, geom, rng)], shared=False,
        above=[False, True, False, True, True])
    # a row that is -inf everywhere but eot: nothing to compare, nothing may turn into NaN; beside it an ordinary row and a row of equal logits
    x = grid_logits([n_valid, 47], 3, n_valid)
    x[0] = NEG
    x[0, eot] = F32(1.5)
    x[2] = F32(0.25)
    add("all -inf outside eot", [history("text", 5, geom, rng), history("text", 5, geom, rng), history("closing", 5, geom, rng)], logits=x)
    # what follows an eot in a row that goes on decoding is arbitrary: ids in any order. Only the largest timestamp and the last two ids count.
    junk = [[ts_begin + 1, 3, eot] + rng.integers(0, n_valid, 20).tolist() for _ in range(3)]
    junk[1] += [5, 6]; junk[2] += [7, last_id - 2]
    junk[0] += [last_id - 1, last_id - 1]
    add("arbitrary ids after eot", [j[:25] for j in junk], openai=False)
    return cases


# ------------------------------------------------------------------------------------------------ a greedy walk
def greedy_walk(geom, seed, steps, max_initial=-1, scale=1.0):
    """Arg-max decoding with rules_reduced over fresh random rows: the stream up to (not including) eot."""
    n_valid, eot, ts_begin = geom
    p = params(geom, max_initial)
    ids = []
    for t in range(steps):
        row = grid_logits([n_valid, seed, t], 1, n_valid)[0]
        row[ts_begin:] += F32(scale)                    # tilts the balance between text and timestamps; stays on the grid
        row[eot + 1:ts_begin] = NEG                     # the specials, as Whisper's suppress list takes them out
        y, _ = rules_reduced(row, ids, *p)
        pick = int(thr.argmax_rows(y[None])[0][0])
        if pick == eot:
            break
        ids.append(pick)
    return ids


# ------------------------------------------------------------------------------------------------ the head over several steps
HEAD_GEOM = (257, 200, 220)
HEAD_STEPS = dict(rows=3, steps=9, ld_save=16, range_=4, value=0.5, sampler=(0.7, 10, 0.95, 1.3, 20240913), max_initial=20)


def head_steps(logits, steps, ld_save, range_, value, partial, timestamps, bias=None, sampler=None, noise=None):
    """token_heads_ref.head_steps with the timestamp rules between the penalty and the selection, every pick appended (csrc/decode_head.h).
    Returns (picks [steps][rows], save_ids, n_saved, decided [steps][rows] (the sampler's margins), margins [steps][rows], budgets [steps][rows])."""
    logits = np.asarray(logits, F32)
    rows = len(logits)
    save, n = np.zeros((rows, ld_save), np.int32), 0
    picks, decided = np.zeros((steps, rows), np.int32), np.ones((steps, rows), bool)
    margins, budgets = np.zeros((steps, rows)), np.zeros((steps, rows))
    for t in range(steps):
        penalised = value != 1.0 and sampler is None
        x = thr.apply_penalty(logits, save, n, range_, value, partial) if penalised and t > 0 else logits
        x, margins[t], budgets[t] = apply(x, [save[r, :n].tolist() for r in range(rows)], timestamps)
        if sampler is not None:
            temperature, top_k, top_p, rp, seed = sampler
            picks[t], margin, _ = thr.sample_topk_topp(x, save, n, temperature, top_k, top_p, rp, extra=bias if t == 0 else None,
                                                       noise=noise if t == 0 else None, seed=seed)
            decided[t] = thr.sampler_decided(margin, top_k)
        else:
            picks[t], _ = thr.argmax_rows(x, bias if t == 0 else None)
        save = thr.append_ids(save, picks[t], n)
        n += 1
    return picks, save, n, decided, margins, budgets


def head_steps_inputs():
    """(logits, bias, noise) for HEAD_GEOM: the same rows at every step, the timestamps lifted so that both sides of L > T occur along the way."""
    c = HEAD_STEPS
    n_valid, eot, ts_begin = HEAD_GEOM
    x = grid_logits([n_valid, 29], c["rows"], n_valid)
    x[:, ts_begin:] += F32(1.0)
    x[:, eot + 1:ts_begin] -= F32(64.0)                      # the specials carry Whisper's suppress penalty
    bias = np.zeros(n_valid, F32)
    bias[ts_begin + 2] = NEG                                 # BEGIN_SUPPRESS-like: a step-0 bias on a column the initial rule leaves open
    noise = np.random.default_rng(31).uniform(0.0, 1.0, (c["rows"], c["sampler"][1])).astype(F32)
    return x, bias, noise


def head_steps_cases():
    """name -> keyword arguments of head_steps (and of the probe's) beyond the logits and the shape of HEAD_STEPS."""
    c = HEAD_STEPS
    _, bias, noise = head_steps_inputs()
    ts = params(HEAD_GEOM, c["max_initial"])
    base = dict(range_=c["range_"], partial=0, timestamps=ts)
    return {
        "timestamps alone": dict(base, value=1.0, bias=bias),
        "with the penalty head": dict(base, value=c["value"], bias=bias),
        "with the sampler, noise on step 0": dict(base, value=1.0, bias=bias, sampler=c["sampler"], noise=noise),
    }


# ------------------------------------------------------------------------------------------------ split_segments
def _s(start, end, tokens):
    return {"start": start, "end": end, "tokens": tokens}


TS0 = 1000                                                   # ts_begin of the hand-written streams; TS0 + k is k * 0.02 s
SPLIT_CASES = {
    # name: (ids, window_offset_s, window_len_s, expected segments)
    "one closed segment": ([TS0, 5, 6, TS0 + 50], 0.0, 30.0, [_s(0.0, 1.0, [5, 6])]),
    "a pair at a boundary": ([TS0, 5, TS0 + 50, TS0 + 50, 7, 8, TS0 + 125], 0.0, 30.0, [_s(0.0, 1.0, [5]), _s(1.0, 2.5, [7, 8])]),
    "a gap between segments": ([TS0 + 10, 5, TS0 + 50, TS0 + 100, 7, TS0 + 150], 0.0, 30.0, [_s(0.2, 1.0, [5]), _s(2.0, 3.0, [7])]),
    "an open tail": ([TS0, 5, TS0 + 50, TS0 + 50, 7, 8], 0.0, 12.5, [_s(0.0, 1.0, [5]), _s(1.0, 12.5, [7, 8])]),
    "an empty segment": ([TS0, 5, TS0 + 50, TS0 + 60, TS0 + 70, 9, TS0 + 80], 0.0, 30.0, [_s(0.0, 1.0, [5]), _s(1.4, 1.6, [9])]),
    "an open segment without text": ([TS0, 5, TS0 + 50, TS0 + 50], 0.0, 30.0, [_s(0.0, 1.0, [5])]),
    "a window offset": ([TS0 + 25, 5, TS0 + 75], 30.0, 30.0, [_s(30.5, 31.5, [5])]),
    "an open tail in an offset window": ([TS0 + 25, 5], 28.0, 30.0, [_s(28.5, 58.0, [5])]),
    "nothing but eot (not emitted)": ([], 0.0, 30.0, []),
    "a lone timestamp": ([TS0 + 3], 0.0, 30.0, []),
}
