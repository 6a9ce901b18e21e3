"""Float64 numpy statement of hotword boosting in the autoregressive decoders (csrc/hotword.hip, csrc/decode_head.h), not circular: the trie
and its transition are tests/ctc_beam_ref.py's (build_trie, trie_step), the heads tests/token_heads_ref.py's.

Every row carries a trie node: the root after a prefill, then trie_step over the row's own picks. delta(c) is the change trie_step would make to the
bonus for token c from that node:
    child of the node                                +boost
    no child of the node, but a child of the root    boost - depth * boost
    everything else                                  -depth * boost
Selection head: the row is biased before the selection by delta + the row constant depth * boost -- children of the node + (depth + 1) * boost, the
root's other children + boost, nothing else (`bias_sparse`; `bias_dense` adds delta itself to every column). Arg-max, soft-max and log-soft-max do not
see a row constant. The update is f32: logit + float32(depth + 1) * boost. Order inside a step: penalty, hotword bias, timestamp rules, selection, append.
Beam ranker: a hypothesis score is log-soft-max(model)(c) + delta(c). `rerank` is the device's merge rule -- the K best of (plain top-K) u S, S = children
of the node + children of the root -- and `rank_dense` the ranking over every column it must equal.

Elementwise f32 steps are done in np.float32, as token_heads_ref does; sums and transcendentals are float64."""
import numpy as np

import token_heads_ref as thr
import token_scores_ref as tsr
from ctc_beam_ref import build_trie, trie_step

F32 = np.float32
EVENTS = ("advance", "end", "refund", "restart")


def children(trie, node):
    lo, hi = int(trie["child_off"][node]), int(trie["child_off"][node + 1])
    return [int(t) for t in trie["child_tok"][lo:hi]]


def classify(trie, node, c):
    """Which of the four events appending c at `node` is (None: nothing happens at the root), and the node afterwards."""
    kids, root = children(trie, node), children(trie, 0)
    nxt, _ = trie_step(trie, node, 0.0, int(c), 1.0)
    if c in kids:
        ch = int(trie["child_node"][int(trie["child_off"][node]) + kids.index(c)])
        return ("end" if int(trie["is_end"][ch]) else "advance"), nxt
    if node != 0:
        return ("restart" if c in root else "refund"), nxt
    return None, nxt


def delta_dense(trie, node, boost, n):
    """float64 [n]: delta(c) for every column, by trie_step itself."""
    d = np.full(n, -float(int(trie["depth"][node])) * float(boost))
    for c in set(children(trie, node)) | set(children(trie, 0)):
        if c < n:
            d[c] = trie_step(trie, node, 0.0, c, float(boost))[1]
    return d


def bias_sparse(row, trie, node, boost):
    """The kernel's update of one f32 row: children of the node + float32(depth + 1) * boost, the root's other children + boost; -inf stays -inf."""
    x = np.asarray(row, F32).copy()
    kids = children(trie, node)
    add = F32(F32(int(trie["depth"][node]) + 1) * F32(boost))
    for c in kids:
        x[c] = F32(x[c] + add)
    for c in children(trie, 0):
        if c not in kids:
            x[c] = F32(x[c] + F32(boost))
    return x


def bias_dense(row, trie, node, boost):
    """float64 row + delta on every column: what the sparse form must select and score like."""
    return np.asarray(row, F32).astype(np.float64) + delta_dense(trie, node, boost, len(row))


def log_softmax64(v):
    v = np.asarray(v, np.float64)
    m = v.max()
    with np.errstate(divide="ignore"):
        return v - (m + np.log(np.exp(v - m).sum()))


# ------------------------------------------------------------------------------------------------ the head over several steps
def head_steps_hot(logits, phrases, boost, ld_save, range_=4, value=1.0, partial=0, bias=None, sampler=None, noise=None, timestamps=None):
    """token_scores_ref.head_steps with a row per step (logits [steps][rows][n]) and hotwords: the sessions' sequence penalty (decode steps, not under
    the sampler) -> hotword bias -> timestamp rules -> sampler or arg-max -> append, every pick joining the history; the node follows the pick. An
    empty phrase list is the plain head. noise: [steps][rows][top_k] caller uniforms for every step.
    -> dict: picks / nodes (after the step) / decided / scores / budgets / margins [steps][rows], save, n, events {name: count}, deep_restarts (phrases
    abandoned at depth >= 2 onto a root child), rows_seen [steps][rows][n] (the row the selection saw, before the sampler's own in-place penalty)."""
    logits = np.asarray(logits, F32)
    steps, rows, n_valid = logits.shape
    trie = build_trie(phrases) if len(phrases) else None
    save, n = np.zeros((rows, ld_save), np.int32), 0
    node = np.zeros(rows, np.int64)
    out = dict(picks=np.zeros((steps, rows), np.int32), nodes=np.zeros((steps, rows), np.int32), decided=np.ones((steps, rows), bool),
               scores=np.zeros((steps, rows)), budgets=np.zeros((steps, rows)), margins=np.full((steps, rows), np.inf),
               rows_seen=np.zeros((steps, rows, n_valid), F32), events={k: 0 for k in EVENTS}, deep_restarts=0)
    for t in range(steps):
        penalised = value != 1.0 and sampler is None
        x = thr.apply_penalty(logits[t], save, n, range_, value, partial) if penalised and t > 0 else logits[t].copy()
        if trie is not None:
            x = np.stack([bias_sparse(x[r], trie, int(node[r]), boost) for r in range(rows)])
        if timestamps is not None:
            import whisper_timestamps_ref as wtr
            x, margins, tb = wtr.apply(x, [save[r, :min(n, ld_save)].tolist() for r in range(rows)], timestamps)
            out["decided"][t] &= np.asarray(margins) >= np.asarray(tb)
        out["rows_seen"][t] = x
        b = bias if t == 0 else None
        if sampler is not None:
            temperature, top_k, top_p, rp, seed = sampler
            picks, margin, x = thr.sample_topk_topp(x, save, n, temperature, top_k, top_p, rp, extra=b, noise=None if noise is None else noise[t], seed=seed)
            out["decided"][t] &= thr.sampler_decided(margin, top_k)
            out["margins"][t] = margin[:, 0]
            sc, M, lse = tsr.scores_at(x, picks, b)
            out["budgets"][t] = tsr.at_id_budget(n_valid, M, lse, sc)
        else:
            picks, out["margins"][t] = thr.argmax_rows(x, b)
            _, sc, M, lse = tsr.argmax_scores(x, b)
            out["budgets"][t] = tsr.fused_budget(n_valid, M, lse)
        out["picks"][t], out["scores"][t] = picks, sc
        save = thr.append_ids(save, picks, n)
        n += 1
        if trie is not None:
            for r in range(rows):
                ev, nxt = classify(trie, int(node[r]), int(picks[r]))
                if ev:
                    out["events"][ev] += 1
                    out["deep_restarts"] += int(ev == "restart" and int(trie["depth"][node[r]]) >= 2)
                node[r] = nxt
        out["nodes"][t] = node
    out["save"], out["n"] = save, n
    return out


# ------------------------------------------------------------------------------------------------ the ranker's merge
def _by_score_then_id(cands):
    return sorted(cands, key=lambda q: (-q[0], q[1]))


def rank_dense(row, trie, node, boost, K, bias=None):
    """The K best (score, id, log-prob + delta) over EVERY column of the f32 row (+ bias, f32): score key = x + delta, exact in float64 for inputs on a
    grid, so ties are decided by the id. A -inf column is no candidate. Also the smallest key gap between consecutive ranks 1 .. K + 1 whose deltas
    differ (inf when there is none): two f32 roundings separate such a pair on the device, so a tie between them is not bit-defined."""
    x = np.asarray(row, F32)
    if bias is not None:
        x = (x + np.asarray(bias, F32)).astype(F32)
    x64 = x.astype(np.float64)
    d = delta_dense(trie, node, boost, len(x))
    fin = np.nonzero(x64 > -np.inf)[0]
    lse = x64[fin].max() + np.log(np.exp(x64[fin] - x64[fin].max()).sum())
    cands = _by_score_then_id([(x64[c] + d[c], int(c)) for c in fin])[:K + 1]
    cross = np.inf
    for a, b in zip(cands[:-1], cands[1:]):
        if d[a[1]] != d[b[1]]:
            cross = min(cross, a[0] - b[0])
    best = [(key - lse, c) for key, c in cands[:K]]
    best += [(-np.inf, 0)] * (K - len(best))
    return np.array([v for v, _ in best]), np.array([c for _, c in best], np.int32), lse, cross


def rerank(row, trie, node, boost, K, bias=None):
    """The device's merge rule: plain top-K of the row (value descending, id ascending) u S, each scored log-prob + delta, the K best by (score, id).
    A top-K entry that is also in S counts once."""
    x = np.asarray(row, F32)
    if bias is not None:
        x = (x + np.asarray(bias, F32)).astype(F32)
    x64 = x.astype(np.float64)
    d = delta_dense(trie, node, boost, len(x))
    fin = np.nonzero(x64 > -np.inf)[0]
    lse = x64[fin].max() + np.log(np.exp(x64[fin] - x64[fin].max()).sum())
    top = [int(c) for c in thr.order(x)[:K] if x64[c] > -np.inf]
    S = [c for c in dict.fromkeys(children(trie, node) + children(trie, 0)) if c < len(x) and x64[c] > -np.inf]
    ids = list(dict.fromkeys(top + S))
    best = [(key - lse, c) for key, c in _by_score_then_id([(x64[c] + d[c], c) for c in ids])[:K]]
    best += [(-np.inf, 0)] * (K - len(best))
    return np.array([v for v, _ in best]), np.array([c for _, c in best], np.int32), lse


def rerank_budget(n_valid, row, lse, topv, boost, depth):
    """Bound on |topv_gpu - topv| after the re-rank: token_heads_ref.beam_topv_budget for (x - lse), plus one rounding of the delta add at the size of the sum."""
    row_max = np.asarray(row, np.float64)[np.isfinite(row)].max()
    return thr.beam_topv_budget(n_valid, row_max, lse, np.abs(topv) + (depth + 1) * abs(boost)) + thr.U32 * (np.abs(topv) + (depth + 1) * abs(boost))


def select_hot(trie, boost, beam, topv, topi, cum, fin, length, nxt, done, node, stop=(), first=False):
    """launch_beam_select's ranking on re-ranked pairs with the node hand-over, for one pass over [n_utt] utterances: -> (cum, fin, len, next, done, node,
    parent, tok) per row; tok -1 = nothing appended. Order: score descending, then hypothesis, then rank inside the hypothesis."""
    n_utt = len(done)
    o = dict(cum=np.array(cum, F32), fin=np.array(fin, np.int32), len=np.array(length, np.int32), next=np.array(nxt, np.int32), done=np.array(done, np.int32),
             node=np.array(node, np.int32), parent=np.zeros(n_utt * beam, np.int32), tok=np.full(n_utt * beam, -1, np.int32))
    for b in range(n_utt):
        base = b * beam
        frozen_utt = (not first) and done[b] != 0
        cands = []
        for r in range(beam if not first else 1):
            row = base + r
            if first:
                cands += [(F32(topv[b][k]), r, k, int(topi[b][k]), False) for k in range(beam)]
            elif frozen_utt or fin[row]:
                cands.append((F32(cum[row]), r, 0, None, True))
            else:
                cands += [(F32(F32(cum[row]) + F32(topv[row][k])), r, k, int(topi[row][k]), False) for k in range(beam)]
        cands = [q for q in cands if q[0] > -np.inf]
        if not frozen_utt:
            cands.sort(key=lambda q: (-float(q[0]), q[1], q[2]))
        for rank, (score, r, _, v, frozen) in enumerate(cands[:beam]):
            prow, orow = base + r, base + rank
            o["parent"][orow] = r
            o["cum"][orow] = score
            if frozen:
                o["fin"][orow], o["len"][orow], o["next"][orow], o["node"][orow] = fin[prow], length[prow], nxt[prow], node[prow]
            else:
                is_stop = v in set(int(s) for s in stop)
                o["fin"][orow], o["len"][orow], o["next"][orow] = int(is_stop), (0 if first else length[prow]) + (0 if is_stop else 1), v
                o["tok"][orow] = -1 if is_stop else v
                o["node"][orow] = trie_step(trie, 0 if first else int(node[prow]), 0.0, v, float(boost))[0]
        o["done"][b] = o["fin"][base]
    return o


# ------------------------------------------------------------------------------------------------ beam search
def beam_search_core_hot(first_logits, state0, step, beam, max_new, phrases, boost, stop_ids=(), margins=None):
    """oracle/qwen_asr_oracle.py:beam_search_core with hypothesis scores log-soft-max(model)(c) + delta(c): every hypothesis carries its trie node (the
    root at the first ranking), each live one offers its `beam` best extensions by log-prob + delta over all columns, a finished one stands as itself. A
    stop id pays the refund of a partial match like any other non-child; a hypothesis cut off at max_new keeps a pending bonus. Scores accumulate in f32
    as the device's do. -> best-first list of (token ids, score)."""
    from oracle.qwen_asr_oracle import log_softmax_f32
    trie = build_trie(phrases)
    stop = set(int(t) for t in stop_ids)

    def offers(logits, node):
        lp = log_softmax_f32(logits).astype(np.float64)
        sc = lp + delta_dense(trie, node, boost, lp.size)
        o = np.lexsort((np.arange(sc.size), -sc))[:beam + 1]
        return [(F32(sc[v]), int(v)) for v in o if sc[v] > -np.inf]

    off = offers(first_logits, 0)
    if margins is not None:
        margins.append(float(np.min(-np.diff([float(s) for s, _ in off]))))
    hyps = [dict(tokens=[] if v in stop else [v], last=v, score=s, fin=v in stop, state=state0, node=trie_step(trie, 0, 0.0, v, float(boost))[0]) for s, v in off[:beam]]
    for _ in range(max_new - 1):
        if hyps[0]["fin"]:
            break
        cands = []
        for r, h in enumerate(hyps):
            if h["fin"]:
                cands.append((h["score"], r, 0, None, None))
                continue
            logits, st = step(h["state"], h["last"])
            for k, (s, v) in enumerate(offers(logits, h["node"])[:beam]):
                cands.append((F32(h["score"] + s), r, k, v, st))
        cands.sort(key=lambda q: (-float(q[0]), q[1], q[2]))
        if margins is not None and len(cands) > 1:
            margins.append(float(np.min(-np.diff(np.asarray([float(q[0]) for q in cands[:beam + 1]])))))
        new = []
        for score, r, _, v, st in cands[:beam]:
            h = hyps[r]
            if v is None:
                new.append(h)
            else:
                new.append(dict(tokens=h["tokens"] + ([] if v in stop else [v]), last=v, score=score, fin=v in stop, state=st,
                                node=trie_step(trie, h["node"], 0.0, v, float(boost))[0]))
        hyps = new
    return [(np.asarray(h["tokens"], np.int32), float(h["score"])) for h in hyps]


def greedy_hot(first_logits, state0, step, max_new, phrases, boost):
    """Greedy decoding over a model's own logits with the float64 dense bias: -> (tokens, decision margins [max_new]: best minus runner-up of logits + delta)."""
    trie = build_trie(phrases) if len(phrases) else None
    logits, state, node = np.asarray(first_logits, np.float64), state0, 0
    toks, margins = [], []
    for t in range(max_new):
        v = logits + (delta_dense(trie, node, boost, logits.size) if trie is not None else 0.0)
        o = np.lexsort((np.arange(v.size), -v))[:2]
        toks.append(int(o[0]))
        margins.append(float(v[o[0]] - v[o[1]]))
        if trie is not None:
            node = trie_step(trie, node, 0.0, toks[-1], float(boost))[0]
        if t + 1 < max_new:
            lg, state = step(state, toks[-1])
            logits = np.asarray(lg, np.float64)
    return toks, margins


# ------------------------------------------------------------------------------------------------ seeded inputs of the GPU tests
STEPS = 24
ROWS = [1, 3, 64, 65]
WIDTHS = [5, 129, 4097]
WIDE = 51866
BOOST = F32(1.5)                       # on the 2^-10 grid, as the logits are: every sum is exact


def step_logits(seed, steps, rows, n):
    return np.stack([thr.grid_logits([seed, t, n], rows, n) for t in range(steps)])


def planted_phrases(x):
    """Phrase list for logits x [steps][rows][n]: phrases taken from ranks 0..2 of consecutive step rows of row 0 and the last row (so boosts flip picks
    and matches advance), plus the planted shapes: a one-token phrase, [a] beside [a, b], [a, b] beside [a, c], [a, b] beside [b, x] (b is a child and a
    root child), [a, a, a], and a -inf column's id (the caller masks it)."""
    steps, rows, n = x.shape
    rank = lambda t, r, k: int(thr.order(x[t, r])[min(k, n - 1)])
    ph = []
    for r in sorted({0, rows - 1}):
        for t in range(0, steps - 3, 3):
            ph.append([rank(t, r, 1), rank(t + 1, r, 1), rank(t + 2, r, 2)])
            ph.append([rank(t, r, 1), rank(t + 1, r, 2)])
            ph.append([rank(t + 1, r, 1), rank(t + 2, r, 0)])
    a, b, c, xx = rank(0, 0, 0), rank(1, 0, 1), rank(1, 0, 2), rank(2, 0, 1)
    ph += [[rank(3, 0, 2)], [a], [a, b], [a, c], [b, xx], [c, c, c]]
    return [p for p in ph if len(p)]


def wide_children(n, count=80):
    """More than 64 children at the root and under an inner node: ids spread over the row."""
    ids = [int(i) for i in np.linspace(0, n - 1, count).astype(int)]
    ids = list(dict.fromkeys(ids))
    hub = ids[0]
    return [[i] for i in ids[1:]] + [[hub, i] for i in ids]


from functools import lru_cache


@lru_cache(maxsize=None)
def head_inputs(rows, n, steps=STEPS):
    """(logits [steps][rows][n], phrases, step-0 bias): grid logits, the planted phrase list (+ the wide child lists from 129 columns on), and boosted
    columns at -inf: the first phrase's first token through the step-0 bias, two more in the logits of steps 5 and 6."""
    x = step_logits(77, steps, rows, n)
    ph = planted_phrases(x) + (wide_children(n) if n >= 129 else [])
    bias = np.zeros(n, F32)
    bias[ph[0][0]] = -np.inf
    x[min(5, steps - 2), :, ph[1][0]] = -np.inf
    x[min(6, steps - 1), :, ph[0][1]] = -np.inf
    x.setflags(write=False)
    return x, ph, bias


SAMPLER = (0.7, 10, 0.95, 1.3, 20240913)
HEAD_SETTINGS = {
    "arg-max": dict(),
    "penalty, partial 0": dict(value=0.8, partial=0),
    "penalty, partial 1": dict(value=0.8, partial=1),
    "sampler": dict(sampler=SAMPLER, partial=1),
    "scores": dict(),
}
HEAD_SHAPES = [(3, 129), (65, 4097)]           # the shapes every head setting runs at; arg-max runs at ROWS x WIDTHS


def sampler_noise(rows, n, steps=STEPS):
    return np.random.default_rng([rows, n, 29]).uniform(0.0, 1.0, (steps, rows, min(SAMPLER[1], n))).astype(F32)


def sampler_setting(n):
    return (SAMPLER[0], min(SAMPLER[1], n), SAMPLER[2], SAMPLER[3], SAMPLER[4])


def decided_prefix(decided):
    """[steps][rows] -> per row the number of leading steps whose picks the margins decide (a row is compared up to there: past an undecided pick its
    history and node may differ), and the share of (step, row) entries left out."""
    steps, rows = decided.shape
    upto = np.array([int(np.argmin(decided[:, r])) if not decided[:, r].all() else steps for r in range(rows)])
    return upto, float((steps - upto).sum()) / (steps * rows)


TS_GEOMS = [(129, 90, 100), (4100, 4000, 4096)]       # (n_valid, eot, ts_begin), as whisper_timestamps_ref.GEOMETRIES


@lru_cache(maxsize=None)
def ts_inputs(geom, rows=3, steps=12):
    """Timestamp mode: grid logits with the timestamp columns lifted so that text and timestamps alternate, phrases over text and timestamp ids."""
    n, eot, ts_begin = geom
    x = step_logits(91, steps, rows, n)
    x[1::3, :, ts_begin:] += F32(6.0)
    ph = planted_phrases(x) + [[ts_begin + 3], [int(thr.order(x[1, 0, :eot])[0]), int(thr.order(x[2, 0, :eot])[1])]]
    x.setflags(write=False)
    return x, ph


@lru_cache(maxsize=None)
def rank_inputs(beam, n, first, n_utt=3, tab_ld=12, n_slots=5):
    """One ranking pass: logits, phrases, search state with inner nodes, a finished hypothesis (utterance 1, its second row when beam > 1), a frozen
    utterance (the last), a stop id that row 0 picks inside a partial match, and -- on the first pass -- BEGIN_SUPPRESS on a boosted column."""
    rng = np.random.default_rng([beam, n, int(first), 5])
    N = n_utt * beam
    R = n_utt if first else N
    x = thr.grid_logits([beam, n, int(first), 31], R, n)
    top = [[int(c) for c in thr.order(x[r])[:4]] for r in range(R)]
    ph = [[top[r][1]] for r in range(R)] + [[top[r][2], top[(r + 1) % R][1]] for r in range(R)] + [[top[0][3], top[0][2], top[0][1]]]
    ph += wide_children(n, 70) if n >= 129 else []
    trie = build_trie(ph)
    n_nodes = len(trie["depth"])
    inner = [q for q in range(1, n_nodes) if trie["child_off"][q + 1] > trie["child_off"][q]] or [0]
    node = np.array([inner[int(rng.integers(len(inner)))] if rng.random() < 0.7 else 0 for _ in range(N)], np.int32)
    if first:
        node[:] = 0
    cum = (np.round(rng.normal(-4.0, 2.0, N) / thr.GRID) * thr.GRID).astype(F32)
    fin, done = np.zeros(N, np.int32), np.zeros(n_utt, np.int32)
    length = rng.integers(2, n_slots, N).astype(np.int32)
    nxt = rng.integers(0, n, N).astype(np.int32)
    src = rng.integers(0, beam, (N, tab_ld)).astype(np.int32) + (np.arange(N)[:, None] // beam) * beam
    tok = rng.integers(0, n, (N, tab_ld)).astype(np.int32)
    bias = None
    if first:
        cum[:], length[:], n_slots = 0, 0, 0
        bias = np.zeros(n, F32)
        bias[top[0][1]] = -np.inf                   # a root child that the boost would lift: BEGIN_SUPPRESS keeps it out
    else:
        if beam > 1:
            fin[1 * beam + 1] = 1
            cum[1 * beam + 1] = F32(-1.0)
        done[n_utt - 1] = 1
        fin[(n_utt - 1) * beam] = 1
        from ctc_beam_ref import _child
        node[0] = _child(trie, _child(trie, 0, top[0][3]), top[0][2])     # row 0 sits two tokens inside a phrase and its best column is a stop id
        x[0, top[0][0]] += F32(8.0)                 # ... by enough to stay row 0's best extension after the refund, and row 0 leads its utterance
        cum[0] = F32(2.0)
    stop = (top[0][0],) if not first else (top[1][0],)
    return dict(x=x, phrases=ph, bias=bias, node=node, cum=cum, fin=fin, done=done, len=length, next=nxt, src=src, tok=tok, stop=stop, n_slots=n_slots, tab_ld=tab_ld)


def rank_reference(c, beam, first):
    """The pass on rank_inputs' case: per-row merge (rerank) -> select_hot. Also per row the dense ranking, the cross-delta gap and the select's smallest
    score gap among its first beam + 1 candidates."""
    trie = build_trie(c["phrases"])
    R = len(c["x"])
    topv, topi, lses, dense_ok, cross = [], [], [], True, np.inf
    for r in range(R):
        nd = 0 if first else int(c["node"][r])
        v, i, lse = rerank(c["x"][r], trie, nd, BOOST, beam, c["bias"])
        dv, di, _, cr = rank_dense(c["x"][r], trie, nd, BOOST, beam, c["bias"])
        dense_ok &= np.array_equal(i, di) and np.allclose(v, dv, rtol=0, atol=1e-12, equal_nan=True)
        cross = min(cross, cr)
        topv.append(v); topi.append(i); lses.append(lse)
    topv, topi = np.array(topv), np.array(topi)
    sel = select_hot(trie, BOOST, beam, topv.astype(F32), topi, c["cum"], c["fin"], c["len"], c["next"], c["done"], c["node"], stop=c["stop"], first=first)
    return dict(topv=topv, topi=topi, lse=np.array(lses), sel=sel, dense_ok=dense_ok, cross=cross, trie=trie)


# ------------------------------------------------------------------------------------------------ the CPU oracles' decoders under hotwords (session tests)
def whisper_runs(orc, audio, prompt):
    """(first logits + BEGIN_SUPPRESS, state0, step) of WhisperOracle for one clip, as tests/whisper_beam_ref.py drives it."""
    import torch
    with torch.inference_mode():
        ck, cv = (t.unsqueeze(0) for t in orc.encode(audio))
        logits, sk, sv = orc.decoder(torch.tensor([list(prompt)], dtype=torch.long), 0, None, None, ck, cv)
        first = (logits[0] + orc._c(orc.begin_bias)).float().numpy()

    def step(state, tok):
        hist, k, v = state
        with torch.inference_mode():
            lg, nk, nv = orc.decoder(torch.tensor([[int(tok)]], dtype=torch.long), hist, k, v, ck, cv)
        return lg[0].float().numpy(), (hist + 1, nk, nv)

    return first, (len(prompt), sk, sv), step


def qwen_runs(orc, audio, query_ids=(), language_tail_ids=()):
    """The same for QwenAsrOracle (no bias on the prefill step)."""
    import torch
    with torch.inference_mode():
        x = orc.prompt(orc.encode(audio), query_ids, language_tail_ids)
        logits, ks, vs = orc.decoder(x, 0, None, None)

    def step(state, tok):
        hist, k, v = state
        with torch.inference_mode():
            lg, k2, v2 = orc.decoder(orc.embed([int(tok)]), hist, k, v)
        return lg.numpy(), (hist + 1, k2, v2)

    return logits.numpy(), (x.shape[0], ks, vs), step


def runner_up_phrases(runs, max_new):
    """Phrases from the unbiased greedy walks of `runs` [(first, state0, step)]: per clip the runner-up of step 1 alone, and the runner-ups of steps 2 and 3
    of the walk that took step 2's runner-up as a pair -- a boost flips those picks and the pair is matched or abandoned."""
    ph = []
    for first, state, step in runs:
        logits, toks = np.asarray(first, np.float64), []
        for t in range(min(max_new, 4)):
            o = np.lexsort((np.arange(logits.size), -logits))[:2]
            if t == 1:
                ph.append([int(o[1])])
            take = int(o[1]) if t == 2 else int(o[0])
            if t == 3:
                ph.append([toks[-1], int(o[1])])
            toks.append(take)
            lg, state = step(state, take)
            logits = np.asarray(lg, np.float64)
    return ph
