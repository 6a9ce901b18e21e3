"""Float64 numpy statement of n-gram LM shallow fusion in the autoregressive decoders (csrc/decoder_lm.hip, csrc/decode_head.h), not circular:
the image and its walk are tests/ctc_lm_ref.py's (build_image, view, lm_step), the trie and the heads tests/hotword_heads_ref.py's and token_heads_ref.py's.

Every sequence of the greedy head and every hypothesis of the beam search carries an LM state, a node of the image: start_node after a prefill.
LM term of token c from state s (`lm_term`):
    c one of end_ids and the image lists </s>    alpha * lm_step(s, </s>), no beta, the state stays
    otherwise                                    (lp, s') = lm_step(s, c); alpha * lp + beta (a token without a unigram costs oov and keeps the state)
Candidates (`candidates`): the M = topk best columns of the row as the selection sees it (after the penalty, the hotword bias, the timestamp rules, with
BEGIN_SUPPRESS added), by value descending then id ascending; a -inf column is none; tokens outside the top M are not considered.
Greedy head: the candidate with the largest x + term, ties to the lower id; the state follows the pick; a token score stays the model's log-soft-max of the
row at the pick. The sampling head ignores the model.
Beam ranker: a hypothesis gains (x - lse) + delta_hot + term per token; the candidate set of a row is topM u S, S the trie's node children and root children
(hotword_heads_ref.rerank's set, empty without hotwords); the `beam` best by (score descending, id ascending).

Inputs of the kernel tests are on grids (logits 2^-10, model 2^-6, alpha 0.5), so x + term is exact in f32 and in float64 and ties are real."""
from functools import lru_cache

import numpy as np

import ctc_lm_ref as clr
import hotword_heads_ref as hw
import token_heads_ref as thr
import token_scores_ref as tsr
from ctc_beam_ref import build_trie, trie_step

F32 = np.float32
TOPK_MAX, ENDS_MAX = 32, 8


def model(image, alpha, beta, oov=0.0, topk=16, end_ids=()):
    """The model as every function here (and _probe's lm= argument) takes it."""
    image = np.asarray(image, np.int32)
    return dict(image=image, view=clr.view(image), alpha=float(alpha), beta=float(beta), oov=float(oov), topk=int(topk), end_ids=tuple(int(e) for e in end_ids))


def lm_term(lm, state, c):
    """(the LM term of token c from `state`, the state after it)."""
    v = lm["view"]
    if int(c) in lm["end_ids"] and v["eos"] >= 0:
        return lm["alpha"] * float(clr.lm_step(v, state, v["eos"], lm["oov"])[0]), state
    lp, nxt = clr.lm_step(v, state, int(c), lm["oov"])
    return lm["alpha"] * float(lp) + lm["beta"], nxt


def candidates(x, M):
    """ids of the M best finite columns of the f32 row x, value descending then id ascending."""
    x = np.asarray(x, F32)
    return [int(c) for c in thr.order(x)[:M] if x[c] > -np.inf]


def pick(x, lm, state):
    """The fused greedy pick on the f32 row x (bias added): -> (id, state after, fused keys of the candidates best first as [(key, id)]). No candidate: id 0,
    the state as it stands."""
    x64 = np.asarray(x, F32).astype(np.float64)
    keyed = []
    for c in candidates(x, lm["topk"]):
        t, nxt = lm_term(lm, state, c)
        keyed.append((x64[c] + t, c, nxt))
    keyed.sort(key=lambda q: (-q[0], q[1]))
    if not keyed:
        return 0, state, []
    return keyed[0][1], keyed[0][2], [(k, c) for k, c, _ in keyed]


def pick_margin(x, lm, keyed, state):
    """How far the pick is from changing: the fused gap to the runner-up, and the top-M boundary -- when the M-th and the (M + 1)-th raw values are close the
    candidate set itself is not decided, which matters if the (M + 1)-th would win or the M-th is the winner."""
    x = np.asarray(x, F32)
    gap = keyed[0][0] - keyed[1][0] if len(keyed) > 1 else np.inf
    o = [int(c) for c in thr.order(x)[:lm["topk"] + 1] if x[c] > -np.inf]
    if len(o) <= lm["topk"]:
        return gap
    inside, outside = o[lm["topk"] - 1], o[lm["topk"]]
    edge = float(x[inside]) - float(x[outside])
    best_outside = float(x[outside]) + lm_term(lm, state, outside)[0]
    if keyed[0][1] != inside:
        edge = max(edge, keyed[0][0] - best_outside)
    return min(gap, edge)


# ------------------------------------------------------------------------------------------------ the head over several steps
def head_steps_lm(logits, phrases, boost, ld_save, lm, range_=4, value=1.0, partial=0, bias=None, sampler=None, noise=None, timestamps=None):
    """hotword_heads_ref.head_steps_hot with the model: penalty -> hotword bias -> timestamp rules -> the fused pick (the sampler ignores the model) -> append;
    node and state follow the pick. -> its dict plus "states" [steps][rows] (after the step)."""
    logits = np.asarray(logits, F32)
    steps, rows, n_valid = logits.shape
    trie = build_trie(phrases) if len(phrases) else None
    save, n = np.zeros((rows, ld_save), np.int32), 0
    node = np.zeros(rows, np.int64)
    state = np.full(rows, lm["view"]["start_node"], np.int64)
    out = dict(picks=np.zeros((steps, rows), np.int32), nodes=np.zeros((steps, rows), np.int32), states=np.zeros((steps, rows), np.int32),
               decided=np.ones((steps, rows), bool), scores=np.zeros((steps, rows)), budgets=np.zeros((steps, rows)), rows_seen=np.zeros((steps, rows, n_valid), F32))
    for t in range(steps):
        penalised = value != 1.0 and sampler is None
        x = thr.apply_penalty(logits[t], save, n, range_, value, partial) if penalised and t > 0 else logits[t].copy()
        if trie is not None:
            x = np.stack([hw.bias_sparse(x[r], trie, int(node[r]), boost) for r in range(rows)])
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
        else:
            v = tsr.seen(x, b)
            picks = np.zeros(rows, np.int32)
            for r in range(rows):
                picks[r], state[r], _ = pick(v[r], lm, int(state[r]))
        sc, M, lse = tsr.scores_at(x, picks, b)
        out["budgets"][t] = tsr.at_id_budget(n_valid, M, lse, sc)
        out["picks"][t], out["scores"][t] = picks, sc
        save = thr.append_ids(save, picks, n)
        n += 1
        if trie is not None:
            for r in range(rows):
                node[r] = hw.classify(trie, int(node[r]), int(picks[r]))[1]
        out["nodes"][t], out["states"][t] = node, state
    out["save"], out["n"] = save, n
    return out


# ------------------------------------------------------------------------------------------------ the ranker's merge
def _delta(trie, node, boost, n):
    return hw.delta_dense(trie, node, boost, n) if trie is not None else np.zeros(n)


def _ranked(x64, d, lm, state, ids, K):
    """The K + 1 best of `ids` by (x + delta + term, id): [(key, id, delta + term)]."""
    c = []
    for i in ids:
        t = lm_term(lm, state, i)[0]
        c.append((x64[i] + d[i] + t, int(i), d[i] + t))
    return sorted(c, key=lambda q: (-q[0], q[1]))[:K + 1]


def _row(row, bias):
    x = np.asarray(row, F32)
    if bias is not None:
        x = (x + np.asarray(bias, F32)).astype(F32)
    x64 = x.astype(np.float64)
    fin = np.nonzero(x64 > -np.inf)[0]
    lse = x64[fin].max() + np.log(np.exp(x64[fin] - x64[fin].max()).sum()) if len(fin) else -np.inf
    return x, x64, fin, lse


def _topv(best, lse, K):
    out = [(key - lse, c) for key, c, _ in best[:K]]
    out += [(-np.inf, 0)] * (K - len(out))
    return np.array([v for v, _ in out]), np.array([c for _, c in out], np.int32)


def rank_dense_lm(row, trie, node, boost, lm, state, K, bias=None):
    """The K best over EVERY column by x + delta + term (what the top-M rule gives up: see the CPU test for when the two agree)."""
    x, x64, fin, lse = _row(row, bias)
    best = _ranked(x64, _delta(trie, node, boost, len(x)), lm, state, fin, K)
    return _topv(best, lse, K) + (lse,)


def rerank_lm(row, trie, node, boost, lm, state, K, bias=None):
    """The device's rule: topM u S, each scored (x - lse) + delta + term, the K best by (score, id). Also `cross`: the smallest key gap between consecutive
    ranks 1 .. K + 1 whose delta + term differ (hotword_heads_ref.rank_dense's rule: f32 roundings separate such a pair on the device)."""
    x, x64, fin, lse = _row(row, bias)
    S = []
    if trie is not None:
        S = [c for c in dict.fromkeys(hw.children(trie, node) + hw.children(trie, 0)) if c < len(x) and x64[c] > -np.inf]
    ids = list(dict.fromkeys(candidates(x, lm["topk"]) + S))
    best = _ranked(x64, _delta(trie, node, boost, len(x)), lm, state, ids, K)
    cross = np.inf
    for a, b in zip(best[:-1], best[1:]):
        if a[2] != b[2]:
            cross = min(cross, a[0] - b[0])
    topv, topi = _topv(best, lse, K)
    return topv, topi, lse, cross


def rerank_budget_lm(n_valid, row, lse, topv, boost, depth, lm):
    """hotword_heads_ref.rerank_budget plus one rounding for the term's add, at the size of the sum."""
    return hw.rerank_budget(n_valid, row, lse, topv, boost, depth) + thr.U32 * np.abs(topv)


def select_lm(trie, boost, beam, topv, topi, cum, fin, length, nxt, done, node, state, lm, stop=(), first=False):
    """hotword_heads_ref.select_hot with the state hand-over: a kept row inherits its parent's state advanced by its token, frozen rows keep theirs."""
    o = hw.select_hot(trie, boost, beam, topv, topi, cum, fin, length, nxt, done, node, stop=stop, first=first)
    o["state"] = np.array(state, np.int32)
    for b in range(len(done)):
        base = b * beam
        frozen_utt = (not first) and done[b] != 0
        for rank in range(beam):
            prow = base + int(o["parent"][base + rank])
            if frozen_utt or ((not first) and fin[prow]):
                o["state"][base + rank] = state[prow]
            else:
                o["state"][base + rank] = lm_term(lm, lm["view"]["start_node"] if first else int(state[prow]), int(o["next"][base + rank]))[1]
    return o


# ------------------------------------------------------------------------------------------------ beam search, greedy decoding (CPU and session tests)
def beam_search_core_lm(first_logits, state0, step, beam, max_new, phrases, boost, lm, stop_ids=(), margins=None, dense=False, with_fin=False):
    """hotword_heads_ref.beam_search_core_hot with the model: every hypothesis carries its trie node and its LM state; a live one offers its `beam` best
    extensions of topM u S (every column with dense=True) by log-soft-max + delta + term. margins (a list): per ranking the smallest score gap among the
    first beam + 1 candidates -- and 0 where a row's top-M boundary is not decided and the column outside could reach the offers.
    -> best-first list of (token ids, score); with_fin: (token ids, score, whether the hypothesis took a stop id)."""
    from oracle.qwen_asr_oracle import log_softmax_f32
    trie = build_trie(phrases) if len(phrases) else None
    stop = set(int(t) for t in stop_ids)
    start = lm["view"]["start_node"]

    def offers(logits, node, state):
        x = np.asarray(logits, F32)
        lp = log_softmax_f32(x).astype(np.float64)
        d = _delta(trie, node, boost, lp.size)
        if dense:
            ids = [int(c) for c in np.nonzero(lp > -np.inf)[0]]
        else:
            S = [c for c in dict.fromkeys(hw.children(trie, node) + hw.children(trie, 0)) if c < lp.size and lp[c] > -np.inf] if trie is not None else []
            ids = list(dict.fromkeys(candidates(x, lm["topk"]) + S))
        best = _ranked(lp, d, lm, state, ids, beam)
        if margins is not None and not dense:
            o = [int(c) for c in thr.order(x)[:lm["topk"] + 1] if x[c] > -np.inf]
            if len(o) > lm["topk"] and float(x[o[-2]]) - float(x[o[-1]]) <= 1e-2:
                reach = lp[o[-1]] + d[o[-1]] + lm_term(lm, state, o[-1])[0]
                if len(best) <= beam or reach >= best[beam][0] - 1e-2 or o[-2] in [c for _, c, _ in best]:
                    margins.append(0.0)
        return [(F32(k), c) for k, c, _ in best]

    def advance(node, state, v):
        return trie_step(trie, node, 0.0, v, float(boost))[0], lm_term(lm, state, v)[1]

    off = offers(first_logits, 0, start)
    if margins is not None and len(off) > 1:
        margins.append(float(np.min(-np.diff([float(s) for s, _ in off]))))
    hyps = []
    for s, v in off[:beam]:
        nd, st = advance(0, start, v)
        hyps.append(dict(tokens=[] if v in stop else [v], last=v, score=s, fin=v in stop, state=state0, node=nd, lm=st))
    for _ in range(max_new - 1):
        if hyps[0]["fin"]:
            break
        cands = []
        for r, h in enumerate(hyps):
            if h["fin"]:
                cands.append((h["score"], r, 0, None, None))
                continue
            logits, st = step(h["state"], h["last"])
            for k, (s, v) in enumerate(offers(logits, h["node"], h["lm"])[:beam]):
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
                nd, ls = advance(h["node"], h["lm"], v)
                new.append(dict(tokens=h["tokens"] + ([] if v in stop else [v]), last=v, score=score, fin=v in stop, state=st, node=nd, lm=ls))
        hyps = new
    return [(np.asarray(h["tokens"], np.int32), float(h["score"])) + ((bool(h["fin"]),) if with_fin else ()) for h in hyps]


def greedy_lm(first_logits, state0, step, max_new, phrases, boost, lm):
    """Greedy decoding over a model's own logits with the float64 dense hotword bias and the fused pick -> (tokens, margins [max_new]: pick_margin)."""
    trie = build_trie(phrases) if len(phrases) else None
    logits, dec, node, state = np.asarray(first_logits, np.float64), state0, 0, lm["view"]["start_node"]
    toks, margins = [], []
    for t in range(max_new):
        v = (logits + (_delta(trie, node, boost, logits.size))).astype(np.float64)
        x = v.astype(F32)                  # (candidates are taken from the f32 row; the keys below use the float64 values)
        keyed = []
        for c in candidates(x, lm["topk"]):
            term, nxt = lm_term(lm, state, c)
            keyed.append((v[c] + term, c, nxt))
        keyed.sort(key=lambda q: (-q[0], q[1]))
        toks.append(keyed[0][1])
        margins.append(float(pick_margin(x, lm, [(k, c) for k, c, _ in keyed], state)))
        state = keyed[0][2]
        node = trie_step(trie, node, 0.0, toks[-1], float(boost))[0]
        if t + 1 < max_new:
            lg, dec = step(dec, toks[-1])
            logits = np.asarray(lg, np.float64)
    return toks, margins


# ------------------------------------------------------------------------------------------------ seeded inputs of the tests
LM_GRID = 2.0 ** -6
ALPHA, BETA, TOPK = 0.5, 0.75, 16


def grid_ngrams(seed, vocab, order, words, keep=0.5, eos=True, bos=True, per_context=6):
    """A pruned random model over the tokens `words` (the rest of the vocabulary has no unigram), log-probabilities in [-4, 0) and back-offs in [-1, 1) on
    the 2^-6 grid: with alpha 0.5 every term is a multiple of 2^-7 and every sum along a back-off chain is exact."""
    rng = np.random.default_rng([seed, vocab, order])
    E, B = vocab, vocab + 1
    g = lambda lo, hi: float(np.round(rng.uniform(lo, hi) / LM_GRID) * LM_GRID)
    words = [int(w) for w in words]
    ngrams = {}
    level = [(w,) for w in words] + ([(E,)] if eos else []) + ([(B,)] if bos else [])
    for n in range(1, order + 1):
        for gram in level:
            lp = 0.0 if gram == (B,) else min(g(-4.0, 0.0), 0.0)
            bo = g(-1.0, 1.0) if n < order and gram[-1] != E else 0.0
            ngrams[gram] = (lp, bo)
        if n == order:
            break
        conts = words + ([E] if eos else [])
        nxt = []
        ctxs = [gram for gram in level if gram[-1] != E]
        if len(ctxs) > 400:
            ctxs = [ctxs[i] for i in rng.choice(len(ctxs), 400, replace=False)]
        for gram in ctxs:
            take = rng.choice(len(conts), min(per_context, len(conts)), replace=False)
            nxt.extend(gram + (conts[i],) for i in sorted(take))
        level = nxt
    return ngrams


def words_for(x, share=0.6, seed=3):
    """The tokens with a unigram for logits x [steps][rows][n]: a random share of the vocabulary plus the 24 best columns of every (step, row) but every
    fifth of those (so the candidates mix known and out-of-vocabulary tokens, and the model can flip picks)."""
    n = x.shape[-1]
    rng = np.random.default_rng([seed, n])
    known = set(int(c) for c in np.nonzero(rng.random(n) < share)[0])
    flat = x.reshape(-1, n)
    for r in range(len(flat)):
        top = thr.order(flat[r])[:24]
        for k, c in enumerate(top):
            (known.discard if k % 5 == 4 else known.add)(int(c))
    return sorted(known)


def _model_from(x, seed, topk):
    """A model for step logits x [steps][rows][n]: order 3 with <s> and </s>, part of the vocabulary without a unigram, contexts planted along the best
    columns of consecutive steps so that trigrams and bigrams are found, and an end id: the second-best column of step 2, row 0."""
    steps, rows, n = x.shape
    words = words_for(x)
    ng = grid_ngrams(seed, n, 3, words, per_context=4 if n > 5000 else 6)
    rng = np.random.default_rng([rows, n, 17])
    g = lambda lo, hi: float(np.round(rng.uniform(lo, hi) / LM_GRID) * LM_GRID)
    known = set(words)
    for r in sorted({0, rows - 1}):                      # planted continuations: ranks 0..3 of step t after ranks 0..1 of steps t - 2, t - 1
        for t in range(1, steps):
            for a in thr.order(x[t - 1, r])[:2]:
                for c in thr.order(x[t, r])[:4]:
                    if int(a) in known and int(c) in known:
                        ng.setdefault((int(a), int(c)), (min(g(-4.0, 0.0), 0.0), g(-1.0, 1.0)))
                        if t >= 2:
                            z = int(thr.order(x[t - 2, r])[0])
                            if z in known and (z, int(a)) in ng:
                                ng.setdefault((z, int(a), int(c)), (min(g(-4.0, 0.0), 0.0), 0.0))
    end = int(thr.order(x[min(2, steps - 1), 0])[1])
    return model(clr.build_image(ng, n), ALPHA, BETA, oov=-2.0, topk=topk, end_ids=(end,))


@lru_cache(maxsize=None)
def head_model(rows, n, steps=hw.STEPS, topk=TOPK):
    """The model of the head tests at hotword_heads_ref.head_inputs(rows, n, steps)."""
    return _model_from(hw.head_inputs(rows, n, steps)[0], 11, topk)


@lru_cache(maxsize=None)
def ts_model(geom):
    """... and at hotword_heads_ref.ts_inputs(geom): text and timestamp ids both occur with and without a unigram."""
    return _model_from(hw.ts_inputs(geom)[0], 12, TOPK)


def plant_ties(x, lm, bias=None, phrases=()):
    """A copy of step logits x with two exact ties of the fused key at the top of every row: at step 0 (every row is at start_node) two tokens a < b with a
    unigram and different terms, b the larger raw value -- x[b] = TOP, x[a] = TOP + term(b) - term(a) -- and at step 3 two tokens without a unigram at one
    value (their term is oov whatever the state). Hotwords must not part a pair: a and b are both children of the root or neither, c and d occur in no
    phrase. The lower id must win both. -> (x, (a, b), (c, d)), a pair None where the vocabulary has none."""
    x = np.array(x, F32)
    steps, rows, n = x.shape
    v, start = lm["view"], lm["view"]["start_node"]
    blocked = set(np.nonzero(np.asarray(bias) == -np.inf)[0].tolist()) if bias is not None else set()
    roots, used = set(int(p[0]) for p in phrases), set(int(t) for p in phrases for t in p)
    known = [c for c in range(n) if v["uni"][c] >= 0 and c not in lm["end_ids"] and c not in blocked]
    unknown = [c for c in range(n) if v["uni"][c] < 0 and c not in blocked and c not in used]
    pair = None
    for i, a in enumerate(known[:40]):
        for b in known[i + 1:41]:
            if (a in roots) == (b in roots) and lm_term(lm, start, a)[0] > lm_term(lm, start, b)[0]:
                pair = (a, b)
                break
        if pair:
            break
    TOP = F32(24.0)
    if pair:
        a, b = pair
        x[0, :, b] = TOP
        x[0, :, a] = F32(TOP + F32(lm_term(lm, start, b)[0] - lm_term(lm, start, a)[0]))
    oov = tuple(unknown[:2]) if len(unknown) >= 2 and steps > 3 else None
    if oov:
        x[3, :, list(oov)] = TOP
    return x, pair, oov


RANK_SEEDS = {(8, 4097, True, False): 1}                        # (beam, n, first, hot) -> model seed, where seed 0 leaves a row undecided (chosen on the CPU: test_decoder_lm_ref_cpu.py)


@lru_cache(maxsize=None)
def rank_model(beam, n, first, hot, topk=TOPK, seed=None):
    """The model of a ranking pass at hotword_heads_ref.rank_inputs(beam, n, first) and the rows' states: inner states for most rows, an end id among the
    best columns of the last live row."""
    c = hw.rank_inputs(beam, n, first)
    x = c["x"]
    seed = RANK_SEEDS.get((beam, n, bool(first), bool(hot)), 0) if seed is None else seed
    words = words_for(x[None], seed=5)
    ng = grid_ngrams(13 + int(hot) + 100 * seed, n, 3, words, per_context=4 if n > 5000 else 6)
    lm = model(clr.build_image(ng, n), ALPHA, BETA, oov=-2.0, topk=max(topk, beam), end_ids=(int(thr.order(x[len(x) - 1])[1]),))
    rng = np.random.default_rng([beam, n, int(first), int(hot), 23])
    N = len(c["node"])
    state = rng.integers(0, lm["view"]["n_nodes"], N).astype(np.int32)
    state[rng.random(N) < 0.2] = lm["view"]["start_node"]
    return lm, state


def rank_reference_lm(c, beam, first, lm, state, hot=True):
    """The pass on rank_inputs' case with the model: per-row merge (rerank_lm) -> select_lm; also per row the cross gap."""
    trie = build_trie(c["phrases"]) if hot else None
    R = len(c["x"])
    start = lm["view"]["start_node"]
    topv, topi, lses, cross = [], [], [], []
    for r in range(R):
        nd = 0 if first or not hot else int(c["node"][r])
        v, i, lse, cr = rerank_lm(c["x"][r], trie, nd, hw.BOOST, lm, start if first else int(state[r]), beam, c["bias"])
        cross.append(cr)
        topv.append(v); topi.append(i); lses.append(lse)
    topv, topi = np.array(topv), np.array(topi)
    sel_trie = trie if hot else build_trie([[0]])
    sel = select_lm(sel_trie, hw.BOOST if hot else 0.0, beam, topv.astype(F32), topi, c["cum"], c["fin"], c["len"], c["next"], c["done"], c["node"] if hot else np.zeros_like(c["node"]), state, lm,
                    stop=c["stop"], first=first)
    return dict(topv=topv, topi=topi, lse=np.array(lses), sel=sel, cross=np.array(cross), trie=trie)
