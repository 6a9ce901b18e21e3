"""Float64 numpy statement of the beam search over the token rows of a non-autoregressive decoder (csrc/nar_beam.hip: nar_beam_kernel), with the
hotword context graph of ctc_beam_ref and the back-off n-gram model of ctc_lm_ref. Not circular, and not a CTC search: no blank, no collapse, no merging.

Every hypothesis picks exactly one candidate per row, so all hypotheses have N tokens (N = the number of rows) and hypotheses with different picks differ in
content. Row k, live hypotheses in rank order, candidates in column order: entry e = p * topk + j extends hypothesis p by candidate j; a candidate with
lp = -inf makes no entry. An entry carries
  am' = am[p] + lp[k][j]
  (node', bonus') = trie_step(node[p], bonus[p], token)
  lm' = lm[p] + (alpha * log P(token | state[p]) + beta)       (with a model; an out-of-vocabulary token costs oov and keeps the state)
  key = (am' + bonus') + lm'
in this order of operations (every sum and product rounded to `dtype`: with dtype=np.float32 this is the kernel's arithmetic). The best min(beam, entries)
survive by key descending, ties to the lower e; their rank is their index at the next row. After the last row a hypothesis inside a phrase gives
depth(node) * boost back, with a model that lists </s> it adds alpha * log P(</s> | state), the hypotheses are ranked again by (am + bonus) + lm (stable)
and the best nbest are returned. No rows: the one empty hypothesis, score 0 (+ the </s> term), am_score 0.

`gap` is the smallest score difference a decision rested on: the last kept against the first dropped entry at every row, and neighbouring hypotheses of the
final ranking. Without hotwords and without a model the acoustic term is a sum of independent rows, so the search is exact for the nbest best pick
sequences whenever beam >= nbest: brute_force enumerates them."""
import functools
import itertools

import numpy as np

from ctc_beam_ref import build_trie, random_phrases, trie_step
from ctc_lm_ref import ALPHA, BETA, BOOST, GAP, OOV, ORDERS, lm_step, score_tokens, shape_model, view


def nar_beam(cand_id, cand_lp, beam, nbest, trie=None, boost=0.0, image=None, alpha=0.0, beta=0.0, oov=0.0, dtype=np.float64):
    """cand_id / cand_lp [N, k] (ids distinct inside a row). Returns (hyps, gap): hyps = [{"tokens", "score", "am_score", "logprob", "lm"}] best first."""
    ft = dtype
    cand_id, cand_lp = np.asarray(cand_id), np.asarray(cand_lp).astype(ft)
    assert cand_id.ndim == 2 and cand_id.shape == cand_lp.shape
    N, k = cand_id.shape
    v = view(image) if image is not None else None
    boost, alpha, beta = ft(boost), ft(alpha), ft(beta)
    # a live hypothesis: (am, node, bonus, lm, state, picks) -- picks the list of (token, lp)
    live, gap = [(ft(0.0), 0, ft(0.0), ft(0.0), v["start_node"] if v else 0, [])], np.inf
    for t in range(N):
        ids, lps = [int(c) for c in cand_id[t]], cand_lp[t]
        assert len(set(ids)) == k, "candidate ids of a row must be distinct"
        entries = []
        for am, node, bonus, lm, state, picks in live:
            for c, lp in zip(ids, lps):
                if not lp > -np.inf:
                    continue
                am2 = ft(am + lp)
                node2, bonus2 = trie_step(trie, node, bonus, c, boost)
                key, lm2, state2 = ft(am2 + bonus2), lm, state
                if v is not None:
                    step, state2 = lm_step(v, state, c, oov, ft)
                    lm2 = ft(lm + ft(ft(alpha * step) + beta))
                    key = ft(key + lm2)
                entries.append((key, am2, node2, ft(bonus2), lm2, state2, picks + [(c, lp)]))
        assert entries, f"row {t}: no candidate with a finite log-probability"
        order = sorted(range(len(entries)), key=lambda i: -entries[i][0])          # stable: ties to the earlier entry
        if len(order) > beam:
            gap = min(gap, float(entries[order[beam - 1]][0] - entries[order[beam]][0]))
        live = [entries[i][1:] for i in order[:beam]]
    final = []
    for am, node, bonus, lm, state, picks in live:
        if trie is not None and node != 0:
            bonus = ft(bonus - ft(int(trie["depth"][node])) * boost)
        if v is not None and v["eos"] >= 0:
            lm = ft(lm + ft(alpha * lm_step(v, state, v["eos"], oov, ft)[0]))
        score = ft(am + bonus)
        if v is not None:
            score = ft(score + lm)
        final.append((score, am, lm, picks))
    order = sorted(range(len(final)), key=lambda i: -final[i][0])
    for a, b in zip(order[:-1], order[1:]):
        gap = min(gap, float(final[a][0] - final[b][0]))
    hyps = [{"tokens": [c for c, _ in final[i][3]], "score": float(final[i][0]), "am_score": float(final[i][1]), "lm": float(final[i][2]),
             "logprob": [float(lp) for _, lp in final[i][3]]} for i in order[:nbest]]
    return hyps, gap


def brute_force(cand_id, cand_lp):
    """Every pick sequence: [(tokens, float64 sum of its log-probabilities)], best first (ties to the lexicographically earlier picks). k ** N sequences."""
    cand_id, cand_lp = np.asarray(cand_id), np.asarray(cand_lp, dtype=np.float64)
    N, k = cand_id.shape
    out = []
    for path in itertools.product(range(k), repeat=N):
        if any(cand_lp[t, j] == -np.inf for t, j in enumerate(path)):
            continue
        am = 0.0
        for t, j in enumerate(path):
            am = am + cand_lp[t, j]                                                  # row order, as the search sums
        out.append(([int(cand_id[t, j]) for t, j in enumerate(path)], float(am)))
    out.sort(key=lambda h: -h[1])
    return out


def random_case(seed, N, topk, vocab, sigma=3.0):
    """Token rows as a decoder head gives them: a soft-max of N(0, sigma^2) logits over the vocabulary and its topk best columns, higher first. Returns
    (cand_id int32 [N, topk], cand_lp float32 [N, topk])."""
    rng = np.random.default_rng(9000 + seed)
    logits = rng.normal(0.0, sigma, size=(N, vocab))
    lp = logits - np.logaddexp.reduce(logits, axis=1, keepdims=True)
    ids = np.argsort(-lp, axis=1, kind="stable")[:, :topk].astype(np.int32)
    return ids, np.take_along_axis(lp, ids.astype(np.int64), axis=1).astype(np.float32)


# ---- the cases the CPU and GPU tests share (computed once per process, never modified) ---------------------------------------------------------------
SHAPES = [(1, 2, 1, 6), (5, 2, 2, 5), (6, 4, 4, 12), (9, 3, 16, 8), (40, 8, 8, 20), (137, 4, 3, 8), (64, 16, 16, 40)]          # (N, topk, beam, vocab)
MODELS = (None,) + tuple(ORDERS)                     # no model, order 2, order 4
SEEDS = 64


def case_setting(shape, order, hot, seed):
    """(trie, boost, image, phrases) of a case."""
    vocab = shape[3]
    phrases = random_phrases(seed, 3, vocab) if hot else None
    trie, boost = (build_trie(phrases), BOOST) if hot else (None, 0.0)
    image = shape_model(vocab, order)[1] if order else None
    return trie, boost, image, phrases


@functools.lru_cache(maxsize=None)
def shape_cases(shape, order, hot):
    """Of the seeds 0 .. SEEDS - 1 whose decision gap is >= GAP, two: under a model, first the first seed whose best hypothesis differs from the search
    without a model (when there is one), then the first other seed. Each: (seed, ids, lp, phrases, hyps, gap, differs), hyps the `beam` best."""
    N, topk, beam, vocab = shape
    clear = []
    for seed in range(SEEDS):
        ids, lp = random_case(seed, N, topk, vocab)
        trie, boost, image, phrases = case_setting(shape, order, hot, seed)
        hyps, gap = nar_beam(ids, lp, beam, beam, trie, boost, image, ALPHA, BETA, OOV)
        if gap < GAP:
            continue
        differs = False
        if order:
            plain, _ = nar_beam(ids, lp, beam, beam, trie, boost)
            differs = plain[0]["tokens"] != hyps[0]["tokens"]
        clear.append((seed, ids, lp, phrases, hyps, gap, differs))
        if len(clear) >= 2 and (not order or any(c[6] for c in clear)):
            break
    first = next((c for c in clear if c[6]), None)
    if first is None:
        return clear[:2]
    return [first] + [c for c in clear if c is not first][:1]
