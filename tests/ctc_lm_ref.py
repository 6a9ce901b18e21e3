"""Float64 numpy statement of the CTC prefix beam search with a back-off n-gram language model fused in (csrc/ctc_beam.hip: ctc_prefix_beam_kernel<true>,
csrc/ngram_lm.h), not circular: ctc_beam_ref.prefix_beam's enumeration with the LM term added.

A model here is a dict {tuple of token ids: (logp, backoff)}, natural logs, over ids 0 .. vocab - 1 plus </s> = vocab and <s> = vocab + 1. Every listed
n-gram's context (the n-gram minus its last token) is listed too.

The image (build_image): one int32 blob --
  [order, n_nodes, n_edges, vocab, start_node, eos_edge_token]
  depth [n_nodes] | backoff f32 [n_nodes] | suffix [n_nodes] | child_off [n_nodes + 1] | tok [n_edges] | logp f32 [n_edges] | next [n_edges] | uni [vocab + 2]
Nodes are the contexts: node 0 the empty one, every listed n-gram of order 1 .. N - 1 a node of that depth (numbered by depth, then content); suffix is the
longest proper suffix that is a node. Edges are the listed n-grams, under their context's node, sorted by token; next is the node of the longest suffix of the
full n-gram that is a node. uni[c] is the root's edge for c or -1. start_node = next of the <s> unigram (0 without one); eos_edge_token = vocab when </s> is
listed, else -1.

lm_step(state, c): uni[c] < 0 -> (oov, state): the token is out of vocabulary, it costs oov and the state stays. Otherwise acc = 0, n = state; find c among
n's children (the root's through uni); found -> (acc + logp, next); else acc += backoff[n], n = suffix[n], again.

The search: every prefix carries lm = the sum over its tokens of alpha * logp + beta and the model's state, both functions of its content (so merging by
content is as valid as it is for the hotword bonus). A stay keeps them, an extension steps the model. Entries rank by logaddexp(pb', pnb') + bonus + lm. After
the last frame a prefix adds alpha * lm_step(state, </s>).logp when the model lists </s>; the final order and `score` use ctc + bonus + lm, `ctc_score` is
the CTC figure alone.

arpa_logprob is the textbook back-off recursion straight from the dict; it knows nothing of the image or of suffix links."""
import functools
import itertools

import numpy as np

from ctc_beam_ref import _lae, _P, trie_step

HEADER = 6


def build_image(ngrams, vocab):
    """{tuple: (logp, backoff)} -> the int32 image."""
    eos, bos = vocab, vocab + 1
    assert ngrams and all(len(g) >= 1 for g in ngrams)
    order = max(len(g) for g in ngrams)
    for g in ngrams:
        assert all(0 <= t < vocab + 2 for t in g), g
        assert len(g) == 1 or g[:-1] in ngrams, f"the context of {g} is not listed"
    nodes = [()] + sorted((g for g in ngrams if len(g) < order), key=lambda g: (len(g), g))
    index = {g: i for i, g in enumerate(nodes)}

    def longest_node(g):                                   # the longest suffix of g (g itself included) that is a node
        for k in range(len(g) + 1):
            if g[k:] in index:
                return index[g[k:]]
        raise AssertionError
    kids = {i: [] for i in range(len(nodes))}
    for g, (lp, _) in ngrams.items():
        kids[index[g[:-1]]].append((g[-1], lp, longest_node(g)))
    depth = [len(g) for g in nodes]
    backoff = [0.0] + [ngrams[g][1] for g in nodes[1:]]
    suffix = [0] + [longest_node(g[1:]) for g in nodes[1:]]
    child_off, tok, logp, nxt = [0], [], [], []
    for i in range(len(nodes)):
        for t, lp, nx in sorted(kids[i]):
            tok.append(t); logp.append(lp); nxt.append(nx)
        child_off.append(len(tok))
    uni = [-1] * (vocab + 2)
    for e in range(child_off[0], child_off[1]):
        uni[tok[e]] = e
    start = nxt[uni[bos]] if uni[bos] >= 0 else 0
    header = [order, len(nodes), len(tok), vocab, start, eos if uni[eos] >= 0 else -1]
    i32 = lambda a: np.asarray(a, dtype=np.int32)
    f32 = lambda a: np.asarray(a, dtype=np.float32).view(np.int32)
    return np.concatenate([i32(header), i32(depth), f32(backoff), i32(suffix), i32(child_off), i32(tok), f32(logp), i32(nxt), i32(uni)])


def view(image):
    """The image's arrays by name (views; the float arrays as float32)."""
    image = np.asarray(image, dtype=np.int32)
    order, n, m, vocab, start, eos = (int(x) for x in image[:HEADER])
    assert image.size == HEADER + 4 * n + 1 + 3 * m + vocab + 2
    out, at = {"order": order, "n_nodes": n, "n_edges": m, "vocab": vocab, "start_node": start, "eos": eos}, HEADER
    for name, size, fl in (("depth", n, 0), ("backoff", n, 1), ("suffix", n, 0), ("child_off", n + 1, 0), ("tok", m, 0), ("logp", m, 1), ("next", m, 0),
                           ("uni", vocab + 2, 0)):
        out[name] = image[at:at + size].view(np.float32) if fl else image[at:at + size]
        at += size
    return out


def lm_step(v, state, c, oov=0.0, ft=np.float64):
    """(logp, state') over a view of the image, arithmetic in ft."""
    ue = int(v["uni"][c])
    if ue < 0:
        return ft(oov), state
    acc, n = ft(0.0), state
    while True:
        e = -1
        if n == 0:
            e = ue
        else:
            for i in range(int(v["child_off"][n]), int(v["child_off"][n + 1])):
                if int(v["tok"][i]) == c:
                    e = i
        if e >= 0:
            return ft(acc + ft(v["logp"][e])), int(v["next"][e])
        acc = ft(acc + ft(v["backoff"][n]))
        n = int(v["suffix"][n])


def score_tokens(v, tokens, alpha, beta, oov=0.0, ft=np.float64):
    """The LM total of a token list as the search accumulates it: (sum of alpha * logp + beta, the eos term alpha * logp(</s>) or 0)."""
    lm, state = ft(0.0), v["start_node"]
    for c in tokens:
        lp, state = lm_step(v, state, int(c), oov, ft)
        lm = ft(lm + ft(ft(ft(alpha) * lp) + ft(beta)))
    end = ft(0.0)
    if v["eos"] >= 0:
        end = ft(ft(alpha) * lm_step(v, state, v["eos"], oov, ft)[0])
    return lm, end


def arpa_logprob(ngrams, context, c):
    """log P(c | context) by the textbook recursion: the n-gram if listed, else backoff(context) (0 when the context is not listed) + log P(c | context minus
    its first token). None when c has no unigram."""
    context = tuple(context)
    g = context + (c,)
    if g in ngrams:
        return float(ngrams[g][0])
    if not context:
        return None
    bo = float(ngrams[context][1]) if context in ngrams else 0.0
    rest = arpa_logprob(ngrams, context[1:], c)
    return None if rest is None else bo + rest


def arpa_sequence(ngrams, vocab, tokens, oov=0.0):
    """Per token log P(token | history) by arpa_logprob, the history starting at <s> when the model lists it and skipping out-of-vocabulary tokens (they
    cost oov), plus log P(</s> | history) (None when </s> is not listed)."""
    order = max(len(g) for g in ngrams)
    hist = [vocab + 1] if (vocab + 1,) in ngrams else []
    out = []
    context = lambda: hist[max(0, len(hist) - (order - 1)):] if order > 1 else ()       # the last order - 1 tokens
    for c in tokens:
        c = int(c)
        lp = arpa_logprob(ngrams, context(), c)
        if lp is None:
            out.append(float(oov))
            continue
        out.append(lp)
        hist.append(c)
    end = arpa_logprob(ngrams, context(), vocab) if (vocab,) in ngrams else None
    return out, end


def random_arpa(seed, vocab, order, keep, blank=0, bos=True, eos=True, unigram_keep=0.85):
    """A pruned random model: `unigram_keep` of the non-blank tokens have a unigram (the others are out of vocabulary), and of every listed (n - 1)-gram's
    continuations by a token with a unigram (or </s>) a share `keep` is listed, so every listed n-gram's context is listed. Log-probabilities are drawn, not
    normalised (nothing here needs them to be); n-grams below the top order have random back-offs of either sign."""
    rng = np.random.default_rng(7000 + seed)
    E, B = vocab, vocab + 1
    words = [c for c in range(vocab) if c != blank and rng.random() < unigram_keep]
    if not words:
        words = [c for c in range(vocab) if c != blank][:1]
    ngrams = {}
    level = [(c,) for c in words] + ([(E,)] if eos else []) + ([(B,)] if bos else [])
    for n in range(1, order + 1):
        for g in level:
            lp = 0.0 if (n == 1 and g == (B,)) else -float(rng.uniform(0.05, 4.0))
            bo = float(rng.normal(-0.4, 0.5)) if n < order and g[-1] != E else 0.0
            ngrams[g] = (float(np.float32(lp)), float(np.float32(bo)))
        nxt, conts = [], words + ([E] if eos else [])
        for g in level:
            if g[-1] == E:
                continue
            nxt.extend(g + (conts[i],) for i in np.flatnonzero(rng.random(len(conts)) < keep))
        level = nxt
    return ngrams


def arpa_text(ngrams, vocab, unk=None):
    """The model as ARPA text over decimal token ids (log10), with <unk> at log-probability `unk` (natural log) when given."""
    name = lambda t: "</s>" if t == vocab else "<s>" if t == vocab + 1 else str(t)
    order = max(len(g) for g in ngrams)
    by = [[g for g in sorted(ngrams) if len(g) == n] for n in range(1, order + 1)]
    ln10 = float(np.log(10.0))
    lines = ["\\data\\"] + [f"ngram {n + 1}={len(b) + (1 if unk is not None and n == 0 else 0)}" for n, b in enumerate(by)] + [""]
    for n, b in enumerate(by):
        lines.append(f"\\{n + 1}-grams:")
        if n == 0 and unk is not None:
            lines.append(f"{float(unk) / ln10!r}\t<unk>")
        for g in b:
            lp, bo = ngrams[g]
            lines.append(f"{lp / ln10!r}\t{' '.join(name(t) for t in g)}" + (f"\t{bo / ln10!r}" if n + 1 < order else ""))
        lines.append("")
    lines.append("\\end\\")
    return lines


def prefix_beam_lm(cand_id, cand_lp, blank, beam, nbest, image, alpha, beta, oov=0.0, trie=None, boost=0.0, dtype=np.float64):
    """ctc_beam_ref.prefix_beam with the language model `image`. Returns (hyps, gap): hyps = [{"tokens", "score", "ctc_score", "lm"}] best first, `lm` the
    LM term inside `score` (eos term included); gap as prefix_beam states it."""
    ft = dtype
    v = view(image)
    cand_id, cand_lp = np.asarray(cand_id), np.asarray(cand_lp).astype(ft)
    T, k = cand_id.shape
    boost, alpha, beta = ft(boost), ft(alpha), ft(beta)
    NEG = ft(-np.inf)
    uid = itertools.count(1)
    lm_of, state_of = {(): ft(0.0)}, {(): v["start_node"]}       # by content
    root = _P()
    root.tokens, root.pb, root.pnb, root.node, root.bonus, root.uid, root.parent_uid = (), ft(0.0), NEG, 0, ft(0.0), 0, -1
    live, gap = [root], np.inf
    for t in range(T):
        ids, lps = [int(c) for c in cand_id[t]], cand_lp[t]
        assert len(set(ids)) == k, "candidate ids of a row must be distinct"
        stays = []
        for p in live:
            e = _P()
            e.tokens, e.node, e.bonus, e.uid, e.parent_uid, e.pb, e.pnb = p.tokens, p.node, p.bonus, p.uid, p.parent_uid, NEG, NEG
            tot = _lae(p.pb, p.pnb, ft)
            for c, lp in zip(ids, lps):
                if lp == -np.inf:
                    continue
                if c == blank:
                    e.pb = _lae(e.pb, ft(tot + lp), ft)
                elif p.tokens and c == p.tokens[-1] and p.pnb > -np.inf:
                    e.pnb = _lae(e.pnb, ft(p.pnb + lp), ft)
            stays.append(e)
        new = []
        for p in live:
            tot = _lae(p.pb, p.pnb, ft)
            for c, lp in zip(ids, lps):
                if lp == -np.inf or c == blank:
                    continue
                if p.tokens and c == p.tokens[-1]:
                    if p.pb == -np.inf:
                        continue
                    val = ft(p.pb + lp)
                else:
                    val = ft(tot + lp)
                tokens = p.tokens + (c,)
                hit = [q for q in stays if q.tokens == tokens]
                if hit:
                    hit[0].pnb = _lae(hit[0].pnb, val, ft)
                    continue
                e = _P()
                e.tokens, e.pb, e.pnb, e.uid, e.parent_uid = tokens, NEG, val, next(uid), p.uid
                e.node, e.bonus = trie_step(trie, p.node, p.bonus, c, boost)
                step, state = lm_step(v, state_of[p.tokens], c, oov, ft)
                total = ft(lm_of[p.tokens] + ft(ft(alpha * step) + beta))
                assert tokens not in lm_of or (lm_of[tokens] == total and state_of[tokens] == state)      # a function of the content
                lm_of[tokens], state_of[tokens] = total, state
                new.append(e)
        entries = [e for e in stays + new if max(e.pb, e.pnb) > -np.inf]
        assert entries, f"frame {t}: no candidate with a finite log-probability"
        score = [ft(ft(_lae(e.pb, e.pnb, ft) + e.bonus) + lm_of[e.tokens]) for e in entries]
        order = sorted(range(len(entries)), key=lambda i: -score[i])              # stable: ties to the earlier entry
        if len(order) > beam:
            gap = min(gap, float(score[order[beam - 1]] - score[order[beam]]))
        live = [entries[i] for i in order[:beam]]
    final = []
    for p in live:
        bonus = p.bonus
        if trie is not None and p.node != 0:
            bonus = ft(bonus - ft(int(trie["depth"][p.node])) * boost)
        ctc = _lae(p.pb, p.pnb, ft)
        lm = lm_of[p.tokens]
        if v["eos"] >= 0:
            lm = ft(lm + ft(alpha * lm_step(v, state_of[p.tokens], v["eos"], oov, ft)[0]))
        final.append((ft(ft(ctc + bonus) + lm), ctc, p.tokens, lm))
    order = sorted(range(len(final)), key=lambda i: -final[i][0])
    for a, b in zip(order[:-1], order[1:]):
        gap = min(gap, float(final[a][0] - final[b][0]))
    hyps = [{"tokens": list(final[i][2]), "score": float(final[i][0]), "ctc_score": float(final[i][1]), "lm": float(final[i][3])} for i in order[:nbest]]
    return hyps, gap


# ---- the cases the CPU and GPU tests share (computed once per process, never modified) ---------------------------------------------------------------
SHAPES = [(5, 2, 1, 6), (9, 3, 2, 5), (40, 4, 4, 12), (48, 8, 8, 20), (137, 4, 3, 8), (64, 16, 16, 40)]          # (T, topk, beam, vocab)
ORDERS = (2, 4)
GAP, ALPHA, BETA, OOV, BOOST = 1e-3, 0.5, 0.3, -0.7, 1.5


@functools.lru_cache(maxsize=None)
def shape_model(vocab, order, eos=True):
    """(ngrams, image) of the model the tests use for a vocabulary and order: about six listed continuations per context."""
    ngrams = random_arpa(100 + order, vocab, order, min(0.5, 6.0 / vocab), eos=eos)
    return ngrams, build_image(ngrams, vocab)


@functools.lru_cache(maxsize=None)
def shape_cases(shape, order, hot):
    """Of the seeds 0..31 whose decision gap under the model is >= GAP: the first whose best hypothesis differs from the search without a model, and the first
    other one (just the first two when none differs; the CPU test requires one that does). Each: (seed, ids, lp, phrases, hyps, gap, differs)."""
    from ctc_beam_ref import build_trie, prefix_beam, random_case, random_phrases
    T, topk, beam, vocab = shape
    image = shape_model(vocab, order)[1]
    clear = []
    for seed in range(32):
        ids, lp = random_case(seed, T, topk, vocab)
        phrases = random_phrases(seed, 3, vocab) if hot else None
        trie, boost = (build_trie(phrases), BOOST) if hot else (None, 0.0)
        hyps, gap = prefix_beam_lm(ids, lp, 0, beam, beam, image, ALPHA, BETA, OOV, trie=trie, boost=boost)
        if gap < GAP:
            continue
        plain, _ = prefix_beam(ids, lp, 0, beam, beam, trie=trie, boost=boost)
        clear.append((seed, ids, lp, phrases, hyps, gap, plain[0]["tokens"] != hyps[0]["tokens"]))
        if len(clear) >= 2 and any(c[6] for c in clear):
            break
    first = next((c for c in clear if c[6]), None)
    if first is None:
        return clear[:2]
    return [first] + [c for c in clear if c is not first][:1]
