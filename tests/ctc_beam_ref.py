"""Float64 numpy statement of the CTC prefix beam search with hotwords (csrc/ctc_beam.hip: ctc_prefix_beam_kernel), not circular.

State per live prefix: pb / pnb (log-probability of ending in blank / non-blank; the empty prefix starts at 0 / -inf) and the hotword state
(node, bonus), a function of the prefix's tokens alone. One frame, candidates (c, lp) in column order, prefix p with tot = logaddexp(pb, pnb):
  c == blank    pb'[p]    (+)= tot + lp
  c == last(p)  pnb'[p]   (+)= pnb + lp,  and pnb'[p + c] (+)= pb + lp when pb > -inf
  otherwise     pnb'[p+c] (+)= tot + lp
Contributions to the same prefix (by content) merge with logaddexp. A candidate with lp = -inf contributes nothing; a prefix that received nothing is
not an entry. The entries of a frame are enumerated in a fixed order -- first the live prefixes in their current rank order (their "stay" entries, which
also hold whatever an extension of another live prefix merged into them), then the new prefixes by (rank of the parent, candidate column) -- and the best
`beam` by logaddexp(pb', pnb') + bonus survive, ties to the earlier entry (a stable sort). That order is the live prefixes' rank order of the next frame.
After the last frame a prefix still inside a phrase gives depth(node) * boost back, the list is sorted again by ctc_score + bonus (stable) and the first
`nbest` are returned.

Hotword trie (build_trie): node 0 is the root; per node depth, is_end and its children as a sorted CSR (child_off, child_tok, child_node).
Appending a non-blank c (trie_step): a child c of the current node -> go there, bonus += boost, and back to the root if the child ends a phrase (the
bonus stays); no child c and not at the root -> bonus -= depth(node) * boost, go to the root, and try the root's child c by the same rule. No fail links.

prefix_beam also returns the smallest score difference a decision rested on: last kept against first dropped entry at every frame, and neighbouring
hypotheses of the final list. A discrete result is comparable between two implementations only where that gap clears their arithmetic difference."""
import itertools

import numpy as np


def build_trie(phrases):
    """phrases: lists of token ids -> dict of int32 arrays (depth, is_end, child_off [n + 1], child_tok, child_node). Nodes are numbered breadth first."""
    kids = [{}]
    depth, is_end = [0], [0]
    for ph in phrases:
        ph = [int(t) for t in ph]
        assert len(ph) > 0, "empty phrase"
        n = 0
        for t in ph:
            if t not in kids[n]:
                kids[n][t] = len(kids)
                kids.append({})
                depth.append(depth[n] + 1)
                is_end.append(0)
            n = kids[n][t]
        is_end[n] = 1
    order, remap = [0], {0: 0}                          # breadth-first renumbering, children by token
    for n in order:
        for t in sorted(kids[n]):
            remap[kids[n][t]] = len(order)
            order.append(kids[n][t])
    child_off, child_tok, child_node = [0], [], []
    for n in order:
        for t in sorted(kids[n]):
            child_tok.append(t)
            child_node.append(remap[kids[n][t]])
        child_off.append(len(child_tok))
    i32 = lambda a: np.asarray(a, dtype=np.int32)
    return {"depth": i32([depth[n] for n in order]), "is_end": i32([is_end[n] for n in order]), "child_off": i32(child_off),
            "child_tok": i32(child_tok), "child_node": i32(child_node)}


def _child(trie, node, c):
    lo, hi = int(trie["child_off"][node]), int(trie["child_off"][node + 1])
    for i in range(lo, hi):
        if int(trie["child_tok"][i]) == c:
            return int(trie["child_node"][i])
    return -1


def trie_step(trie, node, bonus, c, boost):
    """(node, bonus) after appending the non-blank token c."""
    if trie is None:
        return 0, bonus
    ch = _child(trie, node, c)
    if ch < 0 and node != 0:
        bonus = bonus - type(bonus)(int(trie["depth"][node])) * boost
        node = 0
        ch = _child(trie, 0, c)
    if ch >= 0:
        return (0 if int(trie["is_end"][ch]) else ch), bonus + boost
    return 0, bonus


class _P:
    __slots__ = ("tokens", "pb", "pnb", "node", "bonus", "uid", "parent_uid")


def _lae(a, b, ft):
    if a == -np.inf:
        return b
    if b == -np.inf:
        return a
    m, d = (a, b - a) if a >= b else (b, a - b)
    return ft(m + np.log1p(np.exp(ft(d)), dtype=ft))


def prefix_beam(cand_id, cand_lp, blank, beam, nbest, trie=None, boost=0.0, dtype=np.float64, identity="content"):
    """cand_id / cand_lp [T, k] (ids distinct inside a row). Returns (hyps, gap): hyps = [{"tokens", "score", "ctc_score"}] best first.
    identity="node" is the WRONG merge rule a device version is tempted by -- a prefix is its (parent node, token) pair, every re-created prefix a new
    node -- kept here only so that a test can construct an input on which the two differ."""
    ft = dtype
    cand_id, cand_lp = np.asarray(cand_id), np.asarray(cand_lp).astype(ft)
    T, k = cand_id.shape
    boost = ft(boost)
    NEG = ft(-np.inf)
    uid = itertools.count(1)
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
                if identity == "content":
                    hit = [q for q in stays if q.tokens == tokens]
                else:
                    hit = [q for q in stays if q.parent_uid == p.uid and q.tokens[-1:] == (c,)]
                if hit:
                    hit[0].pnb = _lae(hit[0].pnb, val, ft)
                    continue
                e = _P()
                e.tokens, e.pb, e.pnb, e.uid, e.parent_uid = tokens, NEG, val, next(uid), p.uid
                e.node, e.bonus = trie_step(trie, p.node, p.bonus, c, boost)
                new.append(e)
        entries = [e for e in stays + new if max(e.pb, e.pnb) > -np.inf]
        assert entries, f"frame {t}: no candidate with a finite log-probability"
        score = [ft(_lae(e.pb, e.pnb, ft) + e.bonus) for e in entries]
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
        final.append((ft(ctc + bonus), ctc, p.tokens))
    order = sorted(range(len(final)), key=lambda i: -final[i][0])
    for a, b in zip(order[:-1], order[1:]):
        gap = min(gap, float(final[a][0] - final[b][0]))
    hyps = [{"tokens": list(final[i][2]), "score": float(final[i][0]), "ctc_score": float(final[i][1])} for i in order[:nbest]]
    return hyps, gap


def collapse(ids, blank):
    out, prev = [], None
    for c in ids:
        c = int(c)
        if c != blank and c != prev:
            out.append(c)
        prev = c
    return out


def brute_force(cand_id, cand_lp, blank):
    """Sum over all alignments restricted to the candidates: {collapsed token tuple: log-probability}. k ** T paths: tiny inputs only."""
    cand_id, cand_lp = np.asarray(cand_id), np.asarray(cand_lp, dtype=np.float64)
    T, k = cand_id.shape
    acc = {}
    for path in itertools.product(range(k), repeat=T):
        lp = float(sum(cand_lp[t, j] for t, j in enumerate(path)))
        key = tuple(collapse([cand_id[t, j] for t, j in enumerate(path)], blank))
        acc[key] = np.logaddexp(acc.get(key, -np.inf), lp)
    return acc


def random_case(seed, T, topk, vocab, blank=0, blank_rate=0.8, sigma=3.0):
    """Candidate rows as the test files use them: a soft-max of N(0, sigma^2) logits over the vocabulary, its topk best columns (higher first), blank forced
    among them in `blank_rate` of the rows (it replaces the last column when absent). Returns (cand_id int32 [T, topk], cand_lp float32 [T, topk])."""
    rng = np.random.default_rng(seed)
    logits = rng.normal(0.0, sigma, size=(T, vocab))
    lp = logits - np.logaddexp.reduce(logits, axis=1, keepdims=True)
    ids = np.argsort(-lp, axis=1, kind="stable")[:, :topk].astype(np.int32)
    want_blank = rng.random(T) < blank_rate
    for t in range(T):
        has = blank in ids[t]
        if want_blank[t] and not has:
            ids[t, -1] = blank
        elif not want_blank[t] and has:
            spare = [c for c in np.argsort(-lp[t], kind="stable") if c != blank and c not in ids[t]]
            if spare:
                ids[t, list(ids[t]).index(blank)] = spare[0]
    return ids, np.take_along_axis(lp, ids.astype(np.int64), axis=1).astype(np.float32)


def random_phrases(seed, n, vocab, blank=0, max_len=3):
    rng = np.random.default_rng(1000 + seed)
    toks = [c for c in range(vocab) if c != blank]
    return [[int(rng.choice(toks)) for _ in range(int(rng.integers(1, max_len + 1)))] for _ in range(n)]


def missed_merge_case():
    """Vocabulary 3 (blank 0), beam 2: [1, 2] is dropped at frame 3 while its descendant [1, 2, 1] lives on, and is created again from [1] at frame 5,
    where its extension by 1 must merge into the live [1, 2, 1]. (Found by search over random rows; the values are rounded.)"""
    ids = np.array([[1, 0], [1, 2], [1, 0], [2, 1], [1, 0], [1, 2]], dtype=np.int32)
    lp = np.array([[-0.9104, -1.4779], [-1.5938, -1.0312], [-0.9326, -0.9549], [-1.3404, -1.2505], [-0.6398, -1.0785], [-0.1438, -3.3798]], dtype=np.float32)
    return ids, lp
