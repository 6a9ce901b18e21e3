"""Float64 numpy statement of the streaming beam search over token rows with carried state and fixed-lag commits (csrc/nar_stream_beam.hip:
nar_stream_beam_kernel). The rule of one row is nar_beam_ref.nar_beam's (entries e = p * topk + j, am' = am[p] + lp, trie_step,
lm' = lm[p] + (alpha * log P + beta), key = (am' + bonus') + lm', the best min(beam, entries) by key descending, ties to the lower e), with the same
`dtype=` switch for the float32 restatement.

Written on TOKEN TUPLES per hypothesis: a hypothesis is its running sums, its trie node, its model state and the tuple of its uncommitted (token,
log-probability) picks. There is no ring, no parent rank and no renumbering here. The fixed-lag rule -- before a row is extended, a stream whose hypotheses
hold pend_cap uncommitted picks commits the first pick of hypothesis 0 and drops every hypothesis whose first pick is another token, the rest keeping their
order -- is stated on the tuples: all live hypotheses share the committed prefix, the search never merges and a row's candidate ids are distinct, so two
hypotheses descend from different entries at a position exactly when their tokens there differ.

`gap` is the smallest score difference a decision rested on since the object was made: the last kept against the first dropped entry at every row,
hypothesis 0 against hypothesis 1 at every forced commit, the neighbours among the reported nbest at the end of every step, and the neighbours of the final
ranking."""
import functools

import numpy as np

from ctc_beam_ref import build_trie, random_phrases, trie_step
from ctc_lm_ref import ALPHA, BETA, BOOST, GAP, OOV, ORDERS, lm_step, shape_model, view
from nar_beam_ref import random_case


class NarStreamBeam:
    def __init__(self, beam, nbest, pend_cap, trie=None, boost=0.0, image=None, alpha=0.0, beta=0.0, oov=0.0, dtype=np.float64):
        assert 1 <= nbest <= beam and pend_cap >= 1
        self.ft = dtype
        self.beam, self.nbest, self.cap, self.trie, self.oov = beam, nbest, pend_cap, trie, oov
        self.v = view(image) if image is not None else None
        self.boost, self.alpha, self.beta = dtype(boost), dtype(alpha), dtype(beta)
        self.gap = np.inf
        self.clear()

    def clear(self):
        ft = self.ft
        # a live hypothesis: (am, node, bonus, lm, state, picks) -- picks the tuple of its uncommitted (token, lp)
        self.live = [(ft(0.0), 0, ft(0.0), ft(0.0), self.v["start_node"] if self.v else 0, ())]
        self.total, self.committed = 0, []                 # rows since the clear; every (token, lp) committed since the clear

    def _key(self, h):
        key = self.ft(h[0] + h[2])
        return self.ft(key + h[3]) if self.v is not None else key

    def _tails(self, order, scores):
        return [{"tokens": [c for c, _ in self.live[i][5]], "logprob": [float(lp) for _, lp in self.live[i][5]], "score": float(scores[i]),
                 "am_score": float(self.live[i][0])} for i in order[:self.nbest]]

    def step(self, cand_id, cand_lp):
        """cand_id / cand_lp [n, k], n = 0 legal. Returns {"commit": [(token, lp)] committed by this call, "pending": the tails of the best nbest live
        hypotheses (no end terms), "total"}."""
        ft, v = self.ft, self.v
        cand_id = np.asarray(cand_id)
        cand_lp = np.asarray(cand_lp).astype(ft).reshape(cand_id.shape)
        commit = []
        for t in range(cand_id.shape[0]):
            if self.live and len(self.live[0][5]) == self.cap:             # the fixed-lag commit
                first = self.live[0][5][0]
                if len(self.live) > 1:
                    self.gap = min(self.gap, float(self._key(self.live[0]) - self._key(self.live[1])))
                self.live = [h[:5] + (h[5][1:],) for h in self.live if h[5][0][0] == first[0]]
                commit.append((int(first[0]), float(first[1])))
            ids, lps = [int(c) for c in cand_id[t]], cand_lp[t]
            assert len(set(ids)) == len(ids), "candidate ids of a row must be distinct"
            entries = []
            for am, node, bonus, lm, state, picks in self.live:
                for c, lp in zip(ids, lps):
                    if not lp > -np.inf:
                        continue
                    am2 = ft(am + lp)
                    node2, bonus2 = trie_step(self.trie, node, bonus, c, self.boost)
                    key, lm2, state2 = ft(am2 + bonus2), lm, state
                    if v is not None:
                        p, state2 = lm_step(v, state, c, self.oov, ft)
                        lm2 = ft(lm + ft(ft(self.alpha * p) + self.beta))
                        key = ft(key + lm2)
                    entries.append((key, am2, node2, ft(bonus2), lm2, state2, picks + ((c, lp),)))
            assert entries, f"row {t}: no candidate with a finite log-probability"
            order = sorted(range(len(entries)), key=lambda i: -entries[i][0])          # stable: ties to the earlier entry
            if len(order) > self.beam:
                self.gap = min(self.gap, float(entries[order[self.beam - 1]][0] - entries[order[self.beam]][0]))
            self.live = [entries[i][1:] for i in order[:self.beam]]
            self.total += 1
        self.committed += commit
        keys = [self._key(h) for h in self.live]
        for a in range(min(self.nbest, len(keys)) - 1):
            self.gap = min(self.gap, float(keys[a] - keys[a + 1]))
        return {"commit": commit, "pending": self._tails(list(range(len(self.live))), keys), "total": self.total}

    def finish(self):
        """The end terms, the final ranking, the best tail committed, the search cleared. Returns {"commit", "pending" (tails with the final scores),
        "total", "hypotheses": the best nbest as full token lists since the clear}."""
        ft, v = self.ft, self.v
        scores = []
        for am, node, bonus, lm, state, picks in self.live:
            if self.trie is not None and node != 0:
                bonus = ft(bonus - ft(int(self.trie["depth"][node])) * self.boost)
            score = ft(am + bonus)
            if v is not None:
                if v["eos"] >= 0:
                    lm = ft(lm + ft(self.alpha * lm_step(v, state, v["eos"], self.oov, ft)[0]))
                score = ft(score + lm)
            scores.append(score)
        order = sorted(range(len(scores)), key=lambda i: -scores[i])
        for a, b in zip(order[:-1], order[1:]):
            self.gap = min(self.gap, float(scores[a] - scores[b]))
        tails = self._tails(order, scores)
        commit = [(int(c), float(lp)) for c, lp in self.live[order[0]][5]]
        prefix = list(self.committed)
        out = {"commit": commit, "pending": tails, "total": self.total,
               "hypotheses": [{"tokens": [c for c, _ in prefix] + t["tokens"], "logprob": [lp for _, lp in prefix] + t["logprob"], "score": t["score"],
                               "am_score": t["am_score"]} for t in tails]}
        self.clear()
        return out


def run_chunks(search, ids, lp, cuts, finish=True):
    """Feeds rows [cuts[i], cuts[i + 1]) step by step (equal neighbours are empty chunks). Returns the list of step results (+ the finish result)."""
    out = [search.step(ids[a:b], lp[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    if finish:
        out.append(search.finish())
    return out


def run_schedule(searches, steps):
    """steps as engine.op_nar_stream_beam takes them: one list per step of (stream id, cand_id, cand_lp, final); searches[id] is the stream's NarStreamBeam.
    A final slot steps through its rows and finishes. Returns, per step, per slot: the step's result, or the finish result with the step's commits in front."""
    out = []
    for st in steps:
        res = []
        for sid, ids, lp, final in st:
            r = searches[sid].step(ids, lp)
            if final:
                f = searches[sid].finish()
                f["commit"] = r["commit"] + f["commit"]
                r = f
            res.append(r)
        out.append(res)
    return out


# ---- the cases the CPU and GPU tests share (computed once per process, never modified) ---------------------------------------------------------------
# (name, N, topk, beam, nbest, vocab, pend_cap, cuts): every shape has more rows than pend_cap, so every one saturates and commits by the fixed-lag rule
SHAPES = [("greedy", 5, 1, 1, 1, 6, 2, (0, 2, 5)),                            # beam = topk = nbest = 1
          ("b16_k8", 12, 8, 16, 4, 20, 4, (0, 5, 5, 12)),                     # a step with 0 rows
          ("b16_k16", 10, 16, 16, 16, 40, 3, (0, 1, 10)),                     # beam * topk = 256, every live hypothesis reported
          ("wrap", 11, 3, 4, 3, 8, 4, (0, 3, 6, 9, 11)),                      # the ring wraps twice; the first commit (before row 4) lands inside chunk 1
          ("cap64", 70, 4, 8, 4, 12, 64, (0, 33, 70))]                        # the largest ring
MODELS = (None,) + tuple(ORDERS)                     # no model, order 2, order 4
SEEDS = 64


def case_phrases(shape, ids, seed):
    """Hotwords of a case: the second-best tokens (the best where topk = 1) of the two rows around the first chunk border, of the three rows around the first
    forced commit (rows pend_cap - 1 .. pend_cap + 1: the commit happens before row pend_cap is extended, and another before the next), and two random ones."""
    _, n, topk, _, _, vocab, cap, cuts = shape
    col = min(1, topk - 1)
    b = next(c for c in cuts if 0 < c < n)
    return [[int(ids[b - 1, col]), int(ids[b, col])], [int(ids[r, col]) for r in range(cap - 1, min(cap + 2, n))]] + random_phrases(seed, 2, vocab)


def case_setting(shape, order, hot, ids, seed):
    """(trie, boost, image, phrases) of a case."""
    phrases = case_phrases(shape, ids, seed) if hot else None
    trie, boost = (build_trie(phrases), BOOST) if hot else (None, 0.0)
    image = shape_model(shape[5], order)[1] if order else None
    return trie, boost, image, phrases


def make_search(shape, order, hot, ids, seed, dtype=np.float64):
    trie, boost, image, _ = case_setting(shape, order, hot, ids, seed)
    return NarStreamBeam(shape[3], shape[4], shape[6], trie, boost, image, ALPHA, BETA, OOV, dtype=dtype)


@functools.lru_cache(maxsize=None)
def shape_cases(shape, order, hot):
    """Of the seeds 0 .. SEEDS - 1 of nar_beam_ref.random_case whose decision gap (over the shape's chunking and the finish) is >= GAP, two: with a model or
    hotwords, first the first seed whose best hypothesis differs from the plain search's (no model, no hotwords) when there is one, then the first other
    seed. Each: (seed, ids, lp, results (the steps' and the finish's), gap, differs)."""
    _, n, topk, beam, nbest, vocab, cap, cuts = shape
    clear = []
    for seed in range(SEEDS):
        ids, lp = random_case(seed, n, topk, vocab)
        search = make_search(shape, order, hot, ids, seed)
        res = run_chunks(search, ids, lp, cuts)
        if search.gap < GAP:
            continue
        differs = False
        if order or hot:
            plain = run_chunks(NarStreamBeam(beam, nbest, cap), ids, lp, cuts)
            differs = plain[-1]["hypotheses"][0]["tokens"] != res[-1]["hypotheses"][0]["tokens"]
        clear.append((seed, ids, lp, res, search.gap, differs))
        if len(clear) >= 2 and (not (order or hot) or topk == 1 or any(c[5] for c in clear)):
            break
    first = next((c for c in clear if c[5]), None)
    if first is None:
        return clear[:2]
    return [first] + [c for c in clear if c is not first][:1]


# ---- several streams in one call: a 4-gram model and hotwords, five streams of which one is never named
SCHEDULE = dict(vocab=12, order=4, topk=3, beam=4, nbest=4, pend_cap=4, n_streams=5, rows=(14, 0, 9, 3, 0), reuse_rows=7)


@functools.lru_cache(maxsize=None)
def schedule_case():
    """(steps, results, gap, setting): the steps as engine.op_nar_stream_beam takes them and the float64 results per step and slot. What the schedule holds:
    stream ids out of order (step 0), a stream absent from a step (2 from steps 1 and 3; 4 from all of them), a step with 0 rows (stream 0 in step 1), fewer
    live hypotheses than nbest (stream 3 after its first row: 3 entries, nbest 4), rows and the finish in one slot (stream 2 in step 2), a finish with L = 0
    (stream 1, never stepped), a finish on its own (streams 3 and 0) and stream 3 used again after its finish. The rows of a stream are the first seed of
    nar_beam_ref.random_case whose decisions over the stream's whole life are clear (gap >= GAP)."""
    c = SCHEDULE
    phrases = random_phrases(0, 3, c["vocab"])
    trie, image = build_trie(phrases), shape_model(c["vocab"], c["order"])[1]
    new = lambda: NarStreamBeam(c["beam"], c["nbest"], c["pend_cap"], trie, BOOST, image, ALPHA, BETA, OOV)

    def plan(sid, ids, lp):
        e = (ids[:0], lp[:0])
        if sid == 0:
            return {0: (ids[:5], lp[:5], False), 1: e + (False,), 2: (ids[5:11], lp[5:11], False), 3: (ids[11:], lp[11:], False), 5: e + (True,)}
        if sid == 2:
            return {0: (ids[:3], lp[:3], False), 2: (ids[3:], lp[3:], True)}
        if sid == 3:                                    # three rows and a finish, then seven more as a new stream
            return {1: (ids[:1], lp[:1], False), 2: (ids[1:3], lp[1:3], False), 3: e + (True,), 4: (ids[3:], lp[3:], False), 5: e + (True,)}
        return {4: e + (True,)} if sid == 1 else {}

    order = {0: (2, 0), 1: (0, 3), 2: (3, 2, 0), 3: (0, 3), 4: (1, 3), 5: (3, 0)}
    plans, gap = {}, np.inf
    for sid, n in enumerate(c["rows"]):
        n += c["reuse_rows"] if sid == 3 else 0
        for seed in range(SEEDS):
            ids, lp = random_case(100 * sid + seed, n, c["topk"], c["vocab"])
            search = new()
            for s in sorted(plan(sid, ids, lp)):
                a, b, final = plan(sid, ids, lp)[s]
                search.step(a, b)
                if final:
                    search.finish()
            if search.gap >= GAP:
                break
        assert search.gap >= GAP
        plans[sid], gap = plan(sid, ids, lp), min(gap, search.gap)
    steps = [[(sid,) + plans[sid][s] for sid in order[s]] for s in sorted(order)]
    results = run_schedule([new() for _ in c["rows"]], steps)
    return steps, results, gap, (phrases, trie, image)
