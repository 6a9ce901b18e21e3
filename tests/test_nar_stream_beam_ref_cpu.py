"""CPU: the float64 statement of the streaming beam search with fixed-lag commits (tests/nar_stream_beam_ref.py) checked against things it does not share
code with -- the offline statement nar_beam_ref.nar_beam, the row-by-row greedy pick, its own results under another chunking -- and the conditions the GPU
test (test_nar_stream_beam_gpu.py) rests on: clear decisions at every cut the search makes, a best hypothesis that the model or the hotwords change, and
the float32 restatement its tolerance is derived from (F32_RESTATEMENT, printed per case set)."""
import numpy as np
import pytest

import ctc_beam_ref as R
import ctc_lm_ref as L
import nar_beam_ref as N
import nar_stream_beam_ref as S

F32_RESTATEMENT = 1.7e-5             # the largest float32-against-float64 score difference over the GPU test's cases (70 rows); test_nar_stream_beam_gpu.py quotes it


def _settings(vocab, seed):
    trie = R.build_trie(R.random_phrases(seed, 3, vocab))
    return [dict(), dict(trie=trie, boost=L.BOOST), dict(image=L.shape_model(vocab, 2)[1], alpha=L.ALPHA, beta=L.BETA, oov=L.OOV),
            dict(trie=trie, boost=L.BOOST, image=L.shape_model(vocab, 4)[1], alpha=L.ALPHA, beta=L.BETA, oov=L.OOV)]


def _cuts(n, seed, empty=False):
    rng = np.random.default_rng(70 + seed)
    inner = sorted(int(x) for x in rng.integers(0, n + 1, size=3))
    cuts = [0] + inner + [n]
    return cuts + [n] if empty else cuts               # (a trailing empty chunk on top of whatever equal neighbours the draw gave)


@pytest.mark.parametrize("shape", N.SHAPES[:5], ids=lambda s: "N%d_k%d_b%d_v%d" % s)
def test_within_pend_cap_any_chunking_and_finish_is_the_offline_search(shape):
    n, topk, beam, vocab = shape
    for seed in range(4):
        ids, lp = N.random_case(seed, n, topk, vocab)
        for kw in _settings(vocab, seed):
            want, gap = N.nar_beam(ids, lp, beam, beam, kw.get("trie"), kw.get("boost", 0.0), kw.get("image"), kw.get("alpha", 0.0), kw.get("beta", 0.0),
                                   kw.get("oov", 0.0))
            for cap in (n, n + 3):
                for cuts in ([0, n], _cuts(n, seed), _cuts(n, seed + 1, empty=True), list(range(n + 1))):
                    search = S.NarStreamBeam(beam, beam, cap, **kw)
                    res = S.run_chunks(search, ids, lp, cuts)
                    assert all(r["commit"] == [] for r in res[:-1]) and res[-1]["total"] == n
                    got = res[-1]["hypotheses"]
                    assert [(h["tokens"], h["score"], h["am_score"], h["logprob"]) for h in got] == \
                        [(h["tokens"], h["score"], h["am_score"], h["logprob"]) for h in want]            # ids and float64 scores, equal
                    assert res[-1]["commit"] == list(zip(want[0]["tokens"], want[0]["logprob"]))
                    assert search.gap <= gap                      # (the streaming statement watches more decisions than the offline one)


def test_two_chunkings_give_the_same_commits_and_the_same_final_nbest():
    for name, n, topk, beam, nbest, vocab, cap, cuts in S.SHAPES:
        for seed in range(3):
            ids, lp = N.random_case(seed, n, topk, vocab)
            for kw in _settings(vocab, seed):
                runs = []
                for c in (cuts, [0, n], _cuts(n, seed, empty=True), list(range(n + 1))):
                    res = S.run_chunks(S.NarStreamBeam(beam, nbest, cap, **kw), ids, lp, c)
                    commits = [x for r in res for x in r["commit"]]
                    runs.append((commits, res[-1]["pending"], res[-1]["hypotheses"]))
                    assert len(commits) == n and n > cap                  # every shape saturates
                    assert sum(len(r["commit"]) for r in res[:-1]) == n - cap
                assert all(r == runs[0] for r in runs[1:])


def test_commits_are_hypothesis_0_and_are_never_revised():
    """Row-by-row chunks, so that every report is the state a forced commit sees: the token a call commits is the first pending token of the best hypothesis
    of the report before it; every report's tails start where the commits so far end; and the commits of all steps followed by the finish's tail 0 are
    hypothesis 0 -- every returned hypothesis begins with everything committed before the finish."""
    for name, n, topk, beam, nbest, vocab, cap, cuts in S.SHAPES:
        for seed in range(3):
            ids, lp = N.random_case(seed, n, topk, vocab)
            for kw in _settings(vocab, seed):
                res = S.run_chunks(S.NarStreamBeam(beam, nbest, cap, **kw), ids, lp, list(range(n + 1)))
                committed, before = [], None
                for r in res[:-1]:
                    assert len(r["commit"]) <= 1
                    if r["commit"]:
                        assert r["commit"][0] == (before["tokens"][0], before["logprob"][0])
                    committed += r["commit"]
                    assert all(len(t["tokens"]) == r["total"] - len(committed) == len(t["logprob"]) for t in r["pending"]) and r["pending"]
                    assert all(a["score"] >= b["score"] for a, b in zip(r["pending"][:-1], r["pending"][1:]))
                    before = r["pending"][0]
                fin = res[-1]
                assert len(committed) == n - cap and fin["total"] == n
                for h in fin["hypotheses"]:
                    assert list(zip(h["tokens"], h["logprob"]))[:len(committed)] == committed and len(h["tokens"]) == n
                committed += fin["commit"]
                best = fin["hypotheses"][0]
                assert [c for c, _ in committed] == best["tokens"] and [p for _, p in committed] == best["logprob"]
                for t, (c, p) in enumerate(committed):             # every pick is one of its row's candidates, with that candidate's log-probability
                    assert p == float(lp[t, ids[t].tolist().index(c)])


def test_pend_cap_one_is_the_row_by_row_greedy_pick_on_the_key():
    """With one pending token every row after the first commits its predecessor, so the descendants of one entry survive each row: the search is the greedy
    pick of the best key per row (the last row's by the key with the end terms), restated here without the class."""
    assert all(beam >= topk for _, topk, beam, _ in N.SHAPES[1:5])
    for n, topk, beam, vocab in N.SHAPES[1:5]:
        for seed in range(3):
            ids, lp = N.random_case(seed, n, topk, vocab)
            for kw in _settings(vocab, seed):
                res = S.run_chunks(S.NarStreamBeam(beam, 1, 1, **kw), ids, lp, _cuts(n, seed))
                got = [c for r in res for c, _ in r["commit"]]
                trie, boost, v = kw.get("trie"), kw.get("boost", 0.0), L.view(kw["image"]) if "image" in kw else None
                am, node, bonus, lm, state, want = 0.0, 0, 0.0, 0.0, v["start_node"] if v else 0, []
                for t in range(n):
                    best = None
                    for c, p in zip(ids[t].tolist(), lp[t].astype(np.float64)):
                        node2, bonus2 = R.trie_step(trie, node, np.float64(bonus), c, np.float64(boost))
                        lm2, state2 = lm, state
                        if v is not None:
                            q, state2 = L.lm_step(v, state, c, kw["oov"])
                            lm2 = lm + (kw["alpha"] * q + kw["beta"])
                        if t == n - 1:                     # the last row's pick is the finish's: the end terms decide with the key (beam >= topk here)
                            if trie is not None and node2 != 0:
                                bonus2 = bonus2 - float(trie["depth"][node2]) * boost
                            if v is not None and v["eos"] >= 0:
                                lm2 = lm2 + kw["alpha"] * L.lm_step(v, state2, v["eos"], kw["oov"])[0]
                        key = ((am + p) + bonus2) + lm2 if v is not None else (am + p) + bonus2
                        if best is None or key > best[0]:
                            best = (key, c, am + p, node2, bonus2, lm2, state2)
                    _, c, am, node, bonus, lm, state = best
                    want.append(c)
                assert got == want


@pytest.mark.parametrize("order", S.MODELS, ids=lambda o: f"order{o}" if o else "no_model")
@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: s[0])
def test_the_gpu_cases_are_clear_change_the_best_hypothesis_and_survive_float32(shape, order):
    """The conditions of test_nar_stream_beam_gpu.py, and the figure its tolerance is 6 x of (F32_RESTATEMENT): the float32 restatement's largest score
    difference over all shapes, models and both hotword settings, printed here per case set. The decision gap covers every cut the search makes: the
    beam-th against the next key at every row, hypothesis 0 against 1 at every forced commit, the order of the reported nbest at the end of every step and
    the final ranking (NarStreamBeam.gap). The cases are picked here, on the CPU: the GPU test takes them as they are and skips none."""
    name, n, topk, beam, nbest, vocab, cap, cuts = shape
    worst = 0.0
    for hot in (False, True):
        cases = S.shape_cases(shape, order, hot)
        assert len(cases) == 2, f"{len(cases)} of {S.SEEDS} seeds have a decision gap >= {L.GAP}"
        assert all(c[4] >= L.GAP for c in cases)
        if (order or hot) and topk > 1:                    # (with one candidate per row there is one path: nothing can change it)
            assert any(c[5] for c in cases), "no chosen case whose best hypothesis the model / the hotwords change"
        for seed, ids, lp, res, gap, differs in cases:
            assert sum(len(r["commit"]) for r in res[:-1]) == n - cap > 0              # forced commits happen, and across them ...
            if hot:                                         # ... the phrases: one over a chunk border, one over the first forced commits
                phrases = S.case_phrases(shape, ids, seed)
                b = next(c for c in cuts if 0 < c < n)
                col = min(1, topk - 1)
                assert phrases[0] == [int(ids[b - 1, col]), int(ids[b, col])] and phrases[1][:2] == [int(ids[cap - 1, col]), int(ids[cap, col])]
            r32 = S.run_chunks(S.make_search(shape, order, hot, ids, seed, dtype=np.float32), ids, lp, cuts)
            for a, b in zip(r32, res):
                assert [c for c, _ in a["commit"]] == [c for c, _ in b["commit"]] and a["total"] == b["total"]
                assert [t["tokens"] for t in a["pending"]] == [t["tokens"] for t in b["pending"]]
                worst = max([worst] + [max(abs(x["score"] - y["score"]), abs(x["am_score"] - y["am_score"])) for x, y in zip(a["pending"], b["pending"])])
    if order == 4:                                         # a 4-gram context is three tokens: from row 3 on it spans every border and every commit behind it
        assert n - 1 >= 3 and any(0 < c < n for c in cuts)
    print(f"shape {name} model {order}: float32 restatement differs by at most {worst:.2e}")
    assert worst <= F32_RESTATEMENT                                     # the figure the GPU tolerance quotes still holds


def test_the_schedule_of_several_streams_is_clear_and_holds_what_it_names():
    steps, results, gap, (phrases, trie, image) = S.schedule_case()
    c = S.SCHEDULE
    assert gap >= L.GAP
    named = {sid for st in steps for sid, _, _, _ in st}
    assert named == {0, 1, 2, 3} and c["n_streams"] == 5                       # stream 4 is in no step
    assert [sl[0] for sl in steps[0]] == [2, 0]                               # out of order
    assert steps[1][0][0] == 0 and steps[1][0][1].shape[0] == 0               # a step with 0 rows
    assert len(results[1][1]["pending"]) == 3 < c["nbest"]                    # fewer live hypotheses than nbest
    assert steps[2][1][0] == 2 and steps[2][1][3] and steps[2][1][1].shape[0] == 6 and len(results[2][1]["commit"]) == 6 + 3
    empty = results[4][0]                                                     # the finish of a stream that was never stepped
    v = L.view(image)
    end = L.ALPHA * float(L.lm_step(v, v["start_node"], v["eos"], L.OOV)[0])
    assert steps[4][0][0] == 1 and empty["total"] == 0 and empty["commit"] == [] and len(empty["pending"]) == 1
    assert empty["pending"][0]["tokens"] == [] and empty["pending"][0]["am_score"] == 0.0 and abs(empty["pending"][0]["score"] - end) <= 1e-12
    assert results[3][1]["total"] == 3 and results[4][1]["total"] == 7 and len(results[4][1]["commit"]) == 3          # stream 3, used again after its finish
    # the float32 restatement of the schedule stays inside the figure the GPU tolerance quotes
    new = lambda: S.NarStreamBeam(c["beam"], c["nbest"], c["pend_cap"], trie, L.BOOST, image, L.ALPHA, L.BETA, L.OOV, dtype=np.float32)
    r32 = S.run_schedule([new() for _ in range(c["n_streams"])], steps)
    worst = 0.0
    for a_step, b_step in zip(r32, results):
        for a, b in zip(a_step, b_step):
            assert [x for x, _ in a["commit"]] == [x for x, _ in b["commit"]] and [t["tokens"] for t in a["pending"]] == [t["tokens"] for t in b["pending"]]
            worst = max([worst] + [max(abs(x["score"] - y["score"]), abs(x["am_score"] - y["am_score"])) for x, y in zip(a["pending"], b["pending"])])
    print(f"schedule: float32 restatement differs by at most {worst:.2e}")
    assert worst <= F32_RESTATEMENT
