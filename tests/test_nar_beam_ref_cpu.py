"""CPU: the float64 statement of the beam search over token rows (tests/nar_beam_ref.py) checked against things it does not share code with -- the
enumeration of every pick sequence, the per-row first candidate, ctc_lm_ref.score_tokens -- and the conditions the GPU test (test_nar_beam_gpu.py) rests on:
clear decisions, a best hypothesis the model changes, and the float32 restatement its tolerance is derived from (F32_RESTATEMENT, printed per case set)."""
import numpy as np
import pytest

import ctc_beam_ref as R
import ctc_lm_ref as L
import nar_beam_ref as N

F32_RESTATEMENT = 4.1e-5             # the largest float32-against-float64 score difference over the GPU test's cases (N = 137); test_nar_beam_gpu.py quotes it


@pytest.mark.parametrize("shape", N.SHAPES[:3], ids=lambda s: "N%d_k%d_b%d_v%d" % s)
def test_without_hotwords_and_model_the_nbest_are_the_best_pick_sequences(shape):
    n, topk, beam, vocab = shape
    for seed in range(6):
        ids, lp = N.random_case(seed, n, topk, vocab)
        every = N.brute_force(ids, lp)
        assert len(every) == topk ** n
        hyps, gap = N.nar_beam(ids, lp, beam, beam)
        assert len(hyps) == min(beam, len(every))
        for h, (tokens, am) in zip(hyps, every):
            assert h["tokens"] == tokens and abs(h["am_score"] - am) <= 1e-12 and h["score"] == h["am_score"]
            assert abs(sum(h["logprob"]) - am) <= 1e-12 and len(h["logprob"]) == n
        assert gap >= 0


def test_beam_one_is_the_first_candidate_of_every_row():
    for n, topk, _, vocab in N.SHAPES:
        ids, lp = N.random_case(1, n, topk, vocab)
        hyps, _ = N.nar_beam(ids, lp, 1, 1)
        assert len(hyps) == 1 and hyps[0]["tokens"] == ids[:, 0].tolist()           # (columns are sorted: column 0 is the row's arg-max)
        assert hyps[0]["logprob"] == [float(x) for x in lp[:, 0]]


def test_no_rows_give_the_one_empty_hypothesis():
    ids, lp = np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32)
    hyps, gap = N.nar_beam(ids, lp, 4, 4)
    assert hyps == [{"tokens": [], "score": 0.0, "am_score": 0.0, "lm": 0.0, "logprob": []}] and gap == np.inf
    image = L.shape_model(12, 2)[1]
    v = L.view(image)
    hyps, _ = N.nar_beam(ids, lp, 4, 4, image=image, alpha=0.5, beta=0.3)
    end = 0.5 * float(L.lm_step(v, v["start_node"], v["eos"])[0])
    assert len(hyps) == 1 and hyps[0]["am_score"] == 0.0 and end < 0 and abs(hyps[0]["score"] - end) <= 1e-12


def test_fewer_hypotheses_than_nbest_in_the_early_rows():
    ids, lp = N.random_case(0, 2, 2, 6)
    hyps, _ = N.nar_beam(ids, lp, 8, 8)
    assert len(hyps) == 4 and [h["tokens"] for h in hyps] == [t for t, _ in N.brute_force(ids, lp)]


def test_a_zero_weight_model_without_end_of_sentence_changes_nothing():
    for shape in N.SHAPES[:5]:
        n, topk, beam, vocab = shape
        image = L.shape_model(vocab, 4, eos=False)[1]
        assert L.view(image)["eos"] == -1
        for seed in range(3):
            ids, lp = N.random_case(seed, n, topk, vocab)
            phrases = R.random_phrases(seed, 3, vocab)
            for trie, boost in ((None, 0.0), (R.build_trie(phrases), L.BOOST)):
                want, gap = N.nar_beam(ids, lp, beam, beam, trie, boost)
                got, gap_lm = N.nar_beam(ids, lp, beam, beam, trie, boost, image, 0.0, 0.0, -0.5)
                key = lambda hs: [(h["tokens"], h["score"], h["am_score"]) for h in hs]
                assert key(got) == key(want) and gap == gap_lm


def test_the_lm_term_is_score_tokens_of_the_hypothesis():
    vocab, alpha, beta, oov = 12, 0.7, 0.3, -0.9
    for order, eos in ((2, True), (4, False), (4, True)):
        image = L.shape_model(vocab, order, eos=eos)[1]
        v = L.view(image)
        for seed in range(3):
            ids, lp = N.random_case(seed, 6, 4, vocab)
            hyps, _ = N.nar_beam(ids, lp, 4, 4, image=image, alpha=alpha, beta=beta, oov=oov)
            for h in hyps:
                lm, end = L.score_tokens(v, h["tokens"], alpha, beta, oov)
                assert abs(h["lm"] - float(lm + end)) <= 1e-12 and abs(h["score"] - (h["am_score"] + h["lm"])) <= 1e-12


def test_a_hotword_changes_the_best_hypothesis():
    """The phrase is the second-best token of rows 2 and 3: from the boost at which two matched tokens outweigh what the two picks lose, the best hypothesis
    spells it, and below that it is the plain one."""
    ids, lp = N.random_case(3, 6, 4, 12)
    phrase = [int(ids[2, 1]), int(ids[3, 1])]
    trie = R.build_trie([phrase])
    plain, _ = N.nar_beam(ids, lp, 4, 1)
    assert plain[0]["tokens"] == ids[:, 0].tolist() and plain[0]["tokens"][2:4] != phrase
    loss = float(lp[2, 0] - lp[2, 1]) + float(lp[3, 0] - lp[3, 1])
    assert loss > 0
    hot, _ = N.nar_beam(ids, lp, 4, 1, trie, 0.5 * loss * 1.05)
    assert hot[0]["tokens"][2:4] == phrase and hot[0]["tokens"][:2] == plain[0]["tokens"][:2] and hot[0]["tokens"][4:] == plain[0]["tokens"][4:]
    assert abs(hot[0]["score"] - hot[0]["am_score"] - loss * 1.05) <= 1e-12
    below, _ = N.nar_beam(ids, lp, 4, 1, trie, 0.5 * loss * 0.95)
    assert below[0]["tokens"] == plain[0]["tokens"]


def test_an_open_match_is_refunded_at_the_end():
    """One row, a two-token phrase whose first token is the second-best candidate: inside the row the boost lifts that pick to rank 0, at the end the open
    match gives the boost back and the final ranking is the plain one again, with the bonus gone from the score."""
    ids = np.array([[4, 7]], dtype=np.int32)
    lp = np.log(np.array([[0.6, 0.3]])).astype(np.float32)
    trie = R.build_trie([[7, 2]])
    hyps, _ = N.nar_beam(ids, lp, 2, 2, trie, 2.0)
    assert [h["tokens"] for h in hyps] == [[4], [7]] and all(h["score"] == h["am_score"] for h in hyps)
    # ... while a longer input keeps the bonus of a phrase that is completed
    ids2 = np.array([[4, 7], [2, 5]], dtype=np.int32)
    lp2 = np.log(np.array([[0.6, 0.3], [0.5, 0.4]])).astype(np.float32)
    hyps2, _ = N.nar_beam(ids2, lp2, 4, 4, trie, 2.0)
    assert hyps2[0]["tokens"] == [7, 2] and abs(hyps2[0]["score"] - hyps2[0]["am_score"] - 4.0) <= 1e-12
    by = {tuple(h["tokens"]): h for h in hyps2}
    assert by[(7, 5)]["score"] == by[(7, 5)]["am_score"]                            # broken off inside the utterance: taken back by trie_step


@pytest.mark.parametrize("order", N.MODELS, ids=lambda o: f"order{o}" if o else "no_model")
@pytest.mark.parametrize("shape", N.SHAPES, ids=lambda s: "N%d_k%d_b%d_v%d" % s)
def test_the_gpu_cases_are_clear_change_the_best_hypothesis_and_survive_float32(shape, order):
    """The conditions of test_nar_beam_gpu.py, and the figure its tolerance is 6 x of (F32_RESTATEMENT): the float32 restatement's largest score difference
    over all shapes, models and both hotword settings, printed here per case set."""
    n, topk, beam, vocab = shape
    worst, changed = 0.0, False
    for hot in (False, True):
        cases = N.shape_cases(shape, order, hot)
        assert len(cases) == 2, f"{len(cases)} of {N.SEEDS} seeds have a decision gap >= {L.GAP}"
        assert all(c[5] >= L.GAP for c in cases)
        changed = changed or any(c[6] for c in cases)
        for seed, ids, lp, phrases, hyps, gap, differs in cases:
            trie, boost, image, _ = N.case_setting(shape, order, hot, seed)
            h32, _ = N.nar_beam(ids, lp, beam, beam, trie, boost, image, L.ALPHA, L.BETA, L.OOV, dtype=np.float32)
            assert [h["tokens"] for h in h32] == [h["tokens"] for h in hyps]
            worst = max([worst] + [max(abs(a["score"] - b["score"]), abs(a["am_score"] - b["am_score"])) for a, b in zip(h32, hyps)])
    if order:
        assert changed, "no chosen case whose best hypothesis the model changes"
    print(f"shape {shape} model {order}: float32 restatement differs by at most {worst:.2e}")
    assert worst <= F32_RESTATEMENT                                     # the figure the GPU tolerance quotes still holds
