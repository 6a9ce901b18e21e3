"""CPU: the float64 statement of the prefix beam search with an n-gram language model (tests/ctc_lm_ref.py) checked against things it does not share code
with -- the textbook back-off recursion over the dict of n-grams, the search without a model, and the brute-force sum over alignments -- and the conditions
the GPU test (test_ctc_lm_beam_gpu.py) rests on: clear decisions, a changed best hypothesis, and the float32 restatement its tolerance is derived from."""
import numpy as np
import pytest

import ctc_beam_ref as R
import ctc_lm_ref as L


@pytest.mark.parametrize("bos, eos", [(True, True), (False, False), (True, False), (False, True)], ids=["s_and_end", "neither", "s_only", "end_only"])
@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_image_walk_equals_the_textbook_recursion(order, bos, eos):
    vocab, worst, oov_seen = 9, 0.0, 0
    for seed in range(8):
        ngrams = L.random_arpa(seed, vocab, order, 0.4, bos=bos, eos=eos)
        v = L.view(L.build_image(ngrams, vocab))
        assert v["order"] == max(len(g) for g in ngrams) and (v["eos"] == vocab) == eos and (v["start_node"] != 0) == (bos and v["order"] > 1)
        tokens = np.random.default_rng(seed).integers(1, vocab, size=24)
        for oov in (0.0, -1.25):                                       # without and with an <unk> cost
            want, end = L.arpa_sequence(ngrams, vocab, tokens, oov)
            state = v["start_node"]
            for c, w in zip(tokens, want):
                known = (int(c),) in ngrams
                before = state
                lp, state = L.lm_step(v, state, int(c), oov)
                worst = max(worst, abs(float(lp) - w))
                if not known:
                    assert state == before and float(lp) == oov
                    oov_seen += 1
            if eos:
                worst = max(worst, abs(float(L.lm_step(v, state, vocab, oov)[0]) - end))
            else:
                assert end is None
    print(f"order {order}: largest difference {worst:.2e}, {oov_seen} out-of-vocabulary steps")
    assert worst <= 1e-12 and oov_seen > 0


def test_zero_weights_give_the_search_without_a_model_exactly():
    for shape in L.SHAPES[:4]:
        T, topk, beam, vocab = shape
        image = L.shape_model(vocab, 4, eos=False)[1]
        for seed in range(3):
            ids, lp = R.random_case(seed, T, topk, vocab)
            phrases = R.random_phrases(seed, 3, vocab)
            for trie, boost in ((None, 0.0), (R.build_trie(phrases), L.BOOST)):
                want, gap = R.prefix_beam(ids, lp, 0, beam, beam, trie=trie, boost=boost)
                got, gap_lm = L.prefix_beam_lm(ids, lp, 0, beam, beam, image, 0.0, 0.0, -0.5, trie=trie, boost=boost)
                assert [(h["tokens"], h["score"], h["ctc_score"]) for h in got] == [(h["tokens"], h["score"], h["ctc_score"]) for h in want] and gap == gap_lm


@pytest.mark.parametrize("T, k", [(3, 2), (4, 3), (5, 3), (5, 2)])
def test_without_pruning_every_score_is_the_brute_force_sum_plus_the_lm_terms(T, k):
    vocab, alpha, beta, oov = 5, 0.7, 0.3, -0.9
    for order, eos in ((2, True), (3, False), (4, True)):
        ngrams = L.random_arpa(order, vocab, order, 0.5, eos=eos)
        image = L.build_image(ngrams, vocab)
        v = L.view(image)
        for seed in range(3):
            ids, lp = R.random_case(seed, T, k, vocab)
            exact = R.brute_force(ids, lp, 0)
            hyps, _ = L.prefix_beam_lm(ids, lp, 0, 10 ** 6, 10 ** 6, image, alpha, beta, oov)
            assert {tuple(h["tokens"]) for h in hyps} == set(exact)
            for h in hyps:
                logps, end = L.arpa_sequence(ngrams, vocab, h["tokens"], oov)                   # the independent scorer
                want = exact[tuple(h["tokens"])] + alpha * sum(logps) + beta * len(h["tokens"]) + (alpha * end if eos else 0.0)
                assert abs(h["ctc_score"] - exact[tuple(h["tokens"])]) <= 1e-9 and abs(h["score"] - want) <= 1e-9, (h, want)
                lm, end_term = L.score_tokens(v, h["tokens"], alpha, beta, oov)
                assert abs(h["lm"] - float(lm + end_term)) <= 1e-12


@pytest.mark.parametrize("order", L.ORDERS)
@pytest.mark.parametrize("shape", L.SHAPES, ids=lambda s: "T%d_k%d_b%d_v%d" % s)
def test_the_gpu_cases_are_clear_change_the_best_hypothesis_and_survive_float32(shape, order):
    """The conditions of test_ctc_lm_beam_gpu.py, and the figure its tolerance is 6 x of: over all shapes, orders and both hotword settings the float32
    restatement's largest score difference is 4.4e-5 (T = 137), printed here per case set."""
    T, topk, beam, vocab = shape
    image = L.shape_model(vocab, order)[1]
    worst = 0.0
    for hot in (False, True):
        cases = L.shape_cases(shape, order, hot)
        assert len(cases) == 2, f"{len(cases)} of 32 seeds have a decision gap >= {L.GAP}"
        assert all(c[5] >= L.GAP for c in cases) and any(c[6] for c in cases), "no chosen case whose best hypothesis the model changes"
        for seed, ids, lp, phrases, hyps, gap, differs in cases:
            trie = R.build_trie(phrases) if hot else None
            h32, _ = L.prefix_beam_lm(ids, lp, 0, beam, beam, image, L.ALPHA, L.BETA, L.OOV, trie=trie, boost=L.BOOST if hot else 0.0, dtype=np.float32)
            assert [h["tokens"] for h in h32] == [h["tokens"] for h in hyps]
            worst = max([worst] + [max(abs(a["score"] - b["score"]), abs(a["ctc_score"] - b["ctc_score"])) for a, b in zip(h32, hyps)])
    print(f"shape {shape} order {order}: float32 restatement differs by at most {worst:.2e}")
    assert 6 * worst <= 6 * 4.4e-5                                     # the figure the GPU tolerance quotes still holds
