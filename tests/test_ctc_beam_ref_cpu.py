"""CPU: the float64 statement of the CTC prefix beam search (tests/ctc_beam_ref.py) against facts that do not depend on it."""
import numpy as np

import ctc_beam_ref as R


def test_beam_one_is_the_collapse_of_the_argmax():
    for seed in range(6):
        ids, lp = R.random_case(seed, 23, 1, 7)
        hyps, gap = R.prefix_beam(ids, lp, 0, beam=1, nbest=1)
        assert len(hyps) == 1 and hyps[0]["tokens"] == R.collapse(ids[:, 0], 0)
        want = float(lp.astype(np.float64).sum())
        assert abs(hyps[0]["ctc_score"] - want) <= 1e-12 * abs(want) and hyps[0]["score"] == hyps[0]["ctc_score"]
        assert gap == np.inf                                          # one entry per frame: nothing was ever dropped


def test_wide_beam_scores_equal_the_sum_over_all_alignments():
    checked = 0
    for seed in range(8):
        ids, lp = R.random_case(seed, 5, 2, 4)
        want = R.brute_force(ids, lp, 0)
        hyps, _ = R.prefix_beam(ids, lp, 0, beam=len(want), nbest=len(want))
        assert len(hyps) == len(want) and {tuple(h["tokens"]) for h in hyps} == set(want)
        for h in hyps:
            assert abs(h["ctc_score"] - want[tuple(h["tokens"])]) <= 1e-12
        assert all(a["score"] >= b["score"] for a, b in zip(hyps[:-1], hyps[1:]))
        checked += len(want) > 2
    assert checked >= 4


def _two_way():
    # frame 0 decides between tokens 1 and 2 (0.6 / 0.4), frame 1 appends 3: hypotheses [1, 3] then [2, 3]
    ids = np.array([[1, 2], [3, 0], [0, 3]], dtype=np.int32)
    lp = np.log(np.array([[0.6, 0.4], [0.9, 0.1], [0.9, 0.1]]))
    return ids, lp


def test_hotword_moves_the_second_hypothesis_to_the_front():
    ids, lp = _two_way()
    plain, _ = R.prefix_beam(ids, lp, 0, beam=4, nbest=4)
    assert plain[0]["tokens"] == [1, 3] and plain[1]["tokens"] == [2, 3]
    diff = plain[0]["score"] - plain[1]["score"]
    boost = diff / 2 + 0.1                                            # two matched tokens: 2 * boost > diff
    hot, _ = R.prefix_beam(ids, lp, 0, beam=4, nbest=4, trie=R.build_trie([[2, 3]]), boost=boost)
    assert hot[0]["tokens"] == [2, 3] and hot[1]["tokens"] == [1, 3]
    by_tokens = {tuple(h["tokens"]): h for h in plain}
    for h in hot:                                                      # the plain CTC score is reported beside the boosted one, unchanged
        assert abs(h["ctc_score"] - by_tokens[tuple(h["tokens"])]["ctc_score"]) <= 1e-12
    assert abs(hot[0]["score"] - hot[0]["ctc_score"] - 2 * boost) <= 1e-12 and hot[1]["score"] == hot[1]["ctc_score"]


def test_half_matched_phrase_ends_without_bonus():
    ids, lp = _two_way()
    trie = R.build_trie([[2, 3, 4], [1, 3, 3, 4]])
    hot, _ = R.prefix_beam(ids, lp, 0, beam=4, nbest=4, trie=trie, boost=5.0)
    assert {tuple(h["tokens"]) for h in hot} >= {(1, 3), (2, 3)}
    for h in hot:                                                      # every hypothesis ends inside a phrase (or never entered one)
        assert h["score"] == h["ctc_score"], h
    # taken back in the middle too: [2, 3] matched, then 1 breaks it and starts the other phrase, which the end takes back as well
    node, bonus = 0, 0.0
    for c, want in ((2, 5.0), (3, 10.0), (1, 5.0), (3, 10.0), (2, 5.0)):
        node, bonus = R.trie_step(trie, node, bonus, c, 5.0)
        assert bonus == want, (c, bonus)
    # a completed phrase keeps its bonus and returns to the root
    t2 = R.build_trie([[7, 8]])
    node, bonus = R.trie_step(t2, 0, 0.0, 7, 1.5)
    node, bonus = R.trie_step(t2, node, bonus, 8, 1.5)
    assert (node, bonus) == (0, 3.0)
    node, bonus = R.trie_step(t2, node, bonus, 9, 1.5)
    assert (node, bonus) == (0, 3.0)


def test_trie_layout():
    t = R.build_trie([[5, 2], [5], [3, 9, 9]])
    assert t["depth"][0] == 0 and t["child_off"][0] == 0 and t["child_off"][-1] == t["child_tok"].size == t["depth"].size - 1
    for n in range(t["depth"].size):
        toks = t["child_tok"][t["child_off"][n]:t["child_off"][n + 1]]
        assert (np.diff(toks) > 0).all()
        for ch in t["child_node"][t["child_off"][n]:t["child_off"][n + 1]]:
            assert t["depth"][ch] == t["depth"][n] + 1
    assert int(t["is_end"].sum()) == 3


def test_content_identity_differs_from_parent_token_identity():
    """The input test_ctc_prefix_beam_gpu.py feeds the kernel: a prefix is dropped and created again while a descendant of its first incarnation
    lives; under (parent node, token) identity the extension of the second incarnation misses that descendant."""
    ids, lp = R.missed_merge_case()
    good, gap = R.prefix_beam(ids, lp, 0, beam=2, nbest=2)
    bad, _ = R.prefix_beam(ids, lp, 0, beam=2, nbest=2, identity="node")
    assert gap >= 1e-3
    assert [h["tokens"] for h in good] != [h["tokens"] for h in bad] or max(abs(a["score"] - b["score"]) for a, b in zip(good, bad)) > 1e-2
