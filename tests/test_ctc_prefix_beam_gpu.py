"""GPU, op level: the CTC prefix beam search kernel (asr_op_ctc_prefix_beam -> ctc_prefix_beam_kernel) against its float64 statement
(tests/ctc_beam_ref.py), plain and with hotwords.

A discrete result can be compared only where the reference's own decisions are no near-ties: per shape the first two seeds in 0..31 whose decision gap
(last kept against first dropped entry at every frame, neighbouring final hypotheses) is >= 1e-3 are used, and fewer than two is a failure. Token lists and
counts must be equal; scores within 2.5e-4 absolute: a float32 restatement of the same recurrences differs from float64 by at most 4.0e-5 over 72 such cases
(T <= 137, beam <= 16) and never in a token; the bound is 6 x that and a quarter of the gap. Measured on an MI355X: at most 5.8e-5 over all cases here."""
import functools

import numpy as np
import pytest

import ctc_beam_ref as R
from conftest import sub

pytestmark = pytest.mark.gpu

SHAPES = [(5, 2, 1, 6), (9, 3, 2, 5), (40, 4, 4, 12), (48, 8, 8, 20), (137, 4, 3, 8), (300, 2, 2, 5), (64, 16, 16, 40)]
GAP, TOL, BOOST = 1e-3, 2.5e-4, 1.5


@functools.lru_cache(maxsize=None)
def _cases(shape, hot):
    """The first two seeds whose reference decisions are clear, with the reference's answer (computed once, shared, never modified)."""
    T, topk, beam, vocab = shape
    out = []
    for seed in range(32):
        ids, lp = R.random_case(seed, T, topk, vocab)
        phrases = R.random_phrases(seed, 3, vocab) if hot else None
        hyps, gap = R.prefix_beam(ids, lp, 0, beam, beam, trie=R.build_trie(phrases) if hot else None, boost=BOOST if hot else 0.0)
        if gap >= GAP:
            out.append((seed, ids, lp, phrases, hyps))
            if len(out) == 2:
                break
    return out


def _run(eng, ids_list, lp_list, beam, nbest, phrases=None, boost=0.0):
    lens = [i.shape[0] for i in ids_list]
    trie = eng.hotword_trie(phrases) if phrases else None
    tok, num, score, ctc = eng.op_ctc_prefix_beam(np.concatenate(ids_list), np.concatenate(lp_list), lens, beam, nbest, blank_id=0, trie=trie, boost=boost)
    return tok, num, score, ctc


def _compare(got, b, hyps, nbest):
    tok, num, score, ctc = got
    for n in range(nbest):
        if n < len(hyps):
            h = hyps[n]
            assert num[b, n] == len(h["tokens"]) and tok[b, n, :num[b, n]].tolist() == h["tokens"], (n, tok[b, n, :num[b, n]].tolist(), h["tokens"])
            err = max(abs(float(score[b, n]) - h["score"]), abs(float(ctc[b, n]) - h["ctc_score"]))
            print(f"  hypothesis {n}: score error {err:.2e}")
            assert err <= TOL, (n, float(score[b, n]), h["score"], float(ctc[b, n]), h["ctc_score"])
        else:
            assert num[b, n] == 0 and score[b, n] == -np.inf and ctc[b, n] == -np.inf


@pytest.mark.parametrize("hot", [False, True], ids=["plain", "hotwords"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d_k%d_b%d_v%d" % s)
def test_search_equals_the_float64_statement(shape, hot):
    eng = sub("engine")
    T, topk, beam, vocab = shape
    cases = _cases(shape, hot)
    assert len(cases) == 2, f"{len(cases)} of 32 seeds have a decision gap >= {GAP}"
    for seed, ids, lp, phrases, hyps in cases:
        print(f"shape {shape} hot {hot} seed {seed}: {len(hyps)} hypotheses")
        _compare(_run(eng, [ids], [lp], beam, beam, phrases, BOOST if hot else 0.0), 0, hyps, beam)


def test_three_ragged_utterances_in_one_call_and_byte_equal_reruns():
    eng = sub("engine")
    picks = [_cases((40, 4, 4, 12), True)[0], _cases((137, 4, 3, 8), True)[0], _cases((9, 3, 2, 5), True)[0]]
    # one hotword list and one (beam, nbest) per call: re-state the reference for the shared setting (decision gaps re-checked)
    phrases, beam, nbest = picks[0][3], 4, 3
    # topk differs between the shapes: narrow every utterance to the smallest
    k = min(p[1].shape[1] for p in picks)
    ids_list, lp_list = [p[1][:, :k] for p in picks], [p[2][:, :k] for p in picks]
    refs = [R.prefix_beam(i, l, 0, beam, nbest, trie=R.build_trie(phrases), boost=BOOST) for i, l in zip(ids_list, lp_list)]
    a = _run(eng, ids_list, lp_list, beam, nbest, phrases, BOOST)
    b = _run(eng, ids_list, lp_list, beam, nbest, phrases, BOOST)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    clear = 0
    for u, (hyps, gap) in enumerate(refs):
        single = _run(eng, [ids_list[u]], [lp_list[u]], beam, nbest, phrases, BOOST)
        for x, y in zip(a, single):                      # an utterance of a batch equals the same utterance alone, bit for bit
            n = y.shape[-1] if x.ndim == 3 else None
            assert (x[u, :, :n] if n else x[u]).tobytes() == y[0].tobytes()
        if gap >= GAP:
            clear += 1
            _compare(a, u, hyps, nbest)
    assert clear >= 2


def test_recreated_prefix_merges_into_its_live_descendant():
    """Vocabulary 3, beam 2: [1, 2] is dropped while [1, 2, 1] lives and is created again later; its extension by 1 must reach the live [1, 2, 1]. A search
    that identifies prefixes by (parent node, token) returns [1, 2, 1] twice with split scores (test_ctc_beam_ref_cpu.py shows the two differ)."""
    eng = sub("engine")
    ids, lp = R.missed_merge_case()
    hyps, gap = R.prefix_beam(ids, lp, 0, 2, 2)
    wrong, _ = R.prefix_beam(ids, lp, 0, 2, 2, identity="node")
    assert gap >= GAP and abs(hyps[0]["score"] - wrong[0]["score"]) > 0.1
    got = _run(eng, [ids], [lp], 2, 2)
    _compare(got, 0, hyps, 2)
    assert got[0][0, 0, :got[1][0, 0]].tolist() != got[0][0, 1, :got[1][0, 1]].tolist()


def test_argument_errors():
    eng, lib = sub("engine"), sub("_lib")
    ids, lp = R.random_case(0, 5, 2, 6)
    with pytest.raises(lib.AsrError):
        eng.op_ctc_prefix_beam(ids, lp, [5], beam=17)
    with pytest.raises(lib.AsrError):
        eng.op_ctc_prefix_beam(ids, lp, [5], beam=2, nbest=3)
    dup = ids.copy()
    dup[2, 1] = dup[2, 0]
    with pytest.raises(lib.AsrError, match="twice"):
        eng.op_ctc_prefix_beam(dup, lp, [5], beam=2)
