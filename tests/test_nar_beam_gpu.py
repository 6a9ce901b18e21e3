"""GPU, op level: the beam search over token rows (asr_op_nar_beam -> nar_beam_kernel, both instantiations) against its float64 statement
(tests/nar_beam_ref.py): no model, orders 2 and 4, plain and with hotwords.

The cases are nar_beam_ref.shape_cases': seeds whose decision gap is >= 1e-3, under a model one of them with a best hypothesis the search without a model does
not return (test_nar_beam_ref_cpu.py holds both as conditions). Token lists and counts must be equal; score and am_score within TOL = 2.46e-4: a float32
restatement of the reference differs from float64 by at most 4.1e-5 over these cases (test_nar_beam_ref_cpu.py prints it), 6 x that is 2.46e-4, and the bound
is never more than a quarter of the gap. Measured on an MI355X: at most 4.1e-5 over all cases here (the kernel's sums are the float32 restatement's)."""
import numpy as np
import pytest

import ctc_beam_ref as R
import ctc_lm_ref as L
import nar_beam_ref as N
from conftest import sub

pytestmark = pytest.mark.gpu

GAP = L.GAP
F32_RESTATEMENT = 4.1e-5
TOL = min(6 * F32_RESTATEMENT, GAP / 4)
assert TOL <= min(6 * F32_RESTATEMENT, GAP / 4) and TOL == pytest.approx(2.46e-4)


def _run(eng, ids_list, lp_list, beam, nbest, image=None, phrases=None, boost=0.0, alpha=L.ALPHA, beta=L.BETA, oov=L.OOV):
    lens = [i.shape[0] for i in ids_list]
    trie = eng.hotword_trie(phrases) if phrases else None
    return eng.op_nar_beam(np.concatenate(ids_list), np.concatenate(lp_list), lens, beam, nbest, trie=trie, boost=boost, lm=image, alpha=alpha, beta=beta,
                           oov_logprob=oov)


def _compare(got, b, hyps, nbest):
    tok, num, score, am, tlp = got
    worst = 0.0
    for n in range(nbest):
        if n < len(hyps):
            h = hyps[n]
            assert num[b, n] == len(h["tokens"]) and tok[b, n, :num[b, n]].tolist() == h["tokens"], (n, tok[b, n, :num[b, n]].tolist(), h["tokens"])
            assert tlp[b, n, :num[b, n]].tolist() == [float(np.float32(x)) for x in h["logprob"]]        # the candidates' own values, bit for bit
            err = max(abs(float(score[b, n]) - h["score"]), abs(float(am[b, n]) - h["am_score"]))
            print(f"  hypothesis {n}: score error {err:.2e}")
            assert err <= TOL, (n, float(score[b, n]), h["score"], float(am[b, n]), h["am_score"])
            worst = max(worst, err)
        else:
            assert num[b, n] == 0 and score[b, n] == -np.inf and am[b, n] == -np.inf
    return worst


@pytest.mark.parametrize("hot", [False, True], ids=["plain", "hotwords"])
@pytest.mark.parametrize("order", N.MODELS, ids=lambda o: f"order{o}" if o else "no_model")
@pytest.mark.parametrize("shape", N.SHAPES, ids=lambda s: "N%d_k%d_b%d_v%d" % s)
def test_search_equals_the_float64_statement(shape, order, hot):
    eng = sub("engine")
    n, topk, beam, vocab = shape
    cases = N.shape_cases(shape, order, hot)
    assert len(cases) == 2
    worst = 0.0
    for seed, ids, lp, phrases, hyps, gap, differs in cases:
        _, boost, image, _ = N.case_setting(shape, order, hot, seed)
        print(f"shape {shape} model {order} hot {hot} seed {seed}: {len(hyps)} hypotheses, gap {gap:.2e}, best differs from the search without a model: {differs}")
        assert gap >= GAP
        got = _run(eng, [ids], [lp], beam, beam, image, phrases, boost)
        worst = max(worst, _compare(got, 0, hyps, beam))
        if differs:                                        # ... and the op without a model really returns something else
            plain = _run(eng, [ids], [lp], beam, beam, None, phrases, boost)
            assert plain[0][0, 0, :plain[1][0, 0]].tolist() != hyps[0]["tokens"]
    print(f"largest score error {worst:.2e}")


def test_a_ragged_batch_with_an_empty_utterance_and_byte_equal_reruns():
    eng = sub("engine")
    vocab, order, beam, nbest, k = 12, 4, 4, 3, 3
    image = L.shape_model(vocab, order)[1]
    v = L.view(image)
    phrases = R.random_phrases(0, 3, vocab)
    trie = R.build_trie(phrases)
    ids_list, lp_list, refs = [], [], []
    for n in (40, 137, 0, 9):                              # seeds by the cases' rule: the first whose decisions are clear under this call's setting
        for seed in range(N.SEEDS):
            ids, lp = N.random_case(seed, n, k, vocab)
            hyps, gap = N.nar_beam(ids, lp, beam, nbest, trie, L.BOOST, image, L.ALPHA, L.BETA, L.OOV)
            if gap >= GAP:
                break
        ids_list.append(ids); lp_list.append(lp); refs.append((hyps, gap))
    a = _run(eng, ids_list, lp_list, beam, nbest, image, phrases, L.BOOST)
    b = _run(eng, ids_list, lp_list, beam, nbest, image, phrases, L.BOOST)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    clear = 0
    for u, (hyps, gap) in enumerate(refs):
        single = _run(eng, [ids_list[u]], [lp_list[u]], beam, nbest, image, phrases, L.BOOST)
        for x, y in zip(a, single):                      # an utterance of a batch equals the same utterance alone, bit for bit
            n = y.shape[-1] if x.ndim == 3 else None
            assert (x[u, :, :n] if n else x[u]).tobytes() == y[0].tobytes()
        if gap >= GAP:
            clear += 1
            _compare(a, u, hyps, nbest)
    assert clear == 4
    # the empty utterance: one empty hypothesis, score = the </s> term alone, am_score 0
    tok, num, score, am, _ = a
    end = L.ALPHA * float(L.lm_step(v, v["start_node"], v["eos"], L.OOV)[0])
    assert num[2].tolist() == [0, 0, 0] and am[2, 0] == 0.0 and abs(float(score[2, 0]) - end) <= 1e-6 and np.all(score[2, 1:] == -np.inf) and np.all(am[2, 1:] == -np.inf)
    plain = _run(eng, [ids_list[2]], [lp_list[2]], beam, nbest)
    assert plain[1][0].tolist() == [0, 0, 0] and plain[2][0, 0] == 0.0 and plain[3][0, 0] == 0.0 and np.all(plain[2][0, 1:] == -np.inf)


def test_a_zero_weight_model_is_the_search_without_one_bit_for_bit():
    eng = sub("engine")
    for shape in ((40, 8, 8, 20), (64, 16, 16, 40)):
        n, topk, beam, vocab = shape
        image = L.shape_model(vocab, 4, eos=False)[1]
        assert L.view(image)["eos"] == -1
        ids, lp = N.random_case(3, n, topk, vocab)
        phrases = R.random_phrases(3, 3, vocab)
        want = _run(eng, [ids], [lp], beam, beam, None, phrases, L.BOOST)
        got = _run(eng, [ids], [lp], beam, beam, image, phrases, L.BOOST, alpha=0.0, beta=0.0, oov=-0.5)
        for x, y in zip(want, got):
            assert x.tobytes() == y.tobytes()


def test_out_of_vocabulary_tokens_cost_oov_and_keep_the_state():
    """A model that knows token 5 alone (and <s>): rows that offer only unknown tokens score as without a model at oov 0, cost oov per token otherwise, and
    the 5 after them is scored in the <s> context -- P(5 | <s>), not the unigram reached through a back-off."""
    eng = sub("engine")
    vocab, B = 8, 9
    ln = float(np.log(10.0))
    ngrams = {(B,): (0.0, -1.5 * ln), (5,): (-2.0 * ln, -0.25 * ln), (B, 5): (-0.125 * ln, 0.0)}
    image = L.build_image(ngrams, vocab)
    ids = np.array([[3, 0], [1, 4], [4, 0], [2, 6]], dtype=np.int32)
    lp = np.log(np.array([[0.7, 0.3], [0.6, 0.4], [0.8, 0.2], [0.55, 0.45]])).astype(np.float32)
    want = _run(eng, [ids], [lp], 4, 4)
    got = _run(eng, [ids], [lp], 4, 4, image, alpha=1.0, beta=0.0, oov=0.0)
    for x, y in zip(want, got):
        assert x.tobytes() == y.tobytes()
    cost = _run(eng, [ids], [lp], 4, 4, image, alpha=1.0, beta=0.0, oov=-0.5)
    assert cost[0].tobytes() == want[0].tobytes() and np.allclose(cost[2] - cost[3], -2.0, atol=1e-6)      # four tokens at alpha * oov each
    ids5 = np.concatenate([ids, np.array([[5, 0]], dtype=np.int32)])
    lp5 = np.concatenate([lp, np.log(np.array([[0.9, 0.1]])).astype(np.float32)])
    tok, num, score, am, _ = _run(eng, [ids5], [lp5], 4, 1, image, alpha=1.0, beta=0.0, oov=0.0)
    hyps, gap = N.nar_beam(ids5, lp5, 4, 1, image=image, alpha=1.0, beta=0.0, oov=0.0)
    assert gap >= GAP and tok[0, 0, :num[0, 0]].tolist() == hyps[0]["tokens"] and hyps[0]["tokens"][-1] == 5
    lm = float(score[0, 0]) - float(am[0, 0])
    assert abs(lm - (-0.125 * ln)) <= 1e-5, (lm, -0.125 * ln, (-1.5 - 2.0) * ln)


def test_the_end_of_sentence_term():
    eng = sub("engine")
    n, topk, beam, vocab = 40, 8, 8, 20
    with_eos, image = L.shape_model(vocab, 2)
    without = {g: v for g, v in with_eos.items() if vocab not in g}
    image0 = L.build_image(without, vocab)
    assert L.view(image)["eos"] == vocab and L.view(image0)["eos"] == -1
    seen = 0
    for seed in range(N.SEEDS):
        ids, lp = N.random_case(seed, n, topk, vocab)
        h1, g1 = N.nar_beam(ids, lp, beam, beam, image=image, alpha=L.ALPHA, beta=L.BETA, oov=L.OOV)
        h0, g0 = N.nar_beam(ids, lp, beam, beam, image=image0, alpha=L.ALPHA, beta=L.BETA, oov=L.OOV)
        if min(g0, g1) < GAP:
            continue
        a, b = _run(eng, [ids], [lp], beam, beam, image), _run(eng, [ids], [lp], beam, beam, image0)
        _compare(a, 0, h1, beam)
        _compare(b, 0, h0, beam)
        by0 = {tuple(b[0][0, m, :b[1][0, m]].tolist()): float(b[2][0, m]) for m in range(len(h0))}
        v = L.view(image)
        for m in range(len(h1)):                         # the same live set (the term is added after the last row): scores differ by alpha * log P(</s> | state)
            toks = tuple(a[0][0, m, :a[1][0, m]].tolist())
            end = float(L.score_tokens(v, toks, L.ALPHA, L.BETA, L.OOV)[1])
            assert end < 0 and abs(float(a[2][0, m]) - by0[toks] - end) <= 1e-4
        seen += 1
        if seen == 2:
            break
    assert seen == 2


def test_hypotheses_beyond_those_found_are_empty():
    eng = sub("engine")
    ids, lp = N.random_case(0, 2, 2, 6)
    tok, num, score, am, tlp = _run(eng, [ids], [lp], 8, 8)
    want = N.brute_force(ids, lp)
    assert len(want) == 4
    for m, (tokens, total) in enumerate(want):
        assert num[0, m] == 2 and tok[0, m].tolist() == tokens and abs(float(am[0, m]) - total) <= 1e-6 and score[0, m] == am[0, m]
    assert np.all(num[0, 4:] == 0) and np.all(score[0, 4:] == -np.inf) and np.all(am[0, 4:] == -np.inf)
    inf = lp.copy()
    inf[1, 1] = -np.inf                                    # a candidate without probability makes no entry
    tok, num, score, am, tlp = _run(eng, [ids], [inf], 8, 8)
    assert num[0].tolist() == [2, 2, 0, 0, 0, 0, 0, 0] and tok[0, :2, 1].tolist() == [int(ids[1, 0])] * 2


def test_malformed_arguments_raise():
    eng, lib = sub("engine"), sub("_lib")
    vocab = 12
    image = L.shape_model(vocab, 4)[1]
    ids, lp = N.random_case(0, 9, 3, vocab)
    _run(eng, [ids], [lp], 2, 2, image)                    # the arguments themselves are fine
    with pytest.raises(lib.AsrError):
        _run(eng, [ids], [lp], 17, 1)
    with pytest.raises(lib.AsrError):
        _run(eng, [ids], [lp], 2, 3)
    with pytest.raises(lib.AsrError):
        _run(eng, [np.repeat(ids, 6, axis=1)[:, :17]], [np.repeat(lp, 6, axis=1)[:, :17]], 2, 2)         # topk 17
    dup = ids.copy()
    dup[4, 1] = dup[4, 0]
    with pytest.raises(lib.AsrError, match="twice"):
        _run(eng, [dup], [lp], 2, 2)
    wide = ids.copy()
    wide[4, 0] = vocab + 1                                 # a candidate the model's tables do not cover
    with pytest.raises(lib.AsrError, match="vocabulary"):
        _run(eng, [wide], [lp], 2, 2, image)
    for kw in (dict(alpha=np.nan), dict(alpha=-1.0), dict(beta=np.inf), dict(oov=0.5)):
        with pytest.raises(lib.AsrError):
            _run(eng, [ids], [lp], 2, 2, image, **kw)
    with pytest.raises(lib.AsrError):
        _run(eng, [ids], [lp], 2, 2, image[:-7].copy())
