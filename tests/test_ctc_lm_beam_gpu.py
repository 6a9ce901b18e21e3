"""GPU, op level: the CTC prefix beam search with an n-gram language model fused in (asr_op_ctc_prefix_beam_lm -> ctc_prefix_beam_kernel<true>) against its
float64 statement (tests/ctc_lm_ref.py), orders 2 and 4, plain and with hotwords.

The cases are ctc_lm_ref.shape_cases': seeds whose decision gap under the model is >= 1e-3, one of them with a best hypothesis the search without a model does
not return (test_ctc_lm_ref_cpu.py holds both as conditions). Token lists and counts must be equal; score and ctc_score within TOL = 2.5e-4: a float32
restatement of the reference differs from float64 by at most 4.4e-5 over these cases (test_ctc_lm_ref_cpu.py prints it), 6 x that is 2.6e-4, and the bound is
never more than a quarter of the gap. Measured on an MI355X: at most 4.4e-5 over all cases here."""
import numpy as np
import pytest

import ctc_beam_ref as R
import ctc_lm_ref as L
from conftest import sub

pytestmark = pytest.mark.gpu

GAP, TOL = L.GAP, 2.5e-4
F32_RESTATEMENT = 4.4e-5
assert TOL <= min(6 * F32_RESTATEMENT, GAP / 4)


def _run(eng, ids_list, lp_list, beam, nbest, image=None, phrases=None, boost=0.0, alpha=L.ALPHA, beta=L.BETA, oov=L.OOV):
    lens = [i.shape[0] for i in ids_list]
    trie = eng.hotword_trie(phrases) if phrases else None
    return eng.op_ctc_prefix_beam(np.concatenate(ids_list), np.concatenate(lp_list), lens, beam, nbest, blank_id=0, trie=trie, boost=boost, lm=image, alpha=alpha,
                                  beta=beta, oov_logprob=oov)


def _compare(got, b, hyps, nbest):
    tok, num, score, ctc = got
    worst = 0.0
    for n in range(nbest):
        if n < len(hyps):
            h = hyps[n]
            assert num[b, n] == len(h["tokens"]) and tok[b, n, :num[b, n]].tolist() == h["tokens"], (n, tok[b, n, :num[b, n]].tolist(), h["tokens"])
            err = max(abs(float(score[b, n]) - h["score"]), abs(float(ctc[b, n]) - h["ctc_score"]))
            print(f"  hypothesis {n}: score error {err:.2e}")
            assert err <= TOL, (n, float(score[b, n]), h["score"], float(ctc[b, n]), h["ctc_score"])
            worst = max(worst, err)
        else:
            assert num[b, n] == 0 and score[b, n] == -np.inf and ctc[b, n] == -np.inf
    return worst


@pytest.mark.parametrize("hot", [False, True], ids=["plain", "hotwords"])
@pytest.mark.parametrize("order", L.ORDERS, ids=lambda o: f"order{o}")
@pytest.mark.parametrize("shape", L.SHAPES, ids=lambda s: "T%d_k%d_b%d_v%d" % s)
def test_search_with_a_language_model_equals_the_float64_statement(shape, order, hot):
    eng = sub("engine")
    T, topk, beam, vocab = shape
    cases = L.shape_cases(shape, order, hot)
    assert len(cases) == 2 and any(c[6] for c in cases)
    image = L.shape_model(vocab, order)[1]
    worst = 0.0
    for seed, ids, lp, phrases, hyps, gap, differs in cases:
        print(f"shape {shape} order {order} hot {hot} seed {seed}: {len(hyps)} hypotheses, gap {gap:.2e}, best differs from the plain search: {differs}")
        got = _run(eng, [ids], [lp], beam, beam, image, phrases, L.BOOST if hot else 0.0)
        worst = max(worst, _compare(got, 0, hyps, beam))
        if differs:                                        # ... and the op without a model really returns something else
            plain = _run(eng, [ids], [lp], beam, beam, None, phrases, L.BOOST if hot else 0.0)
            assert plain[0][0, 0, :plain[1][0, 0]].tolist() != hyps[0]["tokens"]
    print(f"largest score error {worst:.2e}")


def test_three_ragged_utterances_in_one_call_and_byte_equal_reruns():
    eng = sub("engine")
    vocab, order, beam, nbest, k = 12, 4, 4, 3, 3
    image = L.shape_model(vocab, order)[1]
    phrases = R.random_phrases(0, 3, vocab)
    trie = R.build_trie(phrases)
    ids_list, lp_list, refs = [], [], []
    for T in (40, 137, 9):                                 # seeds by the same rule: the first whose decisions are clear under this call's setting
        for seed in range(32):
            ids, lp = R.random_case(seed, T, k, vocab)
            hyps, gap = L.prefix_beam_lm(ids, lp, 0, beam, nbest, image, L.ALPHA, L.BETA, L.OOV, trie=trie, boost=L.BOOST)
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
    assert clear >= 2


def test_a_zero_weight_model_is_the_search_without_one_bit_for_bit():
    eng = sub("engine")
    for shape in ((40, 4, 4, 12), (64, 16, 16, 40)):
        T, topk, beam, vocab = shape
        image = L.shape_model(vocab, 4, eos=False)[1]
        assert L.view(image)["eos"] == -1
        ids, lp = R.random_case(3, T, topk, vocab)
        phrases = R.random_phrases(3, 3, vocab)
        want = _run(eng, [ids], [lp], beam, beam, None, phrases, L.BOOST)
        got = _run(eng, [ids], [lp], beam, beam, image, phrases, L.BOOST, alpha=0.0, beta=0.0, oov=-0.5)
        for x, y in zip(want, got):
            assert x.tobytes() == y.tobytes()


def test_out_of_vocabulary_tokens_cost_nothing_by_default_and_keep_the_state():
    """A model that knows token 5 alone (and <s>): rows that emit only unknown tokens score as without a model, and the 5 after them is scored in the <s>
    context -- P(5 | <s>), not the unigram reached through a back-off."""
    eng = sub("engine")
    vocab, E, B = 8, 8, 9
    ln = float(np.log(10.0))
    ngrams = {(B,): (0.0, -1.5 * ln), (5,): (-2.0 * ln, -0.25 * ln), (B, 5): (-0.125 * ln, 0.0)}
    image = L.build_image(ngrams, vocab)
    ids = np.array([[3, 0], [0, 4], [4, 0], [0, 6]], dtype=np.int32)
    lp = np.log(np.array([[0.7, 0.3], [0.6, 0.4], [0.8, 0.2], [0.6, 0.4]])).astype(np.float32)
    want = _run(eng, [ids], [lp], 4, 4)
    got = _run(eng, [ids], [lp], 4, 4, image, alpha=1.0, beta=0.0, oov=0.0)
    for x, y in zip(want, got):
        assert x.tobytes() == y.tobytes()
    ids5 = np.concatenate([ids, np.array([[5, 0]], dtype=np.int32)])
    lp5 = np.concatenate([lp, np.log(np.array([[0.9, 0.1]])).astype(np.float32)])
    tok, num, score, ctc = _run(eng, [ids5], [lp5], 4, 1, image, alpha=1.0, beta=0.0, oov=0.0)
    hyps, gap = L.prefix_beam_lm(ids5, lp5, 0, 4, 1, image, 1.0, 0.0, 0.0)
    assert gap >= GAP and tok[0, 0, :num[0, 0]].tolist() == hyps[0]["tokens"] and hyps[0]["tokens"][-1] == 5
    lm = float(score[0, 0]) - float(ctc[0, 0])
    assert abs(lm - (-0.125 * ln)) <= 1e-5, (lm, -0.125 * ln, (-1.5 - 2.0) * ln)


def test_the_end_of_sentence_term():
    eng = sub("engine")
    T, topk, beam, vocab = 40, 4, 4, 12
    with_eos, image = L.shape_model(vocab, 2)
    without = {g: v for g, v in with_eos.items() if vocab not in g}
    image0 = L.build_image(without, vocab)
    assert L.view(image)["eos"] == vocab and L.view(image0)["eos"] == -1
    seen = 0
    for seed in range(32):
        ids, lp = R.random_case(seed, T, topk, vocab)
        h1, g1 = L.prefix_beam_lm(ids, lp, 0, beam, beam, image, L.ALPHA, L.BETA, L.OOV)
        h0, g0 = L.prefix_beam_lm(ids, lp, 0, beam, beam, image0, L.ALPHA, L.BETA, L.OOV)
        if min(g0, g1) < GAP:
            continue
        a, b = _run(eng, [ids], [lp], beam, beam, image), _run(eng, [ids], [lp], beam, beam, image0)
        _compare(a, 0, h1, beam)
        _compare(b, 0, h0, beam)
        by0 = {tuple(b[0][0, n, :b[1][0, n]].tolist()): float(b[2][0, n]) for n in range(len(h0))}
        v = L.view(image)
        for n in range(len(h1)):                         # the same live set (the term is added after the last frame): scores differ by alpha * log P(</s> | state)
            toks = tuple(a[0][0, n, :a[1][0, n]].tolist())
            end = float(L.score_tokens(v, toks, L.ALPHA, L.BETA, L.OOV)[1])
            assert end < 0 and abs(float(a[2][0, n]) - by0[toks] - end) <= 1e-4
        seen += 1
        if seen == 2:
            break
    assert seen == 2


def test_malformed_images_and_arguments_raise():
    eng, lib = sub("engine"), sub("_lib")
    vocab = 12
    image = L.shape_model(vocab, 4)[1]
    v = L.view(image)
    ids, lp = R.random_case(0, 9, 3, vocab)
    at, n, m = {}, v["n_nodes"], v["n_edges"]
    pos = L.HEADER
    for name, size in (("depth", n), ("backoff", n), ("suffix", n), ("child_off", n + 1), ("tok", m), ("logp", m), ("next", m), ("uni", vocab + 2)):
        at[name] = pos
        pos += size
    run = lambda img, **kw: _run(eng, [ids], [lp], 2, 2, img, **kw)
    run(image)                                             # the image itself is fine
    node = next(i for i in range(n) if v["child_off"][i + 1] - v["child_off"][i] >= 2)
    deep = next(i for i in range(n) if v["depth"][i] == 1)
    deeper = next(i for i in range(n) if v["depth"][i] == 3)
    bad = {}
    bad["unsorted children"] = image.copy()
    e = at["tok"] + int(v["child_off"][node])
    bad["unsorted children"][[e, e + 1]] = bad["unsorted children"][[e + 1, e]]
    bad["a suffix link to a deeper node"] = image.copy()
    bad["a suffix link to a deeper node"][at["suffix"] + deep] = deeper
    bad["next out of range"] = image.copy()
    bad["next out of range"][at["next"] + 3] = n
    bad["NaN logp"] = image.copy()
    bad["NaN logp"][at["logp"] + 5] = np.array([np.nan], dtype=np.float32).view(np.int32)[0]
    bad["wrong vocab"] = L.shape_model(20, 2)[1].copy()
    bad["wrong vocab"][3] = 19
    bad["a truncated blob"] = image[:-7].copy()
    bad["an edge on the blank"] = image.copy()
    bad["an edge on the blank"][at["tok"]] = 0
    for name, img in bad.items():
        with pytest.raises(lib.AsrError):
            run(img)
            pytest.fail(f"{name}: accepted")
    for kw in (dict(alpha=-1.0), dict(alpha=np.nan), dict(beta=np.inf), dict(oov=0.5), dict(oov=np.nan)):
        with pytest.raises(lib.AsrError):
            run(image, **kw)
    wide = ids.copy()
    wide[4, 0] = vocab + 1                                 # a candidate the model's tables do not cover
    with pytest.raises(lib.AsrError, match="vocabulary"):
        _run(eng, [wide], [lp], 2, 2, image)
