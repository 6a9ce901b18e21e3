"""CPU: the ARPA reader and image builder of the product package (lm.NgramLM) against the reference's (tests/ctc_lm_ref.py), and tools/transcribe.py's
language-model arguments (no model is run)."""
import importlib.util
import math
import os
import sys
import types

import numpy as np
import pytest

import ctc_lm_ref as L
from conftest import ROOT, sub

LN10 = math.log(10.0)
TEMPLATE = """\\data\\
ngram 1=5
ngram 2=4
ngram 3=2

\\1-grams:
-1.5\t<unk>
-99\t<s>\t-0.5
-1.0\t</s>
-0.75\t{a}\t-0.25
-1.25\t{b}\t-0.125

\\2-grams:
-0.5\t<s> {a}\t-0.0625
-0.25\t{a} {b}\t-0.5
-0.625\t{b} {a}
-0.375\t{b} </s>

\\3-grams:
-0.125\t<s> {a} {b}
-0.0625\t{a} {b} </s>

\\end\\
"""
TRIGRAM = TEMPLATE.format(a="7", b="3")


def test_a_hand_written_trigram_round_trips(tmp_path):
    lm = sub("lm")
    m = lm.NgramLM.from_arpa(TRIGRAM.splitlines())
    E, B = lm.EOS, lm.BOS
    want = {(B,): (-99.0, -0.5), (E,): (-1.0, 0.0), (7,): (-0.75, -0.25), (3,): (-1.25, -0.125), (B, 7): (-0.5, -0.0625), (7, 3): (-0.25, -0.5), (3, 7): (-0.625, 0.0),
            (3, E): (-0.375, 0.0), (B, 7, 3): (-0.125, 0.0), (7, 3, E): (-0.0625, 0.0)}
    assert m.order == 3 and set(m.ngrams) == set(want)
    for g, (lp, bo) in want.items():
        assert m.ngrams[g] == pytest.approx((lp * LN10, bo * LN10), abs=1e-12)
    assert m.unk_logprob == pytest.approx(-1.5 * LN10) and m.default_oov_logprob == m.unk_logprob
    path = tmp_path / "tri.arpa"                                        # a path reads the same as the lines
    path.write_text(TRIGRAM, encoding="utf-8")
    assert np.array_equal(lm.NgramLM.from_arpa(str(path)).image(10), m.image(10))
    # the image is the reference's image of the same n-grams, and the walk gives the hand-computed figures (log10):
    vocab = 10
    ref = {tuple(vocab if t == E else vocab + 1 if t == B else t for t in g): v for g, v in m.ngrams.items()}
    assert np.array_equal(m.image(vocab), L.build_image(ref, vocab))
    # <s> 7 3 </s>: P(7|<s>) = -0.5, P(3|<s> 7) = -0.125, P(</s>|7 3) = -0.0625
    assert m.score([7, 3], vocab) == pytest.approx((-0.5 - 0.125 - 0.0625) * LN10, abs=1e-6)
    # <s> 3 7 </s>: back off from <s> (-0.5) to P(3) = -1.25; P(7|3) = -0.625; </s> after "3 7": no such trigram, "3 7" is a node with back-off 0, "7 </s>" is not
    # listed: back-off of 7 (-0.25) + P(</s>) = -1.0
    assert m.score([3, 7], vocab) == pytest.approx((-0.5 - 1.25 - 0.625 - 0.25 - 1.0) * LN10, abs=1e-6)
    # token 5 has no unigram: it costs the <unk> figure and the <s> context survives it
    assert m.score([5, 7, 3], vocab) == pytest.approx((-1.5 - 0.5 - 0.125 - 0.0625) * LN10, abs=1e-6)
    assert m.score([5, 7, 3], vocab, alpha=0.5, beta=0.25, oov_logprob=0.0) == pytest.approx(0.5 * (-0.5 - 0.125 - 0.0625) * LN10 + 0.75, abs=1e-6)


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_random_models_through_arpa_text_give_the_reference_image(order):
    lm = sub("lm")
    for seed in range(4):
        vocab = 9
        ngrams = L.random_arpa(seed, vocab, order, 0.4, bos=seed % 2 == 0, eos=seed < 2)
        m = lm.NgramLM.from_arpa(L.arpa_text(ngrams, vocab, unk=-2.0 if seed % 2 else None))
        image = L.build_image(ngrams, vocab)
        assert np.array_equal(m.image(vocab), image)
        assert m.default_oov_logprob == (pytest.approx(-2.0) if seed % 2 else 0.0)
        tokens = np.random.default_rng(seed).integers(1, vocab, size=16)
        total, end = L.score_tokens(L.view(image), tokens, 0.7, 0.2, m.default_oov_logprob)
        assert m.score(tokens, vocab, alpha=0.7, beta=0.2) == pytest.approx(float(total + end), abs=1e-9)


def test_pieces_resolve_through_token_to_id_and_ids_pass_through():
    lm = sub("lm")
    pieces = {"▁the": 7, "cat": 3}
    text = TEMPLATE.format(a="▁the", b="cat")
    by_ids = lm.NgramLM.from_arpa(TRIGRAM.splitlines())
    for table in (pieces, pieces.get):
        assert lm.NgramLM.from_arpa(text.splitlines(), token_to_id=table).ngrams == by_ids.ngrams
    with pytest.raises(ValueError, match="token_to_id"):
        lm.NgramLM.from_arpa(text.splitlines())


def test_malformed_arpa_text_is_rejected_with_the_line():
    lm = sub("lm")
    lines = TRIGRAM.splitlines()
    at = lines.index("-0.125\t<s> 7 3")
    bad = list(lines)
    bad[at] = "-0.125\t3 3 7"                                           # "3 3" is not listed
    with pytest.raises(ValueError, match=f"line {at + 1}: the context"):
        lm.NgramLM.from_arpa(bad)
    bad = list(lines)
    bad[at] = "0.125\t<s> 7 3"
    with pytest.raises(ValueError, match=f"line {at + 1}: positive"):
        lm.NgramLM.from_arpa(bad)
    bad = TEMPLATE.format(a="seven", b="3").splitlines()
    where = next(i for i, x in enumerate(bad) if "seven" in x)
    with pytest.raises(ValueError, match=f"line {where + 1}: the word 'seven' is not in the vocabulary"):
        lm.NgramLM.from_arpa(bad, token_to_id={"3": 3})
    with pytest.raises(ValueError, match="outside the vocabulary"):     # ids are checked against the vocabulary when the image is built
        lm.NgramLM.from_arpa(lines).image(7)
    with pytest.raises(ValueError, match="fields"):
        lm.NgramLM.from_arpa(["\\1-grams:", "-1.0 3 4 5 6"])


def _tool():
    spec = importlib.util.spec_from_file_location("transcribe_tool", os.path.join(ROOT, "tools", "transcribe.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_lm_arguments_parse_and_default(monkeypatch):
    tool = _tool()
    seen = {}
    monkeypatch.setattr(tool, "run", lambda a: seen.update(vars(a)) or {"files": []})
    argv = ["transcribe.py", "run", "--family", "sensevoice", "--model", "m", "--wav", "a.wav", "--out", os.devnull]
    monkeypatch.setattr(sys, "argv", argv)
    tool.main()
    assert seen["lm"] is None and seen["lm_weight"] is None and seen["length_bonus"] is None
    monkeypatch.setattr(sys, "argv", argv + ["--lm", "zh.arpa", "--lm-weight", "0.3", "--length-bonus", "1.5"])
    tool.main()
    assert (seen["lm"], seen["lm_weight"], seen["length_bonus"]) == ("zh.arpa", 0.3, 1.5)


@pytest.mark.parametrize("extra, message", [
    (dict(family="paraformer", lm="x.arpa"), "sensevoice only"),
    (dict(family="whisper", lm="x.arpa"), "sensevoice only"),
    (dict(family="qwen_asr", lm_weight=0.3), "sensevoice only"),
    (dict(family="whisper", length_bonus=1.0), "sensevoice only"),
    (dict(family="sensevoice", lm_weight=0.3), "need --lm"),
    (dict(family="sensevoice", lm="/nonexistent/x.arpa"), "no such file"),
    (dict(family="sensevoice", lm=__file__, timestamps=True), "time spans"),
])
def test_lm_argument_combinations_are_rejected_before_a_model_is_opened(extra, message):
    tool = _tool()
    base = dict(family="sensevoice", model="/nonexistent", wav=[], language="en", tokenizer=None, precision="f32", sliding_window=0, strict_wav=True,
                repeat_penalty=1.0, beam=1)
    with pytest.raises(SystemExit) as e:
        tool.run(types.SimpleNamespace(**{**base, **extra}))
    assert message in str(e.value)
