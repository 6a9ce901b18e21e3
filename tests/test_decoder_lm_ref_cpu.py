"""The float64 statement of n-gram LM fusion in the autoregressive decoders (tests/decoder_lm_ref.py) against the statements it extends, and the new entries'
declarations, exports and bindings. No GPU."""
import os
import re

import numpy as np
import pytest

import ctc_lm_ref as clr
import decoder_lm_ref as dl
import hotword_heads_ref as hw
import token_heads_ref as thr
from conftest import sub
from ctc_beam_ref import build_trie, trie_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _all_known_model(n, alpha, beta, topk=16, end_ids=(), seed=5, backoff_hi=1.0):
    ng = dl.grid_ngrams(seed, n, 3, range(n))
    if backoff_hi <= 0.0:
        ng = {g: (lp, -abs(bo)) for g, (lp, bo) in ng.items()}
    return dl.model(clr.build_image(ng, n), alpha, beta, oov=0.0, topk=topk, end_ids=end_ids)


def _toy_decoder(n, seed):
    """(first logits, state0, step) of a decoder whose logits are a function of the tokens so far: grid logits seeded by the history."""
    def logits(hist):
        return thr.grid_logits([seed, len(hist)] + [int(t) for t in hist], 1, n)[0]

    def step(state, tok):
        hist = state + (int(tok),)
        return logits(hist), hist
    return logits(()), (), step


@pytest.mark.parametrize("phrases", [False, True])
def test_zero_weights_are_the_hotword_statement(phrases):
    rows, n = 3, 129
    x, ph, bias = hw.head_inputs(rows, n)
    ph = ph if phrases else []
    lm = _all_known_model(n, 0.0, 0.0)
    ref = dl.head_steps_lm(x, ph, hw.BOOST, 32, lm, bias=bias)
    plain = hw.head_steps_hot(x, ph, hw.BOOST, 32, bias=bias)
    assert np.array_equal(ref["picks"], plain["picks"]) and np.array_equal(ref["save"], plain["save"])
    if phrases:
        assert np.array_equal(ref["nodes"], plain["nodes"])
    assert np.allclose(ref["scores"], plain["scores"], rtol=0, atol=1e-12)
    assert len(set(ref["states"].ravel().tolist())) > 10                  # the states move all the same
    # the ranker's merge: topM u S with a zero term is the hotword merge of topK u S
    c = hw.rank_inputs(3, 129, False)
    trie = build_trie(c["phrases"]) if phrases else build_trie([[0]])
    boost = hw.BOOST if phrases else 0.0
    lm3 = _all_known_model(129, 0.0, 0.0, seed=6)
    for r in range(len(c["x"])):
        nd = int(c["node"][r]) if phrases else 0
        v, i, lse, _ = dl.rerank_lm(c["x"][r], trie if phrases else None, nd, boost, lm3, 7, 3)
        hv, hi, hl = hw.rerank(c["x"][r], trie, nd, boost, 3)
        assert np.array_equal(i, hi) and np.allclose(v, hv, rtol=0, atol=1e-12) and lse == hl
    # ... and the whole search
    first, s0, step = _toy_decoder(129, 3)
    plist = [[int(thr.order(first)[1])], [int(thr.order(first)[2]), 5]] if phrases else []
    got = dl.beam_search_core_lm(first, s0, step, 3, 6, plist, 1.5, lm3, stop_ids=(7,))
    if phrases:
        want = hw.beam_search_core_hot(first, s0, step, 3, 6, plist, 1.5, stop_ids=(7,))
    else:
        from oracle.qwen_asr_oracle import beam_search_core
        want = beam_search_core(first, s0, step, 3, 6, stop_ids=(7,))
    assert [t.tolist() for t, _ in got] == [np.asarray(t).tolist() for t, _ in want]
    assert np.allclose([s for _, s in got], [s for _, s in want], rtol=0, atol=1e-5)


def test_a_finished_hypothesis_scores_model_plus_bonus_plus_score_tokens():
    from oracle.qwen_asr_oracle import log_softmax_f32
    n, beam, max_new = 60, 4, 9
    finished = 0
    for seed in range(6):
        first, s0, step = _toy_decoder(n, 40 + seed)
        stop = int(thr.order(first)[3])
        o = thr.order(first)
        phrases = [[int(o[1]), int(o[4])], [int(o[2])]]
        first = first.copy()
        ng = dl.grid_ngrams(seed, n, 3, [c for c in range(n) if c % 7 != 3])
        lm = dl.model(clr.build_image(ng, n), 0.5, 0.25, oov=-1.5, topk=12, end_ids=(stop,))
        trie = build_trie(phrases)

        def boosted_step(state, tok, _step=step, _stop=stop):
            lg, st = _step(state, tok)
            lg = lg.copy()
            lg[_stop] += F32(2.0 + 0.5 * len(st))             # the stop id rises with the length: hypotheses finish
            return lg, st
        for toks, score, fin in dl.beam_search_core_lm(first, s0, boosted_step, beam, max_new, phrases, 1.5, lm, stop_ids=(stop,), with_fin=True):
            logits, state, am, node, bonus = first, s0, 0.0, 0, 0.0
            for t in list(toks) + ([stop] if fin else []):          # (a stop id pays the refund of a partial match like any other non-child)
                am += float(log_softmax_f32(logits).astype(np.float64)[t])
                node, bonus = trie_step(trie, node, bonus, int(t), 1.5)
                logits, state = boosted_step(state, t)
            lm_sum, end = clr.score_tokens(lm["view"], toks, 0.5, 0.25, -1.5)
            assert abs(score - (am + bonus + float(lm_sum) + (float(end) if fin else 0.0))) < 1e-4, (seed, toks, fin)
            finished += int(fin)
    assert finished >= 6


def test_top_m_equals_the_dense_ranking_where_the_bound_holds():
    """Every log-probability and back-off <= 0 and alpha >= 0: a column outside topM u S gains at most beta over a raw value of at most the M-th, and its delta
    is the row's smallest. So once the beam-th fused key is above x_M + beta + delta_other, nothing outside can enter."""
    n, K, M = 400, 4, 8
    rng = np.random.default_rng(3)
    lm = _all_known_model(n, 0.5, 0.25, topk=M, seed=9, backoff_hi=0.0)
    v = lm["view"]
    assert (v["backoff"] <= 0).all() and (v["logp"] <= 0).all()
    x_all = thr.grid_logits([n, 77], 60, n)
    x_all[:, :] *= F32(2.0)                                   # wider gaps at the top: the bound holds for most rows
    trie = build_trie([[3, 9], [int(thr.order(x_all[0])[2])], [50, 60, 70]])
    held = differed = 0
    for r in range(len(x_all)):
        state = int(rng.integers(0, v["n_nodes"]))
        node = int(rng.integers(0, len(trie["depth"]))) if r % 2 else 0
        for tr, nd in ((None, 0), (trie, node)):
            tv, ti, lse, _ = dl.rerank_lm(x_all[r], tr, nd, 1.5, lm, state, K)
            dv, di, _ = dl.rank_dense_lm(x_all[r], tr, nd, 1.5, lm, state, K)
            x_m = float(np.sort(x_all[r])[::-1][M - 1])
            d_other = -float(trie["depth"][nd]) * 1.5 if tr is not None else 0.0
            if tv[K - 1] + lse > x_m + lm["beta"] + d_other:
                held += 1
                assert np.array_equal(ti, di) and np.allclose(tv, dv, rtol=0, atol=1e-12), r
            else:
                differed += int(not np.array_equal(ti, di))
    assert held >= 40
    print(f"bound held on {held} of {2 * len(x_all)} rankings; {differed} of the others differ from the dense ranking (tokens outside the top M are not considered)")


@pytest.mark.parametrize("hot", [True, False])
@pytest.mark.parametrize("n", [129, 4097])
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("beam", [1, 3, 8])
def test_ranking_cases_are_decided(beam, first, n, hot):
    c = hw.rank_inputs(beam, n, first)
    lm, state = dl.rank_model(beam, n, first, hot)
    ref = dl.rank_reference_lm(c, beam, first, lm, state, hot)
    assert (ref["cross"] > 0).mean() >= 1.0 - thr.SKIP_CAP, ref["cross"]


def test_head_cases_plant_real_ties_and_flip_picks():
    for rows, n in [(1, 5), (3, 129), (65, 129), (3, 4097)]:
        x, ph, bias = hw.head_inputs(rows, n)
        lm = dl.head_model(rows, n)
        v = lm["view"]
        assert v["order"] == 3 and v["eos"] == n and v["start_node"] != 0 and (v["uni"][:n] < 0).any() and (v["uni"][:n] >= 0).any()
        grid = lambda a: np.array_equal(np.round(np.asarray(a, np.float64) / dl.LM_GRID) * dl.LM_GRID, np.asarray(a, np.float64))
        assert grid(v["logp"]) and grid(v["backoff"])
        x, pair, oov = dl.plant_ties(x, lm, bias, ph)
        ref = dl.head_steps_lm(x, ph, hw.BOOST, 32, lm, bias=bias)
        plain = hw.head_steps_hot(x, ph, hw.BOOST, 32, bias=bias)
        assert (ref["picks"][1:] != plain["picks"][1:]).any()
        if pair is not None:
            a, b = pair
            ta, tb = dl.lm_term(lm, v["start_node"], a)[0], dl.lm_term(lm, v["start_node"], b)[0]
            assert float(x[0, 0, a]) + ta == float(x[0, 0, b]) + tb and x[0, 0, b] > x[0, 0, a] and (ref["picks"][0] == a).all()
        assert n < 129 or (pair is not None and oov is not None)


def test_set_lm_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "asr_mi355x.h"), encoding="utf-8").read()
    sig = sub("_lib").SIGNATURES
    for fam in ("whisper", "qwen"):
        name = f"asr_{fam}_set_lm"
        assert re.search(r"int %s\(asr_session\* s, const int32_t\* image_words, int64_t n_words, float alpha, float beta, float oov_logprob, int topk,\s*"
                         r"const int32_t\* end_ids,\s*int n_end_ids\);" % name, header), name
        assert name in sig and len(sig[name][1]) == 9


def test_the_library_exports_the_entries():
    lib = sub("_lib").load()                                  # (load() resolves every name of SIGNATURES: a missing export raises)
    for fam in ("whisper", "qwen"):
        assert callable(getattr(lib, f"asr_{fam}_set_lm"))
    eng = sub("engine")
    for cls in (eng.WhisperSession, eng.QwenAsrSession):
        assert callable(getattr(cls, "set_lm"))


def test_the_probe_library_exports_the_hooks():
    probe_header = open(os.path.join(ROOT, "include", "asr_mi355x_probe.h"), encoding="utf-8").read()
    names = ("asr_probe_lm_topk", "asr_probe_lm_pick", "asr_probe_lm_head_steps", "asr_probe_lm_rank")
    for name in names:
        assert name in sub("_probe").SIGNATURES and f"int {name}(" in probe_header
    lib = sub("_probe").load()
    for name in names:
        assert callable(getattr(lib, name))


def test_the_abi_version_is_one():
    assert sub("_lib").load().asr_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "asr_mi355x.h"), encoding="utf-8").read()
    assert re.search(r"#define ASR_ABI_VERSION 1\b", header)
    assert "asr_whisper_set_lm" in header and "asr_qwen_set_lm" in header      # ... with the new entries in it


def _tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("transcribe_tool_lm", os.path.join(ROOT, "tools", "transcribe.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_flags(tmp_path):
    tool = _tool()
    import argparse
    arpa = tmp_path / "m.arpa"
    arpa.write_text("\n".join(clr.arpa_text(dl.grid_ngrams(1, 12, 2, range(12)), 12)), encoding="utf-8")
    ns = lambda **kw: argparse.Namespace(**dict(dict(family="whisper", beam=1, decoder_lm=None, decoder_lm_weight=None, decoder_length_bonus=None, decoder_lm_topk=None), **kw))
    assert tool.decoder_lm_options(ns()) is None
    assert tool.decoder_lm_options(ns(decoder_lm=str(arpa))) == {"lm_file": str(arpa), "lm_weight": 0.5, "length_bonus": 0.0, "lm_topk": 16}
    got = tool.decoder_lm_options(ns(family="qwen_asr", beam=4, decoder_lm=str(arpa), decoder_lm_weight=0.3, decoder_length_bonus=0.1, decoder_lm_topk=8))
    assert got == {"lm_file": str(arpa), "lm_weight": 0.3, "length_bonus": 0.1, "lm_topk": 8}
    for bad in (ns(family="sensevoice", decoder_lm=str(arpa)), ns(decoder_lm_weight=0.3), ns(decoder_lm=str(arpa), decoder_lm_topk=33),
                ns(decoder_lm=str(arpa), beam=5, decoder_lm_topk=4), ns(decoder_lm=str(tmp_path / "none.arpa"))):
        with pytest.raises(SystemExit):
            tool.decoder_lm_options(bad)
    kw = tool.load_decoder_lm(tool.decoder_lm_options(ns(decoder_lm=str(arpa))), None)
    assert kw["lm_topk"] == 16 and kw["lm"].image(12).size == clr.build_image(dl.grid_ngrams(1, 12, 2, range(12)), 12).size
