"""CPU: the float64 statement of hotword boosting (tests/hotword_heads_ref.py) is checked against itself -- the sparse logit bias against the dense
delta form, the ranker's merge rule against a dense ranking -- and the seeded inputs of tests/test_hotword_heads_gpu.py are checked to exercise what
they claim to. Also the Python surface that needs no device: hotword_id_variants on the tiny tokenizers, the tool's flags, the ABI's new entries."""
import importlib.util
import os
import re
import sys
import types

import numpy as np
import pytest

import hotword_heads_ref as hw
import token_heads_ref as thr
from conftest import ROOT, sub
from ctc_beam_ref import build_trie, trie_step


@pytest.mark.parametrize("n", [5, 129, 4097])
def test_sparse_bias_selects_and_scores_as_the_dense_delta(n):
    rows, steps = 8, 24
    x = hw.step_logits(3, steps, rows, n)
    ph = hw.planted_phrases(x) + (hw.wide_children(n) if n >= 129 else [])
    trie = build_trie(ph)
    node, moved = np.zeros(rows, np.int64), 0
    for t in range(steps):
        for r in range(rows):
            sparse = hw.bias_sparse(x[t, r], trie, int(node[r]), hw.BOOST)
            dense = hw.bias_dense(x[t, r], trie, int(node[r]), hw.BOOST)
            pick = int(thr.order(sparse)[0])
            assert pick == int(np.lexsort((np.arange(n), -dense))[0])
            assert np.abs(hw.log_softmax64(sparse) - hw.log_softmax64(dense)).max() < 1e-12
            # the sparse form is the dense one plus the row constant depth * boost, exactly (everything is on the grid)
            assert np.array_equal(sparse.astype(np.float64), dense + float(trie["depth"][node[r]]) * float(hw.BOOST))
            node[r] = trie_step(trie, int(node[r]), 0.0, pick, 1.0)[0]
            moved += node[r] != 0
    assert moved > 0


def test_merge_rule_equals_the_dense_ranking():
    rng = np.random.default_rng(11)
    entered = 0
    for case in range(400):
        n, K = int(rng.choice([9, 40, 300])), int(rng.integers(1, 9))
        x = thr.grid_logits([case, 5], 1, n)[0]
        x[rng.integers(0, n, 2)] = -np.inf
        ph = [[int(t) for t in rng.integers(0, n, int(rng.integers(1, 4)))] for _ in range(int(rng.integers(1, 12)))]
        trie = build_trie(ph)
        node = int(rng.integers(0, len(trie["depth"])))
        bias = None
        if case % 3 == 0:
            bias = np.zeros(n, np.float32)
            bias[int(ph[0][0])] = -np.inf
        boost = np.float32(rng.integers(1, 5000) * thr.GRID)
        v, i, _ = hw.rerank(x, trie, node, boost, K, bias)
        dv, di, _, _ = hw.rank_dense(x, trie, node, boost, K, bias)
        assert np.array_equal(i, di) and np.allclose(v, dv, rtol=0, atol=1e-12), case
        xb = x if bias is None else x + bias
        entered += len(set(i[np.isfinite(v)].tolist()) - set(thr.order(xb)[:K].tolist())) > 0
    assert entered > 50                                       # a boosted column from outside the plain top-K enters often


def test_seeded_head_inputs_produce_every_event_and_flip_picks():
    total, deep = {k: 0 for k in hw.EVENTS}, 0
    for rows, n in [(r, w) for r in hw.ROWS for w in hw.WIDTHS]:
        if rows * n > 65 * 129 and (rows, n) not in hw.HEAD_SHAPES:
            continue                                          # (the large shapes are run by the GPU test; the CPU check keeps to the quick ones)
        x, ph, bias = hw.head_inputs(rows, n)
        ref = hw.head_steps_hot(x, ph, hw.BOOST, 32, bias=bias)
        plain = hw.head_steps_hot(x, [], hw.BOOST, 32, bias=bias)
        assert (ref["picks"] != plain["picks"]).any(), (rows, n)
        assert (ref["picks"][0] != ph[0][0]).all()            # the boosted column the step-0 bias holds at -inf is never picked
        for k in hw.EVENTS:
            total[k] += ref["events"][k]
        deep += ref["deep_restarts"]
    assert all(total[k] > 0 for k in hw.EVENTS), total
    assert deep > 0                                           # a phrase abandoned at depth 2 onto a root child
    x, ph, bias = hw.head_inputs(*hw.HEAD_SHAPES[1])
    big = hw.head_steps_hot(x, ph, hw.BOOST, 32, bias=bias)["events"]
    assert all(big[k] > 0 for k in hw.EVENTS), big


def test_planted_phrase_shapes():
    x, ph, _ = hw.head_inputs(3, 129)
    trie = build_trie(ph)
    t = [tuple(p) for p in ph]
    assert any(len(p) == 1 for p in t)
    assert any(p[:1] in t and len(p) == 2 for p in t)                                            # [a] beside [a, b]
    assert any(p[0] == q[0] and p != q and len(p) == len(q) == 2 for p in t for q in t)          # [a, b] beside [a, c]
    assert any(len(p) == 2 and len(q) == 2 and p[1] == q[0] for p in t for q in t)               # [a, b] beside [b, x]: b a child and a root child
    assert any(len(p) == 3 and len(set(p)) == 1 for p in t)                                      # [a, a, a]
    kids = np.diff(trie["child_off"])
    assert kids[0] > 64 and (kids[1:] > 64).any()                                                # a root and an inner node with more than 64 children


@pytest.mark.parametrize("shape", hw.HEAD_SHAPES)
def test_sampler_cases_leave_few_rows_undecided(shape):
    rows, n = shape
    x, ph, bias = hw.head_inputs(rows, n)
    ref = hw.head_steps_hot(x, ph, hw.BOOST, 32, bias=bias, sampler=hw.sampler_setting(n), noise=hw.sampler_noise(rows, n), partial=1)
    upto, skipped = hw.decided_prefix(ref["decided"])
    assert skipped <= thr.SKIP_CAP, (skipped, upto)
    assert sum(ref["events"].values()) > 0


@pytest.mark.parametrize("geom", hw.TS_GEOMS)
def test_timestamp_case_is_decided_and_mixes_text_and_timestamps(geom):
    import whisper_timestamps_ref as wtr
    x, ph = hw.ts_inputs(geom)
    ref = hw.head_steps_hot(x, ph, hw.BOOST, 32, timestamps=wtr.params(geom, 20))
    _, skipped = hw.decided_prefix(ref["decided"])
    assert skipped <= thr.SKIP_CAP
    ts_begin = geom[2]
    assert (ref["picks"] >= ts_begin).any() and (ref["picks"] < geom[1]).any()
    assert sum(ref["events"].values()) > 0


@pytest.mark.parametrize("n", [129, 4097])
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("beam", [1, 3, 8])
def test_ranking_cases(beam, first, n):
    c = hw.rank_inputs(beam, n, first)
    ref = hw.rank_reference(c, beam, first)
    assert ref["dense_ok"]
    assert ref["cross"] > 0                                   # no tie between columns of different delta among the ranks that decide
    sel = ref["sel"]
    if first:
        assert (np.asarray(ref["topi"])[0] != int(np.nonzero(np.isneginf(c["bias"]))[0][0])).all()      # BEGIN_SUPPRESS holds the boosted column out
    else:
        trie = ref["trie"]
        nd, stop = int(c["node"][0]), c["stop"][0]
        assert nd != 0 and stop not in hw.children(trie, nd)
        hit = [r for r in range(beam) if sel["parent"][r] == 0 and sel["fin"][r] == 1 and sel["next"][r] == stop]
        assert hit                                            # the stop id was picked inside a partial match ...
        lp = hw.log_softmax64(c["x"][0].astype(np.float64))[stop]
        refund = -float(trie["depth"][nd]) * float(hw.BOOST) + (float(hw.BOOST) if stop in hw.children(trie, 0) else 0.0)
        assert abs(float(sel["cum"][hit[0]]) - (float(c["cum"][0]) + lp + refund)) < 1e-5        # ... and paid the refund
        assert sel["done"][-1] == 1 and np.array_equal(sel["node"][-beam:], c["node"][-beam:])   # the frozen utterance keeps its nodes


# ------------------------------------------------------------------------------------------------ the Python surface
def test_hotword_id_variants_on_the_tiny_tokenizers(tmp_path):
    transformers = pytest.importorskip("transformers")
    from tiny_tokenizers import qwen_tokenizer_dir, whisper_tokenizer_dir
    variants = sub("engine").hotword_id_variants
    cfg = sub("config").whisper_tiny_test()
    for folder in (whisper_tokenizer_dir(str(tmp_path / "w"), cfg), qwen_tokenizer_dir(str(tmp_path / "q"), 600)):
        tok = transformers.AutoTokenizer.from_pretrained(folder)
        enc = lambda t: tok.encode(t, add_special_tokens=False)
        word = tok.decode(enc("hello")).strip() or "hello"
        out = variants([word, [5, 6, 7]], enc)
        assert out[-1] == [5, 6, 7]
        texts = out[:-1]
        assert 1 <= len(texts) <= 2 and enc(word) in texts and enc(" " + word) in texts
        assert len({tuple(v) for v in texts}) == len(texts)
    assert variants([[1, 2], [1, 2]], None) == [[1, 2], [1, 2]]              # id lists pass through unchanged
    assert variants(None, None) == []
    with pytest.raises(ValueError):
        variants(["text"], None)


def _tool():
    spec = importlib.util.spec_from_file_location("transcribe_tool_hot", os.path.join(ROOT, "tools", "transcribe.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_tool_flags_parse_and_default(monkeypatch):
    tool = _tool()
    seen = {}
    monkeypatch.setattr(tool, "run", lambda a: seen.update(vars(a)) or {"files": []})
    argv = ["transcribe.py", "run", "--family", "whisper", "--model", "m", "--wav", "a.wav", "--out", os.devnull]
    monkeypatch.setattr(sys, "argv", argv)
    tool.main()
    assert seen["decoder_hotwords"] is None and seen["decoder_hotword_boost"] == 2.0
    monkeypatch.setattr(sys, "argv", argv + ["--decoder-hotwords", "hot.txt", "--decoder-hotword-boost", "3.5", "--beam", "3"])
    tool.main()
    assert (seen["decoder_hotwords"], seen["decoder_hotword_boost"], seen["beam"]) == ("hot.txt", 3.5, 3)


def test_tool_rejects_decoder_hotwords_for_the_ctc_families(tmp_path):
    tool = _tool()
    hot = tmp_path / "hot.txt"
    hot.write_text("Mount Erebus\n", encoding="utf-8")
    base = dict(model="/nonexistent", wav=[], language="en", tokenizer=None, precision="f32", sliding_window=0, strict_wav=True, repeat_penalty=1.0, beam=1)
    with pytest.raises(SystemExit) as e:
        tool.run(types.SimpleNamespace(**base, family="sensevoice", decoder_hotwords=str(hot)))
    assert "whisper and --family qwen_asr only" in str(e.value)
    with pytest.raises(SystemExit) as e:                      # text phrases without a tokenizer are refused before a model is opened
        tool.run(types.SimpleNamespace(**base, family="whisper", decoder_hotwords=str(hot)))
    assert "need --tokenizer" in str(e.value)


def test_set_hotwords_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "asr_mi355x.h"), encoding="utf-8").read()
    sig = sub("_lib").SIGNATURES
    for fam in ("whisper", "qwen"):
        name = f"asr_{fam}_set_hotwords"
        assert re.search(r"int %s\(asr_session\* s, const int32_t\* ids, const int32_t\* offsets, int n_phrases, float boost\);" % name, header)
        assert name in sig and len(sig[name][1]) == 5
        assert sig[name] == sig["asr_sensevoice_set_hotwords"]
    lib = sub("_lib").load()                                  # (load() resolves every name of SIGNATURES: a missing export raises)
    assert lib.asr_abi_version() == 1
    eng = sub("engine")
    for cls in (eng.WhisperSession, eng.QwenAsrSession, eng.QwenAlignerSession):
        assert callable(getattr(cls, "set_hotwords"))
    probe_header = open(os.path.join(ROOT, "include", "asr_mi355x_probe.h"), encoding="utf-8").read()
    for name in ("asr_probe_hotword", "asr_probe_hotword_head_steps", "asr_probe_hotword_rank"):
        assert name in sub("_probe").SIGNATURES and f"int {name}(" in probe_header
