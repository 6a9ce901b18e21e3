"""CPU: the host side of SenseVoice forced alignment -- group_words, tools/align.py --family sensevoice against a stub, the one-window rule."""
import importlib.util
import json
import math
import os
import types

import numpy as np
import pytest

from conftest import ROOT, sub
from tiny_tokenizers import sentencepiece_model


def _tool():
    spec = importlib.util.spec_from_file_location("align_tool", os.path.join(ROOT, "tools", "align.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_group_words_latin_pieces(tmp_path):
    from sentencepiece import SentencePieceProcessor
    sp = SentencePieceProcessor()
    sp.Load(sentencepiece_model(str(tmp_path / "tiny.model"), 40))
    ids = [4, 6, 9, 5, 7, 12]
    pieces = [sp.id_to_piece(i) for i in ids]
    assert pieces == ["▁w4", "x6", "x9", "▁w5", "▁w7", "x12"]
    spans = [(0.0, 0.06), (0.06, 0.12), (0.18, 0.24), (0.3, 0.36), (0.36, 0.6), (0.6, 0.66)]
    lps = [-0.1, -0.3, -0.2, -1.0, 0.0, -2.0]
    words = sub("sensevoice").group_words(pieces, spans, lps)
    assert [w["text"] for w in words] == ["w4x6x9", "w5", "w7x12"]
    assert [(w["start"], w["end"]) for w in words] == [(0.0, 0.24), (0.3, 0.36), (0.36, 0.66)]
    assert [w["probability"] for w in words] == pytest.approx([math.exp(-0.2), math.exp(-1.0), math.exp(-1.0)])
    assert sub("sensevoice").group_words([], [], []) == []
    first = sub("sensevoice").group_words(["x6", "x9"], spans[:2], lps[:2])          # the first piece opens a word whatever it looks like
    assert [w["text"] for w in first] == ["x6x9"]


def test_group_words_cjk_pieces():
    pieces = ["▁你", "好", "▁hello", "世", "界", "ab", "c", "▁", "d", "テスト"]
    spans = [(0.1 * i, 0.1 * i + 0.05) for i in range(len(pieces))]
    words = sub("sensevoice").group_words(pieces, spans, [-0.5] * len(pieces))
    assert [w["text"] for w in words] == ["你", "好", "hello", "世", "界", "abc", "d", "テスト"]
    assert words[5]["start"] == spans[5][0] and words[5]["end"] == spans[6][1]          # "ab" + "c": behind a CJK piece a new word opens without a marker
    assert words[6]["start"] == spans[7][0] and words[6]["end"] == spans[8][1]          # a bare marker opens the word that "d" continues
    assert all(w["probability"] == pytest.approx(math.exp(-0.5)) for w in words)


class _StubTranscriber:
    sample_rate = 16000

    def __init__(self, aligned=True):
        self.aligned, self.calls = aligned, []

    def align(self, audio, text):
        self.calls.append((audio, text))
        words = [{"text": "hello", "start": 0.06, "end": 0.42, "probability": 0.9}, {"text": "world", "start": 0.48, "end": 0.9, "probability": 0.5}]
        return {"tokens": [], "words": words if self.aligned else [], "path_score": -1.0, "loglik": -0.5, "aligned": self.aligned}


def test_tool_sensevoice_arguments_and_json_shape(tmp_path, capsys):
    tool = _tool()
    base = ["--model", "m", "--wav", "w.wav"]
    a = tool.parse_args(base + ["--family", "sensevoice", "--text", " hello world\n", "--tokenizer", "bpe.model"])
    assert a.family == "sensevoice" and a.language == "en" and tool.transcript(a) == " hello world\n"
    f = tmp_path / "t.txt"
    f.write_text("from a file", encoding="utf-8")
    a = tool.parse_args(base + ["--family", "sensevoice", "--text-file", str(f), "--tokenizer", "bpe.model", "--language", "zh"])
    assert a.language == "zh" and tool.transcript(a) == "from a file"
    q = tool.parse_args(base + ["--text", str(f)])                   # the Qwen aligner's call is what it was: --text names a file
    assert q.family == "qwen_aligner" and q.language == "English" and tool.transcript(q) == "from a file"
    for bad in (base + ["--family", "sensevoice", "--tokenizer", "t"], base + ["--family", "sensevoice", "--text", "x"],
                base + ["--family", "sensevoice", "--tokenizer", "t", "--text", "x", "--text-file", str(f)], base + ["--family", "whisper", "--text", "x"]):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)
    capsys.readouterr()
    stub = _StubTranscriber()
    audio = np.zeros(16000, np.int16)
    words = tool.sensevoice_words(stub, audio, " hello world\n")
    assert stub.calls[0][1] == "hello world" and stub.calls[0][0] is audio
    assert words == [{"text": "hello", "start_time": 0.06, "end_time": 0.42}, {"text": "world", "start_time": 0.48, "end_time": 0.9}]
    assert json.loads(json.dumps(words, ensure_ascii=False)) == words
    with pytest.raises(SystemExit):
        tool.sensevoice_words(_StubTranscriber(aligned=False), audio, "hello")


def test_align_refuses_audio_longer_than_one_window():
    sv = sub("sensevoice")
    tr = sv.SenseVoiceTranscriber.__new__(sv.SenseVoiceTranscriber)
    calls = []
    native = types.SimpleNamespace(cfg=types.SimpleNamespace(max_audio_len=32000), align_packed=lambda *a, **k: calls.append(a))
    tr.session = types.SimpleNamespace(_native=native)
    tr.audio_meta = types.SimpleNamespace(name="audio", shape=[1, 1, "audio_len"], type="tensor(float)")
    tr.tokenizer, tr.sample_rate, tr.selector_index, tr.input_audio_dtype, tr.audio_pcm_scale = None, 16000, 0, "F32", 32768
    with pytest.raises(ValueError, match="32000"):
        tr.align(np.zeros(32001, np.int16), [5, 6])
    tr.audio_meta = types.SimpleNamespace(name="audio", shape=[1, 1, 16000], type="tensor(float)")          # a static window is the limit when it is shorter
    with pytest.raises(ValueError, match="16000"):
        tr.align(np.zeros(16001, np.int16), [5, 6])
    with pytest.raises(ValueError, match="tokenizer"):
        tr.align(np.zeros(8000, np.int16), "text without a tokenizer")
    assert calls == []
