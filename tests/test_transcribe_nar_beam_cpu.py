"""CPU: tools/transcribe.py's --nar-* arguments (Paraformer's beam search over the decoder's token rows; no model is run) and ParaformerTranscriber's
assembly of the hypotheses -- the n-best list, stop ids dropped, the token times every hypothesis of a window shares -- on a stub session."""
import importlib.util
import os
import sys
import types

import numpy as np
import pytest

from conftest import ROOT, sub


def _tool():
    spec = importlib.util.spec_from_file_location("transcribe_tool", os.path.join(ROOT, "tools", "transcribe.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


NAR = ("nar_beam", "nar_nbest", "nar_hotwords", "nar_hotword_boost", "nar_lm", "nar_lm_weight", "nar_length_bonus")


def test_new_arguments_parse_and_default(monkeypatch):
    tool = _tool()
    seen = {}
    monkeypatch.setattr(tool, "run", lambda a: seen.update(vars(a)) or {"files": []})
    argv = ["transcribe.py", "run", "--family", "paraformer", "--model", "m", "--wav", "a.wav", "--out", os.devnull]
    monkeypatch.setattr(sys, "argv", argv)
    tool.main()
    assert all(seen[k] is None for k in NAR)
    assert tool.nar_options(types.SimpleNamespace(**seen)) is None                       # nothing given: the plain path
    monkeypatch.setattr(sys, "argv", argv + ["--nar-beam", "8", "--nar-nbest", "3", "--nar-hotwords", "hot.txt", "--nar-hotword-boost", "1.5", "--nar-lm", "lm.arpa",
                                             "--nar-lm-weight", "0.7", "--nar-length-bonus", "0.25"])
    tool.main()
    assert tuple(seen[k] for k in NAR) == (8, 3, "hot.txt", 1.5, "lm.arpa", 0.7, 0.25)


def test_options_become_the_transcribers_arguments(tmp_path):
    tool = _tool()
    hot = tmp_path / "hot.txt"
    hot.write_text("12 40\n北京\n", encoding="utf-8")
    lm = tmp_path / "lm.arpa"
    lm.write_text("\\data\\\nngram 1=1\n\n\\1-grams:\n-1.0\t5\n\n\\end\\\n", encoding="utf-8")
    ns = lambda **kw: types.SimpleNamespace(family="paraformer", **kw)
    assert tool.nar_options(ns(nar_beam=4)) == dict(beam_size=4, nbest=1, hotwords=None, hotword_boost=2.0, lm_file=None, lm_weight=0.5, length_bonus=0.0)
    assert tool.nar_options(ns(nar_nbest=3))["beam_size"] == 3                             # the narrowest beam that can return them
    got = tool.nar_options(ns(nar_beam=8, nar_nbest=2, nar_hotwords=str(hot), nar_hotword_boost=1.5, nar_lm=str(lm), nar_lm_weight=0.7, nar_length_bonus=0.25))
    assert got == dict(beam_size=8, nbest=2, hotwords=[[12, 40], "北京"], hotword_boost=1.5, lm_file=str(lm), lm_weight=0.7, length_bonus=0.25)


@pytest.mark.parametrize("extra, message", [
    (dict(family="sensevoice", nar_beam=4), "paraformer only"),
    (dict(family="whisper", nar_hotwords="hot.txt"), "paraformer only"),
    (dict(family="qwen_asr", nar_lm_weight=0.5), "paraformer only"),
    (dict(family="paraformer", nar_beam=2, nar_nbest=3), "--nar-nbest 1..beam"),
    (dict(family="paraformer", nar_beam=17), "--nar-beam 1..16"),
    (dict(family="paraformer", nar_beam=0), "--nar-beam 1..16"),
    (dict(family="paraformer", nar_hotword_boost=1.0), "needs --nar-hotwords"),
    (dict(family="paraformer", nar_lm_weight=0.5), "need --nar-lm"),
    (dict(family="paraformer", nar_length_bonus=0.5), "need --nar-lm"),
    (dict(family="paraformer", nar_lm="/nonexistent/lm.arpa"), "no such file"),
    (dict(family="paraformer", nar_hotwords="/nonexistent/hot.txt"), "no such file"),
    (dict(family="paraformer", nbest=2), "sensevoice only"),                              # the existing flags keep their rejections
    (dict(family="paraformer", lm="x.arpa"), "sensevoice only"),
])
def test_argument_combinations_are_rejected_before_a_model_is_opened(extra, message):
    tool = _tool()
    base = dict(family="paraformer", model="/nonexistent", wav=[], language="zh", tokenizer=None, precision="f32", sliding_window=0, strict_wav=True,
                repeat_penalty=1.0, beam=1)
    with pytest.raises(SystemExit) as e:
        tool.run(types.SimpleNamespace(**{**base, **extra}))
    assert message in str(e.value)


def test_a_negative_lm_weight_is_rejected(tmp_path):
    tool = _tool()
    lm = tmp_path / "lm.arpa"
    lm.write_text("\\data\\\n", encoding="utf-8")
    with pytest.raises(SystemExit, match="weight >= 0"):
        tool.nar_options(types.SimpleNamespace(family="paraformer", nar_lm=str(lm), nar_lm_weight=-0.5))


# ---- the transcriber's result assembly on a stub session -------------------------------------------------------------------------------------------
class _StubNative:
    """run_packed_beam of a session whose every window fires four tokens at rows 1, 3, 4 and 9 (of 10) and returns three hypotheses, the last one not found."""

    def __init__(self, cfg):
        self.cfg, self.calls, self.hot, self.lm = cfg, [], None, None

    def set_hotwords(self, phrases, boost):
        self.hot = (phrases, boost)

    def set_lm(self, lm, alpha, beta):
        self.lm = (lm, alpha, beta)

    def run_packed_beam(self, audio, offsets, beam, topk, nbest):
        self.calls.append((int(audio.size), beam, topk, nbest))
        max_t = self.cfg.seq_len(int(audio.size))
        tok, lp = np.zeros((1, nbest, max_t), np.int32), np.zeros((1, nbest, max_t), np.float32)
        num, score, am = np.zeros((1, nbest), np.int32), np.full((1, nbest), -np.inf, np.float32), np.full((1, nbest), -np.inf, np.float32)
        fire = np.zeros((1, max_t), np.int32)
        fire[0, :4] = [1, 3, 4, 9]
        for n, ids in enumerate(([5, 6, 2, 7], [5, 8, 2, 7])[:nbest]):                     # id 2 is the stop id (</s>)
            tok[0, n, :4], num[0, n], score[0, n], am[0, n] = ids, 4, -1.0 - n, -1.5 - n
            lp[0, n, :4] = [-0.1 * (n + 1), -0.2, -0.3, -0.4]
        return tok, num, score, am, fire, lp


def _transcriber(window):
    pf, cfgm, shim = sub("paraformer"), sub("config"), sub("ort_shim")
    cfg = cfgm.paraformer_tiny()
    tr = pf.ParaformerTranscriber.__new__(pf.ParaformerTranscriber)
    native = _StubNative(cfg)
    tr.session = types.SimpleNamespace(_native=native, io_binding=lambda: None)
    tr.audio_meta = shim.NodeArg("audio", [1, 1, window], np.float32)
    tr.input_audio_dtype, tr.audio_pcm_scale, tr.sample_rate = "F32", 1, cfg.sample_rate
    tr.device_type, tr.device_id = "cpu", 0
    tr.stop_token_ids, tr.language, tr.decode_mode = [2], "zh", "zh"
    tr.tokenizer = np.array([f"t{i}" for i in range(cfg.vocab)], dtype=np.str_)
    tr.tokenizer[2] = "</s>"
    return pf, cfg, tr, native


def test_nbest_assembly_and_shared_token_times(monkeypatch):
    pf, cfg, tr, native = _transcriber(9600)
    monkeypatch.setattr(pf.onnxruntime.OrtValue, "ortvalue_from_numpy", staticmethod(lambda *a, **k: None))
    tr.session.io_binding = lambda: types.SimpleNamespace(bind_ortvalue_input=lambda *a, **k: None)
    pcm = (np.arange(9600 + 4800) % 100).astype(np.int16)                                  # two windows at a 4800-sample stride... the second zero-padded
    out = tr.transcribe(pcm, sliding_window=4800, timestamps=True, beam_size=4, nbest=3, hotwords=[[5, 6], "t9"], hotword_boost=1.25)
    assert native.hot == ([[5, 6], [9]], 1.25) and native.lm == (None, 0.5, 0.0)
    assert out["windows"] == len(native.calls) >= 2 and all(c == (9600, 4, None, 3) for c in native.calls)
    assert len(out["nbest"]) == out["windows"] and all(len(w) == 2 for w in out["nbest"])      # the third hypothesis was not found
    row_s, n_rows, dur = cfg.lfr_n * cfg.hop_length / cfg.sample_rate, cfg.seq_len(9600), pcm.size / cfg.sample_rate
    spans = pf.token_times([1, 3, 4, 9], n_rows, row_s)
    for k, win in enumerate(out["nbest"]):
        off = k * 4800 / cfg.sample_rate
        for n, h in enumerate(win):
            assert set(h) == {"token_ids", "score", "am_score", "text", "tokens"}
            assert h["token_ids"].tolist() == ([5, 6, 7], [5, 8, 7])[n] and h["text"] == ("t5t6t7", "t5t8t7")[n]       # the stop id is dropped everywhere
            assert (h["score"], h["am_score"]) == (-1.0 - n, -1.5 - n)
            assert [t["id"] for t in h["tokens"]] == h["token_ids"].tolist()
            kept = [0, 1, 3]
            assert [(t["start"], t["end"]) for t in h["tokens"]] == [(min(off + spans[i, 0], dur), min(off + spans[i, 1], dur)) for i in kept]
            assert [t["logprob"] for t in h["tokens"]] == [float(np.float32(x)) for x in ([-0.1 * (n + 1), -0.2, -0.4])]
        assert [(t["start"], t["end"]) for t in win[0]["tokens"]] == [(t["start"], t["end"]) for t in win[1]["tokens"]]        # shared fire rows
    assert [i.tolist() for i in out["token_ids"]] == [[5, 6, 7]] * out["windows"] and out["text"] == "t5t6t7" * out["windows"]
    assert out["tokens"] == [t for win in out["nbest"] for t in win[0]["tokens"]]
    plain = tr.transcribe(pcm, sliding_window=4800, beam_size=2, nbest=2)
    assert "tokens" not in plain and all(set(h) == {"token_ids", "score", "am_score", "text"} for win in plain["nbest"] for h in win)
    assert native.hot == ([], 2.0)                                                            # exactly this call's list


def test_bad_beam_arguments_and_unknown_hotword_text():
    pf, cfg, tr, native = _transcriber(9600)
    pcm = np.zeros(9600, np.int16)
    with pytest.raises(ValueError, match="nbest"):
        tr.transcribe(pcm, beam_size=2, nbest=3)
    with pytest.raises(ValueError, match="beam_size"):
        tr.transcribe(pcm, beam_size=17)
    with pytest.raises(ValueError, match="vocabulary"):
        tr.transcribe(pcm, hotwords=["not a token"])
    assert native.calls == []
