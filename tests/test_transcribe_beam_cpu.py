"""CPU: tools/transcribe.py's arguments for the SenseVoice beam search and the hotword file parser (no model is run)."""
import importlib.util
import os
import sys
import types

import pytest

from conftest import ROOT


def _tool():
    spec = importlib.util.spec_from_file_location("transcribe_tool", os.path.join(ROOT, "tools", "transcribe.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_hotword_file_parser(tmp_path):
    tool = _tool()
    path = tmp_path / "hot.txt"
    path.write_text("# names\n4125 77, 9\n\n  12\nMount Erebus\n7 up\n", encoding="utf-8")
    assert tool.parse_hotword_file(str(path)) == [[4125, 77, 9], [12], "Mount Erebus", "7 up"]


def test_new_arguments_parse_and_default(monkeypatch):
    tool = _tool()
    seen = {}
    monkeypatch.setattr(tool, "run", lambda a: seen.update(vars(a)) or {"files": []})
    argv = ["transcribe.py", "run", "--family", "sensevoice", "--model", "m", "--wav", "a.wav", "--out", os.devnull]
    monkeypatch.setattr(sys, "argv", argv)
    tool.main()
    assert seen["beam"] == 1 and seen["nbest"] == 1 and seen["hotwords"] is None and seen["hotword_boost"] == 2.0
    monkeypatch.setattr(sys, "argv", argv + ["--beam", "8", "--nbest", "3", "--hotwords", "hot.txt", "--hotword-boost", "1.5"])
    tool.main()
    assert (seen["beam"], seen["nbest"], seen["hotwords"], seen["hotword_boost"]) == (8, 3, "hot.txt", 1.5)


@pytest.mark.parametrize("extra, message", [
    (dict(family="paraformer", nbest=2), "sensevoice only"),
    (dict(family="whisper", hotwords="hot.txt"), "sensevoice only"),
    (dict(family="sensevoice", beam=4, timestamps=True), "time spans"),
    (dict(family="sensevoice", beam=2, nbest=3), "--nbest 1..beam"),
    (dict(family="sensevoice", beam=17), "--beam 1..16"),
])
def test_argument_combinations_are_rejected_before_a_model_is_opened(extra, message):
    tool = _tool()
    base = dict(family="sensevoice", model="/nonexistent", wav=[], language="en", tokenizer=None, precision="f32", sliding_window=0, strict_wav=True,
                repeat_penalty=1.0, beam=1)
    with pytest.raises(SystemExit) as e:
        tool.run(types.SimpleNamespace(**{**base, **extra}))
    assert message in str(e.value)
