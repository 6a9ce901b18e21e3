"""Captured graphs survive plan growth. A session runs a small batch X until its step graphs are captured and replayed, then a larger batch Y that makes
every plan section and workspace grow (the plan blob and its pinned staging move), then X again: every later X run must give the first X run's tokens,
and its logits where the call returns them, byte for byte. One bf16 session per model family, tiny checkpoints."""
import numpy as np
import pytest

from conftest import sub
from helpers import kaldi_audio, load_golden, sensevoice_setup
from test_oracle_qwen_asr import qwen_setup
from test_oracle_qwen_asr import unit_audio as qwen_audio
from test_oracle_whisper import unit_audio, whisper_setup

pytestmark = pytest.mark.gpu

BF16 = 0
N_DECODE = 6


def _same(later, first, what):
    assert len(later) == len(first), what
    for i, (a, b) in enumerate(zip(later, first)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: output {i} differs from the first run"


def test_sensevoice_replays_after_the_plan_grew():
    cfg, ck = sensevoice_setup("sensevoice_small")
    sess = sub("engine").SenseVoiceSession.from_checkpoint(cfg, ck, precision=BF16)
    x = [kaldi_audio(800 + i, n) for i, n in enumerate((16000, 20000))]
    y = [kaldi_audio(810 + i, 16000 + 4000 * (i % 5)) for i in range(12)]     # >= 12 windows: the block kernel instead of the tile kernel
    first = sess.run(x, [0, 3])
    for k in range(2):                # captured, replayed
        _same(sess.run(x, [0, 3]), first, f"X run {k + 2}")
    assert len(sess.run(y, [i % 7 for i in range(12)])) == 12
    for k in range(3):                # eager again (the workspace moved), captured, replayed
        _same(sess.run(x, [0, 3]), first, f"X run {k + 1} after Y")
    sess.close()


def _decode_calls(prefill, decode):
    """prefill, then N_DECODE device-fed single-token steps: every array the calls return, in order"""
    out = [a for a in prefill() if a is not None]
    for _ in range(N_DECODE):         # eager, captured, then replays
        out += [a for a in decode(None, want_logits=True) if a is not None]
    return out


def test_whisper_replays_after_the_plan_grew():
    cfg, ck, sup, beg = whisper_setup("whisper_tiny_test")
    sess = sub("engine").WhisperSession.from_checkpoint(cfg, ck, precision=BF16, suppress_tokens=sup, begin_suppress_tokens=beg)

    def calls(seed, lengths):
        audios = [unit_audio(seed + i, n) for i, n in enumerate(lengths)]
        prompt = np.array([[cfg.sot_id, cfg.first_language_id, cfg.transcribe_id, cfg.no_timestamps_id]] * len(audios), np.int32)
        return [np.asarray(sess.encode(audios))] + _decode_calls(lambda: sess.prefill(prompt), sess.decode)

    first = calls(820, (26240, 12640))
    _same(calls(820, (26240, 12640)), first, "X again before Y")
    assert len(calls(830, (48000, 26240, 12640, 32000))) == len(first)
    for k in range(2):
        _same(calls(820, (26240, 12640)), first, f"X run {k + 1} after Y")
    sess.close()


def test_qwen_replays_after_the_plan_grew():
    g = load_golden("qwen_asr_tiny")
    cfg, ck = qwen_setup(g)
    sess = sub("engine").QwenAsrSession.from_checkpoint(cfg, ck, precision=BF16)
    head, tail, suffix = g["head_ids"].tolist(), g["tail_ids"].tolist(), g["suffix_ids"].tolist()

    def calls(seed, lengths):
        audios = [qwen_audio(seed + i, n) for i, n in enumerate(lengths)]
        pre, post = [head + suffix] * len(audios), [tail] * len(audios)
        return _decode_calls(lambda: sess.prefill(audios, pre, post), sess.decode)

    first = calls(840, (30000, 9000))
    _same(calls(840, (30000, 9000)), first, "X again before Y")
    assert len(calls(850, (60000, 30000, 9000, 41000))) == len(first)
    for k in range(2):
        _same(calls(840, (30000, 9000)), first, f"X run {k + 1} after Y")
    sess.close()
