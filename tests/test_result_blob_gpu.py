"""GPU, session level: the pinned result buffer of a SenseVoice / Paraformer session moves after every form's step graph has been captured, and nothing is read
from where it was. One session runs every form three times on a small batch X (eager, captured, replayed), once on a batch Y whose result blob
(csrc/result_layout.h) outgrows the buffer's headroom, and three times on X again: every later X result equals the first of its form byte for byte, every Y
result equals the same call on a fresh session. The clips start at the model's minimum (one frame), so one row of the blob is nearly empty beside a full one."""
import numpy as np
import pytest

from conftest import sub
from helpers import kaldi_audio, sensevoice_setup
from test_oracle_paraformer import paraformer_setup

pytestmark = pytest.mark.gpu

BF16 = 0


def _bits(v):
    """ids, counts and spans as they are; scores as their uint32 bit patterns"""
    a = np.asarray(v)
    return a.astype(np.float32).view(np.uint32) if a.dtype.kind == "f" else a


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(_bits(a), _bits(b))


def _clips(cfg):
    """X: two utterances, the first a single frame. Y: five, the longest four times X's longest (max_tokens and the row count both grow)."""
    x = [kaldi_audio(61, cfg.win_length), kaldi_audio(62, 12000)]
    y = [kaldi_audio(63, cfg.win_length), kaldi_audio(64, 9000), kaldi_audio(65, 48000), kaldi_audio(66, 20000), kaldi_audio(67, 30000)]
    assert max(a.size for a in y) >= 2 * max(a.size for a in x)
    return x, y


def _exercise(make, forms, x, y):
    """forms: name -> call(session, audios). Returns the first X result and the Y result of every form."""
    sess, fresh = make(), make()
    try:
        first = {}
        for name, call in forms.items():
            first[name] = call(sess, x)
            for _ in range(2):                                   # the captured and the replayed step
                assert _same(call(sess, x), first[name]), name
        on_y = {name: call(sess, y) for name, call in forms.items()}          # the blob outgrows the buffer: every captured graph is stale
        for name, call in forms.items():
            assert _same(on_y[name], call(fresh, y)), name
        for name, call in forms.items():
            for _ in range(3):                                   # eager again, captured against the new buffer, replayed
                assert _same(call(sess, x), first[name]), name
        return first, on_y
    finally:
        sess.close()
        fresh.close()


def test_sensevoice_results_survive_a_moving_result_buffer():
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    x, y = _clips(cfg)
    langs = [2, 0, 4, 1, 3]
    forms = {"run": lambda s, a: s.run(a, langs[:len(a)]),
             "run_timed": lambda s, a: s.run_timed(a, langs[:len(a)]),
             "run_beam": lambda s, a: s.run_beam(a, langs[:len(a)], beam=4, nbest=2)}
    first, on_y = _exercise(lambda: sub("engine").SenseVoiceSession.from_checkpoint(cfg, ck, precision=BF16), forms, x, y)
    for got in (first, on_y):
        assert sum(len(u) for u in got["run"]) > 0 and sum(len(h) for h in got["run_beam"]) > 0          # something came home to compare
        for u, t in zip(got["run"], got["run_timed"]):
            assert np.array_equal(u, t["ids"]) and len(t["first_frame"]) == len(t["last_frame"]) == len(t["logprob"]) == len(u)
            assert (t["first_frame"] <= t["last_frame"]).all() and (t["logprob"] <= 0).all()


def test_paraformer_results_survive_a_moving_result_buffer():
    cfg, ck = paraformer_setup("paraformer_tiny")
    x, y = _clips(cfg)
    forms = {"run": lambda s, a: s.run(a), "run_timed": lambda s, a: s.run_timed(a)}
    first, on_y = _exercise(lambda: sub("engine").ParaformerSession.from_checkpoint(cfg, ck, precision=BF16), forms, x, y)
    for got, audios in ((first, x), (on_y, y)):
        assert sum(len(u) for u in got["run"]) > 0
        for u, t, a in zip(got["run"], got["run_timed"], audios):
            assert np.array_equal(u, t["ids"]) and len(t["fire_frame"]) == len(t["logprob"]) == len(u)
            assert (np.diff(t["fire_frame"]) > 0).all() and (t["fire_frame"] >= 0).all() and (t["fire_frame"] <= cfg.seq_len(a.size)).all()
            assert (t["logprob"] <= 0).all() and np.isfinite(t["logprob"]).all()
