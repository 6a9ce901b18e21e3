"""GPU, session level: SenseVoiceSession.run_timed / asr_sensevoice_run_timed -- ids equal the untimed run's, the frame log-probabilities match the float64
statement of the logits tap within the derived budget, spans and scores equal the reference collapse of the taps -- and the transcriber's timestamps."""
import numpy as np
import pytest

import ctc_timing_ref as R
from conftest import sub
from helpers import kaldi_audio, sensevoice_setup

pytestmark = pytest.mark.gpu

BF16, F32 = 0, 1


def _audios(cfg):
    # ragged batch of three; the shortest is one frame (win_length samples): a single LFR row behind the prompt rows
    return [kaldi_audio(31, 32000), kaldi_audio(32, cfg.win_length), kaldi_audio(33, 9000)], [2, 0, 4]


def _check_against_taps(cfg, sess, audios, recs):
    rows = sess.utterance_rows([a.size for a in audios])
    logits, ids = sess.tap("logits"), sess.tap("frame_ids", dtype=np.int32)[:, 0]
    flp = sess.tap("frame_logprob")[:, 0]
    for (r0, T), rec in zip(rows, recs):
        ref_ids, ref_lp, spread = R.frame_logprob(logits[r0:r0 + T])
        b = R.budget(cfg.vocab, ref_lp, spread)
        err = np.abs(flp[r0:r0 + T].astype(np.float64) - ref_lp)
        print(f"frame_logprob tap: max err/budget {float((err / b).max()):.3f}, max budget {b.max():.2e}")
        assert (err <= b).all(), (err.max(), b.min())
        assert (flp[r0:r0 + T] <= 0).all()
        tok, first, last, score = R.collapse_timed(ids[r0:r0 + T], flp[r0:r0 + T], cfg.blank_id)
        assert np.array_equal(rec["ids"], tok) and np.array_equal(rec["first_frame"], first) and np.array_equal(rec["last_frame"], last)
        assert np.array_equal(rec["logprob"].view(np.uint32), score.view(np.uint32))


def _invariants(cfg, rec, T):
    n = len(rec["ids"])
    assert len(rec["first_frame"]) == len(rec["last_frame"]) == len(rec["logprob"]) == n
    assert (rec["first_frame"] <= rec["last_frame"]).all() and (rec["ids"] != cfg.blank_id).all()
    assert (rec["first_frame"][1:] > rec["last_frame"][:-1]).all() and (rec["first_frame"] >= 0).all() and (rec["last_frame"] < T).all()
    assert (rec["logprob"] <= 0).all() and np.isfinite(rec["logprob"]).all()


@pytest.mark.parametrize("prec", [F32, BF16])
def test_timed_run_equals_untimed_and_the_reference_collapse(prec):
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    sess = sub("engine").SenseVoiceSession.from_checkpoint(cfg, ck, precision=prec)
    audios, langs = _audios(cfg)
    assert cfg.seq_len(audios[1].size) == cfg.n_prompt + 1
    # graph key: timed, untimed, timed again on the same shapes (the second call of a kind replays its capture) -- nobody replays the other's graph
    t1 = sess.run_timed(audios, langs)
    u1 = sess.run(audios, langs)
    t2 = sess.run_timed(audios, langs)
    u2 = sess.run(audios, langs)
    t3 = sess.run_timed(audios, langs)
    assert sum(len(u) for u in u1) > 0
    for a, b, c, u, v, audio in zip(t1, t2, t3, u1, u2, audios):
        assert np.array_equal(a["ids"], u) and np.array_equal(u, v)
        for k in ("ids", "first_frame", "last_frame"):
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k])
        assert np.array_equal(a["logprob"].view(np.uint32), b["logprob"].view(np.uint32)) and np.array_equal(a["logprob"].view(np.uint32), c["logprob"].view(np.uint32))
        _invariants(cfg, a, cfg.seq_len(audio.size))
    sess.taps(True)
    recs = sess.run_timed(audios, langs)
    _check_against_taps(cfg, sess, audios, recs)
    for a, r in zip(t1, recs):
        assert np.array_equal(a["ids"], r["ids"]) and np.array_equal(a["first_frame"], r["first_frame"]) and np.array_equal(a["last_frame"], r["last_frame"])
    sess.run(audios, langs)                                        # an untimed run with taps: the timed tap is not refreshed, the others are
    sess.close()


def test_real_vocabulary_width_through_a_session():
    """sensevoice_small, batch 2: 25 055 valid of 25 088 columns (392 slabs, the last one partly valid)."""
    cfg, ck = sensevoice_setup("sensevoice_small")
    sess = sub("engine").SenseVoiceSession.from_checkpoint(cfg, ck, precision=BF16)
    audios, langs = [kaldi_audio(41, 24000), kaldi_audio(42, 7777)], [0, 3]
    plain = sess.run(audios, langs)
    sess.taps(True)
    recs = sess.run_timed(audios, langs)
    for rec, u, a in zip(recs, plain, audios):
        assert np.array_equal(rec["ids"], u)
        _invariants(cfg, rec, cfg.seq_len(a.size))
    _check_against_taps(cfg, sess, audios, recs)
    sess.close()


def test_transcriber_timestamps_over_two_windows(tmp_path):
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    folder = str(tmp_path / "SenseVoice_MI355X")
    sv, shim = sub("sensevoice"), sub("ort_shim")
    sv.export_sensevoice(folder, cfg, ck, precision=1)
    tr = sv.SenseVoiceTranscriber(folder, "en")
    assert [a.name for a in tr.session.get_inputs()] == ["audio", "language_idx"] and [a.name for a in tr.session.get_outputs()] == ["token_ids", "num_id"]
    tr.audio_meta = shim.NodeArg("audio", [1, 1, 16000], np.float32)        # a static 1 s window, as the reference's fixed-length exports declare
    pcm = kaldi_audio(51, 26000).astype(np.int16)                           # 1.625 s: two windows at a 0.75 s stride, the second zero-padded
    before = tr.transcribe(pcm, sliding_window=12000)
    out = tr.transcribe(pcm, sliding_window=12000, timestamps=True)
    after = tr.transcribe(pcm, sliding_window=12000)
    assert before["windows"] == out["windows"] == 2
    assert set(before) == set(after) == set(out) - {"tokens"} and "tokens" not in after
    for x, y, z in zip(before["token_ids"], out["token_ids"], after["token_ids"]):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    toks, dur = out["tokens"], pcm.size / 16000
    assert [t["id"] for t in toks] == [int(i) for w in out["token_ids"] for i in w] and len(toks) > 0
    n0 = len(out["token_ids"][0])
    native = tr.session._native
    for k, (win_ids, off) in enumerate(zip(out["token_ids"], (0.0, 0.75))):
        win = np.zeros(16000, np.float32)
        seg = pcm[k * 12000:k * 12000 + 16000].astype(np.float32)
        win[:seg.size] = seg
        rec = native.run_timed([win], [tr.selector_index])[0]
        assert np.array_equal(rec["ids"], win_ids)
        for t, f, l, lp in zip(toks[k * n0:k * n0 + len(win_ids)] if k == 0 else toks[n0:], rec["first_frame"], rec["last_frame"], rec["logprob"]):
            s, e = cfg.row_span_seconds(f, l)
            assert t["start"] == min(off + s, dur) and t["end"] == min(off + e, dur) and t["logprob"] == float(lp)
    assert all(0.0 <= t["start"] <= t["end"] <= dur for t in toks)
    assert any(t["start"] >= 0.75 for t in toks[n0:]) or all(t["end"] == 0.75 for t in toks[n0:])      # window offsets are applied
    last_row_end = 0.75 + cfg.row_span_seconds(cfg.seq_len(16000) - 1, cfg.seq_len(16000) - 1)[1]
    assert last_row_end > dur                                                                            # so clipping is in play for a token on the last rows


def test_tool_dump_with_and_without_timestamps(tmp_path):
    """tools/transcribe.py --family sensevoice --timestamps writes the token list into the dump; without the flag the dump is what it was."""
    import importlib.util
    import json
    import os
    import types
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("transcribe_tool", os.path.join(ROOT, "tools", "transcribe.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    folder = str(tmp_path / "SenseVoice_MI355X")
    sub("sensevoice").export_sensevoice(folder, cfg, ck, precision=1)
    wav = str(tmp_path / "clip.wav")
    sub("audio_io").write_wav_int16(wav, kaldi_audio(61, 20000).astype(np.int16), 16000)
    base = dict(family="sensevoice", model=folder, wav=[wav], language="en", tokenizer=None, precision="f32", sliding_window=0, strict_wav=True,
                repeat_penalty=1.0, beam=1)
    plain = tool.run(types.SimpleNamespace(**base))["files"][0]
    timed = tool.run(types.SimpleNamespace(**base, timestamps=True))["files"][0]
    assert "tokens" not in plain and set(timed) == set(plain) | {"tokens"} and timed["windows"] == plain["windows"]
    assert [t["id"] for t in timed["tokens"]] == plain["windows"][0] and len(timed["tokens"]) > 0
    assert all(set(t) == {"id", "start", "end", "logprob"} and 0.0 <= t["start"] <= t["end"] <= 1.25 and t["logprob"] <= 0 for t in timed["tokens"])
    json.dumps(timed)                                          # plain Python numbers: the dump serialises
    with pytest.raises(SystemExit):
        tool.run(types.SimpleNamespace(**{**base, "family": "paraformer"}, timestamps=True))
