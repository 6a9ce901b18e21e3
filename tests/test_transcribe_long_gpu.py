"""GPU: transcribe_long of the four transcribers (segmenter.run_long over engine.op_vad) on the tiny configurations.

The file is three short loud clips with gaps of digital noise (sigma = 8 LSB). For every family: the segments are op_vad's; per segment the result equals, bit for
bit, the family's existing call on the slice audio[start:end] -- run_packed / run_packed_timed for SenseVoice and Paraformer, transcribe([slice]) for Whisper and
Qwen3-ASR --; times are the per-slice ones plus start / rate; one case runs at 48 kHz stereo through the session's input format; a silent file makes no session
call; and transcribe / transcribe_file without the new arguments return the same before and after, and what the session calls they stand for return."""
import numpy as np
import pytest

from conftest import sub
from helpers import load_golden, sensevoice_setup
from test_oracle_paraformer import paraformer_setup
from test_oracle_qwen_asr import qwen_setup
from test_oracle_whisper import whisper_setup

pytestmark = pytest.mark.gpu

F32 = 1
CLIPS_S, GAP_S, LEAD_S = (0.6, 0.9, 0.5), 0.7, 0.3


def _file(rate=16000, channels=1, seed=0):
    """int16 frames [n, channels]: LEAD_S of noise, then each clip followed by GAP_S of noise."""
    rng = np.random.default_rng(seed)
    noise = lambda s: np.round(rng.standard_normal((int(s * rate), channels)) * 8.0)
    parts = [noise(LEAD_S)]
    for c in CLIPS_S:
        parts += [np.round(rng.standard_normal((int(c * rate), channels)) * 3000.0), noise(GAP_S)]
    return np.clip(np.concatenate(parts), -32768, 32767).astype(np.int16)


def _segments(pcm, rate, channels, cfg):
    """What op_vad reports for the file under transcribe_long's parameters (the defaults; no segment longer than the family's window)."""
    eng, seg = sub("engine"), sub("segmenter")
    limit = seg.limit_frames(cfg.max_audio_len, rate, cfg.sample_rate)
    pc = eng.VadParams().to_c(rate, 32768.0, limit // eng.vad_hop(rate))
    s, _, counts = eng.op_vad(pcm.reshape(-1), [0, pcm.shape[0]], rate=rate, channels=channels, params=pc)
    assert counts[0] == len(CLIPS_S) == s.shape[0]                      # one segment per clip: the gaps are longer than min_pause + 2 pad
    return s


def _check_header(res, segs, rate, n):
    assert [(r["start"], r["end"]) for r in res["segments"]] == [(int(s) / rate, int(e) / rate) for s, e in segs]
    assert res["audio_seconds"] == n / rate and res["speech_seconds"] == float((segs[:, 1] - segs[:, 0]).sum()) / rate
    ids = [np.asarray(r["token_ids"]) for r in res["segments"]]
    assert np.array_equal(res["token_ids"], np.concatenate(ids))


class _NoCalls:
    """Every compute entry of a native session replaced by a refusal, for the silent file."""

    def __init__(self, native, names):
        self.native, self.names = native, names

    def __enter__(self):
        def refuse(*a, **k):
            raise AssertionError("a session call was made for a file with no segment")
        self.saved = {n: getattr(self.native, n) for n in self.names}
        for n in self.names:
            setattr(self.native, n, refuse)

    def __exit__(self, *exc):
        for n in self.names:
            delattr(self.native, n)


def _check_silent(res):
    assert res["segments"] == [] and res["token_ids"].size == 0 and res["speech_seconds"] == 0.0 and res["audio_seconds"] == 2.0


# ------------------------------------------------------------------------------------------------ SenseVoice
@pytest.mark.parametrize("rate,channels", [(16000, 1), (48000, 2)])
def test_sensevoice(tmp_path, rate, channels):
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    sv = sub("sensevoice")
    folder = str(tmp_path / "sv")
    sv.export_sensevoice(folder, cfg, ck, precision=F32)
    tr = sv.SenseVoiceTranscriber(folder, "en")
    native = tr.session._native
    pcm = _file(rate, channels)
    fmt = {} if rate == 16000 else dict(sample_rate=rate, channels=channels)
    before = tr.transcribe(pcm if fmt else pcm.reshape(-1), **fmt)
    segs = _segments(pcm, rate, channels, cfg)
    plain = tr.transcribe_long(pcm, **fmt)
    timed = tr.transcribe_long(pcm, timestamps=True, **fmt)
    assert native.input_format == (16000, 1)
    _check_header(plain, segs, rate, pcm.shape[0])
    _check_header(timed, segs, rate, pcm.shape[0])
    prepared = sv.prepare_audio_input(pcm.reshape(1, 1, -1), tr.input_audio_dtype, audio_pcm_scale=tr.audio_pcm_scale, channels=channels).reshape(-1, channels)
    lang = np.asarray([tr.selector_index], np.int32)
    native.set_input_format(rate, channels)
    for (s, e), a, b in zip(segs, plain["segments"], timed["segments"]):
        clip, offs = prepared[s:e].reshape(-1), np.array([0, e - s], np.int64)
        tok, num = native.run_packed(clip, offs, lang)
        assert np.array_equal(a["token_ids"], tok[0, :num[0]]) and np.array_equal(b["token_ids"], tok[0, :num[0]])
        tok, num, first, last, lp = native.run_packed_timed(clip, offs, lang)
        dur, start = int(e - s) / rate, int(s) / rate
        want = []
        for k in range(num[0]):
            t0, t1 = cfg.row_span_seconds(first[0, k], last[0, k])
            want.append({"id": int(tok[0, k]), "start": start + min(t0, dur), "end": start + min(t1, dur), "logprob": float(lp[0, k])})
        assert b["tokens"] == want
    native.set_input_format(16000, 1)
    assert sum(len(r["token_ids"]) for r in plain["segments"]) > 0
    # the plain call is what it was: the same before and after, and the session's own answer on the whole file
    after = tr.transcribe(pcm if fmt else pcm.reshape(-1), **fmt)
    assert all(np.array_equal(x, y) for x, y in zip(before["token_ids"], after["token_ids"])) and before["windows"] == after["windows"] == 1
    if not fmt:
        tok, num = native.run_packed(prepared.reshape(-1), np.array([0, pcm.shape[0]], np.int64), lang)
        assert np.array_equal(before["token_ids"][0], tok[0, :num[0]])
    with _NoCalls(native, ("run_packed", "run_packed_timed", "run_packed_beam")):
        _check_silent(tr.transcribe_long(np.zeros((2 * rate, channels), np.int16), **fmt))


def test_sensevoice_beam_per_segment(tmp_path):
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    sv = sub("sensevoice")
    folder = str(tmp_path / "sv")
    sv.export_sensevoice(folder, cfg, ck, precision=F32)
    tr = sv.SenseVoiceTranscriber(folder, "en")
    native = tr.session._native
    pcm = _file()
    segs = _segments(pcm, 16000, 1, cfg)
    res = tr.transcribe_long(pcm, beam_size=3, nbest=2)
    _check_header(res, segs, 16000, pcm.shape[0])
    prepared = sv.prepare_audio_input(pcm.reshape(1, 1, -1), tr.input_audio_dtype, audio_pcm_scale=tr.audio_pcm_scale).reshape(-1)
    for (s, e), r in zip(segs, res["segments"]):
        tok, num, score, ctc = native.run_packed_beam(prepared[s:e], np.array([0, e - s], np.int64), np.asarray([tr.selector_index], np.int32), 3, None, 2)
        assert np.array_equal(r["token_ids"], tok[0, 0, :num[0, 0]])
        assert [h["score"] for h in r["nbest"]] == [float(v) for v in score[0] if np.isfinite(v)]


# ------------------------------------------------------------------------------------------------ Paraformer
def test_paraformer(tmp_path):
    cfg, ck = paraformer_setup("paraformer_tiny")
    pf, R = sub("paraformer"), sub("paraformer")
    vocab = [f"t{i}" for i in range(cfg.vocab)]
    vocab[0], vocab[1], vocab[2], vocab[-1] = "<blank>", "<s>", "</s>", "<unk>"
    folder = str(tmp_path / "pf")
    pf.export_paraformer(folder, cfg, ck, vocab, "zh", "zh", precision=F32)
    tr = pf.ParaformerTranscriber(folder)
    native = tr.session._native
    pcm = _file(seed=1)
    before = tr.transcribe(pcm.reshape(-1))
    segs = _segments(pcm, 16000, 1, cfg)
    plain = tr.transcribe_long(pcm)
    timed = tr.transcribe_long(pcm, timestamps=True)
    _check_header(plain, segs, 16000, pcm.shape[0])
    _check_header(timed, segs, 16000, pcm.shape[0])
    prepared = pf.prepare_audio_input(pcm.reshape(1, 1, -1), tr.input_audio_dtype, audio_pcm_scale=tr.audio_pcm_scale).reshape(-1)
    row_s = cfg.lfr_n * cfg.hop_length / cfg.sample_rate
    keep = lambda ids: ids[~np.isin(ids, tr.stop_token_ids)]
    for (s, e), a, b in zip(segs, plain["segments"], timed["segments"]):
        offs = np.array([0, e - s], np.int64)
        tok, num = native.run_packed(prepared[s:e], offs)
        assert np.array_equal(a["token_ids"], keep(tok[0, :num[0]])) and np.array_equal(b["token_ids"], a["token_ids"])
        tok, num, fire, lp = native.run_packed_timed(prepared[s:e], offs)
        n, dur, start = int(num[0]), int(e - s) / 16000, int(s) / 16000
        spans = R.token_times(fire[0, :n], cfg.seq_len(int(e - s)), row_s, 4)
        want = [{"id": int(tok[0, k]), "text": vocab[tok[0, k]], "start": start + min(float(spans[k, 0]), dur), "end": start + min(float(spans[k, 1]), dur),
                 "logprob": float(lp[0, k])} for k in range(n) if int(tok[0, k]) not in tr.stop_token_ids]
        assert b["tokens"] == want
    assert plain["token_ids"].size > 0 and plain["text"] == pf.decode_tokens([vocab[i] for i in plain["token_ids"]], tr.decode_mode)
    after = tr.transcribe(pcm.reshape(-1))
    assert all(np.array_equal(x, y) for x, y in zip(before["token_ids"], after["token_ids"])) and before["text"] == after["text"]
    tok, num = native.run_packed(prepared, np.array([0, prepared.size], np.int64))
    assert np.array_equal(before["token_ids"][0], keep(tok[0, :num[0]]))
    with _NoCalls(native, ("run_packed", "run_packed_timed", "run_packed_beam")):
        _check_silent(tr.transcribe_long(np.zeros(2 * 16000, np.int16)))


# ------------------------------------------------------------------------------------------------ Whisper
def test_whisper():
    eng, wh = sub("engine"), sub("whisper")
    cfg, ck, sup, beg = whisper_setup("whisper_tiny_test")
    sess = eng.WhisperSession.from_checkpoint(cfg, ck, precision=F32, suppress_tokens=sup, begin_suppress_tokens=beg, audio_dtype=np.int16)
    pcm = _file(seed=2)
    segs = _segments(pcm, 16000, 1, cfg)
    kw = dict(suppress_tokens=sup, no_speech_threshold=2.0, detect_language=False, remove_repeats=False)
    plain_tr = wh.WhisperTranscriber(cfg, sess, **kw)
    file_before, _ = plain_tr.transcribe_file(pcm.reshape(-1), max_new=6)
    for tr in (plain_tr, wh.WhisperTranscriber(cfg, sess, timestamps=True, **kw)):
        res, stat = tr.transcribe_long(pcm, max_new=6)
        _check_header(res, segs, 16000, pcm.shape[0])
        assert stat["wall_s"] > 0
        for (s, e), r in zip(segs, res["segments"]):
            one, _ = tr.transcribe([pcm[s:e].reshape(-1)], max_new=6)
            assert np.array_equal(r["tokens"], one[0]["tokens"]) and r["language_id"] == one[0]["language_id"]
            if tr.timestamps:
                start = int(s) / 16000
                assert [(g["start"], g["end"], g["tokens"]) for g in r["segments"]] == [(start + g["start"], start + g["end"], g["tokens"]) for g in one[0]["segments"]]
    file_after, _ = plain_tr.transcribe_file(pcm.reshape(-1), max_new=6)
    assert file_before["windows"] == file_after["windows"] and np.array_equal(file_before["tokens"], file_after["tokens"])
    whole, _ = plain_tr.transcribe([pcm.reshape(-1)], max_new=6)
    assert np.array_equal(np.asarray(file_before["windows"][0], np.int32), whole[0]["tokens"])         # one dynamic window: the clip call's ids
    with _NoCalls(sess, ("encode", "prefill", "generate", "beam_search")):
        res, _ = plain_tr.transcribe_long(np.zeros(2 * 16000, np.int16))
        _check_silent(res)


def test_whisper_48k_stereo():
    eng, wh = sub("engine"), sub("whisper")
    cfg, ck, sup, beg = whisper_setup("whisper_tiny_test")
    sess = eng.WhisperSession.from_checkpoint(cfg, ck, precision=F32, suppress_tokens=sup, begin_suppress_tokens=beg, audio_dtype=np.int16)
    pcm = _file(48000, 2, seed=3)
    segs = _segments(pcm, 48000, 2, cfg)
    tr = wh.WhisperTranscriber(cfg, sess, suppress_tokens=sup, no_speech_threshold=2.0, detect_language=False, remove_repeats=False)
    res, _ = tr.transcribe_long(pcm, sample_rate=48000, channels=2, max_new=6)
    assert sess.input_format == (16000, 1)
    _check_header(res, segs, 48000, pcm.shape[0])
    for (s, e), r in zip(segs, res["segments"]):
        one, _ = tr.transcribe([pcm[s:e]], max_new=6, sample_rate=48000, channels=2)
        assert np.array_equal(r["tokens"], one[0]["tokens"])


# ------------------------------------------------------------------------------------------------ Qwen3-ASR
def test_qwen_asr():
    g = load_golden("qwen_asr_tiny")
    cfg, ck = qwen_setup(g)
    sess = sub("engine").QwenAsrSession.from_checkpoint(cfg, ck, precision=F32)
    special = {"stop": [1, 521], "asr_text": [540], "audio_start": 524, "audio_end": 520, "audio_pad": 525, "im_start": 510, "im_end": 521,
               "system": 511, "user": 523, "assistant": 522, "newline": 512, "language_prefix": [530, 531]}
    langs = {"en": {"name": "English", "aliases": ["english"], "prompt_token_ids": [77, 540]}}
    meta = {"audio_pcm_scale": "32768", "max_seq_len": str(cfg.max_seq_len), "sample_rate": "16000", "special_token_ids": special, "supported_languages": langs}
    tr = sub("qwen_asr").QwenAsrTranscriber(cfg, sess, meta)
    pcm = _file(seed=4)
    segs = _segments(pcm, 16000, 1, cfg)
    before, _ = tr.transcribe([pcm.reshape(-1)], max_new=6)
    res, stat = tr.transcribe_long(pcm, language_prompt="English", max_new=6)
    _check_header(res, segs, 16000, pcm.shape[0])
    for (s, e), r in zip(segs, res["segments"]):
        one, _ = tr.transcribe([pcm[s:e].reshape(-1)], language_prompts=("English",), max_new=6)
        assert np.array_equal(r["tokens"], one[0]["tokens"]) and r["prompt_tokens"] == one[0]["prompt_tokens"]
    after, _ = tr.transcribe([pcm.reshape(-1)], max_new=6)
    assert np.array_equal(before[0]["tokens"], after[0]["tokens"])
    with _NoCalls(sess, ("prefill", "generate", "beam_search")):
        res, _ = tr.transcribe_long(np.zeros(2 * 16000, np.int16))
        _check_silent(res)


# ------------------------------------------------------------------------------------------------ the tool
def test_tool_vad_switch(tmp_path):
    """tools/transcribe.py --vad: the dump's windows are the segments' ids, `segments` carries them in seconds of the file, --vad-dump writes the spans; without
    --vad the dump is what it was."""
    import importlib.util
    import json
    import os
    import types
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("transcribe_tool", os.path.join(ROOT, "tools", "transcribe.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    folder = str(tmp_path / "sv")
    sub("sensevoice").export_sensevoice(folder, cfg, ck, precision=F32)
    pcm = _file(seed=5)
    wav = str(tmp_path / "file.wav")
    sub("audio_io").write_wav_int16(wav, pcm.reshape(-1), 16000)
    base = dict(family="sensevoice", model=folder, wav=[wav], language="en", tokenizer=None, precision="f32", sliding_window=0, strict_wav=True, repeat_penalty=1.0, beam=1)
    plain = tool.run(types.SimpleNamespace(**base))["files"][0]
    dump = str(tmp_path / "segments.json")
    vad = tool.run(types.SimpleNamespace(**base, vad=True, vad_margin_db=None, vad_min_pause=None, vad_pad=None, vad_max_seconds=None, vad_dump=dump, timestamps=True))["files"][0]
    again = tool.run(types.SimpleNamespace(**base))["files"][0]
    assert {k: v for k, v in plain.items() if k != "rtf"} == {k: v for k, v in again.items() if k != "rtf"} and "segments" not in plain
    segs = _segments(pcm, 16000, 1, cfg)
    assert [(g["start"], g["end"]) for g in vad["segments"]] == [(int(s) / 16000, int(e) / 16000) for s, e in segs]
    assert vad["windows"] == [g["token_ids"] for g in vad["segments"]] and all(len(g["tokens"]) == len(g["token_ids"]) for g in vad["segments"])
    json.dumps(vad)                                            # plain Python numbers: the dump serialises
    written = json.load(open(dump))["files"][0]
    assert written["segments"] == [[g["start"], g["end"]] for g in vad["segments"]] and written["path"] == wav
    with pytest.raises(SystemExit):
        tool.run(types.SimpleNamespace(**base, vad=False, vad_pad=0.2))
    with pytest.raises(SystemExit):
        tool.run(types.SimpleNamespace(**{**base, "sliding_window": 8000}, vad=True, vad_margin_db=None, vad_min_pause=None, vad_pad=None, vad_max_seconds=None, vad_dump=None))
