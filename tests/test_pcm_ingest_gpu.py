"""GPU: int16 / f16 audio ingest of every session family (asr_session_set_audio_dtype).

The comparisons are exact (np.array_equal) by arithmetic, not by measurement: int16 -> f32 and f16 -> f32 are exact, and the 2^-15 that the
Whisper / Qwen front end applies to raw PCM at the load is a power of two, which commutes with every later f32 rounding (the CPU test
test_pcm_ingest_cpu.py checks that identity on the reference's own STFT module). So a session fed PCM as int16 must produce, bit for bit, what it
produces for the same samples widened on the host -- front-end tap, logits, token ids -- and likewise f16 against the f32 upcast of the f16 values.
Both runs of a comparison take the same kernel path: batches stay below the block kernel's 12-window threshold and the sessions' diversion
counters (asr_sanm_stats, asr_paraformer_stream_stats) are read around them."""
import ctypes as C
import json

import numpy as np
import pytest

from conftest import sub
from helpers import golden_cases, kaldi_audio, load_golden, sensevoice_setup
from test_oracle_paraformer import paraformer_setup
from test_oracle_paraformer_streaming import streaming_setup
from test_oracle_qwen_asr import qwen_setup, unit_audio
from test_oracle_whisper import whisper_setup
from test_qwen_aligner_cpu import aligner_setup

pytestmark = pytest.mark.gpu

BF16, F32 = 0, 1
LENGTHS = (9001, 12345, 7777)            # odd and different: the second and third utterance start at odd sample offsets (2-byte aligned only)
N_NATURAL = 15999
N_DECODE = 8


def _natural():
    return np.ascontiguousarray(load_golden("audio_natural")["zh_1"][2000:2000 + N_NATURAL])


def _with_extremes(pcm):
    pcm = pcm.copy()
    pcm[17], pcm[18], pcm[-2] = -32768, 32767, -32768
    return pcm


def kaldi_pcm():
    """Ragged int16 batch for the Kaldi front ends: synthetic Kaldi-range clips (|x| > 2048 on most samples), one with both ends of the range, one natural."""
    clips = [np.round(kaldi_audio(900 + i, n)).astype(np.int16) for i, n in enumerate(LENGTHS)]
    clips[1] = _with_extremes(clips[1])
    return clips + [_natural()]


def unit_pcm():
    """The same for the Whisper / Qwen front ends: [-1, 1] clips rounded to PCM."""
    clips = [np.clip(np.round(unit_audio(910 + i, n) * 32768.0), -32768, 32767).astype(np.int16) for i, n in enumerate(LENGTHS)]
    clips[1] = _with_extremes(clips[1])
    return clips + [_natural()]


def as_f32(pcm, unit):
    """What an F32 export is fed for this PCM: int16-range values (Kaldi families) or pcm / 32768 (Whisper / Qwen)."""
    a = pcm.astype(np.float32)
    return a * np.float32(1.0 / 32768.0) if unit else a


def as_f16(pcm, unit):
    return as_f32(pcm, unit).astype(np.float16)


def _rows(tap, rows):
    return np.concatenate([tap[r0:r0 + n] for r0, n in rows])


# ------------------------------------------------------------------------------------------------ one runner per family
class Family:
    unit = False                # True: the Whisper / Qwen front end ([-1, 1] floats, 2^-15 applied to raw PCM)

    def pcm(self):
        return unit_pcm() if self.unit else kaldi_pcm()

    def counters(self):
        return None

    def results(self, clips):
        """Run `clips` (already in the session's type) -> {name: array} of everything the entry returns plus the taps."""
        raise NotImplementedError

    def run(self, dtype, clips):
        self.sess.audio_dtype = dtype
        assert self.sess.audio_dtype == np.dtype(dtype)
        got = C.c_int(-1)
        sub("_lib").check(sub("_lib").load().asr_session_audio_dtype(self.sess._h, C.byref(got)))
        assert got.value == {np.dtype(np.float32): 0, np.dtype(np.int16): 1, np.dtype(np.float16): 2}[np.dtype(dtype)]
        return self.results(clips)


class SenseVoice(Family):
    def __init__(self, prec, cfg_name="sensevoice_tiny"):
        cfg, ck = sensevoice_setup(cfg_name)
        self.sess = sub("engine").SenseVoiceSession.from_checkpoint(cfg, ck, precision=prec)
        self.sess.taps(True)

    def counters(self):
        st = self.sess.sanm_stats()
        return st["giveups"], st["foreign_diverted"], st["cooldown"]

    def results(self, clips):
        toks = self.sess.run(clips, [2, 0, 1, 0][:len(clips)])
        rows = self.sess.utterance_rows([c.size for c in clips])                     # the taps are 16-row aligned per utterance: compare the rows that exist
        return {"mel": self.sess.tap("mel"), "logits": _rows(self.sess.tap("logits"), rows), "frame_ids": _rows(self.sess.tap("frame_ids", np.int32), rows),
                "num": np.asarray([t.size for t in toks]), "tokens": np.concatenate(toks)}


class Paraformer(SenseVoice):
    def __init__(self, prec):
        cfg, ck = paraformer_setup("paraformer_tiny")
        self.sess = sub("engine").ParaformerSession.from_checkpoint(cfg, ck, precision=prec)
        self.sess.taps(True)

    def results(self, clips):
        toks = self.sess.run(clips)
        rows = self.sess.utterance_rows([c.size for c in clips])
        trows = [(r0, t.size) for r0, t in zip(self.sess.token_rows([t.size for t in toks]), toks)]
        return {"mel": self.sess.tap("mel"), "enc_out": _rows(self.sess.tap("enc_out"), rows), "alphas": _rows(self.sess.tap("alphas"), rows),
                "logits": _rows(self.sess.tap("logits"), trows), "num": np.asarray([t.size for t in toks]), "tokens": np.concatenate(toks)}


class ParaformerStream(Family):
    def __init__(self, prec):
        g = load_golden("paraformer_streaming_tiny")
        cfg, ck = streaming_setup(g)
        self.chunk = int(g["chunk"])
        self.sess = sub("engine").ParaformerStreamSession(cfg, ck, precision=prec, chunk=self.chunk, max_streams=2)
        self.sess.taps(True)

    def pcm(self):                                             # two streams, three chunks each (the chunk layout is fixed: [n][chunk])
        clips = [np.round(kaldi_audio(920 + i, 3 * self.chunk)).astype(np.int16) for i in range(2)]
        clips[0] = _with_extremes(clips[0])
        clips[1][:N_NATURAL] = _natural()
        return clips

    def counters(self):
        st = self.sess.stream_stats()
        return st["giveups"], st["shared_steps"], st["cooldown"]

    def results(self, clips):
        self.sess.reset(-1)
        out = {}
        for k in range(3):
            fired = self.sess.step(np.stack([c[k * self.chunk:(k + 1) * self.chunk] for c in clips]), [1, 0])
            n = self.sess.rows_per_chunk                                             # one 16-row slot per stream; logits: the fired rows
            out.update({f"mel{k}": self.sess.tap("mel"), f"enc_out{k}": _rows(self.sess.tap("enc_out"), [(0, n), (16, n)]),
                        f"logits{k}": _rows(self.sess.tap("logits"), [(16 * i, t.size) for i, t in enumerate(fired)]),
                        f"num{k}": np.asarray([t.size for t in fired]), f"tokens{k}": np.concatenate(fired)})
        return out


class Whisper(Family):
    unit = True

    def __init__(self, prec):
        cfg, ck, sup, beg = whisper_setup("whisper_tiny_test")
        self.cfg, self.prec = cfg, prec
        self.sess = sub("engine").WhisperSession.from_checkpoint(cfg, ck, precision=prec, suppress_tokens=sup, begin_suppress_tokens=beg)
        self.sess.taps(True)

    def results(self, clips):
        cfg = self.cfg
        npos = self.sess.encode(clips)
        out = {"npos": npos, "mel_gapped": self.sess.tap("mel_gapped", np.float32 if self.prec == F32 else np.uint16)}
        prompt = np.tile(np.asarray([[cfg.sot_id, cfg.first_language_id, cfg.transcribe_id, cfg.no_timestamps_id]], np.int32), (len(clips), 1))
        nxt, logits = self.sess.prefill(prompt)
        out["ids0"], out["logits0"] = nxt, logits
        for k in range(1, N_DECODE + 1):
            nxt, logits = self.sess.decode(None, want_logits=True)
            out[f"ids{k}"], out[f"logits{k}"] = nxt, logits
        return out


class QwenAsr(Family):
    unit = True

    def __init__(self, prec):
        g = load_golden("qwen_asr_tiny")
        cfg, ck = qwen_setup(g)
        self.pre = [g["head_ids"].tolist() + g["suffix_ids"].tolist()]
        self.post = [g["tail_ids"].tolist()]
        self.sess = sub("engine").QwenAsrSession.from_checkpoint(cfg, ck, precision=prec)
        self.sess.taps(True)

    def results(self, clips):
        nxt, logits, ids_len = self.sess.prefill(clips, self.pre, self.post)
        out = {"mel": self.sess.tap("mel"), "ids_len": ids_len, "ids0": nxt, "logits0": logits}
        for k in range(1, N_DECODE + 1):
            nxt, logits = self.sess.decode(None, want_logits=True)
            out[f"ids{k}"], out[f"logits{k}"] = nxt, logits
        return out


class QwenAligner(Family):
    unit = True

    def __init__(self, prec):
        g = load_golden("qwen_aligner_tiny")
        cfg, ck = aligner_setup(g)
        sp = json.loads(str(g["special"]))
        c0 = next(c for _, c in golden_cases(g))
        self.pre, self.post, self.tid = [[sp["audio_start"]]], [[sp["audio_end"]] + c0["input_ids"].tolist()], int(sp["timestamp"])
        self.sess = sub("engine").QwenAlignerSession.from_checkpoint(cfg, ck, precision=prec)
        self.sess.taps(True)

    def results(self, clips):
        bk, lg, ids_len = self.sess.align(clips, self.pre, self.post, timestamp_id=self.tid, want_logits=True)
        return {"mel": self.sess.tap("mel"), "ids_len": ids_len, "n_slots": np.asarray([b.size for b in bk]), "buckets": np.concatenate(bk),
                "logits": np.concatenate(lg)}


LEGS = [("sensevoice-f32", lambda: SenseVoice(F32)), ("sensevoice-bf16", lambda: SenseVoice(BF16)),
        ("sensevoice_small-bf16", lambda: SenseVoice(BF16, "sensevoice_small")), ("paraformer", lambda: Paraformer(F32)),
        ("paraformer_streaming", lambda: ParaformerStream(F32)), ("whisper-f32", lambda: Whisper(F32)), ("whisper-bf16", lambda: Whisper(BF16)),
        ("qwen_asr", lambda: QwenAsr(F32)), ("qwen_aligner", lambda: QwenAligner(F32))]


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k, a[k].shape, b[k].shape)
        assert np.isfinite(a[k]).all() if a[k].dtype.kind == "f" else True, (what, k)
        assert np.array_equal(a[k], b[k]), (what, k, float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max()))


@pytest.mark.parametrize("leg", [n for n, _ in LEGS])
def test_int16_and_f16_equal_f32_exactly_and_switching_is_clean(leg):
    """One session per leg: F32 (widened PCM) -> I16 (raw PCM) -> F32 again -> F16 -> F32 of the upcast f16 values."""
    fam = dict(LEGS)[leg]()
    pcm = fam.pcm()
    assert all(p.dtype == np.int16 and p.size % 2 == 1 for p in pcm) or leg == "paraformer_streaming"
    assert any(p.min() == -32768 and p.max() == 32767 for p in pcm)
    before = fam.counters()
    first = fam.run(np.float32, [as_f32(p, fam.unit) for p in pcm])
    raw = fam.run(np.int16, pcm)
    assert fam.counters() == before, f"{leg}: a pass was diverted to another kernel path between the two runs ({before} -> {fam.counters()})"
    _assert_same(first, raw, leg + " int16 vs f32")
    again = fam.run(np.float32, [as_f32(p, fam.unit) for p in pcm])                      # F32 -> I16 -> F32 reproduces the first result
    _assert_same(first, again, leg + " f32 after int16")
    halves = [as_f16(p, fam.unit) for p in pcm]
    assert any(not np.array_equal(h.astype(np.float32), as_f32(p, fam.unit)) for h, p in zip(halves, pcm))   # the f16 rounding is real
    half = fam.run(np.float16, halves)
    upcast = fam.run(np.float32, [h.astype(np.float32) for h in halves])
    assert fam.counters() == before, f"{leg}: a pass was diverted to another kernel path between the two runs ({before} -> {fam.counters()})"
    _assert_same(upcast, half, leg + " f16 vs f32 of the upcast")
    mel = next(k for k in first if k.startswith("mel"))
    assert not np.array_equal(first[mel], half[mel])                                   # ... and reaches the front end: not a vacuous leg


def test_switching_with_captured_step_graphs():
    """Taps off, so SenseVoice runs and streaming steps replay captured graphs that hold the front end: every type is run often enough to be captured
    (eager, capture, replay), and the session switched F32 -> I16 -> F32 gives its first result again."""
    eng = sub("engine")
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    sess = eng.SenseVoiceSession.from_checkpoint(cfg, ck, precision=BF16)
    pcm = kaldi_pcm()
    lang = [2, 0, 1, 0]
    want = None
    for dtype, clips in ((np.float32, [as_f32(p, False) for p in pcm]), (np.int16, pcm), (np.float32, [as_f32(p, False) for p in pcm]), (np.int16, pcm)):
        sess.audio_dtype = dtype
        for rep in range(3):
            toks = np.concatenate(sess.run(clips, lang))
            want = toks if want is None else want
            assert np.array_equal(toks, want), (np.dtype(dtype).name, rep)
    g = load_golden("paraformer_streaming_tiny")
    scfg, sck = streaming_setup(g)
    chunk = int(g["chunk"])
    st = eng.ParaformerStreamSession(scfg, sck, precision=F32, chunk=chunk, max_streams=2)
    clips = [np.round(kaldi_audio(930 + i, 4 * chunk)).astype(np.int16) for i in range(2)]
    want = None
    for dtype in (np.float32, np.int16, np.float32, np.int16):
        st.audio_dtype = dtype
        st.reset(-1)
        got = []
        for k in range(4):
            fired = st.step(np.stack([c[k * chunk:(k + 1) * chunk] for c in clips]).astype(dtype), [0, 1])
            got += [np.asarray([f.size for f in fired])] + list(fired)
        got = np.concatenate(got)
        want = got if want is None else want
        assert np.array_equal(got, want), np.dtype(dtype).name


class _DeviceAudio:
    """int16 samples placed in HBM with asr_mem_alloc / asr_mem_copy."""

    def __init__(self, packed):
        self.lib, self.ptr = sub("_lib").load(), C.c_void_p(None)
        sub("_lib").check(self.lib.asr_mem_alloc(0, packed.nbytes, C.byref(self.ptr)))
        sub("_lib").check(self.lib.asr_mem_copy(0, self.ptr, packed.ctypes.data_as(C.c_void_p), packed.nbytes, 0))

    def free(self):
        sub("_lib").check(self.lib.asr_mem_free(0, self.ptr))


def test_device_resident_int16_audio_equals_host_audio():
    eng = sub("engine")
    pcm = kaldi_pcm()
    offs = np.zeros(len(pcm) + 1, np.int64)
    offs[1:] = np.cumsum([p.size for p in pcm])
    lang = np.asarray([2, 0, 1, 0], np.int32)
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    sv = eng.SenseVoiceSession.from_checkpoint(cfg, ck, precision=BF16, audio_dtype=np.int16)
    assert sv.audio_dtype == np.int16
    host_tok, host_num = sv.run_packed(np.concatenate(pcm), offs, lang)
    dev = _DeviceAudio(np.concatenate(pcm))
    dev_tok, dev_num = sv.run_packed(None, offs, lang, audio_device_ptr=dev.ptr.value)
    assert np.array_equal(host_num, dev_num) and np.array_equal(host_tok, dev_tok)
    # a batch that starts inside the buffer, at an odd sample: the pointer steps in int16
    tail_tok, tail_num = sv.run_packed(None, offs[1:], lang[1:], audio_device_ptr=dev.ptr.value)
    assert np.array_equal(tail_num, host_num[1:]) and all(np.array_equal(tail_tok[b, :tail_num[b]], host_tok[b + 1, :host_num[b + 1]]) for b in range(3))
    dev.free()
    upcm = unit_pcm()
    wcfg, wck, sup, beg = whisper_setup("whisper_tiny_test")
    wh = eng.WhisperSession.from_checkpoint(wcfg, wck, precision=BF16, suppress_tokens=sup, begin_suppress_tokens=beg, audio_dtype=np.int16)
    wh.taps(True)
    prompt = np.tile(np.asarray([[wcfg.sot_id, wcfg.first_language_id, wcfg.transcribe_id, wcfg.no_timestamps_id]], np.int32), (len(upcm), 1))
    npos = wh.encode_packed(np.concatenate(upcm), offs)
    mel, (nxt, logits) = wh.tap("mel_gapped", np.uint16), wh.prefill(prompt)
    dev = _DeviceAudio(np.concatenate(upcm))
    assert np.array_equal(wh.encode_packed(None, offs, audio_device_ptr=dev.ptr.value), npos)
    assert np.array_equal(wh.tap("mel_gapped", np.uint16), mel)
    nxt2, logits2 = wh.prefill(prompt)
    assert np.array_equal(nxt, nxt2) and np.array_equal(logits, logits2)
    dev.free()


def test_a_two_byte_session_takes_exactly_its_own_type():
    eng = sub("engine")
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    pcm = kaldi_pcm()
    lang = [2, 0, 1, 0]
    sess = eng.SenseVoiceSession.from_checkpoint(cfg, ck, precision=F32, audio_dtype=np.int16)
    want = sess.run(pcm, lang)
    with pytest.raises(TypeError, match=r"int16.*float32"):
        sess.run([p.astype(np.float32) for p in pcm], lang)
    with pytest.raises(TypeError, match=r"int16.*float32"):
        sess.run_packed(np.concatenate(pcm).astype(np.float32), np.asarray([0, 9001], np.int64), np.asarray([0], np.int32))
    assert all(np.array_equal(a, b) for a, b in zip(sess.run(pcm, lang), want))        # nothing was launched; the session still works
    sess.audio_dtype = np.float16
    with pytest.raises(TypeError, match=r"float16.*int16"):
        sess.run(pcm, lang)
    half = [p.astype(np.float16) for p in pcm]
    sess.run(half, lang)
    with pytest.raises(ValueError):
        sess.audio_dtype = np.float64
    with pytest.raises(sub("_lib").AsrError, match="unknown audio dtype"):
        sub("_lib").check(sub("_lib").load().asr_session_set_audio_dtype(sess._h, 7))
    assert sess.audio_dtype == np.float16
    # an F32 session keeps coercing whatever it is handed, as before
    sess.audio_dtype = np.float32
    assert all(np.array_equal(a, b) for a, b in zip(sess.run(pcm, lang), want))
    wcfg, wck, sup, beg = whisper_setup("whisper_tiny_test")
    wh = eng.WhisperSession.from_checkpoint(wcfg, wck, precision=F32, suppress_tokens=sup, begin_suppress_tokens=beg, audio_dtype="INT16")
    with pytest.raises(TypeError, match=r"int16.*float32"):
        wh.encode([as_f32(p, True) for p in unit_pcm()])
    assert wh.encode(unit_pcm()).size == 4
