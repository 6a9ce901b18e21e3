"""GPU, session level: the streaming input format (asr_session_set_input_format on an asr_paraformer_stream_create session).

1. a session with a format equals, bit for bit, a default-format f32 session fed the first one's "resampled" tap, over step / step_timed / step_beam with a
   changing subset of streams and a mid-run reset; the tap equals engine.op_resample_stream of the same frames;
2. HBM-resident rows equal host rows (captured steps);
3. one session that alternates formats between full resets never replays another format's step;
4. refusals: a format change while a stream carries frames, the rates the offline path refuses, a formatted step of a stream that was stepped at the default
   format; input_frames;
5. ParaformerStreamTranscriber.transcribe_many(sample_rate=, channels=) equals the session calls it stands for."""
import ctypes as C

import numpy as np
import pytest

import resample_stream_ref as RS
from conftest import sub
from helpers import kaldi_audio, load_golden
from test_oracle_paraformer_streaming import streaming_setup

pytestmark = pytest.mark.gpu

BF16, F32 = 0, 1
SCHEDULE = [[0, 1, 2], [2, 0], [1, 2], [0, 1, 2], [1, 0]]          # the streams of each step, in slot order
RESET_BEFORE = {3: 2}                                              # step -> the stream that is reset in front of it


def _setup():
    g = load_golden("paraformer_streaming_tiny")
    cfg, ck = streaming_setup(g)
    return cfg, ck, int(g["chunk"])


def _frames(seed, n, channels, dtype):
    a = kaldi_audio(seed, n * channels).reshape(n, channels)
    return np.clip(np.round(a), -32768, 32767).astype(np.int16) if dtype == np.int16 else a.astype(dtype)


class _Feeder:
    """Per stream its signal since the last reset and its step count: rows(ids) cuts the frames the streams' next steps read into [n, pitch, channels]."""

    def __init__(self, S, rate, channels, dtype, seed, max_steps=len(SCHEDULE)):
        self.S, self.rate, self.channels, self.dtype, self.seed, self.max_steps = S, rate, channels, dtype, seed, max_steps
        self.signal, self.count = {}, {}

    def reset(self, sid):
        self.seed += 1
        self.signal[sid] = _frames(self.seed, RS.start(self.S, self.rate, self.max_steps), self.channels, self.dtype)
        self.count[sid] = 0

    def rows(self, ids, tail=0):
        out = np.full((len(ids), RS.pitch(self.S, self.rate), self.channels), tail, dtype=self.dtype)
        for j, sid in enumerate(ids):
            c = self.count[sid]
            a0, a1 = RS.start(self.S, self.rate, c), RS.start(self.S, self.rate, c + 1)
            out[j, :a1 - a0] = self.signal[sid][a0:a1]
            self.count[sid] = c + 1
        return out


def _bits(x):
    """Everything a step returned as a flat list of comparable pieces (floats by their bits)."""
    if isinstance(x, dict):
        return [p for k in sorted(x) for p in [k] + _bits(x[k])]
    if isinstance(x, (list, tuple)):
        return [len(x)] + [p for v in x for p in _bits(v)]
    a = np.asarray(x)
    return [(a.dtype.str, a.shape, a.view(np.uint32).tolist() if a.dtype == np.float32 else a.tolist())]


@pytest.mark.parametrize("rate,channels,dtype", [(48000, 2, np.int16), (44100, 1, np.float32)], ids=["48000x2-int16", "44100x1-f32"])
@pytest.mark.parametrize("prec", [F32, BF16], ids=["f32", "bf16"])
def test_a_formatted_session_equals_a_default_session_fed_its_resampled_tap(prec, rate, channels, dtype, monkeypatch):
    monkeypatch.setenv("ASR_STREAM_SHARE", "0")          # the twins alternate on this GPU
    eng = sub("engine")
    cfg, ck, S = _setup()
    a = eng.ParaformerStreamSession(cfg, ck, precision=prec, chunk=S, max_streams=3, audio_dtype=dtype)
    b = eng.ParaformerStreamSession(cfg, ck, precision=prec, chunk=S, max_streams=3)
    a.taps(True)
    a.set_input_format(rate, channels)
    assert a.input_format == (rate, channels) and b.input_format == (16000, 1)
    P = RS.pitch(S, rate)
    emitted = 0
    for form in ("step", "step_timed", "step_beam"):
        a.reset(-1), b.reset(-1)
        if form == "step_beam":
            a.set_beam(4), b.set_beam(4)
        feed = _Feeder(S, rate, channels, dtype, seed=8100 + rate // 100)
        for sid in range(3):
            feed.reset(sid)
        op_audio = np.zeros((len(SCHEDULE), 3, P, channels), dtype)
        mode = np.zeros((len(SCHEDULE), 3), np.int32)
        taps = []
        for k, ids in enumerate(SCHEDULE):
            if k in RESET_BEFORE:
                a.reset(RESET_BEFORE[k]), b.reset(RESET_BEFORE[k]), feed.reset(RESET_BEFORE[k])
            need, pitch = a.input_frames(ids)
            assert pitch == P and need.tolist() == [RS.need(S, rate, feed.count[s]) for s in ids]
            rows = feed.rows(ids, tail=7)                 # (whatever lies beyond a row's need is ignored)
            op_audio[k, ids] = rows
            mode[k, ids] = 1
            if k in RESET_BEFORE:
                mode[k, RESET_BEFORE[k]] = 2
            got = getattr(a, form)(rows, ids)
            tap = a.tap("resampled")
            assert tap.shape == (len(ids), S)
            taps.append(tap)
            want = getattr(b, form)(tap, ids)
            assert _bits(got) == _bits(want), (form, k)
            emitted += sum(len(r if form == "step" else r["ids"]) for r in got)
        out, frames, _ = eng.op_resample_stream(op_audio, mode, rate, channels=channels, chunk=S)
        for k, ids in enumerate(SCHEDULE):
            assert np.array_equal(taps[k].view(np.uint32), out[k, ids].view(np.uint32)), (form, k)
    assert emitted > 0
    a.close(), b.close()


class _DeviceAudio:
    """Samples placed in HBM with asr_mem_alloc / asr_mem_copy."""

    def __init__(self, packed):
        self.lib, self.ptr = sub("_lib").load(), C.c_void_p(None)
        sub("_lib").check(self.lib.asr_mem_alloc(0, packed.nbytes, C.byref(self.ptr)))
        sub("_lib").check(self.lib.asr_mem_copy(0, self.ptr, packed.ctypes.data_as(C.c_void_p), packed.nbytes, 0))

    def free(self):
        sub("_lib").check(self.lib.asr_mem_free(0, self.ptr))


def test_device_resident_rows_equal_host_rows():
    eng = sub("engine")
    cfg, ck, S = _setup()
    sess = eng.ParaformerStreamSession(cfg, ck, precision=BF16, chunk=S, max_streams=2, audio_dtype=np.int16)
    sess.set_input_format(48000, 2)
    feed = _Feeder(S, 48000, 2, np.int16, seed=8300, max_steps=4)
    feed.reset(0), feed.reset(1)
    rows = [feed.rows([1, 0]) for _ in range(4)]          # four steps of one set size: eager, captured, replayed twice
    host = [sess.step_timed(r, [1, 0]) for r in rows]
    sess.reset(-1)
    dev = []
    for r in rows:
        d = _DeviceAudio(np.ascontiguousarray(r))
        dev.append(sess.step_timed(None, [1, 0], audio_device_ptr=d.ptr.value))
        d.free()
    assert _bits(host) == _bits(dev)
    assert sum(len(r["ids"]) for step in host for r in step) > 0
    sess.close()


def test_alternating_formats_never_replays_another_formats_step():
    """One bf16 session, taps off (captured steps), f32 audio throughout, two streams: default, 48000 x 2, default, 44100 x 1, default, a full reset between the
    phases and three steps in each (eager, capture, replay). Every phase equals a fresh session's."""
    eng = sub("engine")
    cfg, ck, S = _setup()
    keys = [None, (48000, 2), None, (44100, 1), None]

    def phase_audio(key):
        if key is None:
            return [np.stack([kaldi_audio(8400 + 10 * k + i, S) for i in range(2)]).astype(np.float32) for k in range(3)]
        feed = _Feeder(S, key[0], key[1], np.float32, seed=8500 + key[1], max_steps=3)
        feed.reset(0), feed.reset(1)
        return [feed.rows([0, 1]) for _ in range(3)]
    audio = {key: phase_audio(key) for key in set(keys)}

    def run(sess, key):
        sess.reset(-1)
        sess.set_input_format(*(key or (16000, 1)))
        return _bits([sess.step_timed(r, [0, 1]) for r in audio[key]])

    want = {key: run(eng.ParaformerStreamSession(cfg, ck, precision=BF16, chunk=S, max_streams=2), key) for key in set(keys)}
    assert want[None] != want[(48000, 2)] and want[(48000, 2)] != want[(44100, 1)]          # three different answers: not vacuous
    sess = eng.ParaformerStreamSession(cfg, ck, precision=BF16, chunk=S, max_streams=2)
    for n, key in enumerate(keys):
        assert run(sess, key) == want[key], (n, key)
    sess.close()


def test_refusals_and_input_frames():
    eng, lib = sub("engine"), sub("_lib")
    cfg, ck, S = _setup()
    sess = eng.ParaformerStreamSession(cfg, ck, precision=F32, chunk=S, max_streams=3)
    need, pitch = sess.input_frames([0, 2])
    assert need.tolist() == [S, S] and pitch == S                  # the default format
    sess.set_input_format(48000, 2)
    feed = _Feeder(S, 48000, 2, np.float32, seed=8600)
    feed.reset(0), feed.reset(1)
    first = sess.step(feed.rows([0, 1]), [0, 1])
    need, pitch = sess.input_frames([0, 1, 2])
    assert need.tolist() == [RS.need(S, 48000, 1), RS.need(S, 48000, 1), RS.need(S, 48000, 0)] and pitch == RS.pitch(S, 48000)
    # a stepped stream that has not been reset: the format stays, whatever is asked for
    for rate, channels in ((44100, 1), (16000, 1), (48000, 1)):
        with pytest.raises(lib.AsrError, match="holds audio history") as e:
            sess.set_input_format(rate, channels)
        assert e.value.code == 1 and sess.input_format == (48000, 2)
    sess.reset(0)
    with pytest.raises(lib.AsrError, match="holds audio history"):
        sess.set_input_format(44100, 1)                            # stream 1 still holds frames
    assert sess.input_format == (48000, 2)
    second = sess.step(feed.rows([1]), [1])                        # ... and the session goes on as it was
    assert len(second) == 1
    sess.reset(-1)
    for rate, channels, msg in ((0, 1, "rates are positive"), (48000, 9, "channels"), (16001, 1, "filter phases"), (1_600_000, 1, "too far above")):
        with pytest.raises(lib.AsrError, match=msg) as e:
            sess.set_input_format(rate, channels)
        assert e.value.code == 1 and sess.input_format == (48000, 2)
    sess.set_input_format(44100, 1)                                # accepted behind the reset
    assert sess.input_format == (44100, 1)
    feed = _Feeder(S, 48000, 2, np.float32, seed=8600)             # the same frames as the first step: a reset stream starts over
    sess.set_input_format(48000, 2)
    feed.reset(0), feed.reset(1)
    again = sess.step(feed.rows([0, 1]), [0, 1])
    assert _bits(first) == _bits(again)
    # a stream stepped at the default format carries no frames: the format may change, but until its reset the stream takes model-rate mono
    sess.reset(-1)
    sess.set_input_format(16000, 1)
    sess.step(np.stack([kaldi_audio(8700, S)]).astype(np.float32), [2])
    sess.set_input_format(48000, 2)
    feed.reset(2), feed.reset(0)
    for call in (lambda: sess.step(feed.rows([2]), [2]), lambda: sess.input_frames([2])):
        with pytest.raises(lib.AsrError, match="stepped at the default format") as e:
            call()
        assert e.value.code == 1
    assert len(sess.step(feed.rows([0]), [0])) == 1                # another stream is not held up
    sess.reset(2)
    feed.reset(2)
    assert len(sess.step(feed.rows([2]), [2])) == 1
    sess.close()


def test_transcriber_with_a_format_equals_the_session_calls_it_stands_for():
    eng, ps = sub("engine"), sub("paraformer_streaming")
    cfg, ck, S = _setup()
    rate, channels = 48000, 2
    sess = eng.ParaformerStreamSession(cfg, ck, precision=F32, chunk=S, max_streams=2, audio_dtype=np.int16)
    tr = ps.ParaformerStreamTranscriber(sess, [f"<{i}>" for i in range(cfg.vocab)])
    n_frames = [RS.start(S, rate, 2) + 777, RS.start(S, rate, 4) - 5]
    clips = [_frames(8800 + i, n, channels, np.int16) for i, n in enumerate(n_frames)]
    out, stats = tr.transcribe_many(clips, rng=np.random.default_rng(5), sample_rate=rate, channels=channels)
    assert sess.input_format == (16000, 1) and sess.input_frames([0])[0].tolist() == [S] and stats["chunks"] == 4
    rng = np.random.default_rng(5)
    padded = [ps.pad_frames_to_steps(c, S, rate, 16000, rng) for c in clips]
    assert [c for _, c in padded] == [3, 4] and [p.shape[0] for p, _ in padded] == [RS.start(S, rate, 3), RS.start(S, rate, 4)]
    assert all(np.array_equal(p[:c.shape[0]], c) for (p, _), c in zip(padded, clips))
    sess.reset(-1)
    sess.set_input_format(rate, channels)
    by_hand = [[], []]
    for k in range(4):
        live = [i for i in range(2) if k < padded[i][1]]
        need, pitch = sess.input_frames(live)
        rows = np.zeros((len(live), pitch, channels), np.int16)
        for j, i in enumerate(live):
            rows[j, :need[j]] = padded[i][0][RS.start(S, rate, k):RS.start(S, rate, k + 1)]
        for i, tok in zip(live, sess.step(rows, live)):
            by_hand[i].append(tok[~np.isin(tok, tr.stop)])
    assert sum(t.size for ts in by_hand for t in ts) > 0
    for o, ts in zip(out, by_hand):
        assert np.array_equal(o["token_ids"], np.concatenate(ts))
    sess.close()
