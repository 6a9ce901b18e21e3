"""GPU: the device resampler (asr_session_set_input_format, asr_op_resample; csrc/resample.hip) against its float64 statement, tests/resample_ref.py.

1. the coefficient table: every entry within one rounding to float32 of the statement's;
2. impulses: EQUALITY with the table's float32 coefficients at the indices the statement names and zero elsewhere (one product with 1.0 and zeros is exact in
   any order) -- the impulse at frame 0, at the last frame and either side of a tile's first input frame: this pins every tap index, the outermost included;
3. random ragged batches: every output within (T + C + 2) 2^-24 sum_k |c[p][k]| |x[.]| of the statement (T multiply-adds in any order, the channel mean, the
   coefficient rounding), the bound evaluated per output from the reference; offsets by the n_out rule;
4. sessions of every family: a session with a non-default format equals, bit for bit, a default-format f32 session fed the op's own output;
5. one session that alternates formats never replays a step captured for another;
6. refusals leave the session usable.

TILE is the number of outputs a workgroup of resample.hip owns at the rates used here (its LDS holds their input span, TILE M / L + 2 W frames)."""
import ctypes as C

import numpy as np
import pytest

import resample_ref as R
from conftest import sub
from helpers import kaldi_audio, load_golden, sensevoice_setup
from test_oracle_paraformer import paraformer_setup
from test_oracle_paraformer_streaming import streaming_setup
from test_oracle_qwen_asr import qwen_setup, unit_audio
from test_oracle_whisper import whisper_setup

pytestmark = pytest.mark.gpu

BF16, F32 = 0, 1
TILE = 1024
EPS = 2.0 ** -24


def _frames_for(n_model, rate):
    """The largest frame count that comes out as at most n_model samples (exactly n_model when the rate is above the model's)."""
    L, M = R.design(rate)[:2]
    n = n_model * M // L
    assert n_model - (L - 1) // M <= R.n_out(n, rate) <= n_model
    return n


def _pack(clips, channels, lead=0):
    """Clips [n, C] (or [n] at C = 1) -> (packed interleaved samples behind `lead` frames of other data, frame offsets starting at `lead`)."""
    flat = [np.ascontiguousarray(c).reshape(-1) for c in clips]
    offs = lead + np.concatenate([[0], np.cumsum([f.size // channels for f in flat])]).astype(np.int64)
    junk = np.full(lead * channels, 12345, dtype=flat[0].dtype)
    return np.concatenate([junk] + flat), offs


# ------------------------------------------------------------------------------------------------ 1. table
@pytest.mark.parametrize("rate", R.RATES)
def test_table_is_the_statement_rounded_once(rate):
    L, M, W, c32 = sub("engine").resample_table(rate)
    assert (L, M, W, 2 * W + 1) == R.DESIGN[rate]
    c64 = R.table(rate)
    assert c32.shape == c64.shape and c32.dtype == np.float32
    err = np.abs(c32.astype(np.float64) - c64)
    print(f"{rate} Hz: worst |c32 - c64| / (2^-24 |c64| + 1e-12) = {(err / (EPS * np.abs(c64) + 1e-12)).max():.3f}")
    assert np.all(err <= EPS * np.abs(c64) + 1e-12)


# ------------------------------------------------------------------------------------------------ 2. impulses
@pytest.mark.parametrize("rate", [8000, 48000, 44100])
def test_impulses_return_the_table_exactly(rate):
    eng = sub("engine")
    L, M, W, c32 = eng.resample_table(rate)
    T = 2 * W + 1
    n_in = _frames_for(2 * TILE + 300, rate)
    edge = TILE * M // L                                      # the input frame output TILE starts from: the first tile's last centre is just below it
    where = [0, n_in - 1, edge - 1, edge]
    clips = []
    for i in where:
        x = np.zeros(n_in, np.float32)
        x[i] = 1.0
        clips.append(x)
    packed, offs = _pack(clips, 1, lead=3)
    y, offs_out = eng.op_resample(packed, offs, rate)
    assert np.array_equal(np.diff(offs_out), [R.n_out(n_in, rate)] * len(where))
    n = np.arange(R.n_out(n_in, rate))
    for b, i in enumerate(where):
        k = i - (n * M) // L + W
        ok = (k >= 0) & (k < T)
        want = np.where(ok, c32[(n * M) % L, np.clip(k, 0, T - 1)], np.float32(0))
        got = y[offs_out[b]:offs_out[b + 1]]
        assert np.count_nonzero(want) > W * L // (2 * M)                 # not vacuous: about W L / M outputs see an impulse at a clip's end, twice that inside
        assert np.array_equal(got, want), (rate, i, np.flatnonzero(got != want)[:8])


# ------------------------------------------------------------------------------------------------ 3. random clips against float64
def _random_clip(rng, n, channels, dtype, big):
    if dtype == np.int16:
        lo, hi = (-32768, 32768) if big else (-300, 300)
        x = rng.integers(lo, hi, size=(n, channels)).astype(np.int16)
    else:
        x = (rng.standard_normal((n, channels)) * (1000.0 if big else 1.0)).astype(dtype)
    return x


def _edge_batch(rng, rate, channels, dtype):
    """The smallest batch that can go wrong: 1 frame, W - 1 frames (shorter than the half width), one tile's input span -1 / +0 / +1 frame, about three tiles;
    the short clips between long ones filled with large values, so that a read across an utterance's edge shows."""
    L, M, W = R.design(rate)[:3]
    span = _frames_for(TILE, rate)
    lens = [(3 * TILE + 17) * M // L, 1, 2 * TILE * M // L + 5, max(W - 1, 1), span - 1, span, span + 1, (3 * TILE - 29) * M // L]
    big = [True, False, True, False, False, False, False, True]
    return [_random_clip(rng, n, channels, dtype, b) for n, b in zip(lens, big)]


def _check_against_reference(y, offs_out, clips, rate, channels, int16_scale, what):
    L, M, W, T, _ = R.design(rate)
    c64 = R.table(rate)
    assert offs_out[0] == 0 and np.array_equal(np.diff(offs_out), [R.n_out(c.shape[0], rate) for c in clips]), what
    assert y.dtype == np.float32 and y.size == offs_out[-1] and np.isfinite(y).all()
    worst = 0.0
    for b, c in enumerate(clips):
        y64, mag = R.resample(R.mono(c, int16_scale), rate, c64=c64)
        err = np.abs(y[offs_out[b]:offs_out[b + 1]].astype(np.float64) - y64)
        bound = (T + channels + 2) * EPS * mag
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0)
        bad = np.flatnonzero(err > bound)
        assert bad.size == 0, (what, b, c.shape[0], bad[:8], err[bad[:8]], bound[bad[:8]])
    print(f"{what}: worst error / bound {worst:.4f}")


GRID = [(8000, np.float32, 1, False), (8000, np.int16, 2, True), (48000, np.int16, 2, False), (48000, np.float16, 3, False), (48000, np.float32, 1, False),
        (44100, np.float32, 2, False), (44100, np.int16, 1, True), (22050, np.float16, 1, False), (22050, np.float32, 3, False),
        (16000, np.int16, 2, False), (16000, np.float32, 2, False), (16000, np.float16, 2, True)]


@pytest.mark.parametrize("rate,dtype,channels,scale", GRID, ids=[f"{r}-{np.dtype(d).name}-c{c}{'-scaled' if s else ''}" for r, d, c, s in GRID])
def test_random_ragged_batch_against_the_float64_reference(rate, dtype, channels, scale):
    rng = np.random.default_rng(rate + channels)
    clips = _edge_batch(rng, rate, channels, dtype)
    packed, offs = _pack(clips, channels, lead=5)
    y, offs_out = sub("engine").op_resample(packed, offs, rate, channels=channels, int16_scale=scale)
    _check_against_reference(y, offs_out, clips, rate, channels, scale and dtype == np.int16, f"{rate} Hz {np.dtype(dtype).name} C={channels}")


@pytest.mark.parametrize("rate,dtype,channels", [(48000, np.int16, 2), (44100, np.float32, 1), (8000, np.float16, 3)])
def test_session_buffers_hold_nothing_stale(rate, dtype, channels):
    """In ONE session (its staging, plan and output buffers are reused): the edge batch, then a long batch of other data, then the edge batch again; the
    "resampled" tap -- what the front end read -- against the reference each time. A clip a front end refuses (fewer than 400 samples at the model rate) cannot
    ride in a session call, so the 1-frame and W - 1-frame clips are the op-level test's; here they are replaced by the shortest clip a session takes."""
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    sess = sub("engine").SenseVoiceSession.from_checkpoint(cfg, ck, precision=F32, audio_dtype=dtype)
    sess.taps(True)
    sess.set_input_format(rate, channels)
    assert sess.input_format == (rate, channels)
    rng = np.random.default_rng(7 + rate)
    shortest = _frames_for(400, rate)
    clips = [c if c.shape[0] >= shortest else _random_clip(rng, shortest, channels, dtype, False) for c in _edge_batch(rng, rate, channels, dtype)]
    other = [_random_clip(rng, _frames_for(5 * TILE + 77, rate), channels, dtype, True) for _ in range(3)]

    def run(batch, what):
        sess.run(batch, [0] * len(batch))
        y = sess.tap("resampled").reshape(-1)
        offs_out = np.concatenate([[0], np.cumsum([R.n_out(c.shape[0], rate) for c in batch])])
        _check_against_reference(y, offs_out, batch, rate, channels, False, what)
        return y
    first = run(clips, "edge batch")
    run(other, "long batch")
    again = run(clips, "edge batch again")
    assert np.array_equal(first, again)


# ------------------------------------------------------------------------------------------------ 4. sessions: bits
LENGTHS = (9001, 12345, 7777)                   # at the model rate; the second and third utterance start at odd offsets


def _pcm_clips(rate, channels, unit, seed):
    """int16 clips of the frame counts that come out as LENGTHS: Kaldi-range values, or [-1, 1] rounded to PCM for the Whisper / Qwen front end."""
    out = []
    for i, n in enumerate(LENGTHS):
        m = _frames_for(n, rate) * channels
        a = unit_audio(seed + i, m) * 32768.0 if unit else kaldi_audio(seed + i, m)
        out.append(np.clip(np.round(a), -32768, 32767).astype(np.int16).reshape(-1, channels))
    return out


def _device_output(clips, rate, channels, unit):
    """What the default-format twin is fed: the op's own output (with the 2^-15 the family's front end applies to PCM), cut at the op's offsets."""
    packed, offs = _pack(clips, channels)
    y, o = sub("engine").op_resample(packed, offs, rate, channels=channels, int16_scale=unit)
    assert np.array_equal(np.diff(o), LENGTHS)
    return [y[o[b]:o[b + 1]].copy() for b in range(len(clips))]


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k, a[k].shape, b[k].shape)
        assert np.array_equal(a[k], b[k]), (what, k)


def _sensevoice(prec):
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    mk = lambda dt: sub("engine").SenseVoiceSession.from_checkpoint(cfg, ck, precision=prec, audio_dtype=dt)

    def results(sess, clips):
        lang = [2, 0, 1][:len(clips)]
        toks, timed = sess.run(clips, lang), sess.run_timed(clips, lang)
        out = {"num": np.asarray([t.size for t in toks]), "tokens": np.concatenate(toks)}
        for k in ("ids", "first_frame", "last_frame", "logprob"):
            out["timed_" + k] = np.concatenate([t[k] for t in timed])
        return out
    return mk, results, False


def _paraformer(prec):
    cfg, ck = paraformer_setup("paraformer_tiny")
    mk = lambda dt: sub("engine").ParaformerSession.from_checkpoint(cfg, ck, precision=prec, audio_dtype=dt)

    def results(sess, clips):
        toks = sess.run(clips)
        return {"num": np.asarray([t.size for t in toks]), "tokens": np.concatenate(toks) if toks else np.zeros(0, np.int32)}
    return mk, results, False


def _whisper(prec):
    cfg, ck, sup, beg = whisper_setup("whisper_tiny_test")
    mk = lambda dt: sub("engine").WhisperSession.from_checkpoint(cfg, ck, precision=prec, suppress_tokens=sup, begin_suppress_tokens=beg, audio_dtype=dt)

    def results(sess, clips):
        npos = sess.encode(clips)
        prompt = np.tile(np.asarray([[cfg.sot_id, cfg.first_language_id, cfg.transcribe_id, cfg.no_timestamps_id]], np.int32), (len(clips), 1))
        nxt, logits = sess.prefill(prompt)
        return {"npos": npos, "ids0": nxt, "logits0": logits}
    return mk, results, True


def _qwen(prec):
    g = load_golden("qwen_asr_tiny")
    cfg, ck = qwen_setup(g)
    pre, post = [g["head_ids"].tolist() + g["suffix_ids"].tolist()], [g["tail_ids"].tolist()]
    mk = lambda dt: sub("engine").QwenAsrSession.from_checkpoint(cfg, ck, precision=prec, audio_dtype=dt)

    def results(sess, clips):
        nxt, logits, ids_len = sess.prefill(clips, pre, post)
        return {"ids_len": ids_len, "ids0": nxt, "logits0": logits}
    return mk, results, True


FAMILIES = {"sensevoice": _sensevoice, "paraformer": _paraformer, "whisper": _whisper, "qwen_asr": _qwen}


@pytest.mark.parametrize("prec", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_a_session_with_an_input_format_equals_the_default_session_on_the_device_output(family, prec):
    """A: set_input_format(rate, channels), int16 audio, fed x.  B: default format, f32 audio, fed op_resample(x).  Both hand the same f32 samples to the same
    front end, so everything they return is equal bit for bit. 48 kHz stereo (L = 1), then 44.1 kHz mono (L = 160) on the same two sessions."""
    mk, results, unit = FAMILIES[family](prec)
    a, b = mk(np.int16), mk(np.float32)
    for rate, channels in ((48000, 2), (44100, 1)):
        clips = _pcm_clips(rate, channels, unit, 940 + channels)
        a.set_input_format(rate, channels)
        assert a.input_format == (rate, channels) and b.input_format == (16000, 1)
        got = results(a, clips)
        want = results(b, _device_output(clips, rate, channels, unit))
        assert all(np.isfinite(v).all() for v in want.values() if v.dtype.kind == "f")
        _same(got, want, f"{family} {rate} Hz x{channels}")


class _DeviceAudio:
    """Samples placed in HBM with asr_mem_alloc / asr_mem_copy."""

    def __init__(self, packed):
        self.lib, self.ptr = sub("_lib").load(), C.c_void_p(None)
        sub("_lib").check(self.lib.asr_mem_alloc(0, packed.nbytes, C.byref(self.ptr)))
        sub("_lib").check(self.lib.asr_mem_copy(0, self.ptr, packed.ctypes.data_as(C.c_void_p), packed.nbytes, 0))

    def free(self):
        sub("_lib").check(self.lib.asr_mem_free(0, self.ptr))


def test_device_resident_frames_equal_host_frames():
    """audio_device_ptr with a format: offsets are frames, the pointer steps in frames of `channels` int16 samples (a batch that starts inside the buffer)."""
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    sv = sub("engine").SenseVoiceSession.from_checkpoint(cfg, ck, precision=BF16, audio_dtype=np.int16)
    sv.set_input_format(48000, 2)
    clips = _pcm_clips(48000, 2, False, 950)
    packed, offs = _pack(clips, 2)
    lang = np.asarray([2, 0, 1], np.int32)
    host_tok, host_num = sv.run_packed(packed, offs, lang)
    dev = _DeviceAudio(packed)
    dev_tok, dev_num = sv.run_packed(None, offs, lang, audio_device_ptr=dev.ptr.value)
    assert np.array_equal(host_num, dev_num) and np.array_equal(host_tok, dev_tok)
    tail_tok, tail_num = sv.run_packed(None, offs[1:], lang[1:], audio_device_ptr=dev.ptr.value)
    assert np.array_equal(tail_num, host_num[1:]) and all(np.array_equal(tail_tok[b, :tail_num[b]], host_tok[b + 1, :host_num[b + 1]]) for b in range(2))
    dev.free()


def test_whisper_transcriber_with_a_format_equals_the_session_calls_it_stands_for():
    """WhisperTranscriber.transcribe / transcribe_file(sample_rate=48000, channels=2) on a real session: the ids are the ones the session gives when its format is
    set by hand, the format is back to the default behind the call, and the file loop's windows (cut in input frames) are the batch form's clips."""
    eng, wh = sub("engine"), sub("whisper")
    cfg, ck, sup, beg = whisper_setup("whisper_tiny_test")
    sess = eng.WhisperSession.from_checkpoint(cfg, ck, precision=F32, suppress_tokens=sup, begin_suppress_tokens=beg, audio_dtype=np.int16)
    clips = _pcm_clips(48000, 2, True, 1010)
    kw = dict(suppress_tokens=sup, no_speech_threshold=2.0, detect_language=False, remove_repeats=False)
    tr = wh.WhisperTranscriber(cfg, sess, **kw)
    out, stat = tr.transcribe(clips, max_new=6, sample_rate=48000, channels=2)
    assert sess.input_format == (16000, 1) and stat["rtf"] > 0
    sess.set_input_format(48000, 2)
    npos = sess.encode(clips)
    prompt = np.tile(np.asarray([[cfg.sot_id, cfg.first_language_id, cfg.transcribe_id, cfg.no_timestamps_id]], np.int32), (len(clips), 1))
    sess.prefill(prompt, want_logits=False)
    by_hand = sess.generate(6, eos_id=cfg.eot_id)
    sess.set_input_format(16000, 1)
    assert np.array_equal(npos, [(n // cfg.hop_length + 1) // 2 for n in LENGTHS])
    assert all(np.array_equal(o["tokens"], np.asarray(t, np.int32)) for o, t in zip(out, by_hand))
    # one file of 70000 frames (23334 model-rate samples) as windows of 9600 every 4800: four windows of 28800 frames, the last one zero-padded by 2000
    file48 = np.concatenate(clips)[:70000]
    res, _ = tr.transcribe_file(file48, sliding_window=4800, input_audio_length=9600, max_new=6, sample_rate=48000, channels=2)
    assert (res["n_windows"], res["window"], res["stride"]) == (4, 9600, 4800) and sess.input_format == (16000, 1)
    padded = np.concatenate([file48, np.zeros((2000, 2), np.int16)])
    batch, _ = tr.transcribe([padded[w * 14400:w * 14400 + 28800] for w in range(4)], max_new=6, sample_rate=48000, channels=2)
    assert all(np.array_equal(np.asarray(w, np.int32), b["tokens"]) for w, b in zip(res["windows"], batch))
    with pytest.raises(ValueError, match="not an integer"):
        tr.transcribe_file(file48[:, 0], sliding_window=4801, input_audio_length=9600, sample_rate=44100)
    assert sess.input_format == (16000, 1)


# ------------------------------------------------------------------------------------------------ 5. switching
def test_alternating_formats_never_replays_another_formats_step():
    """One bf16 SenseVoice session, taps off (captured steps), f32 audio throughout, every batch with the SAME model-rate lengths -- so the pointer the front end
    reads and the format are all that tell the steps apart: default, 48000 x 2, default, 44100 x 1, default, each run three times (eager, capture, replay)."""
    eng = sub("engine")
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    lang = [2, 0, 1]
    plain = [kaldi_audio(960 + i, n).astype(np.float32) for i, n in enumerate(LENGTHS)]
    fmt = {(48000, 2): [c.astype(np.float32) for c in _pcm_clips(48000, 2, False, 970)], (44100, 1): [c.astype(np.float32) for c in _pcm_clips(44100, 1, False, 980)]}

    def answer(s, clips):                                        # ids, spans and the float confidences of every token, as one array of bits
        timed = s.run_timed(clips, lang)
        return np.concatenate([np.concatenate([t["ids"], t["first_frame"], t["last_frame"], t["logprob"].view(np.int32)]) for t in timed])

    def fresh(rate_ch, clips):
        s = eng.SenseVoiceSession.from_checkpoint(cfg, ck, precision=BF16)
        if rate_ch:
            s.set_input_format(*rate_ch)
        return answer(s, clips)
    want = {None: fresh(None, plain), **{k: fresh(k, v) for k, v in fmt.items()}}
    assert not np.array_equal(want[None], want[(48000, 2)]) and not np.array_equal(want[(48000, 2)], want[(44100, 1)])      # three different answers: not vacuous
    sess = eng.SenseVoiceSession.from_checkpoint(cfg, ck, precision=BF16)
    for step, key in enumerate([None, (48000, 2), None, (44100, 1), None]):
        sess.set_input_format(*(key or (16000, 1)))
        for rep in range(3):
            got = answer(sess, plain if key is None else fmt[key])
            assert np.array_equal(got, want[key]), (step, key, rep)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_session_usable():
    eng, lib = sub("engine"), sub("_lib")
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    sess = eng.SenseVoiceSession.from_checkpoint(cfg, ck, precision=F32)
    plain = [kaldi_audio(990 + i, n).astype(np.float32) for i, n in enumerate(LENGTHS)]
    lang = [2, 0, 1]
    want = np.concatenate(sess.run(plain, lang))
    sess.set_input_format(48000, 2)
    for rate, channels, msg in ((0, 1, "rates are positive"), (-8000, 1, "rates are positive"), (48000, 9, "channels"), (48000, 0, "channels"),
                                (16001, 1, "filter phases"), (1_600_000, 1, "too far above")):
        with pytest.raises(lib.AsrError, match=msg) as e:
            sess.set_input_format(rate, channels)
        assert e.value.code == 1                                 # ASR_ERR_INVALID
        assert sess.input_format == (48000, 2)                   # the format in force stays
    stereo = [c.astype(np.float32) for c in _pcm_clips(48000, 2, False, 995)]
    got48 = np.concatenate(sess.run(stereo, lang))
    with pytest.raises(lib.AsrError):
        sess.run([np.zeros((100, 2), np.float32)], [0])           # 34 samples at the model rate: the front end's own length check, on the resampled length
    assert np.array_equal(np.concatenate(sess.run(stereo, lang)), got48)
    sess.set_input_format(16000, 1)                              # ... and the default format is the default path again
    assert sess.input_format == (16000, 1)
    assert np.array_equal(np.concatenate(sess.run(plain, lang)), want)
    with pytest.raises(lib.AsrError, match="rates are positive"):
        eng.op_resample(np.zeros(10, np.float32), [0, 10], 0)
    with pytest.raises(lib.AsrError, match="filter phases"):
        eng.resample_table(16001)

    g = load_golden("paraformer_streaming_tiny")
    scfg, sck = streaming_setup(g)
    chunk = int(g["chunk"])
    st = eng.ParaformerStreamSession(scfg, sck, precision=F32, chunk=chunk, max_streams=2)
    audio = np.stack([kaldi_audio(996 + i, chunk) for i in range(2)]).astype(np.float32)
    first = st.step(audio, [0, 1])
    st.set_input_format(48000, 1)
    for step in (st.step, st.step_timed):
        with pytest.raises(lib.AsrError, match="streaming sessions take model-rate mono") as e:
            step(audio, [0, 1])
        assert e.value.code == 1
    st.set_input_format(16000, 1)
    st.reset(-1)
    again = st.step(audio, [0, 1])
    assert all(np.array_equal(x, y) for x, y in zip(first, again))
