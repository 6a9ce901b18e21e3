"""CPU: the host side of a session's input format -- wav frames as the file holds them, windows cut in input frames, and transcriber results that stay in the
same seconds (a stub session: nothing here needs a device)."""
import types
import wave

import numpy as np
import pytest

from conftest import sub


def test_read_wav_native_returns_the_files_own_frames(tmp_path):
    rng = np.random.default_rng(0)
    frames = rng.integers(-32768, 32768, size=(4411, 2)).astype(np.int16)
    path = str(tmp_path / "stereo_44k1.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(frames.astype("<i2").tobytes())
    got, rate, channels = sub("audio_io").read_wav_native(path)
    assert (rate, channels) == (44100, 2) and got.dtype == np.int16 and got.shape == (4411, 2)
    assert np.array_equal(got, frames)                       # no down-mix, no rate conversion
    mono = str(tmp_path / "mono_16k.wav")
    sub("audio_io").write_wav_int16(mono, frames[:, 0])
    got, rate, channels = sub("audio_io").read_wav_native(mono)
    assert (rate, channels) == (16000, 1) and np.array_equal(got[:, 0], frames[:, 0])
    assert np.array_equal(sub("audio_io").read_wav_int16(mono), frames[:, 0])      # the parity ingest is what it was


def test_sixteen_bit_wav_needs_no_audioop(tmp_path, monkeypatch):
    """audioop left the standard library in Python 3.13: reading 16-bit PCM as it is must not touch it."""
    aio = sub("audio_io")

    def gone():
        raise ImportError("no audioop")
    monkeypatch.setattr(aio, "_audioop", gone)
    path = str(tmp_path / "a.wav")
    aio.write_wav_int16(path, np.arange(100, dtype=np.int16), 8000)
    got, rate, channels = aio.read_wav_native(path)
    assert (rate, channels) == (8000, 1) and np.array_equal(got[:, 0], np.arange(100))
    with pytest.raises(ImportError):
        aio.read_wav_int16(path)


def test_windows_are_cut_in_input_frames():
    fmt = sub("input_format")
    assert fmt.ratio(48000, 16000) == (1, 3) and fmt.ratio(44100, 16000) == (160, 441) and fmt.ratio(8000, 16000) == (2, 1)
    assert [fmt.model_samples(n, 44100, 16000) for n in (0, 1, 440, 441, 442)] == [0, 1, 160, 160, 161]
    assert fmt.input_frames(16000, 48000, 16000) == 48000 and fmt.input_frames(16000, 44100, 16000) == 44100 and fmt.input_frames(320, 44100, 16000) == 882
    with pytest.raises(ValueError, match="not an integer"):
        fmt.input_frames(16001, 44100, 16000)                # 16001 * 441 / 160
    with pytest.raises(ValueError, match="not an integer"):
        fmt.input_frames(15, 8000, 16000)                    # 7.5 frames
    frames = np.arange(2 * 100000, dtype=np.int64).astype(np.int16).reshape(-1, 2)       # 100000 stereo frames at 48 kHz = 33334 samples
    window, cuts = fmt.cut_windows(frames, 16000, 8000, 48000, 16000)
    assert window == 16000 and [s for s, _ in cuts] == [0, 8000, 16000, 24000]           # ceil((33334 - 16000) / 8000) + 1 windows, as the model-rate loop plans
    assert all(w.shape == (48000, 2) for _, w in cuts)
    assert np.array_equal(cuts[1][1], frames[24000:72000])
    assert np.array_equal(cuts[3][1][:28000], frames[72000:]) and not cuts[3][1][28000:].any()      # the tail is zero frames
    window, cuts = fmt.cut_windows(frames, None, None, 48000, 16000)                     # a dynamic axis: the clip is the window
    assert window == 33334 and len(cuts) == 1 and cuts[0][1] is frames
    with pytest.raises(ValueError, match="stride"):
        fmt.cut_windows(frames[:, :1], 16000, 8001, 44100, 16000)
    assert fmt.as_frames(np.arange(6, dtype=np.int16), 2).shape == (3, 2)
    with pytest.raises(ValueError):
        fmt.as_frames(np.arange(7, dtype=np.int16), 2)


def test_prepare_audio_input_refuses_to_normalise_interleaved_channels():
    pcm = np.ones(8, np.int16)
    with pytest.raises(ValueError, match="mono"):
        sub("sensevoice").prepare_audio_input(pcm.reshape(1, 1, -1), "F32", audio_pcm_scale=1, normalise=True, channels=2)
    with pytest.raises(ValueError, match="mono"):
        sub("whisper").prepare_audio_input(pcm, normalise=True, channels=2)
    assert sub("whisper").prepare_audio_input(pcm, normalise=False, channels=2).shape == (8,)
    assert sub("sensevoice").prepare_audio_input(pcm.reshape(1, 1, -1), "F32", audio_pcm_scale=1, normalise=True).shape == (1, 1, 8)


class _Native:
    """What a SenseVoiceSession shows a transcriber, recording how it was called: two tokens per window at fixed rows."""

    def __init__(self):
        self.cfg = sub("config").sensevoice_tiny()
        self.calls, self.formats, self._fmt = [], [], (16000, 1)

    @property
    def input_format(self):
        return self._fmt

    def set_input_format(self, sample_rate, channels=1):
        if sample_rate == 16001:
            raise sub("_lib").AsrError(1, "refused")
        self._fmt = (sample_rate, channels)
        self.formats.append(self._fmt)

    def run_packed_timed(self, audio, offsets, lang):
        self.calls.append((audio.dtype, audio.size, offsets.tolist(), self._fmt))
        tok, num = np.asarray([[7, 9]], np.int32), np.asarray([2], np.int32)
        return tok, num, np.asarray([[5, 11]], np.int32), np.asarray([[8, 13]], np.int32), np.asarray([[-0.5, -0.25]], np.float32)


def _stub_transcriber(window):
    sv = sub("sensevoice")
    tr = sv.SenseVoiceTranscriber.__new__(sv.SenseVoiceTranscriber)
    native = _Native()
    binding = types.SimpleNamespace(bind_cpu_input=lambda *a: None)
    tr.session = types.SimpleNamespace(_native=native, io_binding=lambda: binding)
    tr.audio_meta = types.SimpleNamespace(name="audio", shape=[1, 1, window], type="tensor(int16)")
    tr.lang_meta = types.SimpleNamespace(name="language_idx", shape=[1], type="tensor(int32)")
    tr.tokenizer, tr.sample_rate, tr.selector_index, tr.input_audio_dtype, tr.audio_pcm_scale = None, 16000, 0, "INT16", 1
    tr.device_type, tr.device_id, tr.language = "cpu", 0, "en"
    return tr, native


def test_transcriber_seconds_do_not_change_with_the_input_format():
    """The same three seconds as 16 kHz mono and as 48 kHz stereo: the same windows, the same token times; the format is set for the call only."""
    tr, native = _stub_transcriber(16000)
    plain = tr.transcribe(np.zeros(40000, np.int16), timestamps=True)
    assert native.formats == [] and [c[2] for c in native.calls] == [[0, 16000]] * 3 and all(c[3] == (16000, 1) for c in native.calls)
    native.calls.clear()
    stereo = tr.transcribe(np.zeros((120000, 2), np.int16), timestamps=True, sample_rate=48000, channels=2)
    assert [c[2] for c in native.calls] == [[0, 48000]] * 3                          # offsets count frames ...
    assert all(c[1] == 96000 and c[3] == (48000, 2) for c in native.calls)           # ... of two samples, under the call's format
    assert native.formats == [(48000, 2), (16000, 1)] and native.input_format == (16000, 1)      # put back behind the call
    assert stereo["windows"] == plain["windows"] == 3
    assert stereo["tokens"] == plain["tokens"]
    assert [t["start"] for t in plain["tokens"][2:4]] == [1.0 + t["start"] for t in plain["tokens"][:2]]      # window 1 starts a second in, in both
    assert plain["tokens"][-1]["end"] <= 2.5                                          # clipped to the audio's 2.5 s
    for k in ("token_ids", "windows", "language"):
        assert np.array_equal(np.asarray(stereo[k]), np.asarray(plain[k]))
    # 44.1 kHz: a 16000-sample window is 44100 frames; one of 16001 samples is no whole number of frames
    native.calls.clear()
    tr.transcribe(np.zeros(110250, np.int16), timestamps=True, sample_rate=44100)
    assert [c[2] for c in native.calls] == [[0, 44100]] * 3
    tr441, native441 = _stub_transcriber(16001)
    with pytest.raises(ValueError, match="not an integer"):
        tr441.transcribe(np.zeros(110250, np.int16), timestamps=True, sample_rate=44100)
    assert native441.calls == [] and native441.input_format == (16000, 1)
    # a failing call still puts the format back; a refused format leaves the one in force
    def boom(*a):
        raise RuntimeError("device lost")
    native.run_packed_timed = boom
    with pytest.raises(RuntimeError):
        tr.transcribe(np.zeros((48000, 2), np.int16), timestamps=True, sample_rate=48000, channels=2)
    assert native.input_format == (16000, 1)
    with pytest.raises(sub("_lib").AsrError):
        tr.transcribe(np.zeros(48000, np.int16), timestamps=True, sample_rate=16001)
    assert native.input_format == (16000, 1)
    with pytest.raises(ValueError, match="mono"):
        tr.transcribe(np.zeros((48000, 2), np.int16), normalise=True, sample_rate=48000, channels=2)


def test_session_counts_frames_and_model_lengths():
    """engine._Session without a library handle: packing divides by the channel count, lengths follow the resampler's rule."""
    eng = sub("engine")
    s = eng._Session.__new__(eng._Session)
    s._audio_np, s._format, s.cfg = np.dtype(np.int16), (44100, 2), types.SimpleNamespace(sample_rate=16000)
    flat, packed, offs = s._pack([np.zeros((441, 2), np.int16), np.zeros(10, np.int16)])
    assert offs.tolist() == [0, 441, 446] and packed.size == 892
    assert s.model_lengths(np.diff(offs)).tolist() == [160, 2]
    with pytest.raises(ValueError, match="channels"):
        s._pack([np.zeros(7, np.int16)])
    s._format = None
    assert s._pack([np.zeros(7, np.int16)])[2].tolist() == [0, 7] and s.model_lengths([7]).tolist() == [7]
    s._h = None                                               # (nothing to destroy)
