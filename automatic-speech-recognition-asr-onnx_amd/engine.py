"""Python handles over the C ABI: sessions, taps, profiling, operator hooks."""
from __future__ import annotations

import ctypes as C
import dataclasses
import warnings
from typing import Sequence

import numpy as np

from . import _lib
from .arena import PRECISION_BF16, PRECISION_F32, PRECISION_FP8MM, PRECISION_FP8W, PRECISION_MXFP4W, build_sensevoice_arena
from .config import SenseVoiceConfig

MEM_HOST, MEM_DEVICE = 0, 1
AUDIO_F32, AUDIO_I16, AUDIO_F16 = 0, 1, 2                         # asr_audio_dtype
# the reference's INPUT_AUDIO_DTYPE names (Export_*.py) <-> sample types
AUDIO_DTYPE_NAMES = {"F32": np.dtype(np.float32), "INT16": np.dtype(np.int16), "F16": np.dtype(np.float16)}
_AUDIO_CODES = {np.dtype(np.float32): AUDIO_F32, np.dtype(np.int16): AUDIO_I16, np.dtype(np.float16): AUDIO_F16}


def audio_np_dtype(audio_dtype) -> np.dtype:
    """"INT16" | "F32" | "F16" (the reference's INPUT_AUDIO_DTYPE) or a numpy dtype -> one of the three sample types; ValueError otherwise."""
    if isinstance(audio_dtype, str):
        if audio_dtype not in AUDIO_DTYPE_NAMES:
            raise ValueError(f"input audio dtype {audio_dtype!r}: expected one of {sorted(AUDIO_DTYPE_NAMES)}")
        return AUDIO_DTYPE_NAMES[audio_dtype]
    dt = np.dtype(audio_dtype)
    if dt not in _AUDIO_CODES:
        raise ValueError(f"audio dtype {dt.name}: expected float32, int16 or float16")
    return dt


def audio_dtype_name(audio_dtype) -> str:
    dt = audio_np_dtype(audio_dtype)
    return next(k for k, v in AUDIO_DTYPE_NAMES.items() if v == dt)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def sensevoice_config_c(cfg: SenseVoiceConfig) -> _lib.SenseVoiceConfigC:
    c = _lib.SenseVoiceConfigC()
    c.sample_rate, c.n_mels, c.nfft, c.win_length, c.hop_length = cfg.sample_rate, cfg.n_mels, cfg.nfft, cfg.win_length, cfg.hop_length
    c.lfr_m, c.lfr_n = cfg.lfr_m, cfg.lfr_n
    c.d_model, c.n_heads, c.d_head, c.d_ffn = cfg.d_model, cfg.n_heads, cfg.d_head, cfg.d_ffn
    c.n_blocks, c.n_main = cfg.n_blocks, cfg.n_enc0 + cfg.n_enc
    c.fsmn_kernel, c.vocab, c.blank_id = cfg.fsmn_kernel, cfg.vocab, cfg.blank_id
    c.n_prompt, c.n_languages, c.max_audio_len = cfg.n_prompt, len(cfg.language_prompt_token_ids), cfg.max_audio_len
    return c


class _Session:
    """Common session utilities (stream, profiling, taps)."""

    def __init__(self):
        self._h = C.c_void_p(None)
        self._keep = None
        self._audio_np = np.dtype(np.float32)
        self._format = None                       # (sample rate, channels) once set_input_format has been called

    @property
    def audio_dtype(self) -> np.dtype:
        """Sample type of the audio entries (asr_session_set_audio_dtype): float32 (default), int16 or float16. What a type means follows the
        family's export (include/asr_mi355x.h, asr_audio_dtype). May be set between any two calls."""
        return self._audio_np

    @audio_dtype.setter
    def audio_dtype(self, audio_dtype):
        dt = audio_np_dtype(audio_dtype)
        _lib.check(_lib.load().asr_session_set_audio_dtype(self._h, _AUDIO_CODES[dt]))
        self._audio_np = dt

    def _audio(self, a) -> np.ndarray:
        """Clips in the session's sample type. A float32 session coerces whatever it is given; a 2-byte session takes exactly its own type: nothing is
        rounded or rescaled silently."""
        if self._audio_np == np.float32:
            return _f32(a)
        got = a.dtype if isinstance(a, np.ndarray) else np.asarray(a).dtype
        if got != self._audio_np:
            raise TypeError(f"{type(self).__name__}: the session's audio_dtype is {self._audio_np.name}, the audio given is {got.name} "
                            f"(convert it explicitly, or set audio_dtype)")
        return np.ascontiguousarray(a)

    @property
    def input_format(self) -> tuple[int, int]:
        """(sample rate in Hz, interleaved channels) of the audio entries (asr_session_input_format); the default is (the model's rate, 1)."""
        rate, ch = C.c_int(0), C.c_int(0)
        _lib.check(_lib.load().asr_session_input_format(self._h, C.byref(rate), C.byref(ch)))
        return rate.value, ch.value

    def set_input_format(self, sample_rate: int, channels: int = 1):
        """Sample rate and interleaved channel count of the audio entries (asr_session_set_input_format). With anything but (the model's rate, 1) every
        `audio` / `offsets` of this session counts frames of `channels` interleaved samples at `sample_rate`, a clip is [frames, channels] (or flat
        interleaved), and the library resamples to model-rate mono on the device; frame counts and result frames refer to the resampled clip
        (`model_lengths`). May be set between any two calls; a refused format raises AsrError and leaves the one in force."""
        _lib.check(_lib.load().asr_session_set_input_format(self._h, int(sample_rate), int(channels)))
        self._format = self.input_format

    def model_lengths(self, frames) -> np.ndarray:
        """Input frames per utterance -> samples at the model's rate: ceil(n * rate_model / rate_in), the resampler's own count."""
        n = np.asarray(frames, dtype=np.int64)
        rate, _ = self._format or (0, 1)
        model = int(self.cfg.sample_rate)
        if not rate or rate == model:
            return n
        g = int(np.gcd(rate, model))
        return -((-n * (model // g)) // (rate // g))

    def _pack(self, audios):
        ch = (self._format or (0, 1))[1]
        flat = [self._audio(a).reshape(-1) for a in audios]
        if any(a.size % ch for a in flat):
            raise ValueError(f"{type(self).__name__}: a clip's sample count is not a multiple of the {ch} interleaved channels of the input format")
        offs = np.zeros(len(flat) + 1, dtype=np.int64)
        offs[1:] = np.cumsum([a.size // ch for a in flat])
        return flat, np.concatenate(flat), offs

    def close(self):
        if self._h:
            _lib.check(_lib.load().asr_session_destroy(self._h))
            self._h = C.c_void_p(None)
        self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream: int):
        _lib.check(_lib.load().asr_session_set_stream(self._h, C.c_void_p(hip_stream)))

    def profile(self, enable: bool):
        _lib.check(_lib.load().asr_session_profile_enable(self._h, int(enable)))

    def profile_reset(self):
        _lib.check(_lib.load().asr_session_profile_reset(self._h))

    def profile_read(self) -> dict:
        cap = 64
        names = C.create_string_buffer(32 * cap)
        ms = (C.c_double * cap)()
        cnt = (C.c_int64 * cap)()
        n = C.c_int(0)
        _lib.check(_lib.load().asr_session_profile_read(self._h, cap, names, ms, cnt, C.byref(n)))
        out = {}
        for i in range(n.value):
            nm = names.raw[i * 32:(i + 1) * 32].split(b"\0", 1)[0].decode()
            out[nm] = {"total_ms": ms[i], "launches": int(cnt[i])}
        return out

    def sanm_stats(self) -> dict:
        """SenseVoice / Paraformer sessions: counters of the cluster kernels (asr_sanm_stats)."""
        out = np.zeros(8, dtype=np.int32)
        _lib.check(_lib.load().asr_sanm_stats(self._h, _ip(out)))
        return {"giveups": int(out[0]), "cooldown": int(out[1]), "foreign_diverted": int(out[2]), "block_kernel": bool(out[3])}

    def taps(self, enable: bool):
        _lib.check(_lib.load().asr_session_taps_enable(self._h, int(enable)))

    def tap(self, name: str, dtype=np.float32) -> np.ndarray:
        rows, cols = C.c_int64(0), C.c_int64(0)
        _lib.check(_lib.load().asr_session_tap_shape(self._h, name.encode(), C.byref(rows), C.byref(cols)))
        out = np.empty((rows.value, cols.value), dtype=dtype)
        _lib.check(_lib.load().asr_session_tap_read(self._h, name.encode(), out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out


class SenseVoiceSession(_Session):
    """HIP replacement of `SenseVoiceSmall.onnx` (SENSE_VOICE.forward, Export_SenseVoice.py:271-296)."""

    def __init__(self, cfg: SenseVoiceConfig, arena, precision: int = PRECISION_BF16, device_id: int = 0,
                 arena_device_ptr: int | None = None, arena_bytes: int | None = None, audio_dtype=np.float32):
        super().__init__()
        self.cfg, self.precision, self.device_id = cfg, precision, device_id
        self._cfg_c = sensevoice_config_c(cfg)
        lib = _lib.load()
        if arena_device_ptr is not None:
            self._keep = arena          # whatever owns the device memory (e.g. a torch tensor)
            _lib.check(lib.asr_sensevoice_create(C.byref(self._cfg_c), C.c_void_p(arena_device_ptr), arena_bytes, MEM_DEVICE,
                                                 device_id, precision, C.byref(self._h)))
        else:
            blob = np.ascontiguousarray(arena, dtype=np.uint8)
            _lib.check(lib.asr_sensevoice_create(C.byref(self._cfg_c), blob.ctypes.data_as(C.c_void_p), blob.nbytes, MEM_HOST,
                                                 device_id, precision, C.byref(self._h)))
        self.audio_dtype = audio_dtype

    @classmethod
    def from_checkpoint(cls, cfg, ck, precision=PRECISION_BF16, device_id=0, audio_dtype=np.float32):
        return cls(cfg, build_sensevoice_arena(cfg, ck, precision), precision, device_id, audio_dtype=audio_dtype)

    def seq_len(self, n_samples: int) -> int:
        return self.cfg.seq_len(n_samples)

    def run_packed(self, audio, offsets: np.ndarray, language_idx: np.ndarray, audio_device_ptr: int | None = None):
        """audio: packed samples of the session's audio_dtype (host ndarray) or None with `audio_device_ptr` (HBM-resident, same type).
        Returns (token_ids [B, max_T] int32, num_id [B] int32)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        lang = np.ascontiguousarray(language_idx, dtype=np.int32)
        B = lang.shape[0]
        assert offsets.shape[0] == B + 1
        max_t = max(self.cfg.seq_len(int(n)) for n in self.model_lengths(np.diff(offsets))) if B else 1
        tok = np.zeros((B, max_t), dtype=np.int32)
        num = np.zeros((B,), dtype=np.int32)
        lib = _lib.load()
        if audio_device_ptr is not None:
            ap, mem = C.c_void_p(audio_device_ptr), MEM_DEVICE
        else:
            audio = self._audio(audio).reshape(-1)
            ap, mem = audio.ctypes.data_as(C.c_void_p), MEM_HOST
        _lib.check(lib.asr_sensevoice_run(self._h, ap, mem, offsets.ctypes.data_as(C.POINTER(C.c_int64)), B, _ip(lang),
                                          _ip(tok), max_t, _ip(num)))
        return tok, num

    def run(self, audios: Sequence[np.ndarray], language_idx: Sequence[int]):
        """List of 1-D utterances -> list of int32 token-id arrays (one per utterance)."""
        flat, packed, offs = self._pack(audios)
        tok, num = self.run_packed(packed, offs, np.asarray(language_idx, dtype=np.int32))
        return [tok[b, :num[b]].copy() for b in range(len(flat))]

    def run_packed_timed(self, audio, offsets: np.ndarray, language_idx: np.ndarray, audio_device_ptr: int | None = None):
        """run_packed with a frame span and a confidence per token (asr_sensevoice_run_timed). Returns (token_ids, num_id, first_frame, last_frame,
        logprob): the three new arrays are [B, max_T] like token_ids (int32, int32, float32), row b valid up to num_id[b]. Frames are rows of the
        utterance's sequence, prompt rows included (SenseVoiceConfig.row_span_seconds maps them to seconds); logprob is the mean over the token's
        frames of log soft-max at the frame's arg-max."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        lang = np.ascontiguousarray(language_idx, dtype=np.int32)
        B = lang.shape[0]
        assert offsets.shape[0] == B + 1
        max_t = max(self.cfg.seq_len(int(n)) for n in self.model_lengths(np.diff(offsets))) if B else 1
        tok = np.zeros((B, max_t), dtype=np.int32)
        first, last = np.zeros((B, max_t), dtype=np.int32), np.zeros((B, max_t), dtype=np.int32)
        logprob = np.zeros((B, max_t), dtype=np.float32)
        num = np.zeros((B,), dtype=np.int32)
        lib = _lib.load()
        if audio_device_ptr is not None:
            ap, mem = C.c_void_p(audio_device_ptr), MEM_DEVICE
        else:
            audio = self._audio(audio).reshape(-1)
            ap, mem = audio.ctypes.data_as(C.c_void_p), MEM_HOST
        _lib.check(lib.asr_sensevoice_run_timed(self._h, ap, mem, offsets.ctypes.data_as(C.POINTER(C.c_int64)), B, _ip(lang),
                                                _ip(tok), max_t, _ip(num), _ip(first), _ip(last), _fp(logprob)))
        return tok, num, first, last, logprob

    def run_timed(self, audios: Sequence[np.ndarray], language_idx: Sequence[int]):
        """List of 1-D utterances -> one record per utterance: {"ids", "first_frame", "last_frame", "logprob"}, arrays of equal length."""
        flat, packed, offs = self._pack(audios)
        tok, num, first, last, logprob = self.run_packed_timed(packed, offs, np.asarray(language_idx, dtype=np.int32))
        return [{"ids": tok[b, :num[b]].copy(), "first_frame": first[b, :num[b]].copy(), "last_frame": last[b, :num[b]].copy(),
                 "logprob": logprob[b, :num[b]].copy()} for b in range(len(flat))]

    def set_hotwords(self, phrases: Sequence[Sequence[int]], boost: float = 2.0):
        """Hotwords of run_beam (asr_sensevoice_set_hotwords): token-id lists; a hypothesis gains `boost` per token while it spells one of them, and a
        partial match gives its part back. An empty list clears them. Empty phrases, the blank id and ids outside the vocabulary raise AsrError."""
        phrases = [np.asarray(p, dtype=np.int32).reshape(-1) for p in phrases]
        offs = np.zeros(len(phrases) + 1, dtype=np.int32)
        offs[1:] = np.cumsum([p.size for p in phrases])
        ids = np.ascontiguousarray(np.concatenate(phrases) if phrases else np.zeros(0, np.int32), dtype=np.int32)
        ids = ids if ids.size else np.zeros(1, np.int32)
        _lib.check(_lib.load().asr_sensevoice_set_hotwords(self._h, _ip(ids), _ip(offs), len(phrases), float(boost)))

    def set_lm(self, lm, alpha: float = 0.5, beta: float = 0.0, oov_logprob: float | None = None):
        """The n-gram language model of run_beam (asr_sensevoice_set_lm; shallow fusion): `lm` an lm.NgramLM, or an int32 image as NgramLM.image returns it;
        None clears it. Every token a hypothesis appends adds alpha * log P(token | history) + beta to its ranking score (alpha the LM weight, beta a
        length bonus); a token the model has no unigram for costs oov_logprob (default: the model's <unk>, else 0) and leaves the history alone. A
        malformed image or a bad weight raises AsrError and the model in force stays."""
        _lib.check(_lib.load().asr_sensevoice_set_lm(self._h, *_lm_args(lm, self.cfg.vocab, oov_logprob, alpha, beta)))

    def run_packed_beam(self, audio, offsets: np.ndarray, language_idx: np.ndarray, beam: int, topk: int | None = None, nbest: int = 1,
                        audio_device_ptr: int | None = None):
        """run_packed with a CTC prefix beam search instead of the arg-max collapse (asr_sensevoice_run_beam): the `topk` (default: beam) best tokens
        of every row, `beam` live prefixes, the `nbest` best hypotheses. Returns (token_ids [B, nbest, max_T] int32, num_id [B, nbest] int32, score
        [B, nbest], ctc_score [B, nbest] float32), best first; hypotheses beyond the number found have num 0 and score -inf."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        lang = np.ascontiguousarray(language_idx, dtype=np.int32)
        B = lang.shape[0]
        assert offsets.shape[0] == B + 1
        topk = int(beam if topk is None else topk)
        max_t = max(self.cfg.seq_len(int(n)) for n in self.model_lengths(np.diff(offsets))) if B else 1
        tok = np.zeros((B, nbest, max_t), dtype=np.int32)
        num = np.zeros((B, nbest), dtype=np.int32)
        score, ctc = np.zeros((B, nbest), dtype=np.float32), np.zeros((B, nbest), dtype=np.float32)
        if audio_device_ptr is not None:
            ap, mem = C.c_void_p(audio_device_ptr), MEM_DEVICE
        else:
            audio = self._audio(audio).reshape(-1)
            ap, mem = audio.ctypes.data_as(C.c_void_p), MEM_HOST
        _lib.check(_lib.load().asr_sensevoice_run_beam(self._h, ap, mem, offsets.ctypes.data_as(C.POINTER(C.c_int64)), B, _ip(lang), int(beam), topk,
                                                       int(nbest), _ip(tok), max_t, _ip(num), _fp(score), _fp(ctc)))
        return tok, num, score, ctc

    def run_beam(self, audios: Sequence[np.ndarray], language_idx: Sequence[int], beam: int, topk: int | None = None, nbest: int = 1):
        """List of 1-D utterances -> per utterance the list of hypotheses found (at most nbest), best first: {"tokens", "score", "ctc_score"}."""
        flat, packed, offs = self._pack(audios)
        tok, num, score, ctc = self.run_packed_beam(packed, offs, np.asarray(language_idx, dtype=np.int32), beam, topk, nbest)
        return [[{"tokens": tok[b, n, :num[b, n]].copy(), "score": float(score[b, n]), "ctc_score": float(ctc[b, n])}
                 for n in range(nbest) if np.isfinite(score[b, n])] for b in range(len(flat))]

    def align_packed(self, audio, offsets: np.ndarray, language_idx: np.ndarray, target_ids: np.ndarray, target_offsets: np.ndarray,
                     audio_device_ptr: int | None = None, fill=None):
        """CTC forced alignment of given transcripts (asr_sensevoice_align): utterance b's targets are target_ids[target_offsets[b]:target_offsets[b + 1]].
        Returns (first_frame, last_frame, logprob, path_score, loglik, status): the first three ragged in the layout of target_ids (int32, int32, float32; rows
        of the utterance's sequence as run_packed_timed reports them, logprob the mean over the span of log soft-max at the target), the last three [B].
        status 1: no alignment exists; that utterance's spans keep `fill` = (int, float) (default zeros) and both scores are -inf."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        lang = np.ascontiguousarray(language_idx, dtype=np.int32)
        B = lang.shape[0]
        toff = np.ascontiguousarray(target_offsets, dtype=np.int32)
        tids = np.ascontiguousarray(target_ids, dtype=np.int32).reshape(-1)
        assert offsets.shape[0] == B + 1 and toff.shape[0] == B + 1 and tids.size == int(toff[-1])
        n = max(tids.size, 1)
        fi, ff = (0, 0.0) if fill is None else fill
        tids_c = tids if tids.size else np.zeros(1, np.int32)
        first, last = np.full(n, fi, dtype=np.int32), np.full(n, fi, dtype=np.int32)
        logprob = np.full(n, ff, dtype=np.float32)
        path, lik = np.zeros(B, dtype=np.float32), np.zeros(B, dtype=np.float32)
        status = np.zeros(B, dtype=np.int32)
        if audio_device_ptr is not None:
            ap, mem = C.c_void_p(audio_device_ptr), MEM_DEVICE
        else:
            audio = self._audio(audio).reshape(-1)
            ap, mem = audio.ctypes.data_as(C.c_void_p), MEM_HOST
        _lib.check(_lib.load().asr_sensevoice_align(self._h, ap, mem, offsets.ctypes.data_as(C.POINTER(C.c_int64)), B, _ip(lang), _ip(tids_c), _ip(toff),
                                                    _ip(first), _ip(last), _fp(logprob), _fp(path), _fp(lik), _ip(status)))
        return first[:tids.size], last[:tids.size], logprob[:tids.size], path, lik, status

    def align(self, audios: Sequence[np.ndarray], language_idx: Sequence[int], targets: Sequence[Sequence[int]]):
        """List of 1-D utterances and one token-id list each -> one record per utterance: {"first_frame", "last_frame", "logprob", "path_score", "loglik",
        "aligned"}; the three arrays have the transcript's length and are empty when `aligned` is False (no alignment exists: the scores are -inf)."""
        flat, packed, offs = self._pack(audios)
        targets = [np.asarray(t, dtype=np.int32).reshape(-1) for t in targets]
        if len(targets) != len(flat):
            raise ValueError(f"align: {len(flat)} utterances, {len(targets)} transcripts")
        toff = np.zeros(len(targets) + 1, dtype=np.int32)
        toff[1:] = np.cumsum([t.size for t in targets])
        tids = np.concatenate(targets) if targets else np.zeros(0, np.int32)
        first, last, logprob, path, lik, status = self.align_packed(packed, offs, np.asarray(language_idx, dtype=np.int32), tids, toff)
        out = []
        for b in range(len(flat)):
            ok = status[b] == 0
            sl = slice(int(toff[b]), int(toff[b + 1]) if ok else int(toff[b]))
            out.append({"first_frame": first[sl].copy(), "last_frame": last[sl].copy(), "logprob": logprob[sl].copy(), "path_score": float(path[b]),
                        "loglik": float(lik[b]), "aligned": bool(ok)})
        return out

    def utterance_rows(self, lengths: Sequence[int]):
        """(row_off, T) of each utterance inside the packed tap tensors (16-row aligned)."""
        out, r = [], 0
        for n in lengths:
            t = self.cfg.seq_len(int(n))
            out.append((r, t))
            r += (t + 15) // 16 * 16
        return out


# ------------------------------------------------------------------------------- operator hooks
def op_gemm(a, w, bias=None, act=0, precision=PRECISION_BF16):
    a, w = _f32(a), _f32(w)
    M, K = a.shape
    N = w.shape[0]
    out = np.empty((M, N), dtype=np.float32)
    b = _f32(bias) if bias is not None else None
    _lib.check(_lib.load().asr_op_gemm(precision, _fp(a), _fp(w), _fp(b), M, N, K, act, _fp(out)))
    return out


def op_gemm_ln(x, w, bias=None, gamma=None, beta=None):
    x, w = _f32(x), _f32(w)
    out = np.empty((x.shape[0], w.shape[0]), dtype=np.float32)
    b, g, be = (_f32(a) if a is not None else None for a in (bias, gamma, beta))
    _lib.check(_lib.load().asr_op_gemm_ln(_fp(x), _fp(w), _fp(b), _fp(g), _fp(be), x.shape[0], w.shape[0], x.shape[1], _fp(out)))
    return out


def op_layernorm(x, gamma=None, beta=None, eps=1e-5, precision=PRECISION_F32):
    x = _f32(x)
    rows, D = x.shape
    out = np.empty_like(x)
    g = _f32(gamma) if gamma is not None else None
    b = _f32(beta) if beta is not None else None
    _lib.check(_lib.load().asr_op_layernorm(precision, _fp(x), rows, D, _fp(g), _fp(b), eps, _fp(out)))
    return out


def op_attention(q, k, v, seq_lens, n_heads, d_head, precision=PRECISION_BF16):
    q, k, v = _f32(q), _f32(k), _f32(v)
    sl = np.ascontiguousarray(seq_lens, dtype=np.int32)
    out = np.empty_like(q)
    _lib.check(_lib.load().asr_op_attention(precision, _fp(q), _fp(k), _fp(v), _ip(sl), sl.size, n_heads, d_head, _fp(out)))
    return out


def op_fsmn(v, w, b, seq_lens, precision=PRECISION_F32):
    v, w, b = _f32(v), _f32(w), _f32(b)
    sl = np.ascontiguousarray(seq_lens, dtype=np.int32)
    out = np.empty_like(v)
    _lib.check(_lib.load().asr_op_fsmn(precision, _fp(v), _fp(w), _fp(b), _ip(sl), sl.size, v.shape[1], w.shape[1], _fp(out)))
    return out


def resample_table(sample_rate: int, model_rate: int = 16000):
    """The resampler's filter (asr_resample_table) -> (L, M, W, coeffs [L, 2 W + 1] float32): output n reads input frames floor(n M / L) - W .. + W against
    row (n M) mod L."""
    L, M, W = C.c_int(0), C.c_int(0), C.c_int(0)
    lib = _lib.load()
    _lib.check(lib.asr_resample_table(int(sample_rate), int(model_rate), C.byref(L), C.byref(M), C.byref(W), None))
    coeffs = np.empty((L.value, 2 * W.value + 1), dtype=np.float32)
    _lib.check(lib.asr_resample_table(int(sample_rate), int(model_rate), C.byref(L), C.byref(M), C.byref(W), _fp(coeffs)))
    return L.value, M.value, W.value, coeffs


def op_resample(audio, offsets, sample_rate: int, model_rate: int = 16000, channels: int = 1, int16_scale: bool = False):
    """The device resampler on host arrays (asr_op_resample, the launch of set_input_format): audio = packed frames of `channels` interleaved float32 / int16 /
    float16 samples at sample_rate, offsets [B + 1] in frames (any first offset) -> (packed model-rate mono float32, offsets [B + 1] from 0)."""
    audio = np.ascontiguousarray(audio).reshape(-1)
    code = _AUDIO_CODES[audio_np_dtype(audio.dtype)]
    offs = np.ascontiguousarray(offsets, dtype=np.int64)
    if offs.size < 2 or np.any(np.diff(offs) < 0) or offs[0] < 0 or int(offs[-1]) * int(channels) > audio.size:
        raise ValueError("op_resample: offsets must be non-decreasing frame offsets inside the audio given")
    L, M, W = C.c_int(0), C.c_int(0), C.c_int(0)
    _lib.check(_lib.load().asr_resample_table(int(sample_rate), int(model_rate), C.byref(L), C.byref(M), C.byref(W), None))      # (refuses bad rates)
    n_out = -((-np.diff(offs) * L.value) // M.value)
    out = np.empty(max(int(n_out.sum()), 1), dtype=np.float32)
    offs_out = np.zeros(offs.size, dtype=np.int64)
    lp = C.POINTER(C.c_int64)
    _lib.check(_lib.load().asr_op_resample(audio.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(lp), offs.size - 1, code, int(sample_rate), int(model_rate),
                                           int(channels), int(bool(int16_scale)), _fp(out), out.size, offs_out.ctypes.data_as(lp)))
    return out[:int(offs_out[-1])], offs_out


def op_resample_stream(audio, mode, sample_rate: int, model_rate: int = 16000, channels: int = 1, int16_scale: bool = False, chunk: int = 960):
    """The streaming input format's launches on host arrays (asr_op_resample_stream): audio [n_steps, n_streams, pitch, channels] (or [.., pitch] at one channel)
    float32 / int16 / float16 frames at sample_rate, pitch = input_format.stream_pitch(chunk, sample_rate, model_rate); mode [n_steps, n_streams]: 0 = the stream
    is not in the step, 1 = stepped, 2 = reset, then stepped; every stream starts reset. -> (out [n_steps, n_streams, chunk] float32, rows of streams not in a step
    zero; frames [n_steps, n_streams] the frames each step read, 0 where not in it; pitch)."""
    from .input_format import stream_pitch
    audio = np.ascontiguousarray(audio)
    code = _AUDIO_CODES[audio_np_dtype(audio.dtype)]
    mode = np.ascontiguousarray(mode, dtype=np.int32)
    if mode.ndim != 2 or mode.size == 0:
        raise ValueError("op_resample_stream: mode is [n_steps, n_streams]")
    L, M, W = C.c_int(0), C.c_int(0), C.c_int(0)
    _lib.check(_lib.load().asr_resample_table(int(sample_rate), int(model_rate), C.byref(L), C.byref(M), C.byref(W), None))      # (refuses bad rates)
    pitch = stream_pitch(chunk, sample_rate, model_rate)
    if audio.size != mode.size * pitch * int(channels):
        raise ValueError(f"op_resample_stream: audio holds {audio.size} samples, {mode.shape[0]} steps x {mode.shape[1]} streams x pitch {pitch} x {channels} channels "
                         f"is {mode.size * pitch * int(channels)}")
    out = np.zeros(mode.shape + (int(chunk),), dtype=np.float32)
    frames, pitch_c = np.zeros(mode.shape, dtype=np.int32), C.c_int32(0)
    _lib.check(_lib.load().asr_op_resample_stream(audio.ctypes.data_as(C.c_void_p), code, int(sample_rate), int(model_rate), int(channels), int(bool(int16_scale)),
                                                  int(chunk), mode.shape[1], mode.shape[0], _ip(mode), _fp(out), _ip(frames), C.byref(pitch_c)))
    assert pitch_c.value == pitch, (pitch_c.value, pitch)
    return out, frames, pitch


VAD_LEVEL_DB = 10.0 * np.log10(2.0) / 8.0         # one level step in dB of power: 8 steps per octave
VAD_MAX_F = 1 << 20


def vad_hop(rate: int) -> int:
    """Input frames per analysis frame: max(1, (rate + 50) // 100), about 10 ms."""
    return max(1, (int(rate) + 50) // 100)


def vad_level(energy) -> np.ndarray:
    """The detector's level of float32 frame energies: min(1023, (bits(max(e, 2^-40)) >> 20) - (bits(2^-40) >> 20))."""
    e = np.asarray(energy, dtype=np.float32)
    m = np.where(e > np.float32(2.0 ** -40), e, np.float32(2.0 ** -40)).astype(np.float32)
    return np.minimum(1023, (m.view(np.uint32) >> 20).astype(np.int64) - ((87 << 23) >> 20))


@dataclasses.dataclass
class VadParams:
    """The energy detector's parameters in seconds and dB (asr_vad_params holds them in analysis frames and level steps; `to_c` converts). The defaults are
    design choices, not measurements. max_seconds None: the caller's limit (a transcriber's window), or 30 s."""
    p_floor: float = 0.10
    margin_db: float = 9.0
    peak_drop_db: float = 6.0
    abs_dbfs: float = -60.0
    min_speech: float = 0.1
    min_pause: float = 0.5
    pad: float = 0.1
    max_seconds: float | None = None

    def to_c(self, rate: int, full_scale: float, max_frames: int | None = None) -> _lib.VadParamsC:
        H = vad_hop(rate)
        frames = lambda sec: max(0, int(round(float(sec) * rate / H)))
        c = _lib.VadParamsC()
        c.p_floor = float(self.p_floor)
        c.margin, c.peak_drop = int(round(self.margin_db / VAD_LEVEL_DB)), int(round(self.peak_drop_db / VAD_LEVEL_DB))
        amp = float(np.float32(full_scale)) * 10.0 ** (self.abs_dbfs / 20.0)
        c.abs_level = int(vad_level(np.float32(H * amp * amp)))
        c.min_speech, c.min_pause, c.pad = frames(self.min_speech), frames(self.min_pause), frames(self.pad)
        limit = int(self.max_seconds * rate) // H if self.max_seconds is not None else None
        if max_frames is not None:
            limit = max_frames if limit is None else min(limit, max_frames)
        c.max_frames = limit if limit is not None else (30 * int(rate)) // H
        return c


def vad_default_params(rate: int, full_scale: float) -> _lib.VadParamsC:
    """asr_vad_default_params: the library's own defaults for this rate and sample scale."""
    c = _lib.VadParamsC()
    _lib.check(_lib.load().asr_vad_default_params(int(rate), float(full_scale), C.byref(c)))
    return c


def op_vad(audio, offsets, rate: int = 16000, channels: int = 1, params=None, full_scale: float | None = None, audio_device_ptr: int | None = None,
           details: bool = False, seg_cap: int | None = None):
    """The energy speech / pause detector on a ragged batch (asr_op_vad): audio = packed frames of `channels` interleaved float32 / int16 / float16 samples at
    `rate` Hz, offsets [B + 1] in frames (any first offset). params: a VadParams (seconds, dB), an asr_vad_params struct, or None = the library's defaults.
    full_scale: 32768 for int16-range samples, 1 for unit-range ones (default: 32768 for int16 audio, else 1). audio_device_ptr: the same packed frames in
    device memory, read there instead of `audio` (which then only gives the sample type and size).
    -> (segments [S, 2] int64 input-frame offsets in the coordinates of `offsets`, seg_utt [S] int32, counts [B] int32); with details also
    (energy [sum F] float32, level [sum F] int32, stats [B, 3] int32 = floor, peak, thr). seg_cap: write at most that many segments (counts stay full)."""
    audio = np.ascontiguousarray(audio).reshape(-1)
    code = _AUDIO_CODES[audio_np_dtype(audio.dtype)]
    offs = np.ascontiguousarray(offsets, dtype=np.int64)
    if offs.size < 2 or np.any(np.diff(offs) < 0) or offs[0] < 0 or int(offs[-1]) * max(int(channels), 1) > audio.size:
        raise ValueError("op_vad: offsets must be non-decreasing frame offsets inside the audio given")
    if full_scale is None:
        full_scale = 32768.0 if audio.dtype == np.int16 else 1.0
    if params is None:
        pc = vad_default_params(rate, full_scale)
    elif isinstance(params, VadParams):
        pc = params.to_c(rate, full_scale)
    else:
        pc = params
    H = vad_hop(rate) if rate >= 1 else 1
    F = -((-np.diff(offs)) // H)
    total_f = int(F.sum())
    cap = total_f if seg_cap is None else int(seg_cap)
    seg = np.zeros((max(cap, 1), 2), dtype=np.int64)
    utt = np.zeros(max(cap, 1), dtype=np.int32)
    counts = np.zeros(offs.size - 1, dtype=np.int32)
    energy = np.zeros(max(total_f, 1), dtype=np.float32) if details else None
    level = np.zeros(max(total_f, 1), dtype=np.int32) if details else None
    stats = np.zeros((offs.size - 1, 3), dtype=np.int32) if details else None
    lp = C.POINTER(C.c_int64)
    ptr = C.c_void_p(int(audio_device_ptr)) if audio_device_ptr is not None else audio.ctypes.data_as(C.c_void_p)
    _lib.check(_lib.load().asr_op_vad(ptr, MEM_DEVICE if audio_device_ptr is not None else MEM_HOST, offs.ctypes.data_as(lp), offs.size - 1, code, int(rate),
                                      int(channels), C.byref(pc), seg.ctypes.data_as(lp), cap, _ip(utt), _ip(counts), _fp(energy),
                                      _ip(level) if details else None, _ip(stats) if details else None))
    n = min(int(counts.sum()), cap)
    res = (seg[:n].copy(), utt[:n].copy(), counts)
    return res + (energy[:total_f], level[:total_f], stats) if details else res


def op_ctc_collapse(frame_ids, seq_lens, blank_id=0):
    ids = np.ascontiguousarray(frame_ids, dtype=np.int32)
    sl = np.ascontiguousarray(seq_lens, dtype=np.int32)
    max_t = int(sl.max())
    tok = np.zeros((sl.size, max_t), dtype=np.int32)
    num = np.zeros((sl.size,), dtype=np.int32)
    _lib.check(_lib.load().asr_op_ctc_collapse(_ip(ids), _ip(sl), sl.size, blank_id, _ip(tok), max_t, _ip(num)))
    return [tok[b, :num[b]].copy() for b in range(sl.size)]


def op_ctc_collapse_timed(frame_ids, frame_logprob, seq_lens, blank_id=0, max_tokens=None, fill=None):
    """The collapse with spans on host arrays (asr_op_ctc_collapse_timed). Returns (token_ids, first_frame, last_frame, token_logprob, num_id): the four
    arrays are [B, max_tokens] (default: the longest sequence) and start out holding `fill` = (int, float) (default zeros), which slots the kernel does
    not write keep; num_id holds the full token count."""
    ids = np.ascontiguousarray(frame_ids, dtype=np.int32)
    lp = _f32(frame_logprob)
    sl = np.ascontiguousarray(seq_lens, dtype=np.int32)
    assert ids.size == lp.size == int(sl.sum())
    max_t = int(sl.max()) if max_tokens is None else int(max_tokens)
    fi, ff = (0, 0.0) if fill is None else fill
    tok, first, last = (np.full((sl.size, max_t), fi, dtype=np.int32) for _ in range(3))
    tlp = np.full((sl.size, max_t), ff, dtype=np.float32)
    num = np.zeros((sl.size,), dtype=np.int32)
    _lib.check(_lib.load().asr_op_ctc_collapse_timed(_ip(ids), _fp(lp), _ip(sl), sl.size, blank_id, _ip(tok), _ip(first), _ip(last), _fp(tlp), max_t,
                                                     _ip(num)))
    return tok, first, last, tlp, num


def hotword_trie(phrases):
    """Token-id lists -> the trie arrays of op_ctc_prefix_beam (depth, is_end, child_off, child_tok, child_node; node 0 the root, nodes numbered breadth
    first, children sorted by token)."""
    kids, depth, is_end = [{}], [0], [0]
    for ph in phrases:
        ph = [int(t) for t in ph]
        if not ph:
            raise ValueError("empty hotword phrase")
        n = 0
        for t in ph:
            if t not in kids[n]:
                kids[n][t] = len(kids)
                kids.append({})
                depth.append(depth[n] + 1)
                is_end.append(0)
            n = kids[n][t]
        is_end[n] = 1
    order, remap = [0], {0: 0}
    for n in order:
        for t in sorted(kids[n]):
            remap[kids[n][t]] = len(order)
            order.append(kids[n][t])
    off, tok, node = [0], [], []
    for n in order:
        for t in sorted(kids[n]):
            tok.append(t)
            node.append(remap[kids[n][t]])
        off.append(len(tok))
    i32 = lambda a: np.asarray(a, dtype=np.int32)
    return {"depth": i32([depth[n] for n in order]), "is_end": i32([is_end[n] for n in order]), "child_off": i32(off), "child_tok": i32(tok),
            "child_node": i32(node)}


def _lm_image(lm, vocab, oov_logprob):
    """(int32 image, oov_logprob) of an lm.NgramLM or a ready image"""
    if hasattr(lm, "image"):
        if vocab is None:
            raise ValueError("an lm.NgramLM needs the vocabulary size (vocab=) to become an image")
        img, default = lm.image(vocab), lm.default_oov_logprob
    else:
        img, default = lm, 0.0
    img = np.ascontiguousarray(img, dtype=np.int32).reshape(-1)
    img = img if img.size else np.zeros(1, np.int32)
    return img, float(default if oov_logprob is None else oov_logprob)


def _trie_args(trie):
    """the five trie arrays and the node count as the host-array searches take them (`trie` as hotword_trie returns it; None or a lone root: no hotwords)"""
    if trie is None or trie["depth"].size <= 1:
        return [None] * 5 + [0]
    t = [np.ascontiguousarray(trie[k], dtype=np.int32) for k in ("depth", "is_end", "child_off", "child_tok", "child_node")]
    return [_ip(a) for a in t] + [int(t[0].size)]


def _lm_args(lm, vocab, oov_logprob, alpha, beta):
    """(image, words, alpha, beta, oov_logprob) as the entry points take a language model (`lm` as _lm_image takes it; None: no model)"""
    if lm is None:
        return [None, 0, 0.0, 0.0, 0.0]
    img, oov = _lm_image(lm, vocab, oov_logprob)
    return [_ip(img), img.size, float(alpha), float(beta), oov]


def op_ctc_prefix_beam(cand_id, cand_logprob, seq_lens, beam, nbest=1, blank_id=0, trie=None, boost=0.0, max_tokens=None, lm=None, alpha=0.5, beta=0.0,
                       oov_logprob=None, vocab=None):
    """The CTC prefix beam search on host arrays (asr_op_ctc_prefix_beam): cand_id / cand_logprob [sum T, topk], `trie` as hotword_trie returns it (None:
    no hotwords). Returns (token_ids [B, nbest, max_tokens], num_id [B, nbest], score [B, nbest], ctc_score [B, nbest]), best first. With `lm` (an
    lm.NgramLM, built for `vocab` ids, or an int32 image) the search runs with that language model (asr_op_ctc_prefix_beam_lm; alpha, beta and oov_logprob
    as SenseVoiceSession.set_lm takes them) and score includes its term."""
    ids = np.ascontiguousarray(cand_id, dtype=np.int32)
    lp = _f32(cand_logprob)
    sl = np.ascontiguousarray(seq_lens, dtype=np.int32)
    assert ids.ndim == 2 and ids.shape == lp.shape and ids.shape[0] == int(sl.sum())
    max_t = int(sl.max()) if max_tokens is None else int(max_tokens)
    tok = np.zeros((sl.size, nbest, max_t), dtype=np.int32)
    num = np.zeros((sl.size, nbest), dtype=np.int32)
    score, ctc = np.zeros((sl.size, nbest), dtype=np.float32), np.zeros((sl.size, nbest), dtype=np.float32)
    targs = _trie_args(trie)
    if lm is not None:
        _lib.check(_lib.load().asr_op_ctc_prefix_beam_lm(_ip(ids), _fp(lp), ids.shape[1], _ip(sl), sl.size, blank_id, *targs, float(boost), int(beam),
                                                         int(nbest), _ip(tok), max_t, _ip(num), _fp(score), _fp(ctc),
                                                         *_lm_args(lm, vocab, oov_logprob, alpha, beta)))
        return tok, num, score, ctc
    _lib.check(_lib.load().asr_op_ctc_prefix_beam(_ip(ids), _fp(lp), ids.shape[1], _ip(sl), sl.size, blank_id, *targs, float(boost), int(beam),
                                                  int(nbest), _ip(tok), max_t, _ip(num), _fp(score), _fp(ctc)))
    return tok, num, score, ctc


def op_nar_beam(cand_id, cand_logprob, seq_lens, beam, nbest=1, trie=None, boost=0.0, max_tokens=None, lm=None, alpha=0.5, beta=0.0, oov_logprob=None,
                vocab=None):
    """The beam search over the token rows of a non-autoregressive decoder on host arrays (asr_op_nar_beam): cand_id / cand_logprob [sum N, topk], seq_lens the
    token counts (0 is legal), `trie` as hotword_trie returns it, `lm` an lm.NgramLM (built for `vocab` ids) or an int32 image, or None. Returns (token_ids
    [B, nbest, max_tokens], num_id [B, nbest], score [B, nbest], am_score [B, nbest], token_logprob [B, nbest, max_tokens]), best first; every hypothesis of a
    sequence has its N tokens, hypotheses beyond the number found have num 0 and both scores -inf."""
    ids = np.ascontiguousarray(cand_id, dtype=np.int32)
    lp = _f32(cand_logprob)
    sl = np.ascontiguousarray(seq_lens, dtype=np.int32)
    assert ids.ndim == 2 and ids.shape == lp.shape and ids.shape[0] == int(sl.sum())
    max_t = max(int(sl.max()), 1) if max_tokens is None else int(max_tokens)
    tok = np.zeros((sl.size, nbest, max_t), dtype=np.int32)
    tlp = np.zeros((sl.size, nbest, max_t), dtype=np.float32)
    num = np.zeros((sl.size, nbest), dtype=np.int32)
    score, am = np.zeros((sl.size, nbest), dtype=np.float32), np.zeros((sl.size, nbest), dtype=np.float32)
    targs = _trie_args(trie)
    largs = _lm_args(lm, vocab, oov_logprob, alpha, beta)
    ids_c, lp_c = (ids, lp) if ids.size else (np.zeros((1, ids.shape[1]), np.int32), np.zeros((1, ids.shape[1]), np.float32))
    _lib.check(_lib.load().asr_op_nar_beam(_ip(ids_c), _fp(lp_c), ids.shape[1], _ip(sl), sl.size, *targs, float(boost), *largs, int(beam), int(nbest),
                                           _ip(tok), max_t, _ip(num), _fp(score), _fp(am), _fp(tlp)))
    return tok, num, score, am, tlp


def nar_stream_beam_state_words(beam, pend_cap):
    """int32 words of one stream's search state (asr_nar_stream_beam_state_words)"""
    n = _lib.load().asr_nar_stream_beam_state_words(int(beam), int(pend_cap))
    if n < 0:
        raise ValueError(f"beam {beam} (1..16), pend_cap {pend_cap} (1..64)")
    return n


def op_nar_stream_beam(steps, n_streams, beam, nbest=1, pend_cap=16, trie=None, boost=0.0, lm=None, alpha=0.5, beta=0.0, oov_logprob=None, vocab=None,
                       state=None, fill=None):
    """The streaming beam search with carried state and fixed-lag commits on host arrays (asr_op_nar_stream_beam; the build's own mode). `steps`: one list per
    step of (stream id, cand_id [n, topk], cand_logprob [n, topk], final) -- any subset of the streams in any order, n = 0 is legal, `final` ends the stream
    behind its rows. One launch per step over state kept between them; `state` (int32 [n_streams, nar_stream_beam_state_words], None: all cleared) is the
    streams' state before the call and is updated in place; a stream whose first word is 0 is cleared. Returns one dict per step with, per slot of the step:
    commit_ids / commit_logprob [n, cap], commit_num [n], pend_ids / pend_logprob [n, nbest, pend_cap], pend_num / pend_score / pend_am [n, nbest], total [n];
    array slots the search does not write hold `fill` = (int, float) (default zeros)."""
    slots = [sl for st in steps for sl in st]
    assert steps and all(len(st) > 0 for st in steps)
    ids_l = [np.ascontiguousarray(sl[1], dtype=np.int32) for sl in slots]
    lp_l = [_f32(sl[2]) for sl in slots]
    topk = ids_l[0].shape[1]
    assert all(i.ndim == 2 and i.shape[1] == topk and i.shape == l.shape for i, l in zip(ids_l, lp_l))
    ids = np.ascontiguousarray(np.concatenate(ids_l + [np.zeros((1, topk), np.int32)]))
    lp = np.ascontiguousarray(np.concatenate(lp_l + [np.zeros((1, topk), np.float32)]))
    off = np.zeros(len(steps) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(st) for st in steps])
    sid = np.ascontiguousarray([sl[0] for sl in slots], dtype=np.int32)
    rows = np.ascontiguousarray([i.shape[0] for i in ids_l], dtype=np.int32)
    fin = np.ascontiguousarray([1 if sl[3] else 0 for sl in slots], dtype=np.int32)
    n, cap = len(slots), int(pend_cap) + max(int(rows.max()), 0)
    fi, ff = (0, 0.0) if fill is None else fill
    commit_ids, commit_lp = np.full((n, cap), fi, dtype=np.int32), np.full((n, cap), ff, dtype=np.float32)
    pend_ids, pend_lp = np.full((n, nbest, pend_cap), fi, dtype=np.int32), np.full((n, nbest, pend_cap), ff, dtype=np.float32)
    commit_num, total = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    pend_num = np.zeros((n, nbest), dtype=np.int32)
    pend_score, pend_am = np.zeros((n, nbest), dtype=np.float32), np.zeros((n, nbest), dtype=np.float32)
    targs = _trie_args(trie)
    largs = _lm_args(lm, vocab, oov_logprob, alpha, beta)
    if state is not None:
        assert state.dtype == np.int32 and state.flags["C_CONTIGUOUS"] and state.ndim == 2 and state.shape[0] == n_streams
        sargs = [_ip(state), state.shape[1]]
    else:
        sargs = [None, 0]
    _lib.check(_lib.load().asr_op_nar_stream_beam(_ip(ids), _fp(lp), topk, int(n_streams), len(steps), _ip(off), _ip(sid), _ip(rows), _ip(fin), *targs,
                                                  float(boost), *largs, int(beam), int(nbest), int(pend_cap), *sargs, _ip(commit_ids), _fp(commit_lp), cap,
                                                  _ip(commit_num), _ip(pend_ids), _fp(pend_lp), _ip(pend_num), _fp(pend_score), _fp(pend_am), _ip(total)))
    out = []
    for s in range(len(steps)):
        a, b = int(off[s]), int(off[s + 1])
        out.append({"commit_ids": commit_ids[a:b], "commit_logprob": commit_lp[a:b], "commit_num": commit_num[a:b], "pend_ids": pend_ids[a:b],
                    "pend_logprob": pend_lp[a:b], "pend_num": pend_num[a:b], "pend_score": pend_score[a:b], "pend_am": pend_am[a:b], "total": total[a:b]})
    return out


def op_ctc_align(em, seq_lens, targets, row0=0, max_tokens=None, fill=None):
    """The forced-alignment trellis on host arrays (asr_op_ctc_align): em [sum T, ld] log-probabilities (slot 0 the blank, slot j target j - 1 of the row's
    sequence), `targets` one id list per sequence; each sequence is aligned against its rows row0 .. T - 1. Returns (first_frame, last_frame, token_logprob
    [B, max_tokens], path_score, loglik, status [B]); the three arrays start out holding `fill` = (int, float) (default zeros), which slots the kernel does
    not write keep."""
    em = _f32(em)
    sl = np.ascontiguousarray(seq_lens, dtype=np.int32)
    assert em.ndim == 2 and em.shape[0] == int(sl.sum()) and len(targets) == sl.size
    targets = [np.asarray(t, dtype=np.int32).reshape(-1) for t in targets]
    toff = np.zeros(sl.size + 1, dtype=np.int32)
    toff[1:] = np.cumsum([t.size for t in targets])
    tids = np.ascontiguousarray(np.concatenate(targets + [np.zeros(1, np.int32)]), dtype=np.int32)
    max_t = max(1, max(t.size for t in targets)) if max_tokens is None else int(max_tokens)
    fi, ff = (0, 0.0) if fill is None else fill
    first, last = np.full((sl.size, max_t), fi, dtype=np.int32), np.full((sl.size, max_t), fi, dtype=np.int32)
    tlp = np.full((sl.size, max_t), ff, dtype=np.float32)
    path, lik = np.zeros(sl.size, dtype=np.float32), np.zeros(sl.size, dtype=np.float32)
    status = np.zeros(sl.size, dtype=np.int32)
    _lib.check(_lib.load().asr_op_ctc_align(_fp(em), em.shape[1], _ip(sl), sl.size, int(row0), _ip(tids), _ip(toff), _ip(first), _ip(last), _fp(tlp), max_t,
                                            _fp(path), _fp(lik), _ip(status)))
    return first, last, tlp, path, lik, status


def op_cif_scan_timed(alpha, enc, seq_lens, tail_threshold, max_tokens=None, fill=0):
    """The CIF scan with fire rows on host arrays (asr_op_cif_scan_timed). alpha [sum T], enc [sum T, d]. Returns (acoustic [sum T, d], fire_frame
    [B, max_tokens] int32, num_id [B]): fire_frame starts out holding `fill`, which slots the kernel does not write keep; num_id holds the full count."""
    al, en = _f32(alpha).reshape(-1), _f32(enc)
    sl = np.ascontiguousarray(seq_lens, dtype=np.int32)
    assert al.size == en.shape[0] == int(sl.sum())
    max_t = int(sl.max()) + 1 if max_tokens is None else int(max_tokens)
    ac = np.zeros_like(en)
    fire = np.full((sl.size, max_t), fill, dtype=np.int32)
    num = np.zeros((sl.size,), dtype=np.int32)
    _lib.check(_lib.load().asr_op_cif_scan_timed(_fp(al), _fp(en), en.shape[1], _ip(sl), sl.size, float(tail_threshold), _fp(ac), _ip(fire), max_t,
                                                 _ip(num)))
    return ac, fire, num


def op_gemm_bench(M, N, K, variant=-1, epilogue=0, iters=50) -> float:
    """Tuning hook (probe library, not the product ABI): average milliseconds per launch of the bf16 GEMM."""
    from . import _probe
    return _probe.gemm_bench(M, N, K, variant, epilogue, iters)


def op_gemm_set_variant(variant: int = -1) -> None:
    """Pin the bf16 GEMM kernel variant for the following op_gemm calls (-1 = heuristic); probe-library hook."""
    from . import _probe
    _probe.gemm_set_variant(variant)


# =============================================================================== Whisper
def whisper_config_c(cfg, gelu_tanh: bool = False) -> _lib.WhisperConfigC:
    c = _lib.WhisperConfigC()
    c.sample_rate, c.n_mels, c.nfft, c.hop_length = cfg.sample_rate, cfg.n_mels, cfg.nfft, cfg.hop_length
    c.d_model, c.n_heads, c.d_head, c.d_ffn = cfg.d_model, cfg.n_heads, cfg.d_head, cfg.d_ffn
    c.n_enc_layers, c.n_dec_layers, c.vocab = cfg.n_enc_layers, cfg.n_dec_layers, cfg.vocab
    c.max_source_positions, c.max_target_positions, c.max_audio_len = cfg.max_source_positions, cfg.max_target_positions, cfg.max_audio_len
    c.gelu_tanh = int(gelu_tanh)
    return c


def _token_head(prefix: str, default_range: int, penalty_doc: str):
    """The four decode-head methods of a decoder family, over its asr_<prefix>_* entries (csrc/decode_head.h holds the one head behind them)."""

    def entry(name):
        return getattr(_lib.load(), f"asr_{prefix}_{name}")

    class TokenHeadMixin:
        def set_penalty(self, repeat_penalty: float = 1.0, penalty_range: int = default_range):
            _lib.check(entry("set_penalty")(self._h, C.c_float(repeat_penalty), int(penalty_range)))

        def track_history(self, enable: bool):
            """Append every pick to the device-side id history whatever the penalty value is (what the penalty-greedy graphs do, also at 1.0)."""
            _lib.check(entry("track_history")(self._h, int(enable)))

        def set_sampling(self, enable: bool, temperature: float = 0.8, top_k: int = 10, top_p: float = 0.95,
                         repetition_penalty: float = 1.0, seed: int = 0):
            """TOPK_TOPP_SAMPLING head (USE_SAMPLING in the reference host); enable=False restores arg-max / penalty-greedy."""
            _lib.check(entry("set_sampling")(self._h, int(enable), C.c_float(temperature), int(top_k), C.c_float(top_p),
                                             C.c_float(repetition_penalty), C.c_uint64(seed)))

        def set_sampling_noise(self, uniforms):
            """Parity hook: uniforms [batch, top_k] for the next prefill / decode step (otherwise the device generator is used)."""
            u = _f32(uniforms).reshape(-1)
            _lib.check(entry("set_sampling_noise")(self._h, _fp(u), u.size))

        def set_token_scores(self, enable: bool):
            """Token scores (asr_<family>_set_token_scores): every pick of the arg-max, penalty-greedy and sampling heads is scored by the natural-log
            soft-max of the logits row the selection sees (temperature, top-k and top-p apart). Switch it before the prefill; off, no step changes."""
            _lib.check(entry("set_token_scores")(self._h, int(enable)))

        def token_scores(self) -> np.ndarray:
            """float32 [batch][count]: the log-probabilities of the picks since the last prefill, oldest first (column 0 is the prefill's pick; after
            generate() the stop pick and what finished sequences picked while others went on are included). Drains the stream."""
            cap = self._score_capacity()
            out = np.full((max(self.batch, 1), cap), np.nan, dtype=np.float32)
            n = np.zeros(1, dtype=np.int32)
            _lib.check(entry("token_scores")(self._h, _fp(out), cap, _ip(n)))
            return out[:self.batch, :int(n[0])].copy()

        def set_hotwords(self, phrases: Sequence[Sequence[int]], boost: float = 2.0):
            """Hotword boosting of the decoder (asr_<family>_set_hotwords): token-id lists. Every sequence -- every hypothesis of beam_search -- carries a
            node of the phrases' context graph that follows its own picks from the root after a prefill: a token that continues a phrase gains `boost`, a
            token that breaks a partial match of depth d gives d * boost back. The selection heads see it as a sparse logit bias (a token score is the
            log-soft-max of the biased row), beam_search as log-probability + bonus change. An empty list switches the mode off. Set it before the prefill.
            Empty phrases, ids outside the vocabulary and a boost that is not finite raise AsrError and leave the list in force alone."""
            ids, offs = _flatten_phrases(phrases)
            _lib.check(entry("set_hotwords")(self._h, _ip(ids), _ip(offs), len(offs) - 1, C.c_float(boost)))

        def set_lm(self, lm, alpha: float = 0.5, beta: float = 0.0, oov_logprob: float | None = None, topk: int = 16, end_ids: Sequence[int] = ()):
            """n-gram LM shallow fusion in the decoder's selection (asr_<family>_set_lm): `lm` an lm.NgramLM, or an int32 image as NgramLM.image returns
            it; None clears it. Every sequence -- every hypothesis of beam_search -- carries a state of the model that follows its own picks from the start
            state after a prefill. Of the `topk` (1..32) best columns of the row the selection sees, the greedy heads pick the one with the largest logit +
            alpha * log P(token | history) + beta; beam_search ranks by log-probability + hotword bonus change + that term (its scores include it; topk
            must reach the beam width). A token without a unigram costs oov_logprob (default: the model's <unk>, else 0) and leaves the history alone; one
            of `end_ids` (at most 8: the family's end-of-text ids) costs alpha * log P(</s> | history). Tokens outside the topk columns are not considered.
            The sampling head ignores the model. A malformed image or a bad argument raises AsrError and leaves the model in force."""
            if lm is None:
                _lib.check(entry("set_lm")(self._h, None, 0, 0.0, 0.0, 0.0, 0, None, 0))
                return
            img, oov = _lm_image(lm, self.cfg.vocab, oov_logprob)
            end_ids = [int(e) for e in end_ids]
            ends = np.ascontiguousarray(end_ids or [0], dtype=np.int32)
            _lib.check(entry("set_lm")(self._h, _ip(img), img.size, float(alpha), float(beta), oov, int(topk), _ip(ends), len(end_ids)))

    TokenHeadMixin.set_penalty.__doc__ = penalty_doc
    return TokenHeadMixin


def _flatten_phrases(phrases):
    """Token-id lists -> (ids int32 [sum, at least 1], offsets int32 [n + 1]): the shape of the asr_*_set_hotwords entries."""
    phrases = [np.asarray(p, dtype=np.int32).reshape(-1) for p in phrases]
    offs = np.zeros(len(phrases) + 1, dtype=np.int32)
    offs[1:] = np.cumsum([p.size for p in phrases])
    ids = np.ascontiguousarray(np.concatenate(phrases) if phrases else np.zeros(0, np.int32), dtype=np.int32)
    return (ids if ids.size else np.zeros(1, np.int32)), offs


def hotword_id_variants(phrases, encode):
    """Hotwords as the decoders' set_hotwords takes them: a text phrase becomes the distinct tokenisations of `phrase` and " " + phrase (byte-level BPE spells
    a word differently at the start of the text and inside it; `encode`: text -> id list, without special tokens); id lists pass through unchanged. Order is
    kept; duplicate and empty tokenisations of a text are dropped."""
    out, seen = [], set()
    for ph in phrases or []:
        if isinstance(ph, str):
            if encode is None:
                raise ValueError("hotwords given as text need a tokenizer (tokenizer_path); pass token-id lists instead")
            text = ph.strip()
            variants = [list(map(int, encode(text))), list(map(int, encode(" " + text)))] if text else []
        else:
            out.append([int(t) for t in ph])
            continue
        for v in variants:
            if v and tuple(v) not in seen:
                seen.add(tuple(v))
                out.append(v)
    return out


class WhisperSession(_token_head("whisper", 20, "Decode head: 1.0 = plain arg-max; else penalty-greedy (APPLY_PENALTY + GREEDY_SEARCH, the reference host's default)."),
                     _Session):
    """HIP replacement of the merged Whisper graphs (encoder + KV-cache decoder + greedy heads)."""

    def __init__(self, cfg, arena, precision: int = PRECISION_BF16, device_id: int = 0, gelu_tanh: bool = False,
                 arena_device_ptr: int | None = None, arena_bytes: int | None = None, audio_dtype=np.float32):
        super().__init__()
        self.cfg, self.precision, self.device_id = cfg, precision, device_id
        self._cfg_c = whisper_config_c(cfg, gelu_tanh)
        lib = _lib.load()
        if arena_device_ptr is not None:
            self._keep = arena
            _lib.check(lib.asr_whisper_create(C.byref(self._cfg_c), C.c_void_p(arena_device_ptr), arena_bytes, MEM_DEVICE,
                                              device_id, precision, C.byref(self._h)))
        else:
            blob = np.ascontiguousarray(arena, dtype=np.uint8)
            _lib.check(lib.asr_whisper_create(C.byref(self._cfg_c), blob.ctypes.data_as(C.c_void_p), blob.nbytes, MEM_HOST,
                                              device_id, precision, C.byref(self._h)))
        self.batch = 0
        self.audio_dtype = audio_dtype

    @classmethod
    def from_checkpoint(cls, cfg, ck, precision=PRECISION_BF16, device_id=0, suppress_tokens=None, begin_suppress_tokens=(),
                        gelu_tanh=False, audio_dtype=np.float32):
        from .arena import build_whisper_arena
        arena_precision = PRECISION_BF16 if precision in (PRECISION_FP8W, PRECISION_FP8MM, PRECISION_MXFP4W) else precision
        return cls(cfg, build_whisper_arena(cfg, ck, arena_precision, suppress_tokens, begin_suppress_tokens), precision, device_id, gelu_tanh,
                   audio_dtype=audio_dtype)

    def encode_packed(self, audio, offsets, audio_device_ptr: int | None = None) -> np.ndarray:
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        B = offsets.size - 1
        npos = np.zeros(B, dtype=np.int32)
        if audio_device_ptr is not None:
            ap, mem = C.c_void_p(audio_device_ptr), MEM_DEVICE
        else:
            audio = self._audio(audio).reshape(-1)
            ap, mem = audio.ctypes.data_as(C.c_void_p), MEM_HOST
        _lib.check(_lib.load().asr_whisper_encode(self._h, ap, mem, offsets.ctypes.data_as(C.POINTER(C.c_int64)), B, _ip(npos)))
        self.batch = B
        if self.precision == PRECISION_FP8MM:                     # a GELU operand that met the e4m3 clamp: loud, not silent (the scale is static)
            n, shift = self.fp8_stats()
            if n > getattr(self, "_fp8_saturated", 0):
                warnings.warn(f"Whisper FP8MM: {n - getattr(self, '_fp8_saturated', 0)} activation elements saturated at 448 * 2^{shift} in this encode; "
                              f"raise the shift (set_fp8_act_shift / ASR_FP8MM_ACT_SHIFT)", RuntimeWarning, stacklevel=2)
            self._fp8_saturated = n
        return npos

    def fp8_stats(self) -> tuple[int, int]:
        """(activation elements that met the e4m3 clamp since creation, activation shift in use) -- asr_whisper_fp8_stats; zeros outside FP8MM."""
        st = (C.c_uint64 * 2)()
        _lib.check(_lib.load().asr_whisper_fp8_stats(self._h, st))
        return int(st[0]), int(st[1])

    def set_fp8_act_shift(self, shift: int):
        """FP8MM: store fc2's GELU operand as value * 2^-shift (asr_whisper_set_fp8_act_shift)."""
        _lib.check(_lib.load().asr_whisper_set_fp8_act_shift(self._h, int(shift)))

    def encode(self, audios: Sequence[np.ndarray]) -> np.ndarray:
        _, packed, offs = self._pack(audios)
        return self.encode_packed(packed, offs)

    def prefill(self, ids, want_logits: bool = True):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        assert ids.ndim == 2
        if self.batch and ids.shape[0] != self.batch:
            raise ValueError(f"prompt batch {ids.shape[0]} != encoded batch {self.batch}")
        nxt = np.zeros(ids.shape[0], dtype=np.int32)
        logits = np.empty((ids.shape[0], self.cfg.vocab), dtype=np.float32) if want_logits else None
        _lib.check(_lib.load().asr_whisper_prefill(self._h, _ip(ids), ids.shape[1], _ip(nxt), _fp(logits)))
        return nxt, logits

    def prefill_prompts(self, prompts, want_logits: bool = True):
        """Prefill with one prompt (an array of ids, 1 .. max_target_positions of them) per sequence -- asr_whisper_prefill_prompts. Ragged or long prompts
        are left-padded to the longest one on the device; decode / generate / beam_search / token scores / align then work as after prefill(), with the
        longest prompt as the prompt length (it bounds the whole batch: longest + new positions <= max_target_positions)."""
        prompts = [np.ascontiguousarray(p, dtype=np.int32).reshape(-1) for p in prompts]
        if not self.batch or len(prompts) != self.batch:
            raise ValueError(f"{len(prompts)} prompts != encoded batch {self.batch}")
        offs = np.zeros(len(prompts) + 1, dtype=np.int32)
        offs[1:] = np.cumsum([p.size for p in prompts])
        ids = np.ascontiguousarray(np.concatenate(prompts + [np.zeros(1, dtype=np.int32)]))      # (never empty: a prompt of 0 ids is the library's error)
        nxt = np.zeros(self.batch, dtype=np.int32)
        logits = np.empty((self.batch, self.cfg.vocab), dtype=np.float32) if want_logits else None
        _lib.check(_lib.load().asr_whisper_prefill_prompts(self._h, _ip(ids), _ip(offs), _ip(nxt), _fp(logits)))
        return nxt, logits

    def decode(self, ids=None, want_logits: bool = False, sync: bool = True):
        nxt = np.zeros(self.batch, dtype=np.int32) if sync else None
        logits = np.empty((self.batch, self.cfg.vocab), dtype=np.float32) if want_logits else None
        idp = _ip(np.ascontiguousarray(ids, dtype=np.int32)) if ids is not None else None
        _lib.check(_lib.load().asr_whisper_decode(self._h, idp, _ip(nxt) if nxt is not None else None, _fp(logits)))
        return nxt, logits

    def _score_capacity(self) -> int:
        return int(self.cfg.max_target_positions)

    def generate(self, max_new: int, eos_id: int):
        tok = np.zeros((self.batch, max_new), dtype=np.int32)
        n = np.zeros(self.batch, dtype=np.int32)
        _lib.check(_lib.load().asr_whisper_generate(self._h, max_new, eos_id, _ip(tok), _ip(n)))
        return [tok[b, :n[b]].copy() for b in range(self.batch)]

    def beam_search(self, beam: int, max_new: int, eos_id: int):
        """Width-`beam` search after a prefill -> per utterance a best-first list of (token ids, summed log-probability). Leaves the session's
        greedy state as the prefill left it (generate() afterwards continues the same prefill)."""
        tok = np.zeros((self.batch, beam, max_new), dtype=np.int32)
        n = np.zeros((self.batch, beam), dtype=np.int32)
        score = np.zeros((self.batch, beam), dtype=np.float32)
        _lib.check(_lib.load().asr_whisper_beam_search(self._h, int(beam), int(max_new), int(eos_id), _ip(tok), _ip(n), _fp(score)))
        return [[(tok[b, r, :n[b, r]].copy(), float(score[b, r])) for r in range(beam)] for b in range(self.batch)]

    def set_timestamps(self, enable: bool, max_initial_index: int | None = 50):
        """Timestamp mode (asr_whisper_set_timestamps; the build's own, the reference always decodes behind <|notimestamps|>): OpenAI Whisper's timestamp
        rules run on the device before every selection, the prompt carries no <|notimestamps|>. The ids come from the config; timestamps start right after
        <|notimestamps|>. max_initial_index: the latest first timestamp, in 0.02 s steps (None: no limit). Switch it off for the [SOT] probe."""
        cfg = self.cfg
        _lib.check(_lib.load().asr_whisper_set_timestamps(self._h, int(enable), cfg.no_timestamps_id + 1, cfg.no_timestamps_id, cfg.eot_id,
                                                          -1 if max_initial_index is None else int(max_initial_index)))

    def default_alignment_heads(self):
        """OpenAI's documented fallback when a checkpoint names no alignment heads: every head of the upper half of the decoder layers."""
        cfg = self.cfg
        return [(l, h) for l in range(cfg.n_dec_layers // 2, cfg.n_dec_layers) for h in range(cfg.n_heads)]

    def set_word_timestamps(self, enable: bool, alignment_heads=None, max_rows: int | None = None):
        """Token / word timestamps (asr_whisper_set_word_timestamps; the build's own mode): while on, the last position of a prefill and every single-token
        decode step capture the raw cross-attention scores of `alignment_heads` [(layer, head)] (None: default_alignment_heads()) for up to max_rows
        positions (None: max_target_positions); align() turns them into frames. Device memory: batch x pairs x max_rows x ld x 4 bytes -- with the fallback
        list of a large checkpoint that is 32 times the ten heads such a checkpoint ships, so pass its own list. Beam search is refused while it is on."""
        if not enable:
            _lib.check(_lib.load().asr_whisper_set_word_timestamps(self._h, 0, None, 0, 0))
            return
        heads = self.default_alignment_heads() if alignment_heads is None else alignment_heads
        pairs = np.ascontiguousarray(np.asarray(heads, dtype=np.int32).reshape(-1, 2))
        rows = self.cfg.max_target_positions if max_rows is None else int(max_rows)
        _lib.check(_lib.load().asr_whisper_set_word_timestamps(self._h, 1, _ip(pairs), pairs.shape[0], rows))

    def align(self, n_rows, n_frames=None, medfilt_width: int = 7):
        """asr_whisper_align over the rows captured since the last prefill: per utterance an int32 array of n_rows[b] encoder frames (0.02 s each), the first
        frame of every row on the DTW path. n_rows[b] = text tokens + 1 (0 skips the utterance); n_frames[b]: the encoder positions that hold audio
        (None: the whole encoder length)."""
        nr = np.ascontiguousarray(n_rows, dtype=np.int32).reshape(-1)
        if n_frames is None:
            n_frames = [self.align_read_shape(0, b)[2] for b in range(self.batch)]
        nf = np.ascontiguousarray(n_frames, dtype=np.int32).reshape(-1)
        if nr.size != self.batch or nf.size != self.batch:
            raise ValueError(f"align: {nr.size} n_rows / {nf.size} n_frames for a batch of {self.batch}")
        stride = max(1, int(nr.max()))
        out = np.zeros((self.batch, stride), dtype=np.int32)
        _lib.check(_lib.load().asr_whisper_align(self._h, _ip(nr), _ip(nf), int(medfilt_width), _ip(out), stride))
        return [out[b, :nr[b]].copy() for b in range(self.batch)]

    def align_read_shape(self, what: int, b: int):
        shape = np.zeros(3, dtype=np.int32)
        _lib.check(_lib.load().asr_whisper_align_read(self._h, int(what), int(b), None, 0, _ip(shape)))
        return tuple(int(v) for v in shape)

    def align_read(self, what: int, b: int) -> np.ndarray:
        """Tests / debugging: what = 0 the captured scores of utterance b, f32 [pairs][rows captured][encoder length] (read them before align(): its soft-max
        runs in place); what = 1 the cost matrix of the last align, f32 [n_rows][n_frames]."""
        shape = self.align_read_shape(what, b)
        out = np.zeros(shape, dtype=np.float32)
        _lib.check(_lib.load().asr_whisper_align_read(self._h, int(what), int(b), out.ctypes.data_as(C.c_void_p), out.nbytes, None))
        return out if what == 0 else out[0]

    def no_speech_prob(self, no_speech_id: int | None = None) -> np.ndarray:
        """NO_SPEECH_DETECTION on the device-resident logits of the last prefill (the probe): (B,) probabilities."""
        out = np.zeros(self.batch, dtype=np.float32)
        _lib.check(_lib.load().asr_whisper_no_speech_prob(self._h, int(self.cfg.no_speech_id if no_speech_id is None else no_speech_id), _fp(out)))
        return out

    def cross_kv(self, lengths_pos: Sequence[int]):
        """Debug: (K, V) per utterance as (L, H, T, 64) arrays from the 'cross' tap (f32 mode)."""
        cfg = self.cfg
        raw = self.tap("cross", dtype=np.float32 if self.precision == PRECISION_F32 else np.uint16)
        G = 2 * cfg.n_dec_layers * cfg.n_heads
        mpad = raw.shape[0] // G
        slabs = raw.reshape(2, cfg.n_dec_layers, cfg.n_heads, mpad, 64)
        out, r = [], 0
        for t in lengths_pos:
            out.append((slabs[0, :, :, r:r + t], slabs[1, :, :, r:r + t]))
            r += (t + 15) // 16 * 16
        return out


# =============================================================================== Paraformer
class ParaformerSession(_Session):
    """HIP replacement of `Paraformer.onnx` (PARAFORMER.forward, Export_Paraformer.py:474-563)."""

    def __init__(self, cfg, arena, precision: int = PRECISION_BF16, device_id: int = 0, arena_device_ptr: int | None = None,
                 arena_bytes: int | None = None, audio_dtype=np.float32):
        super().__init__()
        self.cfg, self.precision, self.device_id = cfg, precision, device_id
        c = _lib.ParaformerConfigC()
        for f in ("sample_rate", "n_mels", "nfft", "win_length", "hop_length", "lfr_m", "lfr_n", "d_model", "n_heads", "d_head", "d_ffn",
                  "fsmn_kernel", "n_dec", "n_dec3", "d_dec_ffn", "cif_kernel", "vocab", "max_audio_len"):
            setattr(c, f, getattr(cfg, f))
        c.n_blocks = cfg.n_enc0 + cfg.n_enc
        c.tail_threshold = cfg.tail_threshold
        self._cfg_c = c
        lib = _lib.load()
        if arena_device_ptr is not None:
            self._keep = arena
            _lib.check(lib.asr_paraformer_create(C.byref(c), C.c_void_p(arena_device_ptr), arena_bytes, MEM_DEVICE, device_id, precision,
                                                 C.byref(self._h)))
        else:
            blob = np.ascontiguousarray(arena, dtype=np.uint8)
            _lib.check(lib.asr_paraformer_create(C.byref(c), blob.ctypes.data_as(C.c_void_p), blob.nbytes, MEM_HOST, device_id, precision,
                                                 C.byref(self._h)))
        self.audio_dtype = audio_dtype

    @classmethod
    def from_checkpoint(cls, cfg, ck, precision=PRECISION_BF16, device_id=0, audio_dtype=np.float32):
        from .arena import build_paraformer_arena
        return cls(cfg, build_paraformer_arena(cfg, ck, precision), precision, device_id, audio_dtype=audio_dtype)

    def run_packed(self, audio, offsets, audio_device_ptr: int | None = None):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        B = offsets.size - 1
        max_t = max(self.cfg.seq_len(int(n)) for n in self.model_lengths(np.diff(offsets))) if B else 1
        tok = np.zeros((B, max_t), dtype=np.int32)
        num = np.zeros((B,), dtype=np.int32)
        if audio_device_ptr is not None:
            ap, mem = C.c_void_p(audio_device_ptr), MEM_DEVICE
        else:
            audio = self._audio(audio).reshape(-1)
            ap, mem = audio.ctypes.data_as(C.c_void_p), MEM_HOST
        _lib.check(_lib.load().asr_paraformer_run(self._h, ap, mem, offsets.ctypes.data_as(C.POINTER(C.c_int64)), B, _ip(tok), max_t, _ip(num)))
        return tok, num

    def run(self, audios: Sequence[np.ndarray]):
        flat, packed, offs = self._pack(audios)
        tok, num = self.run_packed(packed, offs)
        return [tok[b, :num[b]].copy() for b in range(len(flat))]

    def run_packed_timed(self, audio, offsets, audio_device_ptr: int | None = None):
        """run_packed with the CIF fire row and the log-probability of every token (asr_paraformer_run_timed). Returns (token_ids, num_id, fire_frame,
        logprob): the two new arrays are [B, max_T] like token_ids (int32, float32), row b valid up to num_id[b]. fire_frame is the utterance's LFR row
        at which the token fired, in [0, T]; T means the tail threshold fired it behind the last row (paraformer.token_times maps rows to seconds)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        B = offsets.size - 1
        max_t = max(self.cfg.seq_len(int(n)) for n in self.model_lengths(np.diff(offsets))) if B else 1
        tok = np.zeros((B, max_t), dtype=np.int32)
        fire = np.zeros((B, max_t), dtype=np.int32)
        logprob = np.zeros((B, max_t), dtype=np.float32)
        num = np.zeros((B,), dtype=np.int32)
        if audio_device_ptr is not None:
            ap, mem = C.c_void_p(audio_device_ptr), MEM_DEVICE
        else:
            audio = self._audio(audio).reshape(-1)
            ap, mem = audio.ctypes.data_as(C.c_void_p), MEM_HOST
        _lib.check(_lib.load().asr_paraformer_run_timed(self._h, ap, mem, offsets.ctypes.data_as(C.POINTER(C.c_int64)), B, _ip(tok), max_t, _ip(num),
                                                        _ip(fire), _fp(logprob)))
        return tok, num, fire, logprob

    def run_timed(self, audios: Sequence[np.ndarray]):
        """List of 1-D utterances -> one record per utterance: {"ids", "fire_frame", "logprob"}, arrays of equal length."""
        flat, packed, offs = self._pack(audios)
        tok, num, fire, logprob = self.run_packed_timed(packed, offs)
        return [{"ids": tok[b, :num[b]].copy(), "fire_frame": fire[b, :num[b]].copy(), "logprob": logprob[b, :num[b]].copy()}
                for b in range(len(flat))]

    def set_hotwords(self, phrases: Sequence[Sequence[int]], boost: float = 2.0):
        """Hotwords of run_beam (asr_paraformer_set_hotwords): token-id lists; a hypothesis gains `boost` per token while it spells one of them, and a partial
        match gives its part back. An empty list clears them. Empty phrases and ids outside the vocabulary raise AsrError (this family has no blank id)."""
        ids, offs = _flatten_phrases(phrases)
        _lib.check(_lib.load().asr_paraformer_set_hotwords(self._h, _ip(ids), _ip(offs), len(phrases), float(boost)))

    def set_lm(self, lm, alpha: float = 0.5, beta: float = 0.0, oov_logprob: float | None = None):
        """The n-gram language model of run_beam (asr_paraformer_set_lm; shallow fusion), arguments as SenseVoiceSession.set_lm takes them: every token of a
        hypothesis adds alpha * log P(token | history) + beta to its ranking score. None clears it; a malformed image or a bad weight raises AsrError and the
        model in force stays."""
        _lib.check(_lib.load().asr_paraformer_set_lm(self._h, *_lm_args(lm, self.cfg.vocab, oov_logprob, alpha, beta)))

    def run_packed_beam(self, audio, offsets, beam: int, topk: int | None = None, nbest: int = 1, audio_device_ptr: int | None = None):
        """run_packed with a beam search over the decoder's token rows instead of the per-row arg-max (asr_paraformer_run_beam): the `topk` (default: beam)
        best tokens of every row, `beam` live hypotheses, the `nbest` best of them. Returns (token_ids [B, nbest, max_T] int32, num_id [B, nbest] int32, score
        [B, nbest], am_score [B, nbest] float32, fire_frame [B, max_T] int32, logprob [B, nbest, max_T] float32), best first. Every hypothesis of utterance b
        has its CIF fire count as length and shares row b of fire_frame; hypotheses beyond the number found have num 0 and score -inf."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        B = offsets.size - 1
        topk = int(beam if topk is None else topk)
        max_t = max(self.cfg.seq_len(int(n)) for n in self.model_lengths(np.diff(offsets))) if B else 1
        tok = np.zeros((B, nbest, max_t), dtype=np.int32)
        logprob = np.zeros((B, nbest, max_t), dtype=np.float32)
        fire = np.zeros((B, max_t), dtype=np.int32)
        num = np.zeros((B, nbest), dtype=np.int32)
        score, am = np.zeros((B, nbest), dtype=np.float32), np.zeros((B, nbest), dtype=np.float32)
        if audio_device_ptr is not None:
            ap, mem = C.c_void_p(audio_device_ptr), MEM_DEVICE
        else:
            audio = self._audio(audio).reshape(-1)
            ap, mem = audio.ctypes.data_as(C.c_void_p), MEM_HOST
        _lib.check(_lib.load().asr_paraformer_run_beam(self._h, ap, mem, offsets.ctypes.data_as(C.POINTER(C.c_int64)), B, int(beam), topk, int(nbest), _ip(tok), max_t,
                                                       _ip(num), _fp(score), _fp(am), _ip(fire), _fp(logprob)))
        return tok, num, score, am, fire, logprob

    def run_beam(self, audios: Sequence[np.ndarray], beam: int, topk: int | None = None, nbest: int = 1):
        """List of 1-D utterances -> per utterance (hyps, fire_frame): hyps the hypotheses found (at most nbest), best first, each {"tokens", "score",
        "am_score", "logprob"}; fire_frame the utterance's CIF fire rows, one per token, shared by all of its hypotheses."""
        flat, packed, offs = self._pack(audios)
        tok, num, score, am, fire, logprob = self.run_packed_beam(packed, offs, beam, topk, nbest)
        out = []
        for b in range(len(flat)):
            hyps = [{"tokens": tok[b, n, :num[b, n]].copy(), "score": float(score[b, n]), "am_score": float(am[b, n]), "logprob": logprob[b, n, :num[b, n]].copy()}
                    for n in range(nbest) if np.isfinite(score[b, n])]
            out.append((hyps, fire[b, :num[b, 0]].copy()))
        return out

    def utterance_rows(self, lengths: Sequence[int]):
        out, r = [], 0
        for n in lengths:
            t = self.cfg.seq_len(int(n))
            out.append((r, t))
            r += (t + 15) // 16 * 16
        return out

    @staticmethod
    def token_rows(num_tokens: Sequence[int]):
        """First row of each utterance's tokens in the decoder-side taps ('logits'): the fired frames are packed, 16-row aligned
        per utterance (a zero-token utterance keeps one dummy row)."""
        out, r = [], 0
        for n in num_tokens:
            out.append(r)
            r += (max(int(n), 1) + 15) // 16 * 16
        return out


def stream_absolute_rows(fire_step, chunk_index: int, rows_new: int, rows_carried: int) -> np.ndarray:
    """Integration step t of a stream's chunk_index-th chunk since its reset -> the stream's absolute LFR row chunk_index * B + t - C (B new and C
    carried rows per step: a step integrates the C carried rows, then the first B - C new ones; t = -1 is the previous chunk's last integrated row).
    Rows in front of the stream's first one (the zero rows carried into chunk 0) clip to 0."""
    rows = int(chunk_index) * int(rows_new) + np.asarray(fire_step, dtype=np.int64) - int(rows_carried)
    return np.maximum(rows, 0)


class ParaformerStreamSession(_Session):
    """Streaming Paraformer: per-stream recurrent state (encoder K/V histories, carried LFR rows, CIF state, decoder FSMN / cross
    K/V histories) lives in the session; `step` advances a set of streams by one chunk (Export_Paraformer_Streaming.py:386-553)."""

    def __init__(self, cfg, ck_or_arena, precision: int = PRECISION_BF16, device_id: int = 0, chunk: int = 8000, look_back_encoder: int = 4,
                 look_back_decoder: int = 1, max_streams: int = 8, max_continue: int = 502, audio_dtype=np.float32):
        super().__init__()
        import dataclasses
        from .arena import build_paraformer_arena
        n_pos = max_continue - 1                                          # rows of the position table (positions 1 .. max_continue - 1)
        cfg = dataclasses.replace(cfg, max_audio_len=cfg.win_length + cfg.hop_length * (n_pos * cfg.lfr_n - 1))
        assert cfg.seq_len(cfg.max_audio_len) == n_pos
        self.cfg, self.precision, self.chunk, self.max_streams = cfg, precision, int(chunk), int(max_streams)
        n_frames = (chunk - cfg.win_length) // cfg.hop_length + 1
        self.rows_per_chunk = ((cfg.lfr_m - 1) // 2 + n_frames) // cfg.lfr_n + 1
        self.rows_carried = self.rows_per_chunk // 2                      # rows carried into the next step (the session's st_C)
        self.chunks_done = np.zeros(int(max_streams), dtype=np.int64)     # timed steps: chunks of each stream since its reset
        blob = build_paraformer_arena(cfg, ck_or_arena, precision, streaming=True) if isinstance(ck_or_arena, dict) else ck_or_arena
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        c = _lib.ParaformerConfigC()
        for f in ("sample_rate", "n_mels", "nfft", "win_length", "hop_length", "lfr_m", "lfr_n", "d_model", "n_heads", "d_head", "d_ffn",
                  "fsmn_kernel", "n_dec", "n_dec3", "d_dec_ffn", "cif_kernel", "vocab", "max_audio_len"):
            setattr(c, f, getattr(cfg, f))
        c.n_blocks = cfg.n_enc0 + cfg.n_enc
        c.tail_threshold = cfg.tail_threshold
        _lib.check(_lib.load().asr_paraformer_stream_create(C.byref(c), blob.ctypes.data_as(C.c_void_p), blob.nbytes, MEM_HOST, device_id, precision,
                                                            int(chunk), look_back_encoder, look_back_decoder, int(max_streams), C.byref(self._h)))
        self.audio_dtype = audio_dtype

    def reset(self, stream_id: int = -1):
        _lib.check(_lib.load().asr_paraformer_stream_reset(self._h, int(stream_id)))
        if stream_id < 0:
            self.chunks_done[:] = 0
        else:
            self.chunks_done[int(stream_id)] = 0
        for s in (range(self.max_streams) if stream_id < 0 else [int(stream_id)]):      # (the stream's beam search, if the mode is on, was cleared with it)
            if getattr(self, "_beam", None):
                self._fire_rows[s] = []

    def input_frames(self, stream_ids):
        """(frames, pitch) of the listed streams' next step (asr_paraformer_stream_input_frames): frames[i] = the input frames the step reads from row i of its
        audio, pitch = the row pitch in frames. The default format gives (chunk, chunk). With a format set, step c of a stream reads
        input_format.stream_frames(chunk, rate, model_rate, c) frames: W more at its first step than later (the filter's look-ahead)."""
        sid = np.ascontiguousarray(stream_ids, dtype=np.int32)
        frames, pitch = np.zeros(sid.size, dtype=np.int32), C.c_int32(0)
        _lib.check(_lib.load().asr_paraformer_stream_input_frames(self._h, _ip(sid), sid.size, _ip(frames), C.byref(pitch)))
        return frames, int(pitch.value)

    def _step_rows(self, chunks, sid):
        """The host rows of a step: (n, chunk) at the default format, else (n, pitch * channels) from (n, pitch, channels) or (n, pitch) arrays."""
        rate, ch = self._format or (int(self.cfg.sample_rate), 1)
        if (rate, ch) == (int(self.cfg.sample_rate), 1):
            return self._audio(chunks).reshape(sid.size, self.chunk)
        _, pitch = self.input_frames(sid)
        return self._audio(chunks).reshape(sid.size, pitch * ch)

    def step(self, chunks, stream_ids, audio_device_ptr: int | None = None):
        """chunks: (n, chunk) int16-range samples of the session's audio_dtype (or None with `audio_device_ptr`: HBM-resident [n][chunk]); stream_ids: n
        distinct ids -> list of n int32 arrays (tokens fired by this chunk). With an input format set (set_input_format) chunks is (n, pitch, channels) -- or
        (n, pitch) -- frames at the format's rate, row i filled with the input_frames(stream_ids)[0][i] frames stream i's step reads (the rest of a row is
        ignored), and the library resamples each stream on the device with its own carried frames; step_timed and step_beam take the same rows."""
        sid = np.ascontiguousarray(stream_ids, dtype=np.int32)
        if audio_device_ptr is not None:
            ap, mem = C.c_void_p(audio_device_ptr), MEM_DEVICE
        else:
            a = self._step_rows(chunks, sid)
            ap, mem = a.ctypes.data_as(C.c_void_p), MEM_HOST
        cap = self.rows_per_chunk + 1
        tok = np.zeros((sid.size, cap), dtype=np.int32)
        num = np.zeros(sid.size, dtype=np.int32)
        _lib.check(_lib.load().asr_paraformer_stream_step(self._h, ap, mem, _ip(sid), sid.size, _ip(tok), cap, _ip(num)))
        self.chunks_done[sid] += 1
        return [tok[i, :num[i]].copy() for i in range(sid.size)]

    def absolute_rows(self, fire_step, chunk_index: int) -> np.ndarray:
        return stream_absolute_rows(fire_step, chunk_index, self.rows_per_chunk, self.rows_carried)

    def step_timed(self, chunks, stream_ids, audio_device_ptr: int | None = None):
        """`step` with the fire step and the log-probability of every token (asr_paraformer_stream_step_timed) -> one record per stream:
        {"ids", "fire_step", "row", "logprob"}; "row" is the stream's absolute LFR row of the fire (absolute_rows: the session counts each stream's chunks
        since its reset, over `step` and `step_timed` alike)."""
        sid = np.ascontiguousarray(stream_ids, dtype=np.int32)
        if audio_device_ptr is not None:
            ap, mem = C.c_void_p(audio_device_ptr), MEM_DEVICE
        else:
            a = self._step_rows(chunks, sid)
            ap, mem = a.ctypes.data_as(C.c_void_p), MEM_HOST
        cap = self.rows_per_chunk + 1
        tok = np.zeros((sid.size, cap), dtype=np.int32)
        fire = np.zeros((sid.size, cap), dtype=np.int32)
        logprob = np.zeros((sid.size, cap), dtype=np.float32)
        num = np.zeros(sid.size, dtype=np.int32)
        _lib.check(_lib.load().asr_paraformer_stream_step_timed(self._h, ap, mem, _ip(sid), sid.size, _ip(tok), cap, _ip(num), _ip(fire), _fp(logprob)))
        rows = np.maximum(self.chunks_done[sid][:, None] * self.rows_per_chunk + fire - self.rows_carried, 0)      # stream_absolute_rows, every stream at once
        self.chunks_done[sid] += 1
        return [{"ids": tok[i, :n].copy(), "fire_step": fire[i, :n].copy(), "row": rows[i, :n].copy(), "logprob": logprob[i, :n].copy()}
                for i, n in enumerate(num)]

    # ---- beam search with hotwords and a language model, fixed-lag commits (the build's own mode)
    def set_beam(self, beam: int, topk: int | None = None, nbest: int = 1, pend_cap: int = 16):
        """Switches the streaming beam search on (asr_paraformer_stream_set_beam): `beam` live hypotheses (1..16) over the `topk` (default min(beam, 8); 1..8)
        best tokens of every token row, the `nbest` best reported, at most `pend_cap` (1..64) uncommitted tokens per stream. beam = 0 switches it off. Fails
        while a stream holds search history (tokens since its last finish_beam or reset), as set_hotwords and set_lm do."""
        beam = int(beam)
        topk = min(beam, 8) if topk is None else int(topk)
        _lib.check(_lib.load().asr_paraformer_stream_set_beam(self._h, beam, topk if beam else 0, int(nbest) if beam else 0, int(pend_cap) if beam else 0))
        self._beam = (beam, topk, int(nbest), int(pend_cap)) if beam else None
        self._fire_rows = [[] for _ in range(self.max_streams)]           # absolute fire rows of each stream's tokens that are searched but not yet committed

    def set_hotwords(self, phrases: Sequence[Sequence[int]], boost: float = 2.0):
        """Hotwords of step_beam (asr_paraformer_stream_set_hotwords), as ParaformerSession.set_hotwords takes them. An empty list clears them."""
        ids, offs = _flatten_phrases(phrases)
        _lib.check(_lib.load().asr_paraformer_stream_set_hotwords(self._h, _ip(ids), _ip(offs), len(phrases), float(boost)))

    def set_lm(self, lm, alpha: float = 0.5, beta: float = 0.0, oov_logprob: float | None = None):
        """The n-gram language model of step_beam (asr_paraformer_stream_set_lm), as ParaformerSession.set_lm takes it. None clears it."""
        _lib.check(_lib.load().asr_paraformer_stream_set_lm(self._h, *_lm_args(lm, self.cfg.vocab, oov_logprob, alpha, beta)))

    def _beam_arrays(self, n, max_tokens):
        _, _, nbest, cap = self._beam
        return (np.zeros((n, cap + max_tokens), np.int32), np.zeros((n, cap + max_tokens), np.float32), np.zeros(n, np.int32), np.zeros((n, nbest, cap), np.int32),
                np.zeros((n, nbest, cap), np.float32), np.zeros((n, nbest), np.int32), np.zeros((n, nbest), np.float32), np.zeros((n, nbest), np.float32),
                np.zeros(n, np.int32))

    def _beam_records(self, sid, arrays):
        cid, clp, cnum, pid, plp, pnum, pscore, pam, total = arrays
        out = []
        for i, s in enumerate(sid):
            k = int(cnum[i])
            rows, self._fire_rows[s] = self._fire_rows[s][:k], self._fire_rows[s][k:]
            pending = [{"ids": pid[i, m, :pnum[i, m]].copy(), "logprob": plp[i, m, :pnum[i, m]].copy(), "score": float(pscore[i, m]), "am_score": float(pam[i, m])}
                       for m in range(pid.shape[1]) if np.isfinite(pscore[i, m])]
            out.append({"committed": {"ids": cid[i, :k].copy(), "logprob": clp[i, :k].copy(), "row": np.asarray(rows, dtype=np.int64)}, "pending": pending,
                        "total": int(total[i])})
        return out

    def step_beam(self, chunks, stream_ids, audio_device_ptr: int | None = None):
        """`step_timed` followed by the streaming beam search over the step's token rows (asr_paraformer_stream_step_beam) -> one record per stream: "ids",
        "fire_step", "row", "logprob" as step_timed gives them (the greedy picks), plus "committed" = {"ids", "logprob", "row"}: the tokens this step
        committed, final from now on, with the absolute LFR rows their token rows fired at; "pending" = the uncommitted tails of the best nbest live
        hypotheses, best first, each {"ids", "logprob", "score", "am_score"} (scores since the stream's search was cleared, without the end terms); "total" =
        token rows searched since the clear. What a caller shows: everything committed so far, then pending[0]."""
        assert getattr(self, "_beam", None), "set_beam first"
        sid = np.ascontiguousarray(stream_ids, dtype=np.int32)
        if audio_device_ptr is not None:
            ap, mem = C.c_void_p(audio_device_ptr), MEM_DEVICE
        else:
            a = self._step_rows(chunks, sid)
            ap, mem = a.ctypes.data_as(C.c_void_p), MEM_HOST
        cap = self.rows_per_chunk + 1
        tok = np.zeros((sid.size, cap), dtype=np.int32)
        fire = np.zeros((sid.size, cap), dtype=np.int32)
        logprob = np.zeros((sid.size, cap), dtype=np.float32)
        num = np.zeros(sid.size, dtype=np.int32)
        arrays = self._beam_arrays(sid.size, cap)
        cid, clp, cnum, pid, plp, pnum, pscore, pam, total = arrays
        _lib.check(_lib.load().asr_paraformer_stream_step_beam(self._h, ap, mem, _ip(sid), sid.size, _ip(tok), cap, _ip(num), _ip(fire), _fp(logprob), _ip(cid), _fp(clp),
                                                               _ip(cnum), _ip(pid), _fp(plp), _ip(pnum), _fp(pscore), _fp(pam), _ip(total)))
        rows = np.maximum(self.chunks_done[sid][:, None] * self.rows_per_chunk + fire - self.rows_carried, 0)
        self.chunks_done[sid] += 1
        for i, s in enumerate(sid):
            self._fire_rows[s] += [int(r) for r in rows[i, :num[i]]]
        out = self._beam_records(sid, arrays)
        for i, n in enumerate(num):
            out[i].update({"ids": tok[i, :n].copy(), "fire_step": fire[i, :n].copy(), "row": rows[i, :n].copy(), "logprob": logprob[i, :n].copy()})
        return out

    def finish_beam(self, stream_ids):
        """The end of the named streams' searches (asr_paraformer_stream_finish_beam; no audio): the end terms, the final ranking, the best hypothesis' tail
        committed, the search state cleared -> one record per stream: "committed" (the tail of the best hypothesis), "pending" (the nbest tails with their final
        scores; pending[0] is what was committed), "total". The acoustic state is left alone: `reset` the stream before it takes another utterance."""
        assert getattr(self, "_beam", None), "set_beam first"
        sid = np.ascontiguousarray(stream_ids, dtype=np.int32)
        arrays = self._beam_arrays(sid.size, 0)
        cid, clp, cnum, pid, plp, pnum, pscore, pam, total = arrays
        _lib.check(_lib.load().asr_paraformer_stream_finish_beam(self._h, _ip(sid), sid.size, _ip(cid), _fp(clp), _ip(cnum), _ip(pid), _fp(plp), _ip(pnum), _fp(pscore),
                                                                 _fp(pam), _ip(total)))
        return self._beam_records(sid, arrays)

    def stream_stats(self) -> dict:
        """Which path the chunk steps took (asr_paraformer_stream_stats): give-ups recovered, steps moved to the per-launch path because the GPU was shared,
        snapshots taken, the stream count above which steps stay on the per-launch path, cool-down steps left, whether the session fuses at all."""
        out = np.zeros(8, dtype=np.int32)
        _lib.check(_lib.load().asr_paraformer_stream_stats(self._h, _ip(out)))
        return {"giveups": int(out[0]), "shared_steps": int(out[1]), "snapshots": int(out[2]), "fused_max": int(out[3]), "cooldown": int(out[4]),
                "can_fuse": bool(out[5])}


# =============================================================================== Qwen3-ASR
class QwenAsrSession(_token_head("qwen", 10, "Decode head: 1.0 = plain arg-max; else penalty-greedy (the reference host's default is 0.8 over the last 10 ids)."),
                     _Session):
    """HIP replacement of the merged Qwen3-ASR graphs (audio encoder + prompt assembly + Qwen3 decoder prefill / decode + arg-max;
    Qwen_ASR/Inference_Qwen_ASR_ONNX.py:424-760 drives them)."""

    def __init__(self, cfg, arena, precision: int = PRECISION_BF16, device_id: int = 0, arena_device_ptr: int | None = None,
                 arena_bytes: int | None = None, audio_dtype=np.float32):
        super().__init__()
        self.cfg, self.precision, self.device_id = cfg, precision, device_id
        c = _lib.QwenConfigC()
        for f in ("sample_rate", "n_mels", "nfft", "hop_length", "enc_d", "enc_heads", "enc_ffn", "n_enc_layers", "conv_channels", "n_window",
                  "n_window_infer", "max_source_positions", "d_model", "n_heads", "n_kv_heads", "d_head", "d_ffn", "n_layers", "vocab",
                  "max_seq_len", "max_audio_len", "rms_eps", "rope_theta"):
            setattr(c, f, getattr(cfg, f))
        c.classify_num = int(getattr(cfg, "classify_num", 0))
        self._cfg_c = c
        if arena_device_ptr is not None:
            self._keep = arena
            _lib.check(_lib.load().asr_qwen_create(C.byref(c), C.c_void_p(arena_device_ptr), arena_bytes, MEM_DEVICE, device_id, precision,
                                                   C.byref(self._h)))
        else:
            blob = np.ascontiguousarray(arena, dtype=np.uint8)
            _lib.check(_lib.load().asr_qwen_create(C.byref(c), blob.ctypes.data_as(C.c_void_p), blob.nbytes, MEM_HOST, device_id, precision,
                                                   C.byref(self._h)))
        self.batch = 0
        self.audio_dtype = audio_dtype

    @classmethod
    def from_checkpoint(cls, cfg, ck, precision=PRECISION_BF16, device_id=0, audio_dtype=np.float32):
        from .arena import build_qwen_asr_arena
        arena_precision = PRECISION_BF16 if precision in (PRECISION_FP8W, PRECISION_MXFP4W) else precision
        return cls(cfg, build_qwen_asr_arena(cfg, ck, arena_precision), precision, device_id, audio_dtype=audio_dtype)

    @staticmethod
    def _ragged(seqs, B):
        seqs = [np.asarray(x, dtype=np.int32).reshape(-1) for x in seqs]
        if len(seqs) == 1 and B > 1:
            seqs = seqs * B
        if len(seqs) != B:
            raise ValueError(f"{len(seqs)} prompts for a batch of {B}")
        offs = np.zeros(B + 1, dtype=np.int32)
        offs[1:] = np.cumsum([x.size for x in seqs])
        flat = np.concatenate(seqs) if offs[-1] else np.zeros(1, dtype=np.int32)
        return np.ascontiguousarray(flat, dtype=np.int32), offs

    def prefill_packed(self, audio, offsets, pre_ids, post_ids, want_logits: bool = True, audio_device_ptr: int | None = None):
        """pre_ids / post_ids: one id list per utterance (or one shared list): the prompt is [pre | audio embeddings | post].
        -> (next_ids (B,), logits (B, vocab) | None, ids_len (B,))"""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        B = offsets.size - 1
        pre, pre_off = self._ragged(pre_ids, B)
        post, post_off = self._ragged(post_ids, B)
        nxt = np.zeros(B, dtype=np.int32)
        ids_len = np.zeros(B, dtype=np.int32)
        logits = np.empty((B, self.cfg.vocab), dtype=np.float32) if want_logits else None
        if audio_device_ptr is not None:
            ap, mem = C.c_void_p(audio_device_ptr), MEM_DEVICE
        else:
            audio = self._audio(audio).reshape(-1)
            ap, mem = audio.ctypes.data_as(C.c_void_p), MEM_HOST
        _lib.check(_lib.load().asr_qwen_prefill(self._h, ap, mem, offsets.ctypes.data_as(C.POINTER(C.c_int64)), B, _ip(pre), _ip(pre_off),
                                                _ip(post), _ip(post_off), _ip(nxt), _fp(logits), _ip(ids_len)))
        self.batch = B
        return nxt, logits, ids_len

    def prefill(self, audios: Sequence[np.ndarray], pre_ids, post_ids, want_logits: bool = True):
        _, packed, offs = self._pack(audios)
        return self.prefill_packed(packed, offs, pre_ids, post_ids, want_logits)

    def decode(self, ids=None, want_logits: bool = False, sync: bool = True):
        nxt = np.zeros(self.batch, dtype=np.int32) if sync else None
        logits = np.empty((self.batch, self.cfg.vocab), dtype=np.float32) if want_logits else None
        idp = _ip(np.ascontiguousarray(ids, dtype=np.int32)) if ids is not None else None
        _lib.check(_lib.load().asr_qwen_decode(self._h, idp, _ip(nxt) if nxt is not None else None, _fp(logits)))
        return nxt, logits

    def audio_tokens(self, n_samples: int) -> int:
        """_get_feat_extract_output_lengths (Export_Qwen_ASR.py:519-527) of a clip's mel frames."""
        n = int(n_samples) // self.cfg.hop_length
        f = n % self.cfg.chunk
        for _ in range(3):
            f = (max(f - 1, 0) // 2 + 1) if f > 0 else 0
        return f + (n // self.cfg.chunk) * 13

    def audio_hidden(self, n_samples: Sequence[int]):
        """Debug: per-utterance audio embeddings (tokens, d_model) from the 'audio_hidden' tap (rows live in window slots)."""
        cfg = self.cfg
        raw = self.tap("audio_hidden", dtype=np.float32)
        cpw = cfg.chunks_per_window
        rpw = (cpw * 13 + 15) // 16 * 16
        out, win = [], 0
        for n in n_samples:
            frames = int(n) // cfg.hop_length
            n_win = ((frames + cfg.chunk - 1) // cfg.chunk + cpw - 1) // cpw
            rows = raw[win * rpw:(win + n_win) * rpw].reshape(n_win, rpw, -1)[:, :cpw * 13].reshape(n_win * cpw * 13, -1)
            out.append(rows[:self.audio_tokens(n)].copy())
            win += n_win
        return out

    def _score_capacity(self) -> int:
        return int(self.cfg.max_seq_len)

    def generate(self, max_new: int, stop_ids=()):
        tok = np.zeros((self.batch, max_new), dtype=np.int32)
        n = np.zeros(self.batch, dtype=np.int32)
        stop = np.ascontiguousarray(list(stop_ids), dtype=np.int32)
        _lib.check(_lib.load().asr_qwen_generate(self._h, max_new, _ip(stop) if stop.size else None, stop.size, _ip(tok), _ip(n)))
        return [tok[b, :n[b]].copy() for b in range(self.batch)]

    def kv_stats(self) -> dict:
        """The KV cache's page accounting (asr_qwen_kv_stats): paged?, pages in the pool, pages held now, high-water mark since the prefill."""
        out = np.zeros(4, dtype=np.int32)
        _lib.check(_lib.load().asr_qwen_kv_stats(self._h, _ip(out)))
        return {"paged": bool(out[0]), "pool_pages": int(out[1]), "held": int(out[2]), "high_water": int(out[3])}

    def beam_search(self, beam: int, max_new: int, stop_ids=()):
        """Width-`beam` search after a prefill -> per utterance a best-first list of (token ids, summed log-probability)."""
        tok = np.zeros((self.batch, beam, max_new), dtype=np.int32)
        n = np.zeros((self.batch, beam), dtype=np.int32)
        score = np.zeros((self.batch, beam), dtype=np.float32)
        stop = np.ascontiguousarray(list(stop_ids), dtype=np.int32)
        _lib.check(_lib.load().asr_qwen_beam_search(self._h, int(beam), int(max_new), _ip(stop) if stop.size else None, stop.size, _ip(tok), _ip(n),
                                                    _fp(score)))
        return [[(tok[b, r, :n[b, r]].copy(), float(score[b, r])) for r in range(beam)] for b in range(self.batch)]


class QwenAlignerSession(QwenAsrSession):
    """HIP replacement of the merged Qwen3-ForcedAligner graph (Qwen_ForcedAligner/Inference_Qwen_ForcedAligner_ONNX.py:540-575): the
    Qwen3-ASR encoder and prompt assembly, one decoder pass over the whole prompt, the timestamp classifier's arg-max on the selected rows.
    The session refuses prefill / decode / generate / beam_search (include/asr_mi355x.h asr_qwen_align)."""

    @classmethod
    def from_checkpoint(cls, cfg, ck, precision=PRECISION_BF16, device_id=0, audio_dtype=np.float32):
        from .arena import build_qwen_aligner_arena
        return cls(cfg, build_qwen_aligner_arena(cfg, ck, cfg.classify_num, precision), precision, device_id, audio_dtype=audio_dtype)

    def align_packed(self, audio, offsets, pre_ids, post_ids, timestamp_id: int = -1, want_logits: bool = False,
                     audio_device_ptr: int | None = None):
        """pre_ids / post_ids: one id list per utterance (or one shared list); prompt = [pre | audio embeddings | post]. timestamp_id < 0
        classifies every position. -> (buckets per utterance, logits per utterance (rows, classify_num) | None, ids_len (B,))"""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        B = offsets.size - 1
        pre, pre_off = self._ragged(pre_ids, B)
        post, post_off = self._ragged(post_ids, B)
        ids_len = np.zeros(B, dtype=np.int32)
        n_audio = [self.audio_tokens(int(offsets[b + 1] - offsets[b])) for b in range(B)]
        if timestamp_id < 0:
            cap = int(sum(n_audio) + pre_off[-1] + post_off[-1])
        else:
            cap = int(np.count_nonzero(pre[:pre_off[-1]] == timestamp_id) + np.count_nonzero(post[:post_off[-1]] == timestamp_id))
        slot_off = np.zeros(B + 1, dtype=np.int32)
        buckets = np.zeros(max(cap, 1), dtype=np.int32)
        logits = np.empty((max(cap, 1), self.cfg.classify_num), dtype=np.float32) if want_logits else None
        if audio_device_ptr is not None:
            ap, mem = C.c_void_p(audio_device_ptr), MEM_DEVICE
        else:
            audio = self._audio(audio).reshape(-1)
            ap, mem = audio.ctypes.data_as(C.c_void_p), MEM_HOST
        _lib.check(_lib.load().asr_qwen_align(self._h, ap, mem, offsets.ctypes.data_as(C.POINTER(C.c_int64)), B, _ip(pre), _ip(pre_off),
                                              _ip(post), _ip(post_off), int(timestamp_id), _ip(slot_off), _ip(buckets), cap, _fp(logits),
                                              _ip(ids_len)))
        self.batch = 0
        bk = [buckets[slot_off[b]:slot_off[b + 1]].copy() for b in range(B)]
        lg = [logits[slot_off[b]:slot_off[b + 1]].copy() for b in range(B)] if want_logits else None
        return bk, lg, ids_len

    def align(self, audios: Sequence[np.ndarray], pre_ids, post_ids, timestamp_id: int = -1, want_logits: bool = False):
        _, packed, offs = self._pack(audios)
        return self.align_packed(packed, offs, pre_ids, post_ids, timestamp_id, want_logits)


def load_session(path: str, device_id: int = 0):
    """Open an `.asrmodel` bundle (tools/convert_checkpoint.py, export_*) as the matching native session."""
    from . import config as cfgm
    from .ort_shim import load_model
    info, blob = load_model(path)
    kind, conf, prec = info["kind"], dict(info["config"] or {}), int(info.get("precision", 0))
    adt = audio_np_dtype(info.get("input_audio_dtype", "F32"))        # the bundle's export type; old bundles carry none: F32
    if kind == "sensevoice":
        conf["language_prompt_token_ids"] = tuple(conf["language_prompt_token_ids"])
        return SenseVoiceSession(cfgm.SenseVoiceConfig(**conf), blob, prec, device_id, audio_dtype=adt)
    if kind == "paraformer":
        return ParaformerSession(cfgm.ParaformerConfig(**conf), blob, prec, device_id, audio_dtype=adt)
    if kind == "whisper":
        return WhisperSession(cfgm.WhisperConfig(**conf), blob, prec, device_id, audio_dtype=adt)
    if kind == "qwen_asr":
        return QwenAsrSession(cfgm.QwenAsrConfig(**conf), blob, prec, device_id, audio_dtype=adt)
    if kind == "paraformer_streaming":
        return ParaformerStreamSession(cfgm.ParaformerConfig(**conf), blob, prec, device_id, chunk=int(info["metadata"].get("chunk", 8000)), audio_dtype=adt)
    if kind == "qwen_aligner":
        return QwenAlignerSession(cfgm.QwenAlignerConfig(**conf), blob, prec, device_id, audio_dtype=adt)
    raise ValueError(f"{path!r}: no native session for bundle kind {kind!r}")
