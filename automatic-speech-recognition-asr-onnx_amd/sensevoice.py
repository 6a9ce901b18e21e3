"""SenseVoice host loop: audio in -> token ids / text out, RTF -- the call surface of
`SenseVoice/Inference_SenseVoice_ONNX.py`, written against the onnxruntime-API shim so the structure
(bind -> run_with_iobinding -> read ids) is the reference's own (:236-310).

  export_sensevoice()      ~ Export_SenseVoice.py tail (:371-405): writes SenseVoiceSmall.asrmodel + ASR_Metadata.asrmodel
  prepare_audio_input()    = :62-86   (int16 PCM -> model dtype, optional RMS normalisation, immutable PCM scale)
  plan_windows()           = :243-260 (pad / sliding-window geometry)
  transcribe()             = :262-310 (per-window bind / run / decode, RTF = wall / audio seconds)
"""
from __future__ import annotations

import os
import time

import numpy as np

from . import ort_shim as onnxruntime
from .arena import build_sensevoice_arena
from .config import SenseVoiceConfig
from .input_format import as_frames, cut_windows, session_input_format
from .segmenter import pack, run_long
from .ort_io import array_for, filled_for, is_dynamic_dim, load_supported_languages, numpy_dtype, resolve_supported_language

C = onnxruntime  # `C.OrtDevice` in the reference scripts


def export_sensevoice(folder: str, cfg: SenseVoiceConfig, ck: dict, precision: int = 0, input_audio_dtype: str = "F32") -> None:
    """`input_audio_dtype`: the reference's INPUT_AUDIO_DTYPE (Export_SenseVoice.py:21): the type the `audio` input is declared and fed with."""
    onnxruntime.input_audio_dtype_name(input_audio_dtype)
    os.makedirs(folder, exist_ok=True)
    meta = onnxruntime.sensevoice_metadata(cfg)
    onnxruntime.save_model(os.path.join(folder, "SenseVoiceSmall.asrmodel"), "sensevoice", cfg.to_dict(),
                           build_sensevoice_arena(cfg, ck, precision), {}, precision, input_audio_dtype)
    onnxruntime.save_model(os.path.join(folder, "ASR_Metadata.asrmodel"), "metadata", None, None, meta)


def prepare_audio_input(audio_int16: np.ndarray, input_audio_dtype: str, *, audio_pcm_scale: int, normalise: bool = False,
                        target_rms: float = 4096.0, channels: int = 1) -> np.ndarray:
    if normalise and channels > 1:
        raise ValueError("RMS normalisation is defined on mono PCM: interleaved channels are mixed on the device, behind it (normalise=False, or mix first)")
    if not normalise and input_audio_dtype == "INT16":
        return np.ascontiguousarray(audio_int16, dtype=np.int16)
    audio = audio_int16.astype(np.float32)
    if normalise:
        rms = np.sqrt(np.mean(audio * audio, dtype=np.float32), dtype=np.float32)
        if rms > 0:
            audio *= (target_rms / (rms + 1e-7))
            np.clip(audio, -32768.0, 32767.0, out=audio)
    if input_audio_dtype == "INT16":
        return audio.astype(np.int16)
    audio *= np.float32(1.0 / audio_pcm_scale)
    return audio.astype(np.float16) if input_audio_dtype == "F16" else audio


def plan_windows(audio: np.ndarray, audio_len: int, window: int, stride: int) -> np.ndarray:
    """Zero-pad (1,1,L) audio so that windows of `window` samples every `stride` cover it."""
    if audio_len > window:
        n = int(np.ceil((audio_len - window) / stride)) + 1
        need = (n - 1) * stride + window
        audio = np.concatenate((audio, np.zeros((1, 1, need - audio_len), dtype=audio.dtype)), axis=-1)
    elif audio_len < window:
        audio = np.concatenate((audio, np.zeros((1, 1, window - audio_len), dtype=audio.dtype)), axis=-1)
    return audio


def _is_cjk(piece: str) -> bool:
    """Every character of the piece is a CJK ideograph, kana or hangul (such scripts write no spaces: a piece is a word)."""
    def cjk(ch):
        c = ord(ch)
        return (0x3040 <= c <= 0x30FF or 0x3400 <= c <= 0x4DBF or 0x4E00 <= c <= 0x9FFF or 0xAC00 <= c <= 0xD7AF or 0xF900 <= c <= 0xFAFF or
                0x20000 <= c <= 0x2FA1F)
    return len(piece) > 0 and all(cjk(ch) for ch in piece)


def group_words(pieces, spans, logprobs):
    """SentencePiece pieces with their (start, end) spans in seconds and log-probabilities -> words: [{"text", "start", "end", "probability"}]. A piece that
    begins with "\u2581" opens a word (the marker is dropped); a CJK piece is a word of its own, and the piece behind it opens a new one; every other piece
    continues the word in front of it (the first piece always opens one). A word spans from its first piece's start to its last piece's end;
    probability = exp(mean logprob of its pieces)."""
    words, lps, closed = [], [], True
    for piece, (start, end), lp in zip(pieces, spans, logprobs):
        text = piece[1:] if piece.startswith("\u2581") else piece
        cjk = _is_cjk(text)
        if closed or cjk or piece.startswith("\u2581"):
            words.append({"text": text, "start": float(start), "end": float(end)})
            lps.append([float(lp)])
        else:
            words[-1]["text"] += text
            words[-1]["end"] = float(end)
            lps[-1].append(float(lp))
        closed = cjk
    for w, l in zip(words, lps):
        w["probability"] = float(np.exp(np.mean(l)))
    return words


class SenseVoiceTranscriber:
    def __init__(self, model_folder: str, target_language: str = "en", tokenizer_path: str | None = None, device_id: int = 0,
                 device_type: str = "cpu"):
        opts = onnxruntime.SessionOptions()
        opts.execution_mode = onnxruntime.ExecutionMode.ORT_SEQUENTIAL
        self.run_options = onnxruntime.RunOptions()
        self.run_options.add_run_config_entry("disable_synchronize_execution_providers", "0")
        self.session_meta = onnxruntime.InferenceSession(os.path.join(model_folder, "ASR_Metadata.onnx"), sess_options=opts)
        self.session = onnxruntime.InferenceSession(os.path.join(model_folder, "SenseVoiceSmall.onnx"), sess_options=opts,
                                                    device_id=device_id)
        ins, outs = self.session.get_inputs(), self.session.get_outputs()
        self.audio_meta, self.lang_meta = ins[0], ins[1]
        self.out_name0 = outs[0].name
        self.device_type, self.device_id = device_type, device_id
        self.ort_device = C.OrtDevice(C.OrtDevice.cuda() if device_type != "cpu" else C.OrtDevice.cpu(),
                                      C.OrtDevice.default_memory(), device_id)
        dt = numpy_dtype(self.audio_meta)
        self.input_audio_dtype = "INT16" if dt == np.int16 else "F16" if dt == np.float16 else "F32"
        meta = self.session_meta.get_modelmeta().custom_metadata_map or {}
        self.sample_rate = int(meta["sample_rate"])
        self.audio_pcm_scale = int(meta["audio_pcm_scale"])
        self.languages = load_supported_languages(meta)
        self.language, entry = resolve_supported_language(self.languages, target_language)
        self.selector_index = entry.get("selector_index")
        self.tokenizer = None
        if tokenizer_path and os.path.isfile(tokenizer_path):
            from sentencepiece import SentencePieceProcessor
            self.tokenizer = SentencePieceProcessor()
            self.tokenizer.Load(tokenizer_path)

    def _run_window_timed(self, win: np.ndarray, language_idx: np.ndarray, offset_s: float, duration_s: float, n_frames: int | None = None):
        """One window through the native session under the shim session (the graph's two outputs carry no spans): (token ids, token records with the
        window's offset added and both ends clipped to the audio's duration). n_frames: the window's length in frames of the session's input format."""
        native = self.session._native
        offsets = np.array([0, win.size if n_frames is None else n_frames], dtype=np.int64)
        tok, num, first, last, logprob = native.run_packed_timed(win.reshape(-1), offsets, np.asarray(language_idx, dtype=np.int32).reshape(-1))
        n = int(num[0])
        tokens = []
        for k in range(n):
            t0, t1 = native.cfg.row_span_seconds(first[0, k], last[0, k])
            tokens.append({"id": int(tok[0, k]), "start": min(offset_s + t0, duration_s), "end": min(offset_s + t1, duration_s),
                           "logprob": float(logprob[0, k])})
        return tok[0, :n].copy(), tokens

    def align(self, audio_int16: np.ndarray, text_or_ids, normalise: bool = False):
        """CTC forced alignment of a transcript the caller supplies against one window of int16 mono PCM (SenseVoiceSession.align_packed). The transcript is
        text (tokenised with the transcriber's tokenizer) or a list of token ids, taken as they are. Returns dict(tokens, words, path_score, loglik, aligned):
        tokens = [{"id", "start", "end", "logprob"}] in seconds (SenseVoiceConfig.row_span_seconds, clipped to the audio's duration; logprob = mean over
        the span of log soft-max at the token), words = group_words over the tokenizer's pieces (None without a tokenizer), path_score / loglik = the best
        path's and the whole transcript's log-probability, aligned = False when the transcript does not fit the audio (tokens and words are then empty
        and the scores -inf). Audio longer than one window raises ValueError: splitting a transcript across windows is not done here."""
        native = self.session._native
        audio_len = int(np.asarray(audio_int16).size)
        shape_in = self.audio_meta.shape[-1]
        limit = int(native.cfg.max_audio_len) if is_dynamic_dim(shape_in) else min(int(shape_in), int(native.cfg.max_audio_len))
        if audio_len > limit:
            raise ValueError(f"align handles one window: {audio_len} samples given, at most {limit} (max_audio_len) fit")
        if isinstance(text_or_ids, str):
            if self.tokenizer is None:
                raise ValueError("a transcript given as text needs a tokenizer (tokenizer_path); pass token ids instead")
            ids = [int(t) for t in self.tokenizer.encode(text_or_ids)]
        else:
            ids = [int(t) for t in text_or_ids]
        audio = prepare_audio_input(np.asarray(audio_int16, dtype=np.int16).reshape(1, 1, -1), self.input_audio_dtype,
                                    audio_pcm_scale=self.audio_pcm_scale, normalise=normalise)
        window = audio_len if is_dynamic_dim(shape_in) else int(shape_in)
        audio = plan_windows(audio, audio_len, window, window)
        win = array_for(self.audio_meta, audio[:, :, :window], axes={0: 1, 1: 1, 2: window})
        offsets = np.array([0, win.size], dtype=np.int64)
        first, last, logprob, path, lik, status = native.align_packed(win.reshape(-1), offsets, np.asarray([self.selector_index], dtype=np.int32),
                                                                      np.asarray(ids, dtype=np.int32), np.asarray([0, len(ids)], dtype=np.int32))
        ok = int(status[0]) == 0
        duration = audio_len / self.sample_rate
        tokens = []
        for k in range(len(ids) if ok else 0):
            t0, t1 = native.cfg.row_span_seconds(first[k], last[k])
            tokens.append({"id": ids[k], "start": min(t0, duration), "end": min(t1, duration), "logprob": float(logprob[k])})
        words = None
        if self.tokenizer is not None:
            words = group_words([self.tokenizer.id_to_piece(t["id"]) for t in tokens], [(t["start"], t["end"]) for t in tokens], [t["logprob"] for t in tokens])
        return {"tokens": tokens, "words": words, "path_score": float(path[0]), "loglik": float(lik[0]), "aligned": ok}

    def _hotword_ids(self, hotwords):
        """Hotwords as token-id lists: id lists pass through, text needs the tokenizer (tokenizer.encode)."""
        out = []
        for h in hotwords or []:
            if isinstance(h, str):
                if self.tokenizer is None:
                    raise ValueError("hotwords given as text need a tokenizer (tokenizer_path); pass token-id lists instead")
                h = self.tokenizer.encode(h)
            out.append([int(t) for t in h])
        return out

    def load_lm(self, arpa_path):
        """An ARPA file as lm.NgramLM: words are token ids, or pieces of this transcriber's tokenizer."""
        from .lm import NgramLM
        tok = self.tokenizer
        if tok is None:
            return NgramLM.from_arpa(arpa_path)

        def piece_id(piece):                               # (SentencePiece answers an unknown piece with the id of <unk>)
            i = int(tok.piece_to_id(piece))
            return i if tok.id_to_piece(i) == piece else None
        return NgramLM.from_arpa(arpa_path, token_to_id=piece_id)

    def _run_window_beam(self, win: np.ndarray, language_idx: np.ndarray, beam_size: int, nbest: int, n_frames: int | None = None):
        """One window through the native session's CTC prefix beam search: (token ids of the best hypothesis, the hypotheses found, best first)."""
        native = self.session._native
        offsets = np.array([0, win.size if n_frames is None else n_frames], dtype=np.int64)
        tok, num, score, ctc = native.run_packed_beam(win.reshape(-1), offsets, np.asarray(language_idx, dtype=np.int32).reshape(-1), beam_size, None, nbest)
        hyps = []
        for n in range(nbest):
            if not np.isfinite(score[0, n]):
                break
            ids = tok[0, n, :num[0, n]].copy()
            hyps.append({"token_ids": ids, "score": float(score[0, n]), "ctc_score": float(ctc[0, n]),
                         "text": self.tokenizer.decode([ids.tolist()])[0] if self.tokenizer is not None else None})
        return hyps[0]["token_ids"], hyps

    def transcribe(self, audio_int16: np.ndarray, sliding_window: int = 0, normalise: bool = False, timestamps: bool = False, beam_size: int = 1,
                   nbest: int = 1, hotwords=None, hotword_boost: float = 2.0, lm=None, lm_weight: float = 0.5, length_bonus: float = 0.0,
                   sample_rate: int | None = None, channels: int = 1):
        """int16 mono PCM at `sample_rate` -> dict(token_ids, text, rtf, windows). timestamps=True adds "tokens": one {"id", "start", "end", "logprob"}
        per token over all windows, in seconds of the whole audio (SenseVoiceConfig.row_span_seconds; logprob = mean frame log-probability).
        beam_size > 1, nbest > 1 or hotwords: every window is decoded by the CTC prefix beam search (SenseVoiceSession.run_packed_beam) instead of the
        arg-max collapse; token_ids / text hold the best hypothesis and "nbest" holds, per window, the hypotheses found, best first:
        {"token_ids", "score", "ctc_score", "text"}. hotwords: token-id lists, or text when a tokenizer is loaded; hotword_boost per matched token.
        lm: an lm.NgramLM (NgramLM.from_arpa; load_lm reads a file with this transcriber's tokenizer) fused into the search, which it implies as hotwords
        do: every token adds lm_weight * log P(token | history) + length_bonus to a hypothesis' score (SenseVoiceSession.set_lm). The call sets exactly
        its own model: None clears one an earlier call set.
        sample_rate / channels: the audio is frames [n, channels] (or flat interleaved) of int16 at that rate, resampled on the device (the session's
        input format, set for this call); windows are cut in input frames (input_format.cut_windows) and every result is what it is for the resampled
        audio, in the same seconds. None: the model's own rate, mono -- the reference's loop, untouched."""
        use_beam = beam_size > 1 or nbest > 1 or bool(hotwords) or lm is not None
        if use_beam:
            if timestamps:
                raise ValueError("timestamps are not available for beam hypotheses")
            if not 1 <= nbest <= beam_size <= 16:
                raise ValueError(f"beam_size {beam_size}, nbest {nbest}: expected 1 <= nbest <= beam_size <= 16")
            self.session._native.set_hotwords(self._hotword_ids(hotwords), hotword_boost)        # exactly this call's list (an empty one clears)
            self.session._native.set_lm(lm, lm_weight, length_bonus)                             # ... and exactly this call's model
        if sample_rate is not None:
            return self._transcribe_frames(audio_int16, sample_rate, channels, sliding_window, normalise, timestamps, use_beam, beam_size, nbest)
        audio_len = int(np.asarray(audio_int16).size)
        audio = prepare_audio_input(np.asarray(audio_int16, dtype=np.int16).reshape(1, 1, -1), self.input_audio_dtype,
                                    audio_pcm_scale=self.audio_pcm_scale, normalise=normalise)
        shape_in = self.audio_meta.shape[-1]
        window = audio_len if is_dynamic_dim(shape_in) else int(shape_in)
        stride = window if sliding_window <= 0 else sliding_window
        audio = plan_windows(audio, audio_len, window, stride)
        aligned = audio.shape[-1]
        binding = self.session.io_binding()
        language_idx = filled_for(self.lang_meta, self.selector_index, axes={0: 1})
        if self.device_type == "cpu":
            audio_buffer = None
            binding.bind_cpu_input(self.lang_meta.name, language_idx)
        else:
            audio_buffer = onnxruntime.OrtValue.ortvalue_from_numpy(
                filled_for(self.audio_meta, axes={0: 1, 1: 1, 2: window}), self.device_type, self.device_id)
            language_buffer = onnxruntime.OrtValue.ortvalue_from_numpy(language_idx, "cpu", 0)
            binding.bind_ortvalue_input(self.audio_meta.name, audio_buffer)
            binding.bind_ortvalue_input(self.lang_meta.name, language_buffer)
        ids_all, text, tokens_all, nbest_all = [], "", [], []
        start, end = 0, window
        t0 = time.time()
        while end <= aligned:
            win = array_for(self.audio_meta, audio[:, :, start:end], axes={0: 1, 1: 1, 2: window})
            if timestamps:
                token_ids, toks = self._run_window_timed(win, language_idx, start / self.sample_rate, audio_len / self.sample_rate)
                tokens_all.extend(toks)
            elif use_beam:
                token_ids, hyps = self._run_window_beam(win, language_idx, beam_size, nbest)
                nbest_all.append(hyps)
            else:
                if audio_buffer is None:
                    binding.bind_cpu_input(self.audio_meta.name, win)
                else:
                    audio_buffer.update_inplace(win)
                binding._iobinding.bind_output(self.out_name0, self.ort_device)     # token count is data dependent: re-bind per run
                self.session.run_with_iobinding(binding, run_options=self.run_options)
                token_ids = binding.get_outputs()[0].numpy()
            ids_all.append(token_ids.copy())
            if self.tokenizer is not None:
                text += self.tokenizer.decode([token_ids.tolist()])[0]
            start += stride
            end = start + window
        wall = time.time() - t0
        out = {"token_ids": ids_all, "text": text if self.tokenizer is not None else None,
               "rtf": wall / (audio_len / self.sample_rate), "windows": len(ids_all), "language": self.language}
        if timestamps:
            out["tokens"] = tokens_all
        if use_beam:
            out["nbest"] = nbest_all
        return out

    def _transcribe_frames(self, audio_int16, sample_rate, channels, sliding_window, normalise, timestamps, use_beam, beam_size, nbest):
        """`transcribe` for audio in another input format: the same windows, cut in input frames, each through the native session (the shim's graph is
        the reference's: model-rate mono), which resamples on the device."""
        native = self.session._native
        frames = as_frames(audio_int16, channels)
        audio = prepare_audio_input(frames.reshape(1, 1, -1), self.input_audio_dtype, audio_pcm_scale=self.audio_pcm_scale, normalise=normalise,
                                    channels=channels).reshape(-1, channels)
        shape_in = self.audio_meta.shape[-1]
        fixed = None if is_dynamic_dim(shape_in) else int(shape_in)
        window, cuts = cut_windows(audio, fixed, fixed if fixed is None or sliding_window <= 0 else sliding_window, sample_rate, self.sample_rate)
        duration = frames.shape[0] / sample_rate
        lang = np.asarray([self.selector_index], dtype=np.int32)
        ids_all, text, tokens_all, nbest_all = [], "", [], []
        t0 = time.time()
        with session_input_format(native, sample_rate, channels):
            for start, win in cuts:
                if timestamps:
                    token_ids, toks = self._run_window_timed(win, lang, start / self.sample_rate, duration, n_frames=win.shape[0])
                    tokens_all.extend(toks)
                elif use_beam:
                    token_ids, hyps = self._run_window_beam(win, lang, beam_size, nbest, n_frames=win.shape[0])
                    nbest_all.append(hyps)
                else:
                    tok, num = native.run_packed(win.reshape(-1), np.array([0, win.shape[0]], dtype=np.int64), lang)
                    token_ids = tok[0, :num[0]]
                ids_all.append(token_ids.copy())
                if self.tokenizer is not None:
                    text += self.tokenizer.decode([token_ids.tolist()])[0]
        wall = time.time() - t0
        out = {"token_ids": ids_all, "text": text if self.tokenizer is not None else None, "rtf": wall / duration, "windows": len(ids_all),
               "language": self.language}
        if timestamps:
            out["tokens"] = tokens_all
        if use_beam:
            out["nbest"] = nbest_all
        return out

    def transcribe_long(self, audio_int16: np.ndarray, vad=None, sample_rate: int | None = None, channels: int = 1, normalise: bool = False,
                        timestamps: bool = False, beam_size: int = 1, nbest: int = 1, hotwords=None, hotword_boost: float = 2.0, lm=None,
                        lm_weight: float = 0.5, length_bonus: float = 0.0, max_batch: int = 32):
        """A long file cut at its pauses instead of at fixed windows: the device VAD (engine.op_vad; vad = an engine.VadParams, None: the defaults) finds
        the speech, no segment longer than max_audio_len, and the segments run as ragged batches of at most max_batch through the native session
        (run_packed / run_packed_timed / run_packed_beam). The other options are `transcribe`'s. With sample_rate the detector works on the frames at
        that rate and the session's input format is set for the calls, so only kept segments are resampled.
        -> dict(segments = [{"start", "end", "token_ids", "text"} + "tokens" (timestamps) / "nbest" (beam)] in seconds of the file, token_ids = the
        segments' ids in file order, text, speech_seconds, audio_seconds, rtf, language). A file with no speech makes no session call."""
        use_beam = beam_size > 1 or nbest > 1 or bool(hotwords) or lm is not None
        if use_beam and timestamps:
            raise ValueError("timestamps are not available for beam hypotheses")
        if use_beam and not 1 <= nbest <= beam_size <= 16:
            raise ValueError(f"beam_size {beam_size}, nbest {nbest}: expected 1 <= nbest <= beam_size <= 16")
        native = self.session._native
        rate = self.sample_rate if sample_rate is None else int(sample_rate)
        decode = (lambda ids: self.tokenizer.decode([ids.tolist()])[0]) if self.tokenizer is not None else (lambda ids: None)

        def prepare(frames):
            return prepare_audio_input(frames.reshape(1, 1, -1), self.input_audio_dtype, audio_pcm_scale=self.audio_pcm_scale, normalise=normalise,
                                       channels=channels).reshape(-1, channels)

        def run_batch(prepared, segs):
            packed, offs = pack(prepared, segs, channels)
            lang = np.full(segs.shape[0], self.selector_index, dtype=np.int32)
            out = []
            if timestamps:
                tok, num, first, last, logprob = native.run_packed_timed(packed, offs, lang)
                for b, (s, e) in enumerate(segs):
                    dur = int(e - s) / rate
                    spans = [native.cfg.row_span_seconds(first[b, k], last[b, k]) for k in range(num[b])]
                    out.append({"token_ids": tok[b, :num[b]].copy(),
                                "tokens": [{"id": int(tok[b, k]), "start": min(t0, dur), "end": min(t1, dur), "logprob": float(logprob[b, k])}
                                           for k, (t0, t1) in enumerate(spans)]})
            elif use_beam:
                tok, num, score, ctc = native.run_packed_beam(packed, offs, lang, beam_size, None, nbest)
                for b in range(segs.shape[0]):
                    hyps = [{"token_ids": tok[b, n, :num[b, n]].copy(), "score": float(score[b, n]), "ctc_score": float(ctc[b, n]),
                             "text": decode(tok[b, n, :num[b, n]])} for n in range(nbest) if np.isfinite(score[b, n])]
                    out.append({"token_ids": hyps[0]["token_ids"], "nbest": hyps})
            else:
                tok, num = native.run_packed(packed, offs, lang)
                out = [{"token_ids": tok[b, :num[b]].copy()} for b in range(segs.shape[0])]
            for r in out:
                r["text"] = decode(r["token_ids"])
            return out

        t0 = time.time()
        if use_beam:
            native.set_hotwords(self._hotword_ids(hotwords), hotword_boost)
            native.set_lm(lm, lm_weight, length_bonus)
        with session_input_format(native, sample_rate, channels):
            records, info = run_long(audio_int16, vad, sample_rate, channels, self.sample_rate, int(native.cfg.max_audio_len), prepare, run_batch, max_batch)
        ids = [r["token_ids"] for r in records]
        return {"segments": records, "token_ids": np.concatenate(ids) if ids else np.zeros(0, np.int32),
                "text": "".join(r["text"] for r in records) if self.tokenizer is not None else None, "speech_seconds": info["speech_seconds"],
                "audio_seconds": info["audio_seconds"], "rtf": (time.time() - t0) / max(info["audio_seconds"], 1e-9), "language": self.language}
