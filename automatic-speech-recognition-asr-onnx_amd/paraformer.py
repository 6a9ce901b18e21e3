"""Paraformer (non-streaming) host loop: audio in -> token ids / text out, RTF -- the call surface of
`Paraformer/Non-Streaming/Inference_Paraformer_ONNX.py`, written against the onnxruntime-API shim:

  export_paraformer()   ~ Export_Paraformer.py tail (:583-640): Paraformer.asrmodel + ASR_Metadata.asrmodel + Vocab_Paraformer.txt
  build_tokenizer_metadata() = :136-159 (blank/eos/stop ids by token role, one artefact language with its decode mode)
  decode_tokens()       = Inference_Paraformer_ONNX.py:86-89 ("en": BPE "@@ " joins; otherwise plain concatenation)
  transcribe()          = :236-297 (window/pad, one pre-bound audio buffer updated in place, per-window run, stop ids stripped)
  token_times()         the build's own rule (no reference counterpart): CIF fire rows -> a (start, end) per token
  transcribe(beam_size=, nbest=, hotwords=, lm=)   the build's own mode: n-best beam search over the decoder's token rows (ParaformerSession.run_beam)
prepare_audio_input / plan_windows are the SenseVoice ones (identical code in the reference, :62-84, :243-259).
"""
from __future__ import annotations

import json
import os
import time
from typing import Sequence

import numpy as np

from . import ort_shim as onnxruntime
from .arena import build_paraformer_arena
from .config import ParaformerConfig
from .ort_io import (array_for, filled_for, is_dynamic_dim, load_special_token_ids, load_supported_languages, numpy_dtype,
                     resolve_supported_language)
from .input_format import as_frames, cut_windows, session_input_format
from .segmenter import pack, run_long
from .sensevoice import plan_windows, prepare_audio_input

C = onnxruntime

_ROLE_TOKENS = {"blank": ("<blank>", "<blk>", "<eps>"), "eos": ("</s>", "<eos>"), "unknown": ("<unk>", "<unknown>", "[UNK]"),
                "pad": ("<pad>", "[PAD]"), "bos": ("<s>", "<bos>", "<sos>")}
_LANGUAGES = {"zh": ("Chinese", ["Chinese", "Mandarin", "zh-CN", "中文"]), "en": ("English", ["English", "en-US"])}


def build_tokenizer_metadata(token_list: Sequence[str], language: str, decode_mode: str):
    tokens = list(token_list)

    def find(role):
        return next((i for i, t in enumerate(tokens) if t in _ROLE_TOKENS[role]), None)

    special = {"blank": find("blank"), "eos": find("eos"), "stop": [find("eos")]}
    for role in ("unknown", "pad", "bos"):
        if find(role) is not None:
            special[role] = find(role)
    name, aliases = _LANGUAGES[language]
    return special, {language: {"name": name, "aliases": aliases, "prompt_token_ids": [], "decode_mode": decode_mode}}


def export_paraformer(folder: str, cfg: ParaformerConfig, ck: dict, token_list: Sequence[str], language: str = "zh",
                      decode_mode: str = "zh", precision: int = 0, input_audio_dtype: str = "F32") -> None:
    """`input_audio_dtype`: the reference's INPUT_AUDIO_DTYPE (Export_Paraformer.py:88): the type the `audio` input is declared and fed with."""
    onnxruntime.input_audio_dtype_name(input_audio_dtype)
    os.makedirs(folder, exist_ok=True)
    special, langs = build_tokenizer_metadata(token_list, language, decode_mode)
    meta = {"sample_rate": str(cfg.sample_rate), "audio_pcm_scale": "1",
            "special_token_ids": json.dumps(special, separators=(",", ":")),
            "supported_languages": json.dumps(langs, ensure_ascii=False, sort_keys=True, separators=(",", ":"))}
    onnxruntime.save_model(os.path.join(folder, "Paraformer.asrmodel"), "paraformer", cfg.to_dict(),
                           build_paraformer_arena(cfg, ck, precision), {}, precision, input_audio_dtype)
    onnxruntime.save_model(os.path.join(folder, "ASR_Metadata.asrmodel"), "metadata", None, None, meta)
    with open(os.path.join(folder, "Vocab_Paraformer.txt"), "w", encoding="utf-8") as f:
        for t in token_list:
            f.write(f"{t}\n")


def decode_tokens(tokens: Sequence[str], mode: str) -> str:
    if mode == "en":
        return " ".join(tokens).replace("@@ ", "").strip()
    return "".join(tokens).strip()


def token_times(fire_frame, n_rows: int, row_seconds: float, max_token_rows: int = 4) -> np.ndarray:
    """CIF fire rows of one utterance -> [n, 2] float64 (start, end) in seconds from the utterance's first sample. The build's own rule -- the reference
    returns ids only. Token k ends behind the row that fired it, min(fire_k + 1, n_rows) rows in (a tail fire, fire_k == n_rows, ends with the last row);
    it starts at the later of the previous token's end (0 for the first token) and end - max_token_rows. A token is thus the interval over which CIF
    integrated it, capped so that silence in front of it is not charged to it. The cap's default, 4 rows (0.24 s at 60 ms rows), is an assumption: it
    follows the 12 frames of 20 ms of FunASR's CIF timestamp rule as remembered, not as read from a file."""
    fire = np.asarray(fire_frame, dtype=np.int64).reshape(-1)
    out = np.zeros((fire.size, 2), dtype=np.float64)
    prev_end = 0
    for k, f in enumerate(fire):
        end = max(min(int(f) + 1, int(n_rows)), prev_end)
        start = max(prev_end, end - int(max_token_rows))
        out[k] = (start * row_seconds, end * row_seconds)
        prev_end = end
    return out


class ParaformerTranscriber:
    def __init__(self, model_folder: str, vocab_path: str | None = None, device_id: int = 0, device_type: str = "cpu"):
        opts = onnxruntime.SessionOptions()
        opts.execution_mode = onnxruntime.ExecutionMode.ORT_SEQUENTIAL
        self.run_options = onnxruntime.RunOptions()
        self.run_options.add_run_config_entry("disable_synchronize_execution_providers", "0")
        self.session_meta = onnxruntime.InferenceSession(os.path.join(model_folder, "ASR_Metadata.onnx"), sess_options=opts)
        self.session = onnxruntime.InferenceSession(os.path.join(model_folder, "Paraformer.onnx"), sess_options=opts, device_id=device_id)
        self.audio_meta = self.session.get_inputs()[0]
        self.out_names = [o.name for o in self.session.get_outputs()]
        self.device_type, self.device_id = device_type, device_id
        self.ort_device = C.OrtDevice(C.OrtDevice.cuda() if device_type != "cpu" else C.OrtDevice.cpu(),
                                      C.OrtDevice.default_memory(), device_id)
        dt = numpy_dtype(self.audio_meta)
        self.input_audio_dtype = "INT16" if dt == np.int16 else "F16" if dt == np.float16 else "F32"
        meta = self.session_meta.get_modelmeta().custom_metadata_map or {}
        self.sample_rate = int(meta["sample_rate"])
        self.audio_pcm_scale = int(meta["audio_pcm_scale"])
        stop = load_special_token_ids(meta)["stop"]
        self.stop_token_ids = stop if isinstance(stop, list) else [stop]
        languages = load_supported_languages(meta)
        self.language, entry = resolve_supported_language(languages, next(iter(languages)))
        self.decode_mode = entry.get("decode_mode")
        with open(vocab_path or os.path.join(model_folder, "Vocab_Paraformer.txt"), "r", encoding="UTF-8") as f:
            self.tokenizer = np.array([line.rstrip("\n") for line in f], dtype=np.str_)

    def _run_window_timed(self, win: np.ndarray, offset_s: float, duration_s: float, max_token_rows: int, n_frames: int | None = None, n_model: int | None = None):
        """One window through the native session under the shim session (the graph's two outputs carry no times): (token ids as the graph returns them,
        one record per token with the window's offset added and both ends clipped to the audio's duration). n_frames / n_model: the window's length in
        frames of the session's input format and in model-rate samples, where they are not win.size."""
        native = self.session._native
        cfg = native.cfg
        n_frames, n_model = win.size if n_frames is None else n_frames, win.size if n_model is None else n_model
        tok, num, fire, logprob = native.run_packed_timed(win.reshape(-1), np.array([0, n_frames], dtype=np.int64))
        n = int(num[0])
        spans = token_times(fire[0, :n], cfg.seq_len(n_model), cfg.lfr_n * cfg.hop_length / cfg.sample_rate, max_token_rows)
        tokens = [{"id": int(tok[0, k]), "text": str(self.tokenizer[tok[0, k]]), "start": min(offset_s + float(spans[k, 0]), duration_s),
                   "end": min(offset_s + float(spans[k, 1]), duration_s), "logprob": float(logprob[0, k])} for k in range(n)]
        return tok[0, :n].copy(), tokens

    def _hotword_ids(self, hotwords):
        """Hotwords as token-id lists: id lists pass through; text is looked up in the vocabulary -- as one entry, else piece by piece ("en": the words
        between blanks, otherwise the characters). A piece the vocabulary does not list is an error."""
        index = None
        out = []
        for h in hotwords or []:
            if isinstance(h, str):
                if index is None:
                    index = {str(t): i for i, t in reversed(list(enumerate(self.tokenizer.tolist())))}
                text = h.strip()
                pieces = [text] if text in index else text.split() if self.decode_mode == "en" else [c for c in text if not c.isspace()]
                missing = [p for p in pieces if p not in index]
                if missing or not pieces:
                    raise ValueError(f"hotword {h!r}: not in the vocabulary: {missing}")
                h = [index[p] for p in pieces]
            out.append([int(t) for t in h])
        return out

    def load_lm(self, arpa_path):
        """An ARPA file as lm.NgramLM: words are token ids, or entries of this transcriber's vocabulary."""
        from .lm import NgramLM
        index = {str(t): i for i, t in reversed(list(enumerate(self.tokenizer.tolist())))}
        return NgramLM.from_arpa(arpa_path, token_to_id=index.get)

    def _run_window_beam(self, win: np.ndarray, beam_size: int, nbest: int, offset_s: float, duration_s: float, timestamps: bool, max_token_rows: int,
                         n_frames: int | None = None, n_model: int | None = None):
        """One window through the native session's beam search: (token ids of the best hypothesis, the hypotheses found, best first). Every hypothesis has
        one token per CIF fire, so with timestamps each carries "tokens" with the times of the window's shared fire rows (as _run_window_timed forms them)
        and its own log-probabilities; stop ids are dropped from a hypothesis' ids, text and records alike."""
        native = self.session._native
        cfg = native.cfg
        n_frames, n_model = win.size if n_frames is None else n_frames, win.size if n_model is None else n_model
        tok, num, score, am, fire, logprob = native.run_packed_beam(win.reshape(-1), np.array([0, n_frames], dtype=np.int64), beam_size, None, nbest)
        return self._assemble_hypotheses(tok[0], num[0], score[0], am[0], fire[0], logprob[0], cfg.seq_len(n_model),
                                         cfg.lfr_n * cfg.hop_length / cfg.sample_rate, offset_s, duration_s, timestamps, max_token_rows)

    def _assemble_hypotheses(self, tok, num, score, am, fire, logprob, n_rows, row_seconds, offset_s, duration_s, timestamps, max_token_rows):
        """The arrays of one utterance as ParaformerSession.run_packed_beam returns them ([nbest, max_T] / [nbest] / fire [max_T]) -> (best ids, hypotheses)."""
        hyps, spans = [], None
        for n in range(len(num)):
            if not np.isfinite(score[n]):
                break
            count = int(num[n])
            ids = np.asarray(tok[n, :count])
            keep = ~np.isin(ids, self.stop_token_ids)
            h = {"token_ids": ids[keep].copy(), "score": float(score[n]), "am_score": float(am[n]),
                 "text": decode_tokens(self.tokenizer[ids[keep]].tolist(), self.decode_mode)}
            if timestamps:
                if spans is None:                                                   # the fire rows are the utterance's, not the hypothesis'
                    spans = token_times(fire[:count], n_rows, row_seconds, max_token_rows)
                h["tokens"] = [{"id": int(ids[k]), "text": str(self.tokenizer[ids[k]]), "start": min(offset_s + float(spans[k, 0]), duration_s),
                                "end": min(offset_s + float(spans[k, 1]), duration_s), "logprob": float(logprob[n, k])} for k in range(count) if keep[k]]
            hyps.append(h)
        return hyps[0]["token_ids"], hyps

    def transcribe(self, audio_int16: np.ndarray, sliding_window: int = 0, normalise: bool = False, timestamps: bool = False, max_token_rows: int = 4,
                   beam_size: int = 1, nbest: int = 1, hotwords=None, hotword_boost: float = 2.0, lm=None, lm_weight: float = 0.5, length_bonus: float = 0.0,
                   sample_rate: int | None = None, channels: int = 1):
        """int16 mono PCM at `sample_rate` -> dict(token_ids per window, text, rtf, windows). timestamps=True adds "tokens": one {"id", "text", "start",
        "end", "logprob"} per kept token over all windows, in seconds of the whole audio (token_times over the CIF fire rows; logprob = log soft-max of the
        decoder head at the pick); records of stop ids are dropped with their ids.
        beam_size > 1, nbest > 1, hotwords or lm: every window is decoded by the beam search over the decoder's token rows (ParaformerSession.run_packed_beam)
        instead of the per-row arg-max; token_ids / text (and "tokens") hold the best hypothesis and "nbest" holds, per window, the hypotheses found, best
        first: {"token_ids", "score", "am_score", "text"} and, with timestamps, "tokens" -- all hypotheses of a window share its CIF fire rows, so each has
        times. hotwords: token-id lists, or text spelled in the vocabulary; hotword_boost per matched token. lm: an lm.NgramLM (load_lm reads an ARPA file
        over this vocabulary): every token adds lm_weight * log P(token | history) + length_bonus to a hypothesis' score. The call sets exactly its own list
        and model. With all of them at their defaults nothing changes.
        sample_rate / channels: the audio is frames [n, channels] (or flat interleaved) of int16 at that rate, resampled on the device (the session's
        input format, set for this call); windows are cut in input frames (input_format.cut_windows) and every result is what it is for the resampled
        audio, in the same seconds. None: the model's own rate, mono -- the reference's loop, untouched."""
        use_beam = beam_size > 1 or nbest > 1 or bool(hotwords) or lm is not None
        if use_beam:
            if not 1 <= nbest <= beam_size <= 16:
                raise ValueError(f"beam_size {beam_size}, nbest {nbest}: expected 1 <= nbest <= beam_size <= 16")
            self.session._native.set_hotwords(self._hotword_ids(hotwords), hotword_boost)        # exactly this call's list (an empty one clears)
            self.session._native.set_lm(lm, lm_weight, length_bonus)                             # ... and exactly this call's model
        if sample_rate is not None:
            return self._transcribe_frames(audio_int16, sample_rate, channels, sliding_window, normalise, timestamps, max_token_rows, use_beam, beam_size, nbest)
        audio_len = int(np.asarray(audio_int16).size)
        audio = prepare_audio_input(np.asarray(audio_int16, dtype=np.int16).reshape(1, 1, -1), self.input_audio_dtype,
                                    audio_pcm_scale=self.audio_pcm_scale, normalise=normalise)
        shape_in = self.audio_meta.shape[-1]
        window = audio_len if is_dynamic_dim(shape_in) else int(shape_in)
        stride = window if sliding_window <= 0 else sliding_window
        audio = plan_windows(audio, audio_len, window, stride)
        aligned = audio.shape[-1]
        binding = self.session.io_binding()
        audio_buffer = onnxruntime.OrtValue.ortvalue_from_numpy(
            filled_for(self.audio_meta, axes={0: 1, 1: 1, 2: window}), self.device_type, self.device_id)
        binding.bind_ortvalue_input(self.audio_meta.name, audio_buffer)
        ids_all, pieces, tokens_all, nbest_all = [], [], [], []
        start, end = 0, window
        t0 = time.time()
        while end <= aligned:
            win = array_for(self.audio_meta, audio[:, :, start:end], axes={0: 1, 1: 1, 2: window})
            if use_beam:
                token_ids, hyps = self._run_window_beam(win, beam_size, nbest, start / self.sample_rate, audio_len / self.sample_rate, timestamps, max_token_rows)
                nbest_all.append(hyps)
                if timestamps:
                    tokens_all.extend(hyps[0]["tokens"])
            elif timestamps:
                token_ids, toks = self._run_window_timed(win, start / self.sample_rate, audio_len / self.sample_rate, max_token_rows)
                tokens_all.extend(t for t in toks if t["id"] not in self.stop_token_ids)
            else:
                audio_buffer.update_inplace(win)
                for name in self.out_names:                                     # data-dependent token count: re-arm per window
                    binding._iobinding.bind_output(name, self.ort_device)
                self.session.run_with_iobinding(binding, run_options=self.run_options)
                token_ids = binding.get_outputs()[0].numpy().reshape(-1)
            token_ids = token_ids[~np.isin(token_ids, self.stop_token_ids)]
            ids_all.append(token_ids.copy())
            pieces.extend(self.tokenizer[token_ids].tolist())
            start += stride
            end = start + window
        wall = time.time() - t0
        out = {"token_ids": ids_all, "text": decode_tokens(pieces, self.decode_mode), "rtf": wall / (audio_len / self.sample_rate),
               "windows": len(ids_all), "language": self.language}
        if timestamps:
            out["tokens"] = tokens_all
        if use_beam:
            out["nbest"] = nbest_all
        return out

    def _transcribe_frames(self, audio_int16, sample_rate, channels, sliding_window, normalise, timestamps, max_token_rows, use_beam, beam_size, nbest):
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
        ids_all, pieces, tokens_all, nbest_all = [], [], [], []
        t0 = time.time()
        with session_input_format(native, sample_rate, channels):
            for start, win in cuts:
                where = dict(n_frames=win.shape[0], n_model=window)
                if use_beam:
                    token_ids, hyps = self._run_window_beam(win, beam_size, nbest, start / self.sample_rate, duration, timestamps, max_token_rows, **where)
                    nbest_all.append(hyps)
                    if timestamps:
                        tokens_all.extend(hyps[0]["tokens"])
                elif timestamps:
                    token_ids, toks = self._run_window_timed(win, start / self.sample_rate, duration, max_token_rows, **where)
                    tokens_all.extend(t for t in toks if t["id"] not in self.stop_token_ids)
                else:
                    tok, num = native.run_packed(win.reshape(-1), np.array([0, win.shape[0]], dtype=np.int64))
                    token_ids = tok[0, :num[0]]
                token_ids = token_ids[~np.isin(token_ids, self.stop_token_ids)]
                ids_all.append(token_ids.copy())
                pieces.extend(self.tokenizer[token_ids].tolist())
        wall = time.time() - t0
        out = {"token_ids": ids_all, "text": decode_tokens(pieces, self.decode_mode), "rtf": wall / duration, "windows": len(ids_all), "language": self.language}
        if timestamps:
            out["tokens"] = tokens_all
        if use_beam:
            out["nbest"] = nbest_all
        return out

    def transcribe_long(self, audio_int16: np.ndarray, vad=None, sample_rate: int | None = None, channels: int = 1, normalise: bool = False,
                        timestamps: bool = False, max_token_rows: int = 4, beam_size: int = 1, nbest: int = 1, hotwords=None, hotword_boost: float = 2.0,
                        lm=None, lm_weight: float = 0.5, length_bonus: float = 0.0, max_batch: int = 32):
        """A long file cut at its pauses instead of at fixed windows: the device VAD (engine.op_vad; vad = an engine.VadParams, None: the defaults) finds
        the speech, no segment longer than max_audio_len, and the segments run as ragged batches of at most max_batch through the native session
        (run_packed / run_packed_timed / run_packed_beam). The other options are `transcribe`'s. With sample_rate the detector works on the frames at
        that rate and the session's input format is set for the calls, so only kept segments are resampled.
        -> dict(segments = [{"start", "end", "token_ids", "text"} + "tokens" (timestamps) / "nbest" (beam)] in seconds of the file, token_ids = the
        segments' ids in file order (stop ids dropped), text, speech_seconds, audio_seconds, rtf, language). A file with no speech makes no session call."""
        use_beam = beam_size > 1 or nbest > 1 or bool(hotwords) or lm is not None
        if use_beam and not 1 <= nbest <= beam_size <= 16:
            raise ValueError(f"beam_size {beam_size}, nbest {nbest}: expected 1 <= nbest <= beam_size <= 16")
        native = self.session._native
        cfg = native.cfg
        rate = self.sample_rate if sample_rate is None else int(sample_rate)
        row_seconds = cfg.lfr_n * cfg.hop_length / cfg.sample_rate

        def prepare(frames):
            return prepare_audio_input(frames.reshape(1, 1, -1), self.input_audio_dtype, audio_pcm_scale=self.audio_pcm_scale, normalise=normalise,
                                       channels=channels).reshape(-1, channels)

        def run_batch(prepared, segs):
            packed, offs = pack(prepared, segs, channels)
            n_rows = [cfg.seq_len(int(n)) for n in native.model_lengths(np.diff(offs))]
            durs = [int(e - s) / rate for s, e in segs]
            out = []
            if use_beam:
                tok, num, score, am, fire, logprob = native.run_packed_beam(packed, offs, beam_size, None, nbest)
                for b in range(segs.shape[0]):
                    best, hyps = self._assemble_hypotheses(tok[b], num[b], score[b], am[b], fire[b], logprob[b], n_rows[b], row_seconds, 0.0, durs[b],
                                                           timestamps, max_token_rows)
                    r = {"token_ids": best, "nbest": hyps}
                    if timestamps:
                        r["tokens"] = [dict(t) for t in hyps[0]["tokens"]]
                    out.append(r)
            elif timestamps:
                tok, num, fire, logprob = native.run_packed_timed(packed, offs)
                for b in range(segs.shape[0]):
                    n = int(num[b])
                    spans = token_times(fire[b, :n], n_rows[b], row_seconds, max_token_rows)
                    toks = [{"id": int(tok[b, k]), "text": str(self.tokenizer[tok[b, k]]), "start": min(float(spans[k, 0]), durs[b]),
                             "end": min(float(spans[k, 1]), durs[b]), "logprob": float(logprob[b, k])} for k in range(n)]
                    out.append({"token_ids": tok[b, :n].copy(), "tokens": [t for t in toks if t["id"] not in self.stop_token_ids]})
            else:
                tok, num = native.run_packed(packed, offs)
                out = [{"token_ids": tok[b, :num[b]].copy()} for b in range(segs.shape[0])]
            for r in out:
                r["token_ids"] = r["token_ids"][~np.isin(r["token_ids"], self.stop_token_ids)]
                r["text"] = decode_tokens(self.tokenizer[r["token_ids"]].tolist(), self.decode_mode)
            return out

        t0 = time.time()
        if use_beam:
            native.set_hotwords(self._hotword_ids(hotwords), hotword_boost)
            native.set_lm(lm, lm_weight, length_bonus)
        with session_input_format(native, sample_rate, channels):
            records, info = run_long(audio_int16, vad, sample_rate, channels, self.sample_rate, int(cfg.max_audio_len), prepare, run_batch, max_batch)
        ids = [r["token_ids"] for r in records]
        all_ids = np.concatenate(ids) if ids else np.zeros(0, np.int32)
        return {"segments": records, "token_ids": all_ids, "text": decode_tokens(self.tokenizer[all_ids].tolist(), self.decode_mode),
                "speech_seconds": info["speech_seconds"], "audio_seconds": info["audio_seconds"],
                "rtf": (time.time() - t0) / max(info["audio_seconds"], 1e-9), "language": self.language}
