"""Whisper host loop: audio in -> token ids out, RTF -- the call surface of `Whisper/Inference_Whisper_ONNX.py`
(:721-842) on the native session (the three merged graphs collapse into `encode` / `prefill` / `generate`):

  prepare_audio_input()   = :103-126  int16 PCM -> model dtype, PCM scale 32768 (floats in [-1, 1])
  remove_repeated_parts() = :129-139  tail-repeat guard applied before detokenisation (:705-708)
  probe                   = _probe_prefill (:493-550): encoder + cross-KV + prefill([SOT]); language = arg-max over the
                            language-token logits (:793-798); no-speech gate: softmax(logits + 128 on suppressed
                            ids)[<|nospeech|>] >= 0.6 => skip (:799-805, NO_SPEECH_DETECTION Export_Whisper.py:334-348)
  prefill                 = _prefill (:437-490) with [SOT, language, task, <|notimestamps|>] (:807)
  decode                  = _decode_tokens (:584-663): greedy (REPEAT_PENALTY = 1.0) or penalty-greedy (any other value; the
                            multiplier applies once PENALTY_RANGE ids were generated, :630-632), limit MAX_SEQ_LEN - 4 (:821);
                            beam_size > 1: the first hypothesis of the device beam search instead (this build's own mode: the
                            reference has none; plain arg-max scores only, so no penalty or sampling beside it)
  windows of one file    = :745-806: stride SLIDING_WINDOW (or the window length), `ceil((len - window) / stride) + 1` windows, the
                            tail window zero-padded to the aligned length; the [SOT] probe (language, no-speech) runs on window 0
                            ONLY, a no-speech verdict aborts the whole file, later windows reuse window 0's language id; the
                            windows' ids are concatenated and the repeat guard sees the concatenation (:705-708)
  timestamps=True         = this build's own mode (the reference defines NO_TIMESTAMPS_TOKEN and always uses it): the prompt is [SOT, language,
                            task], OpenAI Whisper's timestamp rules run in the device decode head (asr_whisper_set_timestamps) from the full-prompt
                            prefill on -- never on the [SOT] probe, which needs raw logits -- and split_segments() turns the <|t.tt|> ids into
                            segments. The limit is max_target_positions - 3. The tail-repeat guard is NOT applied in this mode: it cuts the id
                            stream at an arbitrary id, which would leave a segment without its closing timestamp.
  word_timestamps=True    = this build's own mode as well: OpenAI Whisper's cross-attention DTW (openai-whisper timing.py) on the device
                            (asr_whisper_set_word_timestamps / asr_whisper_align). Behind <|notimestamps|> with a greedy / penalty / sampling head the rows
                            captured while the ids are generated are the alignment sequence already, nothing is decoded twice; with timestamps=True or
                            beam_size > 1 a forced pass over the final text ids behind a <|notimestamps|> prompt captures them, as OpenAI does. Results gain
                            token_times [(start, end)] per text token (and words, with a piece decoder). The repeat guard is not applied; OpenAI's duration
                            heuristics after the DTW are not part of it.
  token_scores=True       = this build's own mode (the reference reports no score): the device decode head scores every pick with the log-soft-max of the
                            logits row it selects from (asr_whisper_set_token_scores). Results gain token_logprobs (one per entry of tokens), avg_logprob
                            (OpenAI's sum_logprobs / (len + 1): every pick, timestamp ids and the stop pick included), compression_ratio (with a piece
                            decoder) and temperature; words gain probability. The repeat guard is not applied (it would break the pairing).
  temperature_fallback    = OpenAI's decode fallback: an utterance whose avg_logprob is below logprob_threshold, or whose compression_ratio is above its
                            threshold, is decoded again by the sampler at the next temperature of the list (seed + attempt); the encoder output and the
                            cross-K/V stay, the full-prompt prefill restarts the rest. The last attempt stands.
  hotwords=[...]          = this build's own mode (the reference has no bias of any kind): phrases -- token-id lists, or text with hotword_encoder -- the
                            decoder favours (asr_whisper_set_hotwords): a pick that continues a phrase gains hotword_boost, a broken partial match gives its
                            part back. In force from the full-prompt prefill to the last id of every decode (fallback attempts and beam_size > 1 included);
                            the [SOT] probe and the forced alignment pass run without it.
  lm=NgramLM              = this build's own mode: a back-off n-gram model fused into the selection (asr_whisper_set_lm; lm_weight * log P(token | history)
                            + length_bonus per token over the lm_topk best columns, eot scored as </s>), in force where the hotwords are; the sampler
                            of a temperature fallback ignores it.
Batch extension: `transcribe` takes a list of independent clips as one batch (language detection / no-speech per clip);
`transcribe_file` is the reference's per-file behaviour (the windows of one file form the batch).
"""
from __future__ import annotations

import string
import time
import zlib
from typing import Sequence

import numpy as np

from .config import WhisperConfig
from .engine import WhisperSession, audio_dtype_name
from .input_format import as_frames, cut_windows, model_samples, session_input_format
from .segmenter import run_long


def prepare_audio_input(audio_int16: np.ndarray, target_dtype=np.float32, *, audio_pcm_scale: int = 32768,
                        normalise: bool = False, target_rms: float = 4096.0, channels: int = 1) -> np.ndarray:
    if normalise and channels > 1:
        raise ValueError("RMS normalisation is defined on mono PCM: interleaved channels are mixed on the device, behind it (normalise=False, or mix first)")
    target_dtype = np.dtype(target_dtype)
    if not normalise and target_dtype == np.int16:
        return np.ascontiguousarray(audio_int16, dtype=np.int16)
    audio = np.asarray(audio_int16).astype(np.float32)
    if normalise:
        rms = np.sqrt(np.mean(audio * audio, dtype=np.float32), dtype=np.float32)
        if rms > 0:
            audio *= target_rms / (rms + 1e-7)
            np.clip(audio, -float(audio_pcm_scale), float(audio_pcm_scale) - 1.0, out=audio)
    if target_dtype == np.int16:
        return np.ascontiguousarray(audio, dtype=np.int16)
    audio *= np.float32(1.0 / audio_pcm_scale)
    return np.ascontiguousarray(audio, dtype=target_dtype)


def remove_repeated_parts(ids: Sequence[int], repeat_words_threshold: int, ids_len: int):
    """Cut the sequence where a window of `threshold` ids re-occurs later (the reference's loop, :129-139)."""
    if ids_len <= repeat_words_threshold:
        return ids
    left = repeat_words_threshold // 2
    right = left + 1
    end = ids_len - left
    for i in range(left, end):
        for j in range(i + repeat_words_threshold, end):
            if all(ids[j + k] == ids[i + k] for k in range(-left, right)):
                return ids[:j - left]
    return ids


def plan_windows(audio_len: int, input_audio_length: int | None, sliding_window: int = 0):
    """(windows, stride, window_length, aligned_length) of one file, Inference_Whisper_ONNX.py:741-757.
    `input_audio_length=None` is the dynamic-axis export: the window is the whole file."""
    window = int(audio_len) if input_audio_length is None else int(input_audio_length)
    stride = window if sliding_window <= 0 else int(sliding_window)
    if audio_len <= window:
        windows = 1
    else:
        windows = int(np.ceil((audio_len - window) / stride)) + 1
    return windows, stride, window, (windows - 1) * stride + window


def no_speech_probability(logits: np.ndarray, suppress_tokens: Sequence[int], no_speech_id: int) -> np.ndarray:
    """softmax(logits + 128 on the permanently suppressed ids)[<|nospeech|>]  (Export_Whisper.py:334-348)."""
    x = np.asarray(logits, dtype=np.float32).copy()
    if suppress_tokens is not None:
        x[:, list(suppress_tokens)] += np.float32(128.0)
    x -= x.max(axis=1, keepdims=True)
    e = np.exp(x)
    return e[:, no_speech_id] / e.sum(axis=1)


TIMESTAMP_PRECISION = 0.02               # seconds per timestamp id: two encoder positions


def split_segments(ids: Sequence[int], ts_begin: int, window_offset_s: float, window_len_s: float, precision: float = TIMESTAMP_PRECISION):
    """Ids of one window decoded in timestamp mode -> [{"start", "end", "tokens"}], times in seconds = (id - ts_begin) * precision + window_offset_s.
    A timestamp opens a segment when none is open, text ids (everything below ts_begin) accumulate, the next timestamp closes it; the second timestamp
    of a pair opens the next segment (a timestamp that follows a timestamp moves the opening). A segment still open with text when the ids end -- the
    decoder met its limit, or stopped without closing -- ends with the window, at window_offset_s + window_len_s. Segments without text are dropped; text
    before any timestamp (no stream of the timestamp rules has it) counts from the window's start."""
    segs, start, toks = [], None, []
    for i in ids:
        i = int(i)
        if i < ts_begin:
            if start is None:
                start = float(window_offset_s)
            toks.append(i)
            continue
        t = (i - ts_begin) * precision + window_offset_s
        if start is not None and toks:
            segs.append({"start": start, "end": t, "tokens": toks})
            start, toks = None, []
        else:
            start = t
    if start is not None and toks:
        segs.append({"start": start, "end": float(window_offset_s) + float(window_len_s), "tokens": toks})
    return segs


# ---- token / word timestamps (OpenAI Whisper timing.py: find_alignment's jump_times, tokenizer.split_tokens_on_spaces, merge_punctuations)
PREPEND_PUNCTUATIONS = "\"'\u201c\u00bf([{-"
APPEND_PUNCTUATIONS = "\"'.\u3002,\uff0c!\uff01?\uff1f:\uff1a\u201d)]}\u3001"


def token_times(frames: Sequence[int], window_offset_s: float = 0.0, window_end_s: float | None = None, precision: float = TIMESTAMP_PRECISION):
    """Frames of the aligned rows (WhisperSession.align: row r predicts text token r, the last row predicts eot) -> [(start, end)] in seconds per text
    token: start = frames[r] * precision, end = frames[r + 1] * precision, both + window_offset_s; the eot row closes the last token. window_end_s given:
    the ids were cut off before eot, every row is a text token and the last one ends with the window (window_end_s, absolute)."""
    f = [float(window_offset_s) + int(v) * precision for v in frames]
    if window_end_s is not None:
        f.append(max(float(window_end_s), f[-1]) if f else float(window_end_s))
    return [(f[r], f[r + 1]) for r in range(len(f) - 1)]


def split_words(pieces: Sequence[str | None], prepended: str = PREPEND_PUNCTUATIONS, appended: str = APPEND_PUNCTUATIONS) -> list[int]:
    """Token counts per word over the decoded pieces of the text tokens, in order (the counts sum to len(pieces)). OpenAI's split_tokens_on_spaces: a piece
    opens a word when it starts with a space, is punctuation, or is the first; otherwise it continues the word. A token that ends inside a UTF-8 sequence
    has no text of its own: its piece is None and it counts with the token that completes the character (split_tokens_on_unicode; decode_pieces below).
    Then merge_punctuations: a word that is a space plus a prepended mark joins the word after it, a word that is an appended mark joins the word before
    it when that one does not end with a space."""
    words: list[list] = []                                   # [text, token count]
    pending = 0
    for piece in pieces:
        if piece is None:
            pending += 1
            continue
        punctuation = piece.strip() in string.punctuation    # (OpenAI's test as written: a substring of the ASCII punctuation run)
        if piece.startswith(" ") or punctuation or not words:
            words.append([piece, 1 + pending])
        else:
            words[-1][0] += piece
            words[-1][1] += 1 + pending
        pending = 0
    if pending:                                              # ids that end inside a character: they stay with the last word
        if words:
            words[-1][1] += pending
        else:
            words.append(["", pending])
    i, j = len(words) - 2, len(words) - 1
    while i >= 0:
        prev, nxt = words[i], words[j]
        if prev[0].startswith(" ") and prev[0].strip() in prepended:
            nxt[0], nxt[1] = prev[0] + nxt[0], prev[1] + nxt[1]
            prev[0], prev[1] = "", 0
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(words):
        prev, nxt = words[i], words[j]
        if not prev[0].endswith(" ") and nxt[0] in appended:
            prev[0], prev[1] = prev[0] + nxt[0], prev[1] + nxt[1]
            nxt[0], nxt[1] = "", 0
        else:
            i = j
        j += 1
    return [n for _, n in words if n]


def decode_pieces(ids: Sequence[int], decode) -> list:
    """One piece per id for split_words: `decode`(list of ids) -> str; ids that end inside a UTF-8 sequence (the run so far decodes with U+FFFD) get None
    and the id that completes the character carries its text (OpenAI's split_tokens_on_unicode)."""
    pieces, run = [], []
    for t in ids:
        run.append(int(t))
        text = decode(run)
        if "\ufffd" in text:
            pieces.append(None)
        else:
            pieces.append(text)
            run = []
    return pieces


def word_times(pieces: Sequence[str], times: Sequence[tuple], logprobs=None):
    """[{"word", "start", "end", "tokens"}]: the pieces grouped by split_words, each word from the start of its first token to the end of its last
    (`times` = token_times(...), one pair per piece; "tokens" = the word's token count). logprobs (one per piece) adds "probability": the mean of
    exp(logprob) over the word's tokens, OpenAI's word probability."""
    assert len(pieces) == len(times), (len(pieces), len(times))
    assert logprobs is None or len(logprobs) == len(pieces), (len(logprobs), len(pieces))
    out, at = [], 0
    for n in split_words(pieces):
        word = {"word": "".join(p for p in pieces[at:at + n] if p), "start": times[at][0], "end": times[at + n - 1][1], "tokens": n}
        if logprobs is not None:
            word["probability"] = float(np.mean(np.exp(np.asarray(logprobs[at:at + n], dtype=np.float64))))
        out.append(word)
        at += n
    return out


# ---- token scores (OpenAI Whisper decoding.py: sum_logprobs / (len + 1); transcribe.py: compression_ratio, the temperature fallback)
def avg_logprob(scores_row, n_tokens: int, ended: bool) -> float:
    """The mean log-probability of an utterance's picks: the n_tokens emitted ones plus, when the utterance ended, the stop pick that follows them in
    scores_row (WhisperSession.token_scores()[b]) -- OpenAI's sum_logprobs / (len + 1). Nothing summed (no id and no stop pick): 0.0."""
    n = int(n_tokens) + int(bool(ended))
    if n == 0:
        return 0.0
    row = np.asarray(scores_row, dtype=np.float64)
    assert row.size >= n, (row.size, n)
    return float(row[:n].sum() / n)


def compression_ratio(text: str) -> float:
    """len(utf8) / len(zlib.compress(utf8)): a transcript stuck in a repetition loop compresses far better than speech does."""
    raw = text.encode("utf-8")
    return len(raw) / len(zlib.compress(raw))


def build_prompt(cfg: WhisperConfig, head_ids: Sequence[int], prev_ids: Sequence[int] | None) -> list[int]:
    """OpenAI Whisper's _get_initial_tokens: [<|startofprev|>] + the last max_target_positions // 2 - 1 ids of the previous text + the decoding head
    ([SOT, language, task(, <|notimestamps|>)]); the head alone when there is no previous text."""
    prev = [int(t) for t in prev_ids] if prev_ids is not None else []
    if not prev:
        return [int(t) for t in head_ids]
    keep = cfg.max_target_positions // 2 - 1
    return [cfg.sot_prev_id] + prev[-keep:] + [int(t) for t in head_ids]


class WhisperTranscriber:
    def __init__(self, cfg: WhisperConfig, session: WhisperSession, suppress_tokens=None, task: str = "transcribe",
                 detect_language: bool = True, no_speech_detection: bool = True, no_speech_threshold: float = 0.6,
                 remove_repeats: bool = True, repeat_penalty: float = 1.0, penalty_range: int = 20,
                 use_sampling: bool = False, temperature: float = 0.8, top_k: int = 10, top_p: float = 0.95,
                 sampling_repetition_penalty: float = 1.0, seed: int = 0, beam_size: int = 1,
                 timestamps: bool = False, max_initial_timestamp: float | None = 1.0, word_timestamps: bool = False, alignment_heads=None,
                 medfilt_width: int = 7, piece_decoder=None, token_scores: bool = False, temperature_fallback=None,
                 compression_ratio_threshold: float | None = 2.4, logprob_threshold: float | None = -1.0,
                 hotwords=None, hotword_boost: float = 2.0, hotword_encoder=None,
                 lm=None, lm_weight: float = 0.5, length_bonus: float = 0.0, lm_topk: int = 16,
                 initial_prompt=None, condition_on_previous_text: bool = False, prompt_encoder=None, prompt_reset_temperature: float = 0.5):
        # text prompts (the build's own mode, OpenAI Whisper's options; WhisperSession.prefill_prompts): initial_prompt = token ids of a glossary / style hint,
        # or text when prompt_encoder(text) -> ids is given (a tokenizer's encode without special tokens); condition_on_previous_text: transcribe_file runs
        # its windows in order, each prompted with the ids kept so far, and forgets them after a window whose fallback ended above prompt_reset_temperature.
        if isinstance(initial_prompt, str):
            if prompt_encoder is None:
                raise ValueError("initial_prompt given as text needs prompt_encoder(text) -> ids")
            initial_prompt = prompt_encoder((" " + initial_prompt.strip()))
        self.initial_prompt = [int(t) for t in initial_prompt] if initial_prompt is not None else []
        if any(t < 0 or t >= cfg.eot_id for t in self.initial_prompt):
            raise ValueError("initial_prompt holds text ids only (0 .. eot_id - 1)")
        self.condition_on_previous_text, self.prompt_reset_temperature = bool(condition_on_previous_text), float(prompt_reset_temperature)
        # hotword boosting (the build's own: asr_whisper_set_hotwords): token-id lists, or text when hotword_encoder(text) -> ids is given (a tokenizer's
        # encode without special tokens; a text phrase is boosted in both of its spellings, at the start of the text and inside it). The list is in force from
        # the full-prompt prefill to the last id of every decode, fallback attempts and the beam search included; the [SOT] probe and the forced alignment
        # pass run without it.
        from .engine import hotword_id_variants
        self.hotwords, self.hotword_boost = hotword_id_variants(hotwords, hotword_encoder), float(hotword_boost)
        # n-gram LM shallow fusion (the build's own: asr_whisper_set_lm): an lm.NgramLM or an image, in force where the hotwords are; eot is scored as </s>
        self.lm, self.lm_weight, self.length_bonus, self.lm_topk = lm, float(lm_weight), float(length_bonus), int(lm_topk)
        if lm is not None and beam_size > self.lm_topk:
            raise ValueError(f"lm_topk {self.lm_topk} is below beam_size {beam_size}")
        if beam_size > 1 and (float(repeat_penalty) != 1.0 or use_sampling):
            raise ValueError("beam_size > 1 does not combine with a repeat penalty or sampling")
        # token scores / the temperature fallback (the build's own; thresholds are OpenAI's defaults, arguments and not measurements)
        self.temperature_fallback = tuple(float(t) for t in temperature_fallback) if temperature_fallback else ()
        self.token_scores = bool(token_scores) or bool(self.temperature_fallback)
        if self.token_scores and beam_size > 1:
            raise ValueError("token_scores / temperature_fallback need beam_size == 1: the beam search reports a score per hypothesis, not per token")
        if any(t <= 0.0 for t in self.temperature_fallback):
            raise ValueError("temperature_fallback: the temperatures after attempt 0 must be > 0")
        self.compression_ratio_threshold, self.logprob_threshold = compression_ratio_threshold, logprob_threshold
        self.cfg, self.sess = cfg, session
        # word timestamps (the build's own): alignment_heads [(layer, head)] of the checkpoint (None: the upper half of the decoder layers, OpenAI's fallback);
        # piece_decoder(list of ids) -> str (a tokenizer's decode), when given, adds words next to token_times
        self.word_timestamps, self.alignment_heads, self.medfilt_width = bool(word_timestamps), alignment_heads, int(medfilt_width)
        self.piece_decoder = piece_decoder
        self.beam_size = int(beam_size)
        # timestamp mode (the build's own; combines with every head): the latest first timestamp in seconds -> an index in TIMESTAMP_PRECISION steps
        self.timestamps = bool(timestamps)
        self.max_initial_index = None if max_initial_timestamp is None else int(round(max_initial_timestamp / TIMESTAMP_PRECISION))
        self.ts_begin = cfg.no_timestamps_id + 1
        self.suppress_tokens = list(suppress_tokens) if suppress_tokens is not None else None
        self.task_token = cfg.transcribe_id if task == "transcribe" else cfg.translate_id
        self.detect_language, self.no_speech_detection = detect_language, no_speech_detection
        self.no_speech_threshold, self.remove_repeats = no_speech_threshold, remove_repeats
        self.language_token_ids = np.arange(cfg.first_language_id, cfg.first_language_id + cfg.n_languages, dtype=np.int64)
        self.stop_tokens = {cfg.eot_id}
        # REPEAT_PENALTY / PENALTY_RANGE (:77-79): 1.0 selects greedy, any other value penalty-greedy (the reference default is 0.8)
        self.repeat_penalty, self.penalty_range = float(repeat_penalty), int(penalty_range)
        # USE_SAMPLING / TEMPERATURE / TOP_K / TOP_P / SAMPLING_REPETITION_PENALTY (:71-75)
        self.sampling = (bool(use_sampling), float(temperature), int(top_k), float(top_p), float(sampling_repetition_penalty), int(seed))

    @property
    def input_audio_dtype(self) -> str:
        """"INT16" | "F32" | "F16": the type of the session's `audio` input (the reference reads it off the graph, Inference_Whisper_ONNX.py:103-126)."""
        return audio_dtype_name(self.sess.audio_dtype)

    def _prompt(self, lang: int) -> list[int]:
        head = [self.cfg.sot_id, int(lang), self.task_token]
        return head if self.timestamps else head + [self.cfg.no_timestamps_id]

    def _prompts(self, langs, prev=None):
        """One prompt per utterance: build_prompt over its decoding head and initial_prompt + its previous-text ids (prev: per utterance, or None)."""
        return [np.asarray(build_prompt(self.cfg, self._prompt(l), self.initial_prompt + ([int(t) for t in prev[b]] if prev is not None else [])), np.int32)
                for b, l in enumerate(langs)]

    def _limit(self, prompts, max_new=None) -> int:
        """New ids a batch may take: the longest prompt bounds all of it (its slots are the batch's), then max_new."""
        limit = max(0, self.cfg.max_target_positions - max(len(p) for p in prompts))
        return limit if max_new is None else min(limit, int(max_new))

    def _prefill(self, prompts):
        """The full-prompt prefill: equal lengths of at most 8 ids are the plain prefill, anything else goes through prefill_prompts (left-padded on the device)."""
        n = len(prompts[0])
        if n <= 8 and all(len(p) == n for p in prompts):
            return self.sess.prefill(np.stack([np.asarray(p, np.int32) for p in prompts]), want_logits=False)
        return self.sess.prefill_prompts(prompts, want_logits=False)

    def _probe_prefill(self, B: int):
        """The [SOT] probe: raw logits from the plain arg-max head (no penalty, no sampling, no timestamp rules)."""
        self.sess.set_sampling(False)
        self.sess.set_penalty(1.0, self.penalty_range)
        if self.timestamps:
            self.sess.set_timestamps(False)
        if self.hotwords:
            self.sess.set_hotwords([])                                      # language detection and the no-speech probability read raw logits
        if self.lm is not None:
            self.sess.set_lm(None)                                          # ... and the probe's pick is the model's own
        return self.sess.prefill(np.full((B, 1), self.cfg.sot_id, dtype=np.int32))[1]

    def _prefill_and_continue(self, prompt: np.ndarray, limit: int, audio_samples=None, skip=None, sampling=None, align: bool = True):
        """The full-prompt prefill and the ids after it under the transcriber's head (sampling: another sampler setting for this call, a fallback attempt);
        timestamp mode and token scores are on from this prefill to the last id only.
        -> (ids, frames, scores). frames: per utterance (the aligned frames of its text tokens -- None: nothing aligned --, whether the ids ended with eot); with
        word_timestamps they are captured live while the ids are generated, or by a forced pass when the ids carry timestamps or come from the beam search
        (align=False: neither, the caller aligns the ids it keeps). scores: sess.token_scores() of this decode, None with token_scores off."""
        B = len(prompt)
        live = self.word_timestamps and not self.timestamps and self.beam_size == 1 and limit > 0 and align
        frames = [(None, True)] * B
        scores = None
        self.sess.set_penalty(self.repeat_penalty, self.penalty_range)
        self.sess.set_sampling(*(self.sampling if sampling is None else sampling))
        if self.timestamps:
            self.sess.set_timestamps(True, self.max_initial_index)
        if self.token_scores:
            self.sess.set_token_scores(True)
        if live:
            self.sess.set_word_timestamps(True, self.alignment_heads, limit + 1)
        if self.hotwords:
            self.sess.set_hotwords(self.hotwords, self.hotword_boost)
        if self.lm is not None:
            self.sess.set_lm(self.lm, self.lm_weight, self.length_bonus, topk=self.lm_topk, end_ids=(self.cfg.eot_id,))
        try:
            self._prefill(prompt)
            toks = self._continue(limit) if limit > 0 else [np.zeros(0, np.int32)] * B
            if self.token_scores:
                scores = self.sess.token_scores()
            if live:
                ended = [len(t) < limit for t in toks]                # fewer ids than the limit: the utterance met eot, whose row was captured too
                frames = self._align([len(t) + int(e) for t, e in zip(toks, ended)], ended, audio_samples, skip)
        finally:
            if self.timestamps:
                self.sess.set_timestamps(False)
            if self.token_scores:
                self.sess.set_token_scores(False)
            if live:
                self.sess.set_word_timestamps(False)
            if self.hotwords:
                self.sess.set_hotwords([])
            if self.lm is not None:
                self.sess.set_lm(None)
        if self.word_timestamps and not live and limit > 0 and align:
            frames = self._forced_alignment(prompt, [self._text_ids(tk) for tk in toks], audio_samples, skip)
        return toks, frames, scores

    def _quality(self, ids, scores_row, limit: int, temperature: float) -> dict:
        """What token scores say about one utterance's decode: its picks' log-probabilities (one per id), avg_logprob (the stop pick included when the ids
        ended before the limit, the rule _prefill_and_continue uses), the compression ratio of its text (None without a piece decoder), the temperature."""
        n = len(ids)
        ratio = compression_ratio(self.piece_decoder(self._text_ids(ids))) if self.piece_decoder is not None else None
        return {"logprobs": np.asarray(scores_row[:n], dtype=np.float32), "avg_logprob": avg_logprob(scores_row, n, n < limit),
                "compression_ratio": ratio, "temperature": float(temperature)}

    def _needs_fallback(self, q: dict) -> bool:
        """OpenAI's test: too repetitive (compression ratio, when it is known) or too unlikely (average log-probability)."""
        if self.compression_ratio_threshold is not None and q["compression_ratio"] is not None and q["compression_ratio"] > self.compression_ratio_threshold:
            return True
        return self.logprob_threshold is not None and q["avg_logprob"] < self.logprob_threshold

    def _decode(self, prompt: np.ndarray, limit: int, audio_samples=None, skip=None):
        """What transcribe and transcribe_file share after the prompt is known -> (ids, frames, quality). quality: None with token_scores off, else one
        _quality dict per utterance. With a temperature_fallback list, attempt 0 is the configured head; attempt k repeats the full-prompt prefill for the
        whole batch (the encoder output and the cross-K/V stay, the prefill restarts the self-KV and both histories) and decodes with the sampler at the
        list's k-th temperature and seed + k; only the utterances that still needed it take its result. A skipped utterance never needs one. The loop ends
        when none needs one or the list is exhausted: the last attempt stands. Word timestamps then come from a forced pass over the ids that were kept."""
        if not self.token_scores:
            toks, frames, _ = self._prefill_and_continue(prompt, limit, audio_samples, skip)
            return toks, frames, None
        B = len(prompt)
        fallback = bool(self.temperature_fallback)
        use, temperature, top_k, top_p, rep_penalty, seed = self.sampling
        toks, quality, frames = [None] * B, [None] * B, [(None, True)] * B
        need = [True] * B
        try:
            for k, t_k in enumerate((temperature if use else 0.0,) + self.temperature_fallback):
                sampling = None if k == 0 else (True, t_k, top_k, top_p, rep_penalty, seed + k)
                got, frames_k, scores = self._prefill_and_continue(prompt, limit, audio_samples, skip, sampling=sampling, align=not fallback)
                if k == 0:
                    frames = frames_k
                for b in range(B):
                    if need[b]:
                        toks[b], quality[b] = got[b], self._quality(got[b], scores[b], limit, t_k)
                        need[b] = fallback and not (skip is not None and skip[b]) and self._needs_fallback(quality[b])
                if not any(need):
                    break
            if fallback and self.word_timestamps and limit > 0:
                frames = self._forced_alignment(prompt, [self._text_ids(tk) for tk in toks], audio_samples, skip)
        finally:
            if fallback:                                         # the head is left as attempt 0 configured it
                self.sess.set_penalty(self.repeat_penalty, self.penalty_range)
                self.sess.set_sampling(*self.sampling)
        return toks, frames, quality

    def _text_ids(self, ids):
        """The ids that carry text (and times): all of them behind <|notimestamps|>, the ones below the first timestamp id in timestamp mode."""
        return [int(t) for t in ids if not self.timestamps or t < self.ts_begin]

    def _align(self, n_rows, ended, audio_samples, skip):
        """sess.align over the captured rows -> [(frames or None, ended)] per utterance. n_frames = the encoder positions that hold real samples (OpenAI's
        num_frames // 2); fewer than two rows, or a skipped utterance: nothing to align."""
        B = len(n_rows)
        n_rows = [0 if n < 2 or (skip is not None and skip[b]) else n for b, n in enumerate(n_rows)]
        n_enc = [self.sess.align_read_shape(0, b)[2] for b in range(B)]
        hop2 = 2 * self.cfg.hop_length
        n_frames = [n_enc[b] if audio_samples is None else max(1, min(n_enc[b], int(audio_samples[b]) // hop2)) for b in range(B)]
        if not any(n_rows):
            return [(None, e) for e in ended]
        frames = self.sess.align(n_rows, n_frames, self.medfilt_width)
        return [(frames[b] if n_rows[b] else None, ended[b]) for b in range(B)]

    def _forced_alignment(self, prompt: np.ndarray, text_ids, audio_samples, skip):
        """What OpenAI does after decoding: the capture over the final text ids only, behind a <|notimestamps|> prompt -- a prefill and host-fed decode steps
        under the plain head, timestamp rules off; an utterance that has run out of ids is fed eot. The row of the last text id predicts eot."""
        cfg, sess = self.cfg, self.sess
        B, longest = len(prompt), max((len(t) for t in text_ids), default=0)
        if longest == 0:
            return [(None, True)] * B
        hl = 3 if self.timestamps else 4                     # the decoding head ends every prompt; what stands in front of it (previous text) stays
        forced = [np.concatenate([np.asarray(p[:len(p) - hl], np.int32), np.asarray(p[len(p) - hl:][:3], np.int32), [cfg.no_timestamps_id]]).astype(np.int32)
                  for p in prompt]
        sess.set_penalty(1.0, self.penalty_range)
        sess.set_sampling(False)
        sess.set_word_timestamps(True, self.alignment_heads, longest + 1)
        try:
            self._prefill(forced)
            for t in range(longest):
                sess.decode(np.asarray([ids[t] if t < len(ids) else cfg.eot_id for ids in text_ids], np.int32))
            return self._align([len(ids) + 1 if ids else 0 for ids in text_ids], [True] * B, audio_samples, skip)
        finally:
            sess.set_word_timestamps(False)

    def _token_times(self, aligned, text_ids, offset_s: float, window_s: float, logprobs=None):
        """token_times (and words; with logprobs, one per text id, their probability) of one utterance's text ids from its entry of _prefill_and_continue's frames."""
        frames, ended = aligned
        n = len(text_ids)
        if frames is None:                                   # nothing aligned (no ids, or a single id cut off at the limit): the ids span the window
            times = [(float(offset_s), float(offset_s) + float(window_s))] * n
        else:
            times = token_times(frames[:n + 1] if ended else frames[:n], offset_s, None if ended else offset_s + window_s)
        out = {"token_times": times}
        if self.piece_decoder is not None:
            out["words"] = word_times(decode_pieces(text_ids, self.piece_decoder), times, logprobs)
        return out

    def _add_segment_times(self, segments, times, words_of=None, logprobs=None):
        """Segments of timestamp mode gain token_times (and words) by token count."""
        at = 0
        for seg in segments:
            n = len(seg["tokens"])
            seg["token_times"] = times[at:at + n]
            if self.piece_decoder is not None:
                seg["words"] = word_times(decode_pieces(seg["tokens"], self.piece_decoder), seg["token_times"],
                                          None if logprobs is None else logprobs[at:at + n])
            at += n

    def _text_logprobs(self, ids, logprobs):
        """The scores of the ids that stay in `tokens`: all of them behind <|notimestamps|>, the text ids in timestamp mode."""
        return np.asarray([lp for t, lp in zip(ids, logprobs) if not self.timestamps or t < self.ts_begin], dtype=np.float32)

    def _continue(self, limit: int):
        """Ids after the full-prompt prefill: greedy / penalty-greedy / sampling, or the first hypothesis of the beam search."""
        if self.beam_size > 1:
            return [hyps[0][0] for hyps in self.sess.beam_search(self.beam_size, limit, eos_id=self.cfg.eot_id)]
        return self.sess.generate(limit, eos_id=self.cfg.eot_id)

    def transcribe(self, clips_int16: Sequence[np.ndarray], language_ids: Sequence[int] | None = None, max_new: int | None = None, prompts=None,
                   sample_rate: int | None = None, channels: int = 1):
        """List of int16 mono 16 kHz clips (each <= 30 s) -> per clip dict(tokens, language_id, no_speech_prob, skipped, prompt_len). Timestamp mode adds
        segments = [{"start", "end", "tokens"}] (seconds from the clip's start) and keeps text ids only in tokens; the repeat guard is not applied.
        prompts: per clip the ids of its previous text (any lengths, None / empty: none) -- how a caller batches window k of many files; initial_prompt goes
        in front of each. The longest prompt bounds the whole batch: new ids <= max_target_positions - longest prompt.
        sample_rate / channels: the clips are frames [n, channels] (or flat interleaved) at that rate, resampled on the device (the session's input
        format, set for this call); lengths and seconds are the resampled clips'. None: 16 kHz mono, nothing changes."""
        with session_input_format(self.sess, sample_rate, channels) as formatted:
            return self._transcribe(clips_int16, language_ids, max_new, prompts, channels if formatted else None)

    def transcribe_long(self, pcm_int16: np.ndarray, vad=None, sample_rate: int | None = None, channels: int = 1, language_id: int | None = None,
                        max_new: int | None = None, prompt=None, max_batch: int = 16):
        """A long file cut at its pauses instead of at fixed 30 s windows: the device VAD (engine.op_vad; vad = an engine.VadParams, None: the defaults)
        finds the speech, no segment longer than cfg.max_audio_len, and the segments go through `transcribe` as clip lists of at most max_batch, with
        this transcriber's settings (timestamps, word timestamps, beam, hotwords, lm, ...) as they are. language_id / prompt (ids of previous text): given
        to every segment. With sample_rate the detector works on the frames at that rate and only kept segments are resampled.
        -> dict(segments = [{"start", "end", ...the clip's result...}] with segments / token_times / words in seconds of the file, token_ids = the
        segments' text ids in file order, text (None without a piece decoder), speech_seconds, audio_seconds), stats. No speech: no session call."""
        wall = [0.0]

        def run_batch(frames, segs):
            clips = [frames[s:e] for s, e in segs]
            out, stats = self.transcribe(clips, None if language_id is None else [language_id] * len(clips), max_new,
                                         None if prompt is None else [prompt] * len(clips), sample_rate, channels)
            wall[0] += stats["wall_s"]
            for r in out:
                r["token_ids"] = r["tokens"]
            return out

        records, info = run_long(pcm_int16, vad, sample_rate, channels, self.cfg.sample_rate, int(self.cfg.max_audio_len), lambda f: f, run_batch, max_batch)
        ids = [r["token_ids"] for r in records]
        all_ids = np.concatenate(ids) if ids else np.zeros(0, np.int32)
        text = None
        if self.piece_decoder is not None:
            text = "".join(p for p in decode_pieces(all_ids.tolist(), self.piece_decoder) if p)
        res = {"segments": records, "token_ids": all_ids, "text": text, "speech_seconds": info["speech_seconds"], "audio_seconds": info["audio_seconds"]}
        return res, {"rtf": wall[0] / max(info["audio_seconds"], 1e-9), "wall_s": wall[0]}

    def _transcribe(self, clips_int16, language_ids, max_new, prompts, channels):
        cfg = self.cfg
        audios = [prepare_audio_input(np.asarray(c, dtype=np.int16).reshape(-1), self.sess.audio_dtype) for c in clips_int16]
        # samples per clip at the model's rate: the clip's own size, or what the resampler makes of its frames
        n_model = [a.size for a in audios] if channels is None else [int(n) for n in self.sess.model_lengths([a.size // channels for a in audios])]
        B = len(audios)
        lang = np.asarray(language_ids if language_ids is not None else [cfg.first_language_id] * B, dtype=np.int64)
        t0 = time.time()
        self.sess.encode(audios)                                         # STFT + encoder + cross-KV, once per window
        probs = np.zeros(B, dtype=np.float32)
        if self.detect_language or self.no_speech_detection:
            logits = self._probe_prefill(B)                                 # probe with [SOT]
            if self.detect_language:
                lang = self.language_token_ids[np.argmax(logits[:, self.language_token_ids], axis=1)]
            if self.no_speech_detection:
                probs = self.sess.no_speech_prob(cfg.no_speech_id)          # device head over the probe's logits
        skipped = probs >= self.no_speech_threshold if self.no_speech_detection else np.zeros(B, dtype=bool)
        if prompts is not None and len(prompts) != B:
            raise ValueError(f"{len(prompts)} prompts for {B} clips")
        prompt = self._prompts(lang, None if prompts is None else [p if p is not None else [] for p in prompts])
        limit = self._limit(prompt, max_new)
        toks, aligned, quality = self._decode(prompt, limit, n_model, skipped)
        wall = time.time() - t0
        out = []
        for b in range(B):
            ids = [] if skipped[b] else toks[b].tolist()
            res = {"language_id": int(lang[b]), "no_speech_prob": float(probs[b]), "skipped": bool(skipped[b]), "prompt_len": len(prompt[b])}
            lps = None
            if quality is not None:
                q = quality[b]
                lps = self._text_logprobs(ids, q["logprobs"])
                res.update(token_logprobs=lps, avg_logprob=0.0 if skipped[b] else q["avg_logprob"],
                           compression_ratio=None if skipped[b] else q["compression_ratio"], temperature=q["temperature"])
            if self.timestamps:
                res["segments"] = split_segments(ids, self.ts_begin, 0.0, n_model[b] / cfg.sample_rate)
                ids = [t for t in ids if t < self.ts_begin]
            elif self.remove_repeats and not self.word_timestamps and not self.token_scores:
                ids = list(remove_repeated_parts(ids, 3, len(ids)))
            res["tokens"] = np.asarray(ids, dtype=np.int32)
            if self.word_timestamps:
                res.update(self._token_times(aligned[b], ids, 0.0, n_model[b] / cfg.sample_rate, lps))
                if self.timestamps:
                    self._add_segment_times(res["segments"], res["token_times"], logprobs=lps)
            out.append(res)
        total_s = sum(n_model) / cfg.sample_rate
        return out, {"rtf": wall / total_s, "wall_s": wall}

    def transcribe_file(self, pcm_int16: np.ndarray, language_id: int | None = None, sliding_window: int = 0,
                        input_audio_length: int | None = -1, max_new: int | None = None, sample_rate: int | None = None, channels: int = 1):
        """One file the way the reference's loop walks it (Inference_Whisper_ONNX.py:741-829). input_audio_length: the encoder's static audio
        dimension, None = dynamic axis (one unpadded window), -1 = dynamic when the file fits the encoder, else windows of cfg.max_audio_len.
        -> dict(tokens = the windows' ids concatenated (repeat guard applied when enabled), windows = per-window ids,
                language_id, no_speech_prob, no_speech), stats.
        The windows are independent once window 0's probe has fixed the language, so they run as ONE batch; the probe's [SOT]
        prefill is evaluated for the batch but only window 0's row is read (the reference never probes a later window).
        Timestamp mode keeps these fixed, independently batched windows (no seek loop): window w's segments are offset by w * stride / sample_rate and
        an open last segment ends with its window; the result gains segments, tokens holds text ids only (windows keeps every id, timestamps
        included) and the repeat guard is not applied.
        With token_scores the result gains token_logprobs (the windows' scores concatenated as their ids are), avg_logprob (pooled over every pick of every
        window), compression_ratio (of the whole text), temperature (the highest any window needed) and window_scores = per window
        {"avg_logprob", "compression_ratio", "temperature"}: the fallback decides window by window, so these are the figures it acted on.
        Text prompts: initial_prompt stands in front of every window's prompt (OpenAI's carry_initial_prompt) and the windows stay one batch. With
        condition_on_previous_text the windows run IN ORDER, one encode each: window w is prompted with initial_prompt + the text ids kept since the last
        reset (build_prompt keeps the last max_target_positions // 2 - 1 of them); a window whose decode ended at a temperature above prompt_reset_temperature
        forgets them (that needs temperature_fallback: without it the temperature never rises and nothing is reset), a later window whose own [SOT] probe says
        no speech is skipped and adds nothing. max_new is clamped to max_target_positions - prompt length. The result gains prompt_len, per window.
        sample_rate / channels: the file is frames [n, channels] (or flat interleaved) at that rate, resampled on the device (the session's input format,
        set for this call). Windows and strides stay model-rate figures and are cut in input frames (input_format.cut_windows: both have to be whole
        numbers of frames); lengths, offsets and seconds are the resampled file's. None: 16 kHz mono, nothing changes."""
        with session_input_format(self.sess, sample_rate, channels) as formatted:
            return self._transcribe_file(pcm_int16, language_id, sliding_window, input_audio_length, max_new, (int(sample_rate), int(channels)) if formatted else None)

    def _transcribe_file(self, pcm_int16, language_id, sliding_window, input_audio_length, max_new, fmt):
        cfg = self.cfg
        if fmt is None:
            raw = np.asarray(pcm_int16, dtype=np.int16).reshape(-1)
            audio_len = int(raw.size)
        else:
            frames = as_frames(pcm_int16, fmt[1])
            audio_len = model_samples(frames.shape[0], fmt[0], cfg.sample_rate)
        if input_audio_length == -1:
            # the reference's default export keeps the audio axis dynamic (Export_Whisper.py:743): the window is the file, unpadded. A file longer than
            # the encoder's position table can only run through the static-axis export: windows of max_audio_len, the tail zero-padded.
            input_audio_length = None if audio_len <= cfg.max_audio_len else cfg.max_audio_len
        n_win, stride, window, aligned = plan_windows(audio_len, input_audio_length, sliding_window)
        if fmt is None:
            audio = prepare_audio_input(raw, self.sess.audio_dtype)
            if audio.size < aligned:                                     # zero-padded tail (:751-757)
                audio = np.concatenate([audio, np.zeros(aligned - audio.size, dtype=audio.dtype)])
            clips = [np.ascontiguousarray(audio[w * stride:w * stride + window]) for w in range(n_win)]
        else:                                                            # the same windows, cut in input frames
            audio = prepare_audio_input(frames.reshape(-1), self.sess.audio_dtype).reshape(-1, fmt[1])
            clips = [np.ascontiguousarray(w) for _, w in cut_windows(audio, None if input_audio_length is None else window, stride, fmt[0], cfg.sample_rate)[1]]
            assert len(clips) == n_win
        lang = cfg.first_language_id if language_id is None else int(language_id)
        t0 = time.time()
        chained = self.condition_on_previous_text and n_win > 1
        self.sess.encode(clips[:1] if chained else clips)                # (chained: one encode per window, as each one's turn comes)
        n_probe = 1 if chained else n_win
        prob, no_speech = 0.0, False
        if self.detect_language or self.no_speech_detection:            # needs_probe: window 0 only (:768)
            logits = self._probe_prefill(n_probe)
            if self.detect_language:
                lang = int(self.language_token_ids[np.argmax(logits[0, self.language_token_ids])])
            if self.no_speech_detection:
                prob = float(self.sess.no_speech_prob(cfg.no_speech_id)[0])
                no_speech = prob >= self.no_speech_threshold             # aborts the file (:801-805)
        windows: list[list[int]] = []
        quality = None
        prompt_lens: list[int] = []
        samples = [min(window, max(1, audio_len - w * stride)) for w in range(n_win)]
        limit = 0
        if not no_speech and not chained:
            prompt = self._prompts([lang] * n_win)
            limit = self._limit(prompt, max_new)
            toks, frames_w, quality = self._decode(prompt, limit, samples)
            windows = [t.astype(int).tolist() for t in toks]
            prompt_lens = [len(p) for p in prompt]
        elif not no_speech:
            # the windows in order: each sees what the ones before it kept. limits[w] is window w's own (its prompt's) limit
            prev: list[int] = []
            frames_w, limits = [], []
            quality = [] if self.token_scores else None
            for w in range(n_win):
                if w > 0:
                    self.sess.encode(clips[w:w + 1])
                    if self.no_speech_detection:
                        self._probe_prefill(1)
                        if float(self.sess.no_speech_prob(cfg.no_speech_id)[0]) >= self.no_speech_threshold:      # nothing said here: nothing decoded, nothing added
                            windows.append([]); frames_w.append((None, True)); limits.append(0); prompt_lens.append(0)
                            if quality is not None:
                                quality.append({"logprobs": np.zeros(0, np.float32), "avg_logprob": 0.0, "compression_ratio": None, "temperature": 0.0})
                            continue
                prompt = self._prompts([lang], [prev])
                lim = self._limit(prompt, max_new)
                toks, fr, q = self._decode(prompt, lim, samples[w:w + 1])
                ids_w = toks[0].astype(int).tolist()
                windows.append(ids_w); frames_w.append(fr[0]); limits.append(lim); prompt_lens.append(len(prompt[0]))
                if quality is not None:
                    quality.append(q[0])
                if q is not None and q[0]["temperature"] > self.prompt_reset_temperature:
                    prev = []                                        # OpenAI's prompt_reset_since: a window decoded that hot is not trusted as context
                else:
                    prev = prev + self._text_ids(ids_w)
            limit = None
        wall = time.time() - t0
        ids = [t for w in windows for t in w]
        res = {"windows": windows, "language_id": lang, "no_speech_prob": prob,
               "no_speech": bool(no_speech), "n_windows": n_win, "stride": stride, "window": window, "prompt_len": prompt_lens}
        if self.timestamps:
            res["segments"] = [seg for w, win in enumerate(windows)
                               for seg in split_segments(win, self.ts_begin, w * stride / cfg.sample_rate, window / cfg.sample_rate)]
            ids = [t for t in ids if t < self.ts_begin]
        elif self.remove_repeats and not self.word_timestamps and not self.token_scores:
            ids = list(remove_repeated_parts(ids, 3, len(ids)))
        res["tokens"] = np.asarray(ids, dtype=np.int32)
        win_lps = None
        if self.token_scores:
            # the windows' scores concatenated as their ids are; avg_logprob pools every pick of every window, window_scores keeps each window's own figures
            quality = quality or []
            win_lps = [self._text_logprobs(win, q["logprobs"]) for win, q in zip(windows, quality)]
            res["token_logprobs"] = np.concatenate(win_lps).astype(np.float32) if win_lps else np.zeros(0, np.float32)
            picks = [len(win) + int(len(win) < (limit if limit is not None else limits[w])) for w, win in enumerate(windows)]
            res["avg_logprob"] = float(sum(q["avg_logprob"] * n for q, n in zip(quality, picks) if n) / max(1, sum(picks)))
            res["compression_ratio"] = compression_ratio(self.piece_decoder(ids)) if self.piece_decoder is not None and windows else None
            res["temperature"] = max((q["temperature"] for q in quality), default=0.0)
            res["window_scores"] = [{k: q[k] for k in ("avg_logprob", "compression_ratio", "temperature")} for q in quality]
        if self.word_timestamps:                                        # per window, offset as the segments are; an open last token ends with its window
            per = [self._token_times(frames_w[w], self._text_ids(win), w * stride / cfg.sample_rate, window / cfg.sample_rate,
                                     None if win_lps is None else win_lps[w])
                   for w, win in enumerate(windows)]
            res["token_times"] = [t for p in per for t in p["token_times"]]
            if self.piece_decoder is not None:
                res["words"] = [x for p in per for x in p["words"]]
            if self.timestamps:
                self._add_segment_times(res["segments"], res["token_times"], logprobs=None if win_lps is None else res["token_logprobs"])
        return res, {"rtf": wall / max(audio_len / cfg.sample_rate, 1e-9), "wall_s": wall}
