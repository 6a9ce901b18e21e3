"""Qwen3-ForcedAligner host side: audio + transcript in -> word timestamps out, on the native aligner session. Restates what
`Qwen_ForcedAligner/Inference_Qwen_ForcedAligner_ONNX.py` does around its one merged-graph launch:

  word_units()          = AlignerTextProcessor.word_units / tokenize_space_lang (:164-262): whitespace split, keep letters, digits and
                          the apostrophe, every CJK ideograph its own unit. Japanese / Korean need external segmenters (nagisa, soynlp)
                          and are refused here.
  alignment_ids()       = _build_alignment_prompt_ids (:137-161) without the three audio ids: each word's token ids followed by
                          `timestamp_tokens_per_word` <timestamp> slots (the merged graph's `input_ids`)
  fix_timestamp()       = :264-325  monotonic repair: keep the longest non-decreasing subsequence, re-fill the rest
  parse_timestamp()     = :327-345  slots -> {text, start_time, end_time} per word (ms)
  QwenForcedAligner     = run_inference (:487-575) for a batch of independent utterances: prompt [<|audio_start|> | audio |
                          <|audio_end|> | words + slots], buckets at the slot positions x timestamp_segment_ms, repair, grouping.
"""
from __future__ import annotations

import json
import unicodedata
from typing import List, Sequence

import numpy as np

from .engine import audio_dtype_name
from .whisper import prepare_audio_input

# (first, last) code points of the CJK ideograph blocks the reference splits per character (:180-190)
_CJK_RANGES = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F), (0x2B820, 0x2CEAF),
               (0xF900, 0xFAFF))
_NEEDS_SEGMENTER = {"japanese": "nagisa", "korean": "soynlp"}


def _kept(ch: str) -> bool:
    return ch == "'" or unicodedata.category(ch)[0] in "LN"


def _is_cjk(ch: str) -> bool:
    cp = ord(ch)
    return any(lo <= cp <= hi for lo, hi in _CJK_RANGES)


def word_units(text: str, language: str = "English") -> List[str]:
    """Alignable units of a transcript: whitespace-separated tokens stripped to letters / digits / apostrophes; inside a token, each
    CJK ideograph stands alone and the runs between them stay whole."""
    lang = str(language).strip().lower()
    if lang in _NEEDS_SEGMENTER:
        raise NotImplementedError(f"{language} word splitting needs the {_NEEDS_SEGMENTER[lang]} segmenter, which this build does not ship")
    units: List[str] = []
    for token in text.split():
        run = ""
        for ch in token:
            if not _kept(ch):
                continue
            if _is_cjk(ch):
                if run:
                    units.append(run)
                    run = ""
                units.append(ch)
            else:
                run += ch
        if run:
            units.append(run)
    return units


def alignment_ids(word_token_ids: Sequence[Sequence[int]], timestamp_id: int, per_word: int = 2) -> List[int]:
    """The text block of the prompt: every word's ids, then `per_word` timestamp slots."""
    out: List[int] = []
    for ids in word_token_ids:
        out.extend(int(t) for t in ids)
        out.extend([int(timestamp_id)] * per_word)
    return out


def _longest_non_decreasing(v: List[int]) -> List[bool]:
    """Membership mask of one longest non-decreasing subsequence: O(n^2) table, the earliest predecessor that gives a longer chain, the
    earliest end among the longest chains (the reference's choice among equally long ones)."""
    n = len(v)
    length, prev = [1] * n, [-1] * n
    for i in range(n):
        for j in range(i):
            if v[j] <= v[i] and length[j] + 1 > length[i]:
                length[i], prev[i] = length[j] + 1, j
    keep = [False] * n
    k = length.index(max(length))
    while k >= 0:
        keep[k] = True
        k = prev[k]
    return keep


def fix_timestamp(values) -> List[int]:
    """Monotonic repair. Values outside the longest non-decreasing subsequence come in runs; a run of one or two takes the nearer kept
    neighbour (the left one on a tie, the only one at either end); a longer run is spread evenly between its neighbours (truncated to
    int), or copies the only neighbour it has."""
    v = [int(x) for x in values]
    n = len(v)
    if n == 0:
        return []
    keep = _longest_non_decreasing(v)
    out: List[float] = list(v)
    i = 0
    while i < n:
        if keep[i]:
            i += 1
            continue
        j = i
        while j < n and not keep[j]:
            j += 1
        left = next((out[k] for k in range(i - 1, -1, -1) if keep[k]), None)
        right = next((out[k] for k in range(j, n) if keep[k]), None)
        run = j - i
        for k in range(i, j):
            if run <= 2:
                if left is None or (right is not None and k - i + 1 > j - k):
                    out[k] = right
                else:
                    out[k] = left
            elif left is not None and right is not None:
                out[k] = left + (right - left) / (run + 1) * (k - i + 1)
            else:
                out[k] = left if left is not None else right
        i = j
    return [int(x) for x in out]


def parse_timestamp(words: Sequence[str], timestamps_ms, per_word: int = 2) -> List[dict]:
    """Repaired slot times grouped per word: the group's first slot is the start, its last the end (ms)."""
    fixed = fix_timestamp(timestamps_ms)
    out = []
    for w, word in enumerate(words):
        group = fixed[w * per_word:(w + 1) * per_word]
        out.append({"text": word, "start_time": group[0], "end_time": group[-1]})
    return out


def aligner_metadata(cfg, special_token_ids: dict) -> dict:
    """The metadata map the exporter writes (Export_Qwen_ForcedAligner.py:1270-1276) plus the head size: every value a string."""
    return {"audio_pcm_scale": "32768", "sample_rate": str(cfg.sample_rate), "max_seq_len": str(cfg.max_seq_len),
            "special_token_ids": json.dumps({k: int(special_token_ids[k]) for k in ("audio_start", "audio_end", "audio_pad", "timestamp")}),
            "timestamp_segment_ms": str(cfg.timestamp_segment_ms), "timestamp_tokens_per_word": str(cfg.timestamp_tokens_per_word),
            "classify_num": str(cfg.classify_num)}


def export_qwen_aligner(cfg, ck: dict, path: str, metadata: dict, precision: int = 0, input_audio_dtype: str = "F32") -> str:
    """Checkpoint (HF state-dict names) -> `.asrmodel` bundle: folded aligner arena + config + metadata map."""
    from .arena import build_qwen_aligner_arena
    from .ort_shim import save_model
    save_model(path, "qwen_aligner", cfg.to_dict(), build_qwen_aligner_arena(cfg, ck, cfg.classify_num, precision), dict(metadata), precision, input_audio_dtype)
    return path


class QwenForcedAligner:
    """Word timestamps for a batch of independent utterances. `tokenizer` needs `encode(text, add_special_tokens=False)`; without one,
    transcripts may be given as lists of (word, token ids) pairs."""

    def __init__(self, cfg, session, metadata: dict, tokenizer=None):
        self.cfg, self.sess, self.tokenizer = cfg, session, tokenizer
        special = metadata["special_token_ids"]
        self.special = json.loads(special) if isinstance(special, str) else dict(special)
        self.segment_ms = int(metadata.get("timestamp_segment_ms", cfg.timestamp_segment_ms))
        self.per_word = int(metadata.get("timestamp_tokens_per_word", cfg.timestamp_tokens_per_word))
        self.pcm_scale = int(metadata.get("audio_pcm_scale", 32768))

    def _words(self, transcript, language):
        if isinstance(transcript, str):
            if self.tokenizer is None:
                raise ValueError("a text transcript needs a tokenizer (or pass [(word, token ids), ...])")
            words = word_units(transcript, language)
            return words, [[int(t) for t in self.tokenizer.encode(w, add_special_tokens=False)] for w in words]
        words = [str(w) for w, _ in transcript]
        return words, [[int(t) for t in ids] for _, ids in transcript]

    @property
    def input_audio_dtype(self) -> str:
        """"INT16" | "F32" | "F16": the type of the session's `audio` input (the reference reads it off the graph, Inference_Qwen_ForcedAligner_ONNX.py prepare_audio_input)."""
        return audio_dtype_name(self.sess.audio_dtype)

    def _audio(self, a):
        """A clip in the session's audio type: int16 PCM goes through the reference's prepare_audio_input (untouched for an INT16 session, / pcm_scale for
        a float one); float samples in [-1, 1] serve a float session only -- nothing is rounded to int16 behind the caller's back."""
        a, dt = np.asarray(a), self.sess.audio_dtype
        if a.dtype == np.int16:
            return prepare_audio_input(a.reshape(-1), dt, audio_pcm_scale=self.pcm_scale)
        if dt == np.int16:
            raise TypeError(f"the aligner session takes int16 PCM (INPUT_AUDIO_DTYPE INT16), the clip given is {a.dtype.name}")
        return np.ascontiguousarray(a, dtype=dt).reshape(-1)

    def align(self, audios: Sequence[np.ndarray], transcripts: Sequence, language="English") -> List[List[dict]]:
        """audios: 16 kHz mono clips (int16 PCM or float in [-1, 1]); transcripts: one per clip; language: one name for all clips or one per
        clip. -> per clip a list of {text, start_time, end_time} in ms (an empty list for a transcript without alignable units)."""
        B = len(audios)
        if len(transcripts) != B:
            raise ValueError(f"{len(transcripts)} transcripts for {B} clips")
        langs = [language] * B if isinstance(language, str) else list(language)
        words, post, clips, live = [None] * B, [], [], []
        tid = int(self.special["timestamp"])
        for b in range(B):
            w, ids = self._words(transcripts[b], langs[b])
            words[b] = w
            if not w:
                continue
            live.append(b)
            clips.append(self._audio(audios[b])[:self.cfg.max_audio_len])
            post.append([int(self.special["audio_end"])] + alignment_ids(ids, tid, self.per_word))
        out: List[List[dict]] = [[] for _ in range(B)]
        if not live:
            return out
        buckets, _, _ = self.sess.align(clips, [[int(self.special["audio_start"])]], post, timestamp_id=tid)
        for k, b in enumerate(live):
            out[b] = parse_timestamp(words[b], buckets[k].astype(np.int64) * self.segment_ms, self.per_word)
        return out
