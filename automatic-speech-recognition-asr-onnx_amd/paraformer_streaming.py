"""Streaming Paraformer host loop -- the call surface of `Paraformer/Streaming/Inference_Paraformer_Streaming_ONNX.py`:

  pad_to_chunks()   = :343-356  the clip is extended to a whole number of chunks with white noise at the RMS of its tail
  transcribe()      = :401-449  per chunk: encoder step; when the CIF fired, decoder step -> ids -> stop ids stripped -> text piece;
                                 per-chunk RTF = step wall time / chunk duration
The 200+ cache tensors the reference re-binds between the two ONNX sessions every chunk (encoder_feedback / decoder_feedback /
encoder_decoder_bridge, :309-338) are device-resident state of `ParaformerStreamSession`, addressed by a stream id, so several
clips can advance in lock-step (`transcribe_many`).

  transcribe_many(beam_size=, nbest=, hotwords=, lm=, revise_tokens=)   the build's own mode: the streaming beam search with fixed-lag commits
                                 (ParaformerStreamSession.step_beam / finish_beam); the reference host loop has no counterpart
"""
from __future__ import annotations

import time
from typing import Sequence

import numpy as np

from .paraformer import decode_tokens, token_times
from . import input_format
from .engine import audio_dtype_name
from .sensevoice import prepare_audio_input


def pad_to_chunks(audio: np.ndarray, chunk: int, rng: np.random.Generator | None = None) -> np.ndarray:
    """(1, 1, L) -> (1, 1, ceil(L / chunk) * chunk), the tail filled with white noise scaled to the RMS of the samples it borders."""
    rng = rng or np.random.default_rng()
    n = audio.shape[-1]
    if n > chunk:
        windows = int(np.ceil((n - chunk) / chunk)) + 1
        pad = (windows - 1) * chunk + chunk - n
        ref = audio[:, :, -pad:].astype(np.float32) if pad else audio[:, :, :0].astype(np.float32)
    elif n < chunk:
        pad, ref = chunk - n, audio.astype(np.float32)
    else:
        pad, ref = 0, audio[:, :, :0].astype(np.float32)
    if pad == 0:
        return audio
    noise = (np.sqrt(np.mean(ref * ref)) * rng.normal(0.0, 1.0, size=(1, 1, pad))).astype(audio.dtype)
    return np.concatenate((audio, noise), axis=-1)


def pad_frames_to_steps(frames: np.ndarray, chunk: int, sample_rate: int, model_rate: int, rng: np.random.Generator | None = None):
    """Frames [n, channels] at sample_rate -> (frames extended to A(C) frames, C): the input of C whole steps of a streaming session with that format
    (input_format.stream_start; C the smallest count that covers the clip, at least 1), the tail filled by pad_to_chunks' rule: white noise scaled to the RMS of
    the frames it borders (as many as it is long, or the whole clip when that is shorter)."""
    rng = rng or np.random.default_rng()
    n, C = frames.shape[0], 1
    while input_format.stream_start(chunk, sample_rate, model_rate, C) < n:
        C += 1
    pad = input_format.stream_start(chunk, sample_rate, model_rate, C) - n
    if pad == 0:
        return frames, C
    ref = frames[-pad:].astype(np.float32) if pad < n else frames.astype(np.float32)
    rms = np.sqrt(np.mean(ref * ref)) if ref.size else 0.0
    noise = (rms * rng.normal(0.0, 1.0, size=(pad, frames.shape[1]))).astype(frames.dtype)
    return np.concatenate((frames, noise), axis=0), C


class ParaformerStreamTranscriber:
    def __init__(self, session, token_list: Sequence[str], stop_token_ids: Sequence[int] = (2,), decode_mode: str = "zh",
                 audio_pcm_scale: int = 1, sample_rate: int = 16000):
        self.sess, self.tokens = session, np.asarray(list(token_list), dtype=np.str_)
        self.stop, self.decode_mode = list(stop_token_ids), decode_mode
        self.audio_pcm_scale, self.sample_rate = audio_pcm_scale, sample_rate

    @property
    def input_audio_dtype(self) -> str:
        """"INT16" | "F32" | "F16": the type of the session's `audio` input (the reference reads it off the graph, Inference_Paraformer_Streaming_ONNX.py prepare_audio_input)."""
        return audio_dtype_name(self.sess.audio_dtype)

    def _hotword_ids(self, hotwords):
        """Hotwords as token-id lists: id lists pass through; text is looked up in the vocabulary as ParaformerTranscriber does -- as one entry, else piece by
        piece ("en": the words between blanks, otherwise the characters). A piece the vocabulary does not list is an error."""
        index, out = None, []
        for h in hotwords or []:
            if isinstance(h, str):
                if index is None:
                    index = {str(t): i for i, t in reversed(list(enumerate(self.tokens.tolist())))}
                text = h.strip()
                pieces = [text] if text in index else text.split() if self.decode_mode == "en" else [c for c in text if not c.isspace()]
                missing = [p for p in pieces if p not in index]
                if missing or not pieces:
                    raise ValueError(f"hotword {h!r}: not in the vocabulary: {missing}")
                h = [index[p] for p in pieces]
            out.append([int(t) for t in h])
        return out

    def _transcribe_many_beam(self, prepared, durs, n_chunks, timestamps, max_token_rows, beam_size, nbest, hotwords, hotword_boost, lm, lm_weight,
                              length_bonus, revise_tokens, block):
        sess, chunk = self.sess, self.sess.chunk
        if not 1 <= nbest <= beam_size <= 16:
            raise ValueError(f"beam_size {beam_size}, nbest {nbest}: expected 1 <= nbest <= beam_size <= 16")
        ids = list(range(len(prepared)))
        for i in ids:
            sess.reset(i)
        sess.set_beam(beam_size, None, nbest, revise_tokens)
        sess.set_hotwords(self._hotword_ids(hotwords), hotword_boost)          # exactly this call's list (an empty one clears)
        sess.set_lm(lm, lm_weight, length_bonus)                               # ... and exactly this call's model
        done = [dict(ids=[], rows=[], logprob=[]) for _ in prepared]             # committed tokens: final when they are appended
        last, rtfs = {}, []
        for k in range(max(n_chunks)):
            live = [i for i in ids if k < n_chunks[i]]
            t0 = time.time()
            recs = sess.step_beam(block(k, live), live)
            ending = [i for i in live if k == n_chunks[i] - 1]
            fins = dict(zip(ending, sess.finish_beam(ending))) if ending else {}
            rtfs.append((time.time() - t0) / (chunk / self.sample_rate))
            for i, r in zip(live, recs):
                for c in [r["committed"]] + ([fins[i]["committed"]] if i in fins else []):
                    done[i]["ids"] += c["ids"].tolist(); done[i]["rows"] += c["row"].tolist(); done[i]["logprob"] += c["logprob"].tolist()
                if i in fins:
                    last[i] = (len(done[i]["ids"]) - len(fins[i]["committed"]["ids"]), fins[i]["pending"])
        cfg = sess.cfg
        row_s = cfg.lfr_n * cfg.hop_length / cfg.sample_rate
        out = []
        for i, (d, dur, n) in enumerate(zip(done, durs, n_chunks)):
            tok, lps = np.asarray(d["ids"], dtype=np.int32), np.asarray(d["logprob"], dtype=np.float32)
            keep = ~np.isin(tok, self.stop)
            o = dict(token_ids=tok[keep], text=decode_tokens(self.tokens[tok[keep]].tolist(), self.decode_mode), pieces=[])
            n_prefix, tails = last[i]
            o["nbest"] = []
            for t in tails:                                                      # full hypotheses: the committed prefix + the tail, with the final scores
                full = np.concatenate([tok[:n_prefix], t["ids"]]).astype(np.int32)
                full = full[~np.isin(full, self.stop)]
                o["nbest"].append({"token_ids": full, "text": decode_tokens(self.tokens[full].tolist(), self.decode_mode), "score": t["score"], "am_score": t["am_score"]})
            o["pieces"] = [o["text"]] if o["text"] else []
            if timestamps:
                spans = token_times(np.asarray(d["rows"], dtype=np.int64), n * sess.rows_per_chunk - sess.rows_carried, row_s, max_token_rows)
                o["tokens"] = [{"id": int(t), "text": str(self.tokens[int(t)]), "start": min(float(s), dur), "end": min(float(e), dur), "logprob": float(lp)}
                               for t, (s, e), lp in zip(tok, spans, lps) if int(t) not in self.stop]
            out.append(o)
        return out, {"rtf_per_chunk": rtfs, "chunks": max(n_chunks)}

    def transcribe_many(self, clips_int16: Sequence[np.ndarray], rng: np.random.Generator | None = None, timestamps: bool = False,
                        max_token_rows: int = 4, beam_size: int = 1, nbest: int = 1, hotwords=None, hotword_boost: float = 2.0, lm=None,
                        lm_weight: float = 0.5, length_bonus: float = 0.0, revise_tokens: int = 16, sample_rate: int | None = None, channels: int = 1):
        """Concurrent streams, one per clip (<= session.max_streams). Returns per clip dict(text, pieces, token_ids), and stats. timestamps=True takes the
        timed step and adds "tokens" per clip: one {"id", "text", "start", "end", "logprob"} per kept token, in seconds of the clip (paraformer.token_times
        over the stream's absolute fire rows, ends clipped to the clip's duration); records of stop ids are dropped with their ids.

        beam_size > 1, nbest > 1, hotwords or lm (the build's own mode): every chunk takes step_beam, and a clip is finished (finish_beam) behind its last
        chunk. A stream's last `revise_tokens` tokens stay open to revision; older ones are committed and final. text / token_ids (and "tokens") are the
        committed tokens, "nbest" the best hypotheses found, best first, each {"token_ids", "text", "score", "am_score"}. hotwords: token-id lists, or text
        spelled in the vocabulary; hotword_boost per matched token. lm: an lm.NgramLM: every token adds lm_weight * log P(token | history) + length_bonus.
        The call sets exactly its own list and model. Without any of these the call does exactly what it did before the mode existed.

        sample_rate / channels (the session's streaming input format): clips are int16 frames [n, channels] (or flat interleaved) at sample_rate; each is padded at
        that rate to the frames of a whole number of steps (pad_frames_to_steps) and every step is fed the frames it reads (session.input_frames), resampled per
        stream on the device. The clips' streams are reset in front of the call and behind it, and the session's format is restored. None: the default format."""
        chunk = self.sess.chunk
        if sample_rate is None:
            if channels != 1:
                raise ValueError("channels needs sample_rate: an input format is (sample rate, channels)")
            prepared = [pad_to_chunks(prepare_audio_input(np.asarray(c, dtype=np.int16).reshape(1, 1, -1), self.input_audio_dtype, audio_pcm_scale=self.audio_pcm_scale),
                                      chunk, rng)[0, 0] for c in clips_int16]
            n_chunks = [a.size // chunk for a in prepared]
            durs = [np.asarray(c).size / self.sample_rate for c in clips_int16]
            block = lambda k, live: np.stack([prepared[i][k * chunk:(k + 1) * chunk] for i in live])
            return self._transcribe_prepared(prepared, durs, n_chunks, block, timestamps, max_token_rows, beam_size, nbest, hotwords, hotword_boost, lm, lm_weight,
                                             length_bonus, revise_tokens)
        sess, model_rate = self.sess, int(self.sess.cfg.sample_rate)
        frames = [input_format.as_frames(c, channels) for c in clips_int16]
        durs = [f.shape[0] / float(sample_rate) for f in frames]
        padded = [pad_frames_to_steps(prepare_audio_input(f.reshape(1, 1, -1), self.input_audio_dtype, audio_pcm_scale=self.audio_pcm_scale,
                                                          channels=channels).reshape(-1, channels), chunk, sample_rate, model_rate, rng) for f in frames]
        prepared, n_chunks = [p for p, _ in padded], [c for _, c in padded]
        ids = list(range(len(prepared)))
        for i in ids:                                        # (a format is accepted only while no stream carries frames of another)
            sess.reset(i)

        def block(k, live):
            need, pitch = sess.input_frames(live)
            rows = np.zeros((len(live), pitch, channels), dtype=prepared[0].dtype)
            for j, i in enumerate(live):
                a0 = input_format.stream_start(chunk, sample_rate, model_rate, k)
                rows[j, :need[j]] = prepared[i][a0:a0 + need[j]]
            return rows
        with input_format.session_input_format(sess, sample_rate, channels):
            try:
                return self._transcribe_prepared(prepared, durs, n_chunks, block, timestamps, max_token_rows, beam_size, nbest, hotwords, hotword_boost, lm, lm_weight,
                                                 length_bonus, revise_tokens)
            finally:
                for i in ids:
                    sess.reset(i)

    def _transcribe_prepared(self, prepared, durs, n_chunks, block, timestamps, max_token_rows, beam_size, nbest, hotwords, hotword_boost, lm, lm_weight, length_bonus,
                             revise_tokens):
        chunk = self.sess.chunk
        if beam_size > 1 or nbest > 1 or bool(hotwords) or lm is not None:
            return self._transcribe_many_beam(prepared, durs, n_chunks, timestamps, max_token_rows, beam_size, nbest, hotwords, hotword_boost, lm, lm_weight,
                                              length_bonus, revise_tokens, block)
        ids = list(range(len(prepared)))
        for i in ids:
            self.sess.reset(i)
        out = [dict(pieces=[], token_ids=[]) for _ in prepared]
        timed = [dict(ids=[], rows=[], logprob=[]) for _ in prepared]
        rtfs = []
        for k in range(max(n_chunks)):
            live = [i for i in ids if k < n_chunks[i]]
            t0 = time.time()
            rows = block(k, live)
            if timestamps:
                recs = self.sess.step_timed(rows, live)
                fired = [r["ids"] for r in recs]
                for i, r in zip(live, recs):
                    timed[i]["ids"].append(r["ids"]); timed[i]["rows"].append(r["row"]); timed[i]["logprob"].append(r["logprob"])
            else:
                fired = self.sess.step(rows, live)
            rtfs.append((time.time() - t0) / (chunk / self.sample_rate))
            for i, tok in zip(live, fired):
                if tok.size:                                    # the decoder ran for this stream
                    tok = tok[~np.isin(tok, self.stop)]
                    out[i]["token_ids"].append(tok)
                    out[i]["pieces"].append(decode_tokens(self.tokens[tok].tolist(), self.decode_mode))
        for o in out:
            o["text"] = "".join(o["pieces"])
            o["token_ids"] = np.concatenate(o["token_ids"]) if o["token_ids"] else np.zeros(0, np.int32)
        if timestamps:
            cfg = self.sess.cfg
            row_s = cfg.lfr_n * cfg.hop_length / cfg.sample_rate
            for o, t, dur, n in zip(out, timed, durs, n_chunks):
                ids, rows, lps = (np.concatenate(t[k]) if t[k] else np.zeros(0) for k in ("ids", "rows", "logprob"))
                n_rows = n * self.sess.rows_per_chunk - self.sess.rows_carried          # rows integrated by the clip's last step
                spans = token_times(rows, n_rows, row_s, max_token_rows)
                o["tokens"] = [{"id": int(i), "text": str(self.tokens[int(i)]), "start": min(float(s), dur), "end": min(float(e), dur), "logprob": float(lp)}
                               for i, (s, e), lp in zip(ids, spans, lps) if int(i) not in self.stop]
        return out, {"rtf_per_chunk": rtfs, "chunks": max(n_chunks)}

    def transcribe(self, audio_int16: np.ndarray, rng: np.random.Generator | None = None):
        out, stats = self.transcribe_many([audio_int16], rng)
        return out[0], stats
