#!/usr/bin/env python
"""Real-checkpoint transcript harness: wav files + a converted model folder -> a token dump, and a
comparator for two dumps -- the piece that closes "token-for-token against the reference's ONNX CPUExecutionProvider run" on a
machine that has the checkpoints (none exist offline; tests/test_transcribe_cpu.py round-trips synthetic models through it).

    # 1. once: checkpoint -> model folder
    python tools/convert_checkpoint.py --family whisper --checkpoint model.safetensors --out Whisper_MI355X
    # 2. on the MI355X: wavs -> ours.json
    python tools/transcribe.py run --family whisper --model Whisper_MI355X --tokenizer whisper-large-v3/ --language en \
        --wav Test_Examples/en/test_sample.wav Test_Examples/zh/zh_1.wav --precision f32 --out ours.json
    # 3. on any box with onnxruntime + the exported graphs: make the reference dump (same schema; `reference-stub` prints the few
    #    lines to paste at the end of Inference_*_ONNX.py), then
    python tools/transcribe.py compare ours.json reference.json

Dump schema: {"family", "precision", "files": [{"path", "n_samples", "language", "windows": [[token ids], ...], "text"}]}.
Audio ingest = audio_io.read_wav_int16 (the reference's pydub calls restated on stdlib wave / audioop), or with --device-resample the wav's own frames at
its own rate and channel count, resampled by the session on the device (the build's own mode: not sample-exact against the reference); detokenisation: SentencePiece
(SenseVoice, :305), vocabulary join (Paraformer), `tokenizer._decode_asr` (Whisper, Inference_Whisper_ONNX.py:702-715),
`tokenizer.decode(..., skip_special_tokens=True)` + parse_asr_output (Qwen3-ASR, Inference_Qwen_ASR_ONNX.py:746-752) -- each only
when a tokenizer is given; the token ids are what is compared.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "automatic-speech-recognition-asr-onnx_amd"


def _m(name):
    return importlib.import_module(f"{PKG}.{name}")


def whisper_text(tokenizer, ids, remove_repeats=True):
    """Inference_Whisper_ONNX.py:702-715: tail-repeat guard, then the HF tokenizer's ASR decoder."""
    arr = np.asarray(ids, dtype=np.int64)
    if remove_repeats:
        arr = np.asarray(_m("whisper").remove_repeated_parts(arr.tolist(), 3, arr.shape[-1]), dtype=np.int64)
    text, _ = tokenizer._decode_asr([{"tokens": arr.reshape(1, -1)}], return_timestamps=None, return_language=None, time_precision=0)
    return text


def parse_hotword_file(path):
    """One phrase per line: token ids separated by blanks or commas ("4125 77, 9") or text (encoded by the transcriber's tokenizer). Empty lines and lines
    starting with # are skipped. Returns a list of id lists / strings."""
    phrases = []
    with open(path, encoding="utf-8") as f:
        for line in f:
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            parts = line.replace(",", " ").split()
            if all(q.lstrip("-").isdigit() for q in parts):
                phrases.append([int(q) for q in parts])
            else:
                phrases.append(line)
    return phrases


def nar_options(a):
    """The --nar-* flags (Paraformer's beam search over the decoder's token rows), checked before a model is opened: None when none is given, else
    dict(beam_size, nbest, hotwords, hotword_boost, lm_file, lm_weight, length_bonus) as ParaformerTranscriber.transcribe takes them (lm_file still a path)."""
    beam, nbest = getattr(a, "nar_beam", None), getattr(a, "nar_nbest", None)
    hot_file, boost = getattr(a, "nar_hotwords", None), getattr(a, "nar_hotword_boost", None)
    lm_file, weight, bonus = getattr(a, "nar_lm", None), getattr(a, "nar_lm_weight", None), getattr(a, "nar_length_bonus", None)
    if all(v is None for v in (beam, nbest, hot_file, boost, lm_file, weight, bonus)):
        return None
    if a.family != "paraformer":
        raise SystemExit("--nar-beam / --nar-nbest / --nar-hotwords / --nar-hotword-boost / --nar-lm / --nar-lm-weight / --nar-length-bonus exist for "
                         "--family paraformer only")
    if boost is not None and not hot_file:
        raise SystemExit("--nar-hotword-boost needs --nar-hotwords FILE")
    if (weight is not None or bonus is not None) and not lm_file:
        raise SystemExit("--nar-lm-weight / --nar-length-bonus need --nar-lm FILE.arpa")
    if weight is not None and not weight >= 0:
        raise SystemExit("--nar-lm-weight %r: expected a weight >= 0" % weight)
    for flag, path in (("--nar-hotwords", hot_file), ("--nar-lm", lm_file)):
        if path and not os.path.isfile(path):
            raise SystemExit("%s %s: no such file" % (flag, path))
    nbest = 1 if nbest is None else nbest
    beam = max(nbest, 1) if beam is None else beam                      # (--nar-nbest alone: the narrowest beam that can return them)
    if not 1 <= nbest <= beam <= 16:
        raise SystemExit("--family paraformer: --nar-beam 1..16 and --nar-nbest 1..beam (got --nar-beam %d --nar-nbest %d)" % (beam, nbest))
    return {"beam_size": beam, "nbest": nbest, "hotwords": parse_hotword_file(hot_file) if hot_file else None, "hotword_boost": 2.0 if boost is None else boost,
            "lm_file": lm_file, "lm_weight": 0.5 if weight is None else weight, "length_bonus": 0.0 if bonus is None else bonus}


def decoder_lm_options(a):
    """The --decoder-lm* flags of the autoregressive families: None when none is given, else dict(lm_file, lm_weight, length_bonus, lm_topk) as
    WhisperTranscriber / QwenAsrTranscriber take them (lm_file still a path)."""
    lm_file, weight = getattr(a, "decoder_lm", None), getattr(a, "decoder_lm_weight", None)
    bonus, topk = getattr(a, "decoder_length_bonus", None), getattr(a, "decoder_lm_topk", None)
    if not lm_file and weight is None and bonus is None and topk is None:
        return None
    if a.family not in ("whisper", "qwen_asr"):
        raise SystemExit("--decoder-lm / --decoder-lm-weight / --decoder-length-bonus / --decoder-lm-topk exist for --family whisper and --family qwen_asr only "
                         "(SenseVoice: --lm, Paraformer: --nar-lm)")
    if not lm_file:
        raise SystemExit("--decoder-lm-weight / --decoder-length-bonus / --decoder-lm-topk need --decoder-lm FILE.arpa")
    if not os.path.isfile(lm_file):
        raise SystemExit("--decoder-lm %s: no such file" % lm_file)
    topk = 16 if topk is None else topk
    if not 1 <= topk <= 32 or topk < a.beam:
        raise SystemExit("--decoder-lm-topk 1..32 and at least --beam (got --decoder-lm-topk %d --beam %d)" % (topk, a.beam))
    return {"lm_file": lm_file, "lm_weight": 0.5 if weight is None else weight, "length_bonus": 0.0 if bonus is None else bonus, "lm_topk": topk}


def load_decoder_lm(opts, tok):
    """The transcribers' lm keywords from decoder_lm_options: ARPA words are token ids, or tokens of the tokenizer's vocabulary when one is loaded."""
    if not opts:
        return {}
    NgramLM = _m("lm").NgramLM
    if tok is None:
        lm = NgramLM.from_arpa(opts["lm_file"])
    else:
        vocab = tok.get_vocab()
        lm = NgramLM.from_arpa(opts["lm_file"], token_to_id=lambda piece: vocab.get(piece))
    return {"lm": lm, "lm_weight": opts["lm_weight"], "length_bonus": opts["length_bonus"], "lm_topk": opts["lm_topk"]}


def vad_params(a):
    """--vad and its options -> engine.VadParams, or None without --vad."""
    if not getattr(a, "vad", False):
        if any(getattr(a, k, None) is not None for k in ("vad_margin_db", "vad_min_pause", "vad_pad", "vad_max_seconds", "vad_dump")):
            raise SystemExit("--vad-margin-db / --vad-min-pause / --vad-pad / --vad-max-seconds / --vad-dump need --vad")
        return None
    if a.sliding_window:
        raise SystemExit("--vad cuts the file at its pauses: it does not combine with --sliding-window")
    if getattr(a, "condition_on_previous_text", False):
        raise SystemExit("--vad runs a file's segments as batches: it does not combine with --condition-on-previous-text")
    kw = {k: v for k, v in (("margin_db", a.vad_margin_db), ("min_pause", a.vad_min_pause), ("pad", a.vad_pad), ("max_seconds", a.vad_max_seconds)) if v is not None}
    return _m("engine").VadParams(**kw)


def _plain(v):
    """A transcribe_long record as JSON takes it."""
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (np.integer,)):
        return int(v)
    if isinstance(v, (np.floating,)):
        return float(v)
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


def vad_file_record(p, about, r, language, rtf):
    """The dump's entry for a file transcribed with --vad: `windows` holds the segments' ids, `segments` every segment's record in seconds of the file."""
    return {"path": p, **about, "language": language, "windows": [np.asarray(g["token_ids"]).astype(int).tolist() for g in r["segments"]], "text": r.get("text"),
            "rtf": rtf, "vad": True, "speech_seconds": r["speech_seconds"], "audio_seconds": r["audio_seconds"], "segments": _plain(r["segments"])}


def read_audio(a, path, reference_ingest):
    """One wav -> (int16 audio, the transcriber's format arguments, what the dump records about it). Default: reference_ingest(), mono PCM at the model's rate,
    converted on the host as the reference's pydub ingest does. --device-resample: the file's own frames [n, channels] at its own rate; the session resamples
    on the device."""
    if getattr(a, "device_resample", False):
        frames, rate, channels = _m("audio_io").read_wav_native(path)
        return frames, {"sample_rate": rate, "channels": channels}, {"n_samples": int(frames.shape[0]), "sample_rate": rate, "channels": channels}
    pcm = reference_ingest()
    return pcm, {}, {"n_samples": int(pcm.size)}


def run(a) -> dict:
    shim, eng, audio_io, cfgm = _m("ort_shim"), _m("engine"), _m("audio_io"), _m("config")
    prec = 1 if a.precision == "f32" else 0
    if (a.precision == "fp8mm" and a.family != "whisper") or (a.precision in ("fp8w", "mxfp4w") and a.family not in ("whisper", "qwen_asr")):
        raise SystemExit("--precision %s exists for --family whisper%s only" % (a.precision, " / qwen_asr" if a.precision == "fp8w" else ""))
    timestamps = getattr(a, "timestamps", False)
    word_ts = getattr(a, "word_timestamps", False)
    if word_ts and a.family != "whisper":
        raise SystemExit("--word-timestamps exists for --family whisper only")
    if timestamps and a.family not in ("sensevoice", "paraformer", "whisper"):
        raise SystemExit("--timestamps exists for --family sensevoice / paraformer (per token) and --family whisper (per segment), not for --family qwen_asr")
    if (getattr(a, "initial_prompt_ids", None) or getattr(a, "condition_on_previous_text", False)) and a.family != "whisper":
        raise SystemExit("--initial-prompt-ids / --condition-on-previous-text exist for --family whisper only")
    nbest, hot_file = getattr(a, "nbest", 1), getattr(a, "hotwords", None)
    if (nbest > 1 or hot_file) and a.family != "sensevoice":
        raise SystemExit("--nbest / --hotwords exist for --family sensevoice only")
    lm_file, lm_weight, length_bonus = getattr(a, "lm", None), getattr(a, "lm_weight", None), getattr(a, "length_bonus", None)
    if (lm_file or lm_weight is not None or length_bonus is not None) and a.family != "sensevoice":
        raise SystemExit("--lm / --lm-weight / --length-bonus exist for --family sensevoice only")
    if (lm_weight is not None or length_bonus is not None) and not lm_file:
        raise SystemExit("--lm-weight / --length-bonus need --lm FILE.arpa")
    if lm_file and not os.path.isfile(lm_file):
        raise SystemExit("--lm %s: no such file" % lm_file)
    sv_beam = a.family == "sensevoice" and (a.beam > 1 or nbest > 1 or bool(hot_file) or bool(lm_file))
    if sv_beam and timestamps:
        raise SystemExit("--timestamps is not available with --beam / --nbest / --hotwords / --lm (beam hypotheses carry no time spans)")
    if sv_beam and not 1 <= nbest <= a.beam <= 16:
        raise SystemExit("--family sensevoice: --beam 1..16 and --nbest 1..beam (got --beam %d --nbest %d)" % (a.beam, nbest))
    nar = nar_options(a)
    dec_hot_file, dec_hot_boost = getattr(a, "decoder_hotwords", None), getattr(a, "decoder_hotword_boost", 2.0)
    if dec_hot_file and a.family not in ("whisper", "qwen_asr"):
        raise SystemExit("--decoder-hotwords exists for --family whisper and --family qwen_asr only (SenseVoice: --hotwords)")
    dec_hot = parse_hotword_file(dec_hot_file) if dec_hot_file else None
    if dec_hot and any(isinstance(p, str) for p in dec_hot) and not a.tokenizer:
        raise SystemExit("--decoder-hotwords: text phrases need --tokenizer (or give token ids)")
    dec_lm = decoder_lm_options(a)
    bundle = {"sensevoice": "SenseVoiceSmall", "paraformer": "Paraformer", "whisper": "Whisper", "qwen_asr": "Qwen_ASR"}[a.family]
    if not any(os.path.isfile(os.path.join(a.model, bundle + ext)) for ext in (".asrmodel", ".onnx")):
        raise SystemExit("--model %s holds no %s.asrmodel: it is not a --family %s folder" % (a.model, bundle, a.family))
    fallback = getattr(a, "temperature_fallback", None)
    scores = bool(getattr(a, "token_scores", False)) or bool(fallback)
    if fallback and a.family != "whisper":
        raise SystemExit("--temperature-fallback exists for --family whisper only")
    if scores and a.family not in ("whisper", "qwen_asr"):
        raise SystemExit("--token-scores exists for --family whisper and --family qwen_asr only")
    if scores and a.beam > 1:
        raise SystemExit("--token-scores / --temperature-fallback need --beam 1 (the beam search reports a score per hypothesis)")
    files = []
    vad = vad_params(a)
    if a.family in ("sensevoice", "paraformer"):
        mod = _m(a.family)
        if a.family == "sensevoice":
            tr = mod.SenseVoiceTranscriber(a.model, target_language=a.language, tokenizer_path=a.tokenizer, device_type="cuda")
        else:
            tr = mod.ParaformerTranscriber(a.model, vocab_path=a.tokenizer, device_type="cuda")
        lm = tr.load_lm(lm_file) if lm_file else None
        nar_kw = None
        if nar:                             # Paraformer: beam search over the decoder's token rows; its hypotheses keep the CIF times, so --timestamps combines
            nar_kw = {k: v for k, v in nar.items() if k != "lm_file"}
            nar_kw["lm"] = tr.load_lm(nar["lm_file"]) if nar["lm_file"] else None
        for p in a.wav:
            pcm, fmt, about = read_audio(a, p, lambda: audio_io.read_wav_int16(p, tr.sample_rate, exact_width=a.strict_wav))
            if vad is not None:             # cut at the pauses: the same options, the segments as ragged batches
                if nar_kw:
                    kw = dict(timestamps=timestamps, **nar_kw)
                elif sv_beam:
                    kw = dict(beam_size=a.beam, nbest=nbest, hotwords=parse_hotword_file(hot_file) if hot_file else None, hotword_boost=getattr(a, "hotword_boost", 2.0),
                              lm=lm, lm_weight=0.5 if lm_weight is None else lm_weight, length_bonus=0.0 if length_bonus is None else length_bonus)
                else:
                    kw = dict(timestamps=timestamps)
                r = tr.transcribe_long(pcm, vad=vad, **kw, **fmt)
                files.append(vad_file_record(p, about, r, r.get("language", a.language), r["rtf"]))
                continue
            if nar_kw:
                r = tr.transcribe(pcm, sliding_window=a.sliding_window, timestamps=timestamps, **nar_kw, **fmt)
            elif timestamps:
                r = tr.transcribe(pcm, sliding_window=a.sliding_window, timestamps=True, **fmt)
            elif sv_beam:
                r = tr.transcribe(pcm, sliding_window=a.sliding_window, beam_size=a.beam, nbest=nbest, hotwords=parse_hotword_file(hot_file) if hot_file else None,
                                  hotword_boost=getattr(a, "hotword_boost", 2.0), lm=lm, lm_weight=0.5 if lm_weight is None else lm_weight,
                                  length_bonus=0.0 if length_bonus is None else length_bonus, **fmt)
            else:
                r = tr.transcribe(pcm, sliding_window=a.sliding_window, **fmt)
            files.append({"path": p, **about, "language": r.get("language", a.language),
                          "windows": [np.asarray(w).reshape(-1).astype(int).tolist() for w in r["token_ids"]], "text": r.get("text"), "rtf": r["rtf"]})
            if timestamps:
                files[-1]["tokens"] = r["tokens"]
            if sv_beam:                     # per window the hypotheses found, best first (windows[k] is nbest[k][0])
                files[-1]["nbest"] = [[{"ids": np.asarray(h["token_ids"]).astype(int).tolist(), "score": h["score"], "ctc_score": h["ctc_score"], "text": h["text"]}
                                       for h in win] for win in r["nbest"]]
            if nar_kw and "nbest" in r:     # the same for Paraformer: am_score in place of ctc_score, and every hypothesis' token times with --timestamps
                files[-1]["nbest"] = [[dict({"ids": np.asarray(h["token_ids"]).astype(int).tolist(), "score": h["score"], "am_score": h["am_score"], "text": h["text"]},
                                            **({"tokens": h["tokens"]} if timestamps else {})) for h in win] for win in r["nbest"]]
    elif a.family == "whisper":
        info, blob = shim.load_model(os.path.join(a.model, "Whisper.asrmodel"))
        cfg = cfgm.WhisperConfig(**info["config"])
        ckm = _m("checkpoints")
        bundle_prec = int(info.get("precision", prec))
        if a.precision in ("fp8w", "fp8mm", "mxfp4w"):       # opt-in: decoder projections + cross-K/V as e4m3 bytes over a bf16 bundle; fp8mm also runs the encoder FFN pair on the FP8 matrix pipe (include/asr_mi355x.h)
            if bundle_prec != 0:
                raise SystemExit("--precision %s needs a bf16 bundle (convert the checkpoint with --precision bf16)" % a.precision)
            bundle_prec = {"fp8w": 2, "fp8mm": 3, "mxfp4w": 4}[a.precision]
        sess = eng.WhisperSession(cfg, blob, bundle_prec, audio_dtype=shim.bundle_audio_dtype(info))      # the bundle's INPUT_AUDIO_DTYPE
        tok = None
        if a.tokenizer:
            from transformers import AutoTokenizer
            tok = AutoTokenizer.from_pretrained(a.tokenizer)
        # word timestamps align on the checkpoint's own heads (the converter copied generation_config.json's list into the bundle); without one, the fallback
        heads = json.loads(info.get("metadata", {}).get("alignment_heads", "null")) if word_ts else None
        tr = _m("whisper").WhisperTranscriber(cfg, sess, suppress_tokens=ckm.whisper_suppress_tokens(cfg), detect_language=a.language == "auto",
                                              repeat_penalty=a.repeat_penalty, beam_size=a.beam, timestamps=timestamps, word_timestamps=word_ts,
                                              alignment_heads=heads, piece_decoder=tok.decode if tok is not None and (word_ts or scores) else None,
                                              token_scores=scores, temperature_fallback=fallback, hotwords=dec_hot, hotword_boost=dec_hot_boost,
                                              hotword_encoder=(lambda t: tok.encode(t, add_special_tokens=False)) if tok is not None else None,
                                              initial_prompt=parse_prompt_ids_file(a.initial_prompt_ids) if getattr(a, "initial_prompt_ids", None) else None,
                                              condition_on_previous_text=bool(getattr(a, "condition_on_previous_text", False)), **load_decoder_lm(dec_lm, tok))
        lang_id = None
        if a.language != "auto":
            if tok is None:
                raise SystemExit("--language other than 'auto' needs --tokenizer (language token ids come from its vocabulary)")
            lang_id = tok.convert_tokens_to_ids(f"<|{a.language}|>")
        for p in a.wav:
            pcm, fmt, about = read_audio(a, p, lambda: audio_io.read_wav_int16(p, cfg.sample_rate, exact_width=a.strict_wav))
            if vad is not None:             # cut at the pauses: the transcriber's settings as they are, the segments as clip batches
                r, stat = tr.transcribe_long(pcm, vad=vad, language_id=lang_id, **fmt)
                if tok is not None:
                    for g in r["segments"]:
                        g["text"] = whisper_text(tok, np.asarray(g["token_ids"]).tolist(), remove_repeats=False)
                    r["text"] = "".join(g["text"] for g in r["segments"])
                files.append(vad_file_record(p, about, r, a.language, stat["rtf"]))
                continue
            # the reference's per-file loop (Inference_Whisper_ONNX.py:741-829): SLIDING_WINDOW stride, zero-padded tail, probe on window 0 only,
            # a no-speech verdict aborts the file, later windows reuse window 0's language
            r, stat = tr.transcribe_file(pcm, language_id=lang_id, sliding_window=a.sliding_window, **fmt)
            ids = r["windows"]
            flat = r["tokens"].tolist() if timestamps else [t for w in ids for t in w]      # timestamp mode: the text ids, repeat guard not applied
            text = None
            if tok is not None:
                text = "[no speech detected]" if r["no_speech"] else (whisper_text(tok, flat, remove_repeats=not (timestamps or word_ts or scores)) if flat else "")
            files.append({"path": p, **about, "language": a.language, "windows": ids, "text": text, "rtf": stat["rtf"],
                          "language_ids": [r["language_id"]] * len(ids), "no_speech_prob": [r["no_speech_prob"]], "no_speech": r["no_speech"]})
            if tr.initial_prompt or tr.condition_on_previous_text:        # the build's own mode: the prompt length each window was decoded behind
                files[-1]["prompt_len"] = r["prompt_len"]
            if scores:                      # the build's own mode: one log-probability per entry of r["tokens"], OpenAI's avg_logprob / compression ratio per file and per window
                files[-1].update(tokens=r["tokens"].astype(int).tolist(), token_logprobs=[float(v) for v in r["token_logprobs"]], avg_logprob=r["avg_logprob"],
                                 compression_ratio=r["compression_ratio"], temperature=r["temperature"], window_scores=r["window_scores"])
            if word_ts and not r["no_speech"]:          # the build's own mode: seconds from the file's start, one pair per text id; words with --tokenizer
                files[-1]["token_times"] = [[float(s), float(e)] for s, e in r["token_times"]]
                if "words" in r:
                    files[-1]["words"] = r["words"]
                    for w in r["words"]:
                        print("%8.2f %8.2f %s" % (w["start"], w["end"], w["word"]))
            if timestamps:                  # the build's own mode: windows keep every id, <|t.tt|> included; segments in seconds from the file's start
                files[-1]["segments"] = [dict(seg, text=whisper_text(tok, seg["tokens"], remove_repeats=False)) if tok is not None else seg
                                         for seg in r["segments"]]
    elif a.family == "qwen_asr":
        info, blob = shim.load_model(os.path.join(a.model, "Qwen_ASR.asrmodel"))
        cfg = cfgm.QwenAsrConfig(**info["config"])
        bundle_prec = int(info.get("precision", prec))
        if a.precision in ("fp8w", "mxfp4w"):      # opt-in: the decoder's projections as e4m3 bytes / MXFP4 nibbles over a bf16 bundle (include/asr_mi355x.h)
            if bundle_prec != 0:
                raise SystemExit("--precision %s needs a bf16 bundle (convert the checkpoint with --precision bf16)" % a.precision)
            bundle_prec = 2 if a.precision == "fp8w" else 4
        sess = eng.QwenAsrSession(cfg, blob, bundle_prec, audio_dtype=shim.bundle_audio_dtype(info))
        tok = None
        if a.tokenizer:
            from transformers import AutoTokenizer
            tok = AutoTokenizer.from_pretrained(a.tokenizer)
        tr = _m("qwen_asr").QwenAsrTranscriber(cfg, sess, info["metadata"], tokenizer=tok, repeat_penalty=a.repeat_penalty, beam_size=a.beam,
                                               token_scores=scores, hotwords=dec_hot, hotword_boost=dec_hot_boost, **load_decoder_lm(dec_lm, tok))
        for p in a.wav:
            pcm, fmt, about = read_audio(a, p, lambda: audio_io.read_wav_int16(p, cfg.sample_rate, exact_width=a.strict_wav))
            if vad is not None:
                r, stat = tr.transcribe_long(pcm, vad=vad, language_prompt="" if a.language == "auto" else a.language, **fmt)
                files.append(vad_file_record(p, about, r, a.language, stat["rtf"]))
                continue
            out, stat = tr.transcribe([pcm], language_prompts=("" if a.language == "auto" else a.language,), **fmt)
            r = out[0]
            files.append({"path": p, **about, "language": r.get("language") or a.language,
                          "windows": [np.asarray(r["tokens"]).astype(int).tolist()], "text": r.get("text"), "rtf": stat["rtf"]})
            if scores:
                files[-1].update(token_logprobs=[float(v) for v in r["token_logprobs"]], avg_logprob=r["avg_logprob"])
    else:
        raise SystemExit(a.family)
    if vad is not None and getattr(a, "vad_dump", None):
        with open(a.vad_dump, "w", encoding="utf-8") as f:
            json.dump({"files": [{"path": r["path"], "audio_seconds": r["audio_seconds"], "speech_seconds": r["speech_seconds"],
                                  "segments": [[g["start"], g["end"]] for g in r["segments"]]} for r in files]}, f, indent=1)
    return {"family": a.family, "precision": a.precision, "engine": "automatic-speech-recognition-asr-onnx_amd (MI355X)", "files": files}


def compare(ours: dict, ref: dict) -> dict:
    """Token-for-token comparison of two dumps, file by file and window by window (files are matched by base name)."""
    by_name = {os.path.basename(f["path"]): f for f in ref["files"]}
    rep, ok = [], True
    for f in ours["files"]:
        name = os.path.basename(f["path"])
        g = by_name.get(name)
        if g is None:
            rep.append({"file": name, "status": "missing in reference"})
            ok = False
            continue
        wa, wb = f["windows"], g["windows"]
        item = {"file": name, "windows": len(wa), "reference_windows": len(wb), "mismatches": []}
        if len(wa) != len(wb):
            ok = False
        for i, (x, y) in enumerate(zip(wa, wb)):
            if list(x) != list(y):
                ok = False
                first = next((k for k, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
                item["mismatches"].append({"window": i, "first_difference_at": first, "ours": list(x)[first:first + 8], "reference": list(y)[first:first + 8],
                                           "len_ours": len(x), "len_reference": len(y)})
        item["status"] = "equal" if not item["mismatches"] and len(wa) == len(wb) else "DIFFERENT"
        if f.get("text") is not None and g.get("text") is not None:
            item["text_equal"] = f["text"] == g["text"]
        rep.append(item)
    return {"token_for_token": ok, "files": rep}


REFERENCE_STUB = '''# paste at the end of the reference's Inference_<Family>_ONNX.py (after its transcription loop) to write the dump
# `tools/transcribe.py compare` reads; `all_windows` = the per-window id lists the script already collects.
import json
json.dump({"family": "<family>", "precision": "f32", "engine": "onnxruntime CPUExecutionProvider",
           "files": [{"path": test_audio, "n_samples": int(audio_len), "language": LANGUAGE,
                      "windows": [[int(t) for t in w] for w in all_windows], "text": text}]},
          open("reference.json", "w"), ensure_ascii=False, indent=1)
'''


def parse_prompt_ids_file(path):
    """--initial-prompt-ids FILE: text token ids separated by blanks, commas or line ends."""
    with open(path, encoding="utf-8") as f:
        ids = [int(t) for t in f.read().replace(",", " ").split()]
    if not ids:
        raise SystemExit(f"--initial-prompt-ids: {path} holds no ids")
    return ids


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--family", required=True, choices=("sensevoice", "paraformer", "whisper", "qwen_asr"))
    r.add_argument("--model", required=True, help="folder written by tools/convert_checkpoint.py")
    r.add_argument("--wav", nargs="+", required=True)
    r.add_argument("--language", default="auto")
    r.add_argument("--tokenizer", help="SentencePiece model (SenseVoice), vocabulary file (Paraformer) or HF tokenizer directory (Whisper / Qwen3-ASR)")
    r.add_argument("--precision", default="f32", choices=("bf16", "f32", "fp8w", "fp8mm", "mxfp4w"),
                   help="f32 = verification mode (the mode whose tokens equal the reference's); fp8w = Whisper / Qwen3-ASR, opt-in e4m3 decoder weights (Whisper: and cross-K/V); fp8mm = fp8w + encoder FFN on the FP8 matrix pipe; mxfp4w = fp8w with the Whisper decoder weights as OCP MXFP4")
    r.add_argument("--sliding-window", type=int, default=0)
    r.add_argument("--repeat-penalty", type=float, default=1.0, help="1.0 = plain greedy (the comparison default); the reference scripts default to 0.8")
    r.add_argument("--beam", type=int, default=1, help="beam width (Whisper, Qwen3-ASR; 1 = greedy); > 1 takes the first hypothesis and needs --repeat-penalty 1. "
                        "SenseVoice: CTC prefix beam search over the beam best tokens of every frame (1..16)")
    r.add_argument("--nbest", type=int, default=1, help="SenseVoice: keep the N best hypotheses of every window in the dump (1..beam), with their scores")
    r.add_argument("--hotwords", metavar="FILE", help="SenseVoice: phrases the beam search favours, one per line: token ids, or text with --tokenizer")
    r.add_argument("--hotword-boost", type=float, default=2.0, help="SenseVoice: log-probability bonus per matched hotword token")
    r.add_argument("--lm", metavar="FILE.arpa", help="SenseVoice: back-off n-gram language model (ARPA; words are token ids, or pieces with --tokenizer) fused "
                        "into the beam search, which it implies")
    r.add_argument("--lm-weight", type=float, default=None, help="SenseVoice: weight of the language model's log-probability (default 0.5)")
    r.add_argument("--length-bonus", type=float, default=None, help="SenseVoice: bonus per token with --lm (default 0)")
    r.add_argument("--nar-beam", type=int, default=None, metavar="N", help="Paraformer: beam search over the decoder's token rows, N live hypotheses (1..16; default: "
                        "--nar-nbest, else 1); every hypothesis has one token per CIF fire, so --timestamps combines with it")
    r.add_argument("--nar-nbest", type=int, default=None, metavar="M", help="Paraformer: keep the M best hypotheses of every window in the dump (1..beam), with their scores")
    r.add_argument("--nar-hotwords", metavar="FILE", help="Paraformer: phrases the beam search favours, one per line: token ids, or text spelled in the vocabulary")
    r.add_argument("--nar-hotword-boost", type=float, default=None, metavar="X", help="Paraformer: log-probability bonus per matched hotword token (default 2.0)")
    r.add_argument("--nar-lm", metavar="FILE.arpa", help="Paraformer: back-off n-gram language model (ARPA; words are token ids or vocabulary entries) fused into the "
                        "beam search, which it implies")
    r.add_argument("--nar-lm-weight", type=float, default=None, metavar="X", help="Paraformer: weight of the language model's log-probability (default 0.5)")
    r.add_argument("--nar-length-bonus", type=float, default=None, metavar="Y", help="Paraformer: bonus per token with --nar-lm (default 0)")
    r.add_argument("--decoder-hotwords", metavar="FILE", help="Whisper, Qwen3-ASR: phrases the decoder favours (greedy, sampling and --beam alike), one per line: "
                        "token ids, or text with --tokenizer (boosted in both spellings, at the start of the text and inside it)")
    r.add_argument("--decoder-hotword-boost", type=float, default=2.0, help="Whisper, Qwen3-ASR: logit / log-probability bonus per matched hotword token")
    r.add_argument("--decoder-lm", metavar="FILE.arpa", help="Whisper, Qwen3-ASR: back-off n-gram language model (ARPA; words are token ids, or tokens of the "
                   "vocabulary with --tokenizer) fused into the selection head and --beam (shallow fusion over the best --decoder-lm-topk columns)")
    r.add_argument("--decoder-lm-weight", type=float, default=None, metavar="X", help="Whisper, Qwen3-ASR: weight of the model's log-probability (default 0.5)")
    r.add_argument("--decoder-length-bonus", type=float, default=None, metavar="Y", help="Whisper, Qwen3-ASR: bonus per token with --decoder-lm (default 0)")
    r.add_argument("--decoder-lm-topk", type=int, default=None, metavar="M", help="Whisper, Qwen3-ASR: candidate columns per step, 1..32 and at least --beam (default 16)")
    r.add_argument("--timestamps", action="store_true", help="SenseVoice: add each token's start / end (seconds) and mean frame log-probability to the dump; Paraformer: each token's start / end from its CIF fire row and its log-probability; Whisper: decode with timestamp tokens and add "
                        "segments (start / end in seconds, token ids, text with --tokenizer)")
    r.add_argument("--word-timestamps", action="store_true", help="Whisper: add each text token's start / end in seconds (cross-attention DTW on the bundle's "
                        "alignment heads) to the dump; with --tokenizer also words, printed as they are found")
    r.add_argument("--token-scores", action="store_true", help="Whisper, Qwen3-ASR: add each token's log-probability and the average (the stop pick included) to the "
                        "dump; Whisper with --tokenizer also the compression ratio, and with --word-timestamps a probability per word")
    r.add_argument("--temperature-fallback", type=float, nargs="+", metavar="T", help="Whisper: decode an utterance again by sampling at these temperatures, in "
                        "order, while its average log-probability is below -1.0 or its compression ratio above 2.4 (e.g. 0.2 0.4 0.6 0.8 1.0); implies --token-scores")
    r.add_argument("--initial-prompt-ids", metavar="FILE", help="Whisper: text token ids (blank- or comma-separated) put in front of every window's prompt behind "
                        "<|startofprev|>: a glossary or style hint (OpenAI's initial_prompt)")
    r.add_argument("--condition-on-previous-text", action="store_true", help="Whisper: run a file's windows in order, each prompted with the text ids of the windows "
                        "before it; with --temperature-fallback the context is dropped after a window decoded above temperature 0.5")
    r.add_argument("--device-resample", action="store_true", help="feed each wav at its own sample rate and channel count and let the session resample on the "
                   "device (set_input_format: low-pass polyphase filter, channel mean). The build's own mode: without it the ingest is the reference's host-side "
                   "conversion, sample for sample")
    r.add_argument("--vad", action="store_true", help="cut each file at its pauses with the device energy detector (transcribe_long) instead of at fixed windows; "
                   "the dump gains `segments` in seconds of the file. Without it nothing changes")
    r.add_argument("--vad-margin-db", type=float, default=None, metavar="DB", help="--vad: threshold above the noise floor (default 9)")
    r.add_argument("--vad-min-pause", type=float, default=None, metavar="S", help="--vad: shorter pauses between speech are bridged (default 0.5)")
    r.add_argument("--vad-pad", type=float, default=None, metavar="S", help="--vad: every segment grows by this much on both sides (default 0.1)")
    r.add_argument("--vad-max-seconds", type=float, default=None, metavar="S", help="--vad: longest segment (default: the family's window)")
    r.add_argument("--vad-dump", metavar="FILE", default=None, help="--vad: also write the segments' [start, end] per file as JSON")
    r.add_argument("--out", required=True)
    r.add_argument("--any-wav-width", dest="strict_wav", action="store_false",
                   help="accept 8 / 24 / 32-bit wav (rescaled to int16); by default only 16-bit wav is taken: the only width whose samples equal the reference's, "
                        "which is what a dump that `compare` will judge must be made from")
    c = sub.add_parser("compare")
    c.add_argument("ours")
    c.add_argument("reference")
    sub.add_parser("reference-stub")
    return ap


def main():
    a = build_parser().parse_args()
    if a.cmd == "run":
        dump = run(a)
        with open(a.out, "w", encoding="utf-8") as f:
            json.dump(dump, f, ensure_ascii=False, indent=1)
        print(f"wrote {a.out}: {sum(len(x['windows']) for x in dump['files'])} windows over {len(dump['files'])} files")
    elif a.cmd == "compare":
        rep = compare(json.load(open(a.ours, encoding="utf-8")), json.load(open(a.reference, encoding="utf-8")))
        print(json.dumps(rep, ensure_ascii=False, indent=1))
        sys.exit(0 if rep["token_for_token"] else 1)
    else:
        print(REFERENCE_STUB)


if __name__ == "__main__":
    main()
