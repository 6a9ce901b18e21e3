#!/usr/bin/env python
"""Word timestamps for one wav and its transcript.

    python tools/align.py --model Qwen_ForcedAligner_MI355X --wav clip.wav --text transcript.txt [--language English] [--tokenizer DIR] > words.json
    python tools/align.py --family sensevoice --model SenseVoice_MI355X --wav clip.wav --text "the transcript" --tokenizer bpe.model [--language en] > words.json

--family qwen_aligner (default): the Qwen3-ForcedAligner on the native session. --model is a folder written by `tools/convert_checkpoint.py --family
qwen_aligner`; the tokenizer defaults to <model>/tokenizer (a Hugging Face tokenizer directory, loaded offline); --text names the file holding the transcript.
--family sensevoice: CTC forced alignment on a SenseVoice session (SenseVoiceTranscriber.align; one window of audio). --model is a folder written by
`tools/convert_checkpoint.py --family sensevoice`, --tokenizer its SentencePiece model, --text the transcript itself; --language defaults to "en".
--text-file names a file holding the transcript, for either family.
Output: JSON list of {text, start_time, end_time} in seconds.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "automatic-speech-recognition-asr-onnx_amd"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--family", choices=["qwen_aligner", "sensevoice"], default="qwen_aligner")
    ap.add_argument("--model", required=True)
    ap.add_argument("--wav", required=True)
    ap.add_argument("--text", help="qwen_aligner: file holding the transcript; sensevoice: the transcript")
    ap.add_argument("--text-file", help="file holding the transcript")
    ap.add_argument("--language", help="default: English (qwen_aligner), en (sensevoice)")
    ap.add_argument("--tokenizer")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if (a.text is None) == (a.text_file is None):
        ap.error("give the transcript with exactly one of --text and --text-file")
    if a.family == "sensevoice" and not a.tokenizer:
        ap.error("--family sensevoice needs --tokenizer (the SentencePiece model)")
    if a.language is None:
        a.language = "en" if a.family == "sensevoice" else "English"
    return a


def transcript(a) -> str:
    path = a.text_file if a.text_file is not None else a.text if a.family == "qwen_aligner" else None
    if path is None:
        return a.text
    with open(path, "r", encoding="utf-8") as f:
        return f.read()


def sensevoice_words(transcriber, audio, text):
    """The tool's JSON for one clip from SenseVoiceTranscriber.align; a transcript that does not fit the audio is an error."""
    out = transcriber.align(audio, text.strip())
    if not out["aligned"]:
        raise SystemExit("the transcript does not fit the audio: no alignment exists")
    return [{"text": w["text"], "start_time": w["start"], "end_time": w["end"]} for w in out["words"]]


def main(argv=None):
    a = parse_args(argv)
    aio = importlib.import_module(PKG + ".audio_io")
    text = transcript(a)
    if a.family == "sensevoice":
        sv = importlib.import_module(PKG + ".sensevoice")
        tr = sv.SenseVoiceTranscriber(a.model, a.language, tokenizer_path=a.tokenizer, device_id=a.device)
        words = sensevoice_words(tr, aio.read_wav_int16(a.wav, tr.sample_rate), text)
        print(json.dumps(words, ensure_ascii=False))
        return
    eng, ha, shim, wq = (importlib.import_module(PKG + m) for m in (".engine", ".qwen_aligner", ".ort_shim", ".ort_shim_qwen"))
    from transformers import AutoTokenizer
    path = os.path.join(a.model, wq.ALIGNER_MERGED_FILE + ".asrmodel")
    info, _ = shim.load_model(path)
    sess = eng.load_session(path, a.device)
    tok = AutoTokenizer.from_pretrained(a.tokenizer or os.path.join(a.model, "tokenizer"), local_files_only=True)
    aligner = ha.QwenForcedAligner(sess.cfg, sess, info["metadata"], tokenizer=tok)
    audio = aio.read_wav_int16(a.wav, sess.cfg.sample_rate)
    words = aligner.align([audio], [text], a.language)[0]
    print(json.dumps([{"text": w["text"], "start_time": w["start_time"] / 1000.0, "end_time": w["end_time"] / 1000.0} for w in words],
                     ensure_ascii=False))


if __name__ == "__main__":
    main()
