#!/usr/bin/env python
"""Word timestamps for one wav and its transcript (Qwen3-ForcedAligner on the native session).

    python tools/align.py --model Qwen_ForcedAligner_MI355X --wav clip.wav --text transcript.txt [--language English] [--tokenizer DIR] > words.json

--model is a folder written by `tools/convert_checkpoint.py --family qwen_aligner`; the tokenizer defaults to <model>/tokenizer (a Hugging
Face tokenizer directory, loaded offline). Output: JSON list of {text, start_time, end_time} in seconds.
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", required=True)
    ap.add_argument("--wav", required=True)
    ap.add_argument("--text", required=True, help="file holding the transcript")
    ap.add_argument("--language", default="English")
    ap.add_argument("--tokenizer")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    eng, ha, aio, shim, wq = (importlib.import_module(PKG + m) for m in (".engine", ".qwen_aligner", ".audio_io", ".ort_shim", ".ort_shim_qwen"))
    from transformers import AutoTokenizer
    path = os.path.join(a.model, wq.ALIGNER_MERGED_FILE + ".asrmodel")
    info, _ = shim.load_model(path)
    sess = eng.load_session(path, a.device)
    tok = AutoTokenizer.from_pretrained(a.tokenizer or os.path.join(a.model, "tokenizer"), local_files_only=True)
    aligner = ha.QwenForcedAligner(sess.cfg, sess, info["metadata"], tokenizer=tok)
    audio = aio.read_wav_int16(a.wav, sess.cfg.sample_rate)
    with open(a.text, "r", encoding="utf-8") as f:
        text = f.read()
    words = aligner.align([audio], [text], a.language)[0]
    print(json.dumps([{"text": w["text"], "start_time": w["start_time"] / 1000.0, "end_time": w["end_time"] / 1000.0} for w in words],
                     ensure_ascii=False))


if __name__ == "__main__":
    main()
