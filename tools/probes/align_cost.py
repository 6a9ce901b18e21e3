#!/usr/bin/env python3
"""What SenseVoice forced alignment costs per call against run_timed on the same session, at the benchmark's shape (sensevoice_small, bf16, 64 clips of 8 s,
synthetic weights and audio as bench.py makes them), with every clip's greedy transcript (the timed run's tokens behind the prompt rows) as its target.
Wall milliseconds per call with the host clock around calls that end in a stream synchronise (audio uploaded from the host in both forms), the two forms
alternated, warm-up calls first (the third call of a form replays its captured graph); then the per-class split of one profiled call of each form (eager
launches bracketed by device events). Writes one JSON document (default profiles/sensevoice_align_cost.json).

    python tools/probes/align_cost.py [--out PATH] [--calls 30] [--batch 64] [--seconds 8]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PKG = "automatic-speech-recognition-asr-onnx_amd"


def backpointers_in_lds(rows, max_L):
    """launch_ctc_align's rule (csrc/ctc_align.hip): exchange buffers + ceil(rows / 8) x (max_L + 1) words inside 64 KB - 256 B of dynamic LDS."""
    threads = (max_L + 1 + 63) // 64 * 64
    return 16 * (threads + 1) + (max(rows, 1) + 7) // 8 * (max_L + 1) * 4 <= 64 * 1024 - 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensevoice_align_cost.json"))
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=8.0)
    a = ap.parse_args()
    eng, cfgm, ckm, arena = (importlib.import_module(f"{PKG}.{m}") for m in ("engine", "config", "checkpoints", "arena"))
    cfg = cfgm.sensevoice_small()
    n = int(a.seconds * cfg.sample_rate)
    sess = eng.SenseVoiceSession.from_checkpoint(cfg, ckm.synth_sensevoice_checkpoint(cfg, seed=0), precision=arena.PRECISION_BF16)
    audio = np.ascontiguousarray(ckm.synth_audio("kaldi", a.batch, n, seed=1234)[:, 0].reshape(-1), np.float32)
    offs = np.arange(a.batch + 1, dtype=np.int64) * n
    lang = np.zeros(a.batch, np.int32)
    tok, num, first, last, _ = sess.run_packed_timed(audio, offs, lang)
    targets = [tok[b, :num[b]][first[b, :num[b]] >= cfg.n_prompt] for b in range(a.batch)]
    toff = np.zeros(a.batch + 1, np.int32)
    toff[1:] = np.cumsum([t.size for t in targets])
    tids = np.concatenate(targets).astype(np.int32)
    forms = {"run_timed": lambda: sess.run_packed_timed(audio, offs, lang), "align": lambda: sess.align_packed(audio, offs, lang, tids, toff)}
    for _ in range(4):                                   # eager, capture, replay, replay
        for f in forms.values():
            f()
    status = forms["align"]()[5]
    ms = {k: [] for k in forms}
    for _ in range(a.calls):
        for k, f in forms.items():
            t0 = time.perf_counter()
            f()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    split = {}
    sess.profile(True)
    for k, f in forms.items():
        f()
        sess.profile_reset()
        f()
        split[k] = {c: {"ms": round(v["total_ms"], 4), "launches": v["launches"]} for c, v in sess.profile_read().items() if v["launches"]}
    sess.profile(False)
    rows, max_L = cfg.seq_len(n) - cfg.n_prompt, int(max(t.size for t in targets))
    doc = {"shape": {"batch": a.batch, "seconds": a.seconds, "rows_per_clip": cfg.seq_len(n), "speech_rows": rows, "precision": "bf16"},
           "targets": {"total": int(tids.size), "longest": max_L, "aligned": int((status == 0).sum())},
           "backpointers": "LDS" if backpointers_in_lds(rows, max_L) else "workspace",
           "ms_per_call": {k: {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4), "calls": len(v)} for k, v in ms.items()},
           "profile_ms_per_class": split}
    fwd = sum(v["ms"] for c, v in split["align"].items() if c not in ("ctc_align", "ctc_align_em"))
    doc["align_classes_over_forward"] = {c: round(split["align"][c]["ms"] / fwd, 5) for c in ("ctc_align_em", "ctc_align")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
