#!/usr/bin/env python3
"""What a long text prompt costs on Whisper large-v3 (bf16, synthetic checkpoint, 32 x 30 s windows, a uniform prompt of 228 ids): one
prefill_prompts call (every decoder weight read once) against the only emulation the code offered before it -- a prefill of the first 8 ids and 220
host-fed single-token decode steps (every weight read 221 times). Both run in the same process on the same encoded batch, alternated (the order inside a round
swaps from round to round), a warm-up round first; times are host clocks around calls that end in a device synchronise (the logits / next ids come back to the host). A separate profiled pass
(asr_session_profile_read: device events around every launch group, graphs off) gives the prompt-attention kernel's share of the new prefill. Then one
device-fed decode step at 32 sequences and history 228 with key_start set (after prefill_prompts) and without (after the emulation chain), 64 steps per
timing. Writes one JSON document (default profiles/whisper_prompt_prefill.json).

    python tools/probes/whisper_prompt_prefill.py [--out PATH] [--rounds 4] [--batch 32] [--seconds 30] [--prompt 228]
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
cfgm, ckm, eng = (importlib.import_module(f"{PKG}.{m}") for m in ("config", "checkpoints", "engine"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "whisper_prompt_prefill.json"))
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--prompt", type=int, default=228)
    ap.add_argument("--config", default="whisper_large_v3")
    a = ap.parse_args()
    cfg = getattr(cfgm, a.config)()
    B, n, steps = a.batch, a.prompt, 64
    ck = ckm.synth_whisper_checkpoint(cfg, 0)
    sess = eng.WhisperSession.from_checkpoint(cfg, ck, precision=eng.PRECISION_BF16, suppress_tokens=ckm.whisper_suppress_tokens(cfg),
                                              begin_suppress_tokens=ckm.whisper_begin_suppress_tokens(cfg))
    samples = int(a.seconds * cfg.sample_rate)
    audios = [ckm.synth_audio("unit", 1, samples, seed=40 + b)[0, 0] for b in range(B)]
    rng = np.random.default_rng(1)
    head = [cfg.sot_id, cfg.first_language_id, cfg.transcribe_id, cfg.no_timestamps_id]
    ids = np.stack([np.array([cfg.sot_prev_id] + rng.integers(0, cfg.eot_id, n - 5).tolist() + head, np.int32) for _ in range(B)])
    sess.encode(audios)

    def new_path():
        t0 = time.perf_counter()
        sess.prefill_prompts(list(ids), want_logits=False)       # returns the next ids: synchronised
        return 1000.0 * (time.perf_counter() - t0)

    def emulation():
        t0 = time.perf_counter()
        sess.prefill(ids[:, :8], want_logits=False)
        for t in range(8, n):
            sess.decode(ids[:, t])
        return 1000.0 * (time.perf_counter() - t0)

    def decode_steps():
        sess.decode(None)                                         # the eager pass, then the capture
        sess.decode(None)
        t0 = time.perf_counter()
        for _ in range(steps - 1):
            sess.decode(None, sync=False)
        sess.decode(None)
        return 1000.0 * (time.perf_counter() - t0) / steps

    new_path(), emulation()                                       # warm-up: code objects, buffers, clocks
    ms = {"prefill_prompts": [], "emulation": [], "step_key_start": [], "step_plain": []}
    for r in range(a.rounds):
        for arm in (("new", "old") if r % 2 == 0 else ("old", "new")):       # the order inside a round alternates
            if arm == "new":
                ms["prefill_prompts"].append(new_path())
                ms["step_key_start"].append(decode_steps())
            else:
                ms["emulation"].append(emulation())
                ms["step_plain"].append(decode_steps())
    sess.profile(True)                                            # separate pass: device events per launch group
    sess.profile_reset()
    sess.prefill_prompts(list(ids), want_logits=False)
    prof = sess.profile_read()
    sess.profile(False)
    total = sum(v["total_ms"] for k, v in prof.items() if k.startswith("dec_"))
    attn = sum(prof[k]["total_ms"] for k in ("dec_self_attn", "dec_cross_attn") if k in prof)
    stat = lambda v: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    doc = {"what": f"{a.config} bf16 synthetic checkpoint, {B} x {a.seconds:g} s, uniform prompt of {n} ids; host clock around synchronised calls, "
                   f"{a.rounds} alternated rounds after a warm-up round; decode step: {steps} device-fed steps at history {n}",
           "prefill_prompts_ms": stat(ms["prefill_prompts"]), "emulation_8_plus_%d_steps_ms" % (n - 8): stat(ms["emulation"]),
           "speedup": float(np.median(ms["emulation"]) / np.median(ms["prefill_prompts"])),
           "decode_step_ms_key_start": stat(ms["step_key_start"]), "decode_step_ms_plain": stat(ms["step_plain"]),
           "profile_prefill_prompts": {"decoder_total_ms": total, "prompt_attention_ms": attn, "prompt_attention_share": attn / total if total else None,
                                       "scopes": {k: v for k, v in prof.items() if k.startswith("dec_")}}}
    print(json.dumps(doc))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
