#!/usr/bin/env python3
"""What the streaming beam search costs a chunk step: Paraformer-large, synthetic checkpoint, one session, 64 streams, bf16, 0.5 s chunks.
Alternating blocks of step, step_timed and step_beam (beam = topk = 8, nbest = 1) -- plain at pend_cap 16, at pend_cap 4 (every stream saturated: a forced
commit with its ancestor walk before almost every row), with 100 hotword phrases, and with the synthetic 3-gram of about 10^6 n-grams that
tools/probes/lm_beam_cost.py builds. Streams are reset every 8 chunks, as bench.py's streaming workload does; a change of setting needs streams without
search history, so every block starts at a reset. Every step runs under a time limit of its own (an alarm that ends the process). Per setting: the wall time
of a step (host clock around a call that ends in a stream synchronise), median / min / max and the per-block medians, whose spread is the run-to-run figure
to hold a difference against; for the beam settings the `beam_topk` and `nar_stream_beam` profile scopes (eager launches between device events) and what
is left of the difference to step_timed: the second synchronisation with its copy. Writes one JSON document.

    python tools/probes/paraformer_stream_beam_probe.py [--out PATH] [--steps 24] [--blocks 2]
"""
import argparse
import importlib
import importlib.util
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PKG = "automatic-speech-recognition-asr-onnx_amd"
_m = lambda name: importlib.import_module(f"{PKG}.{name}")

STREAMS, CHUNK, N_CHUNKS, BEAM, N_HOTWORDS, STEP_LIMIT_S = 64, 8000, 8, 8, 100, 60


def _trigram(vocab):
    spec = importlib.util.spec_from_file_location("lm_beam_cost", os.path.join(os.path.dirname(os.path.abspath(__file__)), "lm_beam_cost.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.synthetic_trigram(vocab, -1, per_unigram=13, per_bigram=8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paraformer_stream_beam_probe.json"))
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--blocks", type=int, default=2)
    a = ap.parse_args()
    cfgm, ckm, eng = _m("config"), _m("checkpoints"), _m("engine")
    cfg = cfgm.paraformer_large()
    sess = eng.ParaformerStreamSession(cfg, ckm.synth_paraformer_checkpoint(cfg, 0), precision=0, chunk=CHUNK, max_streams=STREAMS)
    audio = np.ascontiguousarray(ckm.synth_audio("kaldi", STREAMS, N_CHUNKS * CHUNK, seed=1234)[:, 0].reshape(STREAMS, N_CHUNKS, CHUNK).transpose(1, 0, 2))
    sids = list(range(STREAMS))
    rng = np.random.default_rng(7)
    phrases = [rng.integers(0, cfg.vocab, int(rng.integers(2, 5))).tolist() for _ in range(N_HOTWORDS)]
    t0 = time.perf_counter()
    image = _trigram(cfg.vocab).image(cfg.vocab)
    doc = {"streams": STREAMS, "chunk": CHUNK, "beam": BEAM, "topk": BEAM, "steps_per_block": a.steps, "blocks": a.blocks,
           "model": {"order": int(image[0]), "nodes": int(image[1]), "ngrams": int(image[2]), "image_mb": round(image.nbytes / 2 ** 20, 1),
                     "host_build_s": round(time.perf_counter() - t0, 1)}}

    def setting(cap, hot, lm):
        def apply():
            sess.reset(-1)
            sess.set_beam(BEAM, BEAM, 1, cap)
            sess.set_hotwords(phrases if hot else [], 2.0)
            sess.set_lm(image if lm else None, 0.5, 0.3)
        return apply
    settings = {"step": (sess.step, None), "step_timed": (sess.step_timed, None), "beam": (sess.step_beam, setting(16, False, False)),
                "beam_cap4": (sess.step_beam, setting(4, False, False)), "beam_hotwords": (sess.step_beam, setting(16, True, False)),
                "beam_lm": (sess.step_beam, setting(16, False, True))}
    wall, scopes, commits, tokens = {k: [] for k in settings}, {k: [] for k in settings}, {k: [0, 0] for k in settings}, [0, 0]

    def one(call, i):
        if i % N_CHUNKS == 0:
            sess.reset(-1)
        signal.alarm(STEP_LIMIT_S)                             # a step that hangs ends the process
        t0 = time.perf_counter()
        out = call(audio[i % N_CHUNKS], sids)
        dt = 1e3 * (time.perf_counter() - t0)
        signal.alarm(0)
        return out, dt

    for _ in range(a.blocks):
        for name, (call, apply) in settings.items():
            if apply:
                apply()
            for i in range(N_CHUNKS):                          # eager, capture, replay of the step's graph; the streams warm
                one(call, i)
            for i in range(a.steps):
                out, dt = one(call, i)
                wall[name].append(dt)
                if apply:
                    commits[name][0] += sum(len(r["committed"]["ids"]) > 0 for r in out)
                    commits[name][1] += sum(len(r["ids"]) > 0 for r in out)
                elif name == "step":
                    tokens[0] += sum(len(r) for r in out)
                    tokens[1] += len(out)
            if apply:
                sess.profile(True)
                one(call, 0)
                sess.profile_reset()
                for i in range(1, N_CHUNKS):
                    one(call, i)
                prof = sess.profile_read()
                sess.profile(False)
                scopes[name].append({k: round(1e3 * prof[k]["total_ms"] / (N_CHUNKS - 1), 1) for k in ("beam_topk", "nar_stream_beam") if k in prof})
    sess.reset(-1)
    sess.set_beam(0)
    for name in settings:
        meds = [float(np.median(wall[name][i * a.steps:(i + 1) * a.steps])) for i in range(a.blocks)]
        doc[name] = {"wall_ms_median": float(np.median(wall[name])), "wall_ms_min": min(wall[name]), "wall_ms_max": max(wall[name]), "wall_ms_block_medians": meds,
                     "run_to_run_spread_ms": max(meds) - min(meds)}
        if scopes[name]:
            doc[name]["scopes_us_per_step"] = scopes[name]
            kernels_ms = float(np.mean([sum(s.values()) for s in scopes[name]])) / 1e3
            doc[name]["over_step_timed_ms"] = doc[name]["wall_ms_median"] - float(np.median(wall["step_timed"]))
            doc[name]["second_sync_and_copy_ms"] = doc[name]["over_step_timed_ms"] - kernels_ms
            doc[name]["stream_steps_with_a_forced_commit"] = commits[name][0] / max(commits[name][1], 1)
    doc["tokens_per_stream_step"] = tokens[0] / max(tokens[1], 1)
    doc["stream_stats"] = sess.stream_stats()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
