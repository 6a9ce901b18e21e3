#!/usr/bin/env python3
"""What the beam search over the decoder's token rows costs offline Paraformer: Paraformer-large, synthetic checkpoint, 64 x 8 s clips, bf16.
One session, five settings alternated in blocks -- run, run_timed, run_beam(beam = topk = 8, nbest = 1) plain, with 100 hotword phrases, and with the
synthetic 3-gram of about 10^6 n-grams that tools/probes/lm_beam_cost.py builds for SenseVoice's figure. A change of setting re-captures the beam step, so
every block starts with warm-up calls. Per setting: the wall time of the graph-replayed call (host clock around a call that ends in a stream synchronise),
median / min / max and the per-block medians, whose spread is the run-to-run figure to hold a difference against; for the beam settings also the
`ctc_topk` and `nar_beam` profile scopes (eager launches between device events). --plain-only measures run and run_timed alone, which also works on a tree
without the beam form (the comparison against the parent commit). Writes one JSON document.

    python tools/probes/paraformer_beam_probe.py [--out PATH] [--calls 12] [--blocks 2] [--plain-only]
"""
import argparse
import importlib
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PKG = "automatic-speech-recognition-asr-onnx_amd"
_m = lambda name: importlib.import_module(f"{PKG}.{name}")

BATCH, SECONDS, BEAM, N_HOTWORDS = 64, 8.0, 8, 100


def _trigram(vocab):
    spec = importlib.util.spec_from_file_location("lm_beam_cost", os.path.join(os.path.dirname(os.path.abspath(__file__)), "lm_beam_cost.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    # no blank: every id has a unigram; 13 continuations per unigram and 8 per bigram make about 10^6 n-grams over the 8404 ids, the size of SenseVoice's model
    return mod.synthetic_trigram(vocab, -1, per_unigram=13, per_bigram=8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paraformer_beam_probe.json"))
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()
    cfgm, ckm, eng = _m("config"), _m("checkpoints"), _m("engine")
    cfg = cfgm.paraformer_large()
    sess = eng.ParaformerSession.from_checkpoint(cfg, ckm.synth_paraformer_checkpoint(cfg, 0), precision=0)
    n = int(SECONDS * cfg.sample_rate)
    audio = ckm.synth_audio("kaldi", BATCH, n, seed=1234).reshape(-1)
    offsets = np.arange(BATCH + 1, dtype=np.int64) * n
    beam = lambda: sess.run_packed_beam(audio, offsets, BEAM, BEAM, 1)
    settings = {"run": (lambda: sess.run_packed(audio, offsets), None), "run_timed": (lambda: sess.run_packed_timed(audio, offsets), None)}
    doc = {"batch": BATCH, "seconds": SECONDS, "beam": BEAM, "topk": BEAM, "calls_per_block": a.calls, "blocks": a.blocks}
    if not a.plain_only:
        rng = np.random.default_rng(7)
        phrases = [rng.integers(0, cfg.vocab, int(rng.integers(2, 5))).tolist() for _ in range(N_HOTWORDS)]
        t0 = time.perf_counter()
        image = _trigram(cfg.vocab).image(cfg.vocab)
        doc["model"] = {"order": int(image[0]), "nodes": int(image[1]), "ngrams": int(image[2]), "image_mb": round(image.nbytes / 2 ** 20, 1),
                        "host_build_s": round(time.perf_counter() - t0, 1)}
        settings["beam"] = (beam, lambda: (sess.set_hotwords([], 0.0), sess.set_lm(None)))
        settings["beam_hotwords"] = (beam, lambda: (sess.set_hotwords(phrases, 2.0), sess.set_lm(None)))
        settings["beam_lm"] = (beam, lambda: (sess.set_hotwords([], 0.0), sess.set_lm(image, 0.5, 0.3)))
    wall, scopes, results = {k: [] for k in settings}, {k: [] for k in settings}, {}
    for _ in range(a.blocks):
        for name, (call, apply) in settings.items():
            if apply:
                apply()
            for _ in range(3):                                      # eager, capture, first replay
                results[name] = call()
            for _ in range(a.calls):
                t0 = time.perf_counter()
                call()
                wall[name].append(1e3 * (time.perf_counter() - t0))
            if apply:
                sess.profile(True)
                call()
                sess.profile_reset()
                for _ in range(5):
                    call()
                prof = sess.profile_read()
                sess.profile(False)
                scopes[name].append({k: round(1e3 * prof[k]["total_ms"] / 5, 1) for k in ("ctc_topk", "nar_beam") if k in prof})
    for name in settings:
        meds = [float(np.median(wall[name][i * a.calls:(i + 1) * a.calls])) for i in range(a.blocks)]
        doc[name] = {"wall_ms_median": float(np.median(wall[name])), "wall_ms_min": min(wall[name]), "wall_ms_max": max(wall[name]), "wall_ms_block_medians": meds,
                     "run_to_run_spread_ms": max(meds) - min(meds)}
        if scopes[name]:
            doc[name]["scopes_us_per_call"] = scopes[name]
    doc["mean_tokens"] = float(results["run"][1].mean())
    if not a.plain_only:
        same = lambda x, y: int(sum(not np.array_equal(x[0][b, 0, :x[1][b, 0]], y[0][b, 0, :y[1][b, 0]]) for b in range(BATCH)))
        tok, num = results["run"]
        doc["beam_best_differs_from_run"] = int(sum(not np.array_equal(tok[b, :num[b]], results["beam"][0][b, 0, :num[b]]) for b in range(BATCH)))
        doc["best_changed_by_hotwords"] = same(results["beam"], results["beam_hotwords"])
        doc["best_changed_by_lm"] = same(results["beam"], results["beam_lm"])
        sess.set_hotwords([], 0.0)
        sess.set_lm(None)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
