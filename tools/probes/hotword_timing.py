#!/usr/bin/env python3
"""What hotword boosting costs per decode step: a TokenHead (csrc/decode_head.h) driven through the probe library's hotword head steps on the two
deployment shapes -- 32 rows x 51866 columns (Whisper large-v3) and 64 rows x 151936 (Qwen3-ASR) -- with 100 phrases of 1..4 tokens, against the same head
with the mode off, plain (launch_argmax_rows alone) and with token scores (which already keeps the id history); and the beam ranker's extra work at width
5 (launch_beam_topk alone against launch_beam_topk with lse_out + launch_hotword_rerank, rows = sequences x 5). Launches run back to back between two
device events, a warm-up call first, modes alternated. Writes one JSON document (default profiles/hotword_head_steps.json).

    python tools/probes/hotword_timing.py [--out PATH] [--calls 5]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
probe = importlib.import_module("automatic-speech-recognition-asr-onnx_amd._probe")

SHAPES = [(32, 51866), (64, 151936)]
STEPS, BEAM, ITERS = 1000, 5, 200


def phrases(n, seed, count=100):
    rng = np.random.default_rng([n, seed])
    return [[int(t) for t in rng.integers(0, n, int(rng.integers(1, 5)))] for _ in range(count)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hotword_head_steps.json"))
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    results = []
    for rows, n in SHAPES:
        x = np.random.default_rng([rows, n]).normal(0.0, 3.0, (1, rows, n)).astype(np.float32)
        ph = phrases(n, 1)
        modes = {"plain": ([], False), "hotwords": (ph, False), "scores": ([], True), "scores + hotwords": (ph, True)}
        run = lambda m, steps=STEPS: probe.hotword_head_steps(x, modes[m][0], 2.0, 1024, scores=modes[m][1], timed=steps)["head_ms"]
        for m in modes:
            run(m, 50)                                            # warm-up: code objects, clocks
        us = {m: [] for m in modes}
        for _ in range(a.calls):
            for m in modes:
                us[m].append(1000.0 * run(m) / STEPS)
        head = {m: {"median": float(np.median(v)), "min": min(v), "max": max(v)} for m, v in us.items()}
        # the ranker: rows x BEAM hypothesis rows somewhere inside phrases
        N = rows * BEAM
        xr = np.random.default_rng([rows, n, 2]).normal(0.0, 3.0, (N, n)).astype(np.float32)
        z = np.zeros(N, np.int32)
        tab = np.zeros((N, 4), np.int32) + (np.arange(N)[:, None] // BEAM) * BEAM
        node = (np.arange(N) % 50 + 1).astype(np.int32)             # root children (breadth-first ids 1 .. ): depth 1, most with children
        rk = {"topk": [], "rerank": []}
        for i in range(a.calls + 1):
            st = probe.hotword_rank(xr, ph, 2.0, BEAM, 1, np.zeros(N, np.float32), z, z + 1, z, np.zeros(rows, np.int32), tab, tab, node, iters=ITERS)
            if i:                                                 # (the first call warms up)
                rk["topk"].append(1000.0 * st["ms_topk"] / ITERS); rk["rerank"].append(1000.0 * st["ms_rerank"] / ITERS)
        results.append({"rows": rows, "n_valid": n, "phrases": len(ph), "steps_per_call": STEPS, "calls_per_mode": a.calls, "head_us_per_step": head,
                        "hotwords_minus_plain_us": head["hotwords"]["median"] - head["plain"]["median"],
                        "hotwords_minus_scores_us": head["scores + hotwords"]["median"] - head["scores"]["median"],
                        "beam": {"width": BEAM, "rows": N, "topk_us": float(np.median(rk["topk"])), "topk_lse_rerank_us": float(np.median(rk["rerank"])),
                                 "difference_us": float(np.median(rk["rerank"]) - np.median(rk["topk"]))}})
        print(json.dumps(results[-1]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"what": "TokenHead steps with hotwords off / on (100 phrases of 1..4 tokens), launches back to back between two device events; "
                           "beam: launch_beam_topk alone against launch_beam_topk (lse_out) + launch_hotword_rerank at width 5", "shapes": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
