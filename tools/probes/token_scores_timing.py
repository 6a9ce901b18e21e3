#!/usr/bin/env python3
"""What token scores cost per decode step in the selection head: TokenHead (csrc/decode_head.h) driven through the probe library's head steps on the two
deployment shapes -- 32 rows x 51866 columns (Whisper large-v3) and 64 rows x 151936 (Qwen3-ASR) -- with scores off (launch_argmax_rows alone) and on
(launch_argmax_logprob_rows, then the history append and its counter). The steps' launches run back to back between two device events, a warm-up call first, calls of both
modes alternated until each mode has at least --min-ms of device time. Writes one JSON document (default profiles/token_scores_head_steps.json).

    python tools/probes/token_scores_timing.py [--out PATH] [--min-ms 300]
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
STEPS = 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_scores_head_steps.json"))
    ap.add_argument("--min-ms", type=float, default=300.0)
    a = ap.parse_args()
    results = []
    for rows, n in SHAPES:
        x = np.random.default_rng([rows, n]).normal(0.0, 3.0, (rows, n)).astype(np.float32)
        run = lambda on, steps=STEPS: probe.head_steps(x, steps, STEPS, 1, 1.0, 0, scores=on, timed=True)["head_ms"]
        for on in (False, True):
            run(on, 50)                                           # warm-up: code objects, clocks
        ms, calls = {False: [], True: []}, 0
        while (min(sum(ms[False]), sum(ms[True])) < a.min_ms) and calls < 100:
            for on in (False, True):
                ms[on].append(run(on))
            calls += 1
        per = {on: [1000.0 * v / STEPS for v in ms[on]] for on in ms}          # us per step, per call
        off_us, on_us = float(np.median(per[False])), float(np.median(per[True]))
        results.append({"rows": rows, "n_valid": n, "steps_per_call": STEPS, "calls_per_mode": calls,
                        "scores_off_us_per_step": {"median": off_us, "min": min(per[False]), "max": max(per[False])},
                        "scores_on_us_per_step": {"median": on_us, "min": min(per[True]), "max": max(per[True])},
                        "difference_us_per_step": on_us - off_us})
        print(json.dumps(results[-1]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"what": "TokenHead steps, the steps' launches back to back between two device events; scores off = argmax_rows, on = argmax_logprob_rows + append_ids + counter",
                   "shapes": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
