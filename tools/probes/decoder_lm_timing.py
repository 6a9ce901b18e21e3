#!/usr/bin/env python3
"""What n-gram LM fusion costs per decode step of the autoregressive decoders, after hotword_timing.py: a TokenHead (csrc/decode_head.h) driven through the
probe library on the two deployment shapes -- 32 rows x 51866 columns (Whisper large-v3) and 64 rows x 151936 (Qwen3-ASR) -- with an order-3 model (80% of
the vocabulary with a unigram, 20000 bigrams, 20000 trigrams) at topk 16, against the same head without a model, plain (launch_argmax_rows alone) and with
token scores (launch_argmax_logprob_rows); launch_lm_topk alone against launch_beam_topk at K = 8 on the same rows, and how many rows took its strict-order
passes; and a ranking pass at width 5 (launch_lm_topk + launch_lm_rerank against launch_beam_topk at K = 5 with lse_out + launch_hotword_rerank, 100 phrases,
rows = sequences x 5). The rows are N(0, 3^2) draws with the 40 best columns of every row lifted by up to 12, the peaked shape of a trained checkpoint's
logits. Launches run back to back between two device events, a warm-up call first, modes alternated. Writes one JSON document (default
profiles/decoder_lm_timing.json).

    python tools/probes/decoder_lm_timing.py [--out PATH] [--calls 5]
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
lmm = importlib.import_module("automatic-speech-recognition-asr-onnx_amd.lm")

SHAPES = [(32, 51866), (64, 151936)]
STEPS, BEAM, ITERS, TOPK = 1000, 5, 200, 16


def phrases(n, seed, count=100):
    rng = np.random.default_rng([n, seed])
    return [[int(t) for t in rng.integers(0, n, int(rng.integers(1, 5)))] for _ in range(count)]


def peaked_rows(seed, rows, n):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 3.0, (rows, n)).astype(np.float32)
    for r in range(rows):
        top = np.argpartition(-x[r], 40)[:40]
        x[r, top] += rng.uniform(0.0, 12.0, 40).astype(np.float32)
    return x


def model(n, x, seed=7):
    """An order-3 model over n ids whose bigrams and trigrams continue into the rows' best columns, so the walks find n-grams and back off alike."""
    rng = np.random.default_rng([n, seed])
    known = np.nonzero(rng.random(n) < 0.8)[0]
    lp = lambda: -float(rng.uniform(0.05, 6.0))
    ng = {(int(c),): (lp(), -float(rng.uniform(0.0, 1.0))) for c in known}
    ng[(lmm.BOS,)] = (0.0, -0.5)
    ng[(lmm.EOS,)] = (lp(), 0.0)
    best = np.unique(np.argsort(-x, axis=1)[:, :24])
    best = best[np.isin(best, known)]
    for _ in range(20000):
        a, b = int(rng.choice(known)), int(rng.choice(best))
        ng.setdefault((a, b), (lp(), -float(rng.uniform(0.0, 1.0))))
    bigrams = [g for g in ng if len(g) == 2]
    for _ in range(20000):
        g = bigrams[int(rng.integers(len(bigrams)))]
        ng.setdefault(g + (int(rng.choice(best)),), (lp(), 0.0))
    return dict(image=lmm.NgramLM(ng).image(n), alpha=0.5, beta=0.25, oov=-4.0, topk=TOPK, end_ids=(int(known[0]),))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_lm_timing.json"))
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    results = []
    for rows, n in SHAPES:
        x = peaked_rows([rows, n], rows, n)[None]
        lm = model(n, x[0])
        modes = {"plain": (None, False), "lm": (lm, False), "scores": (None, True), "scores + lm": (lm, True)}
        run = lambda m, steps=STEPS: probe.hotword_head_steps(x, [], 0.0, 1024, scores=modes[m][1], timed=steps, lm=modes[m][0])["head_ms"]
        for m in modes:
            run(m, 50)                                            # warm-up: code objects, clocks
        us = {m: [] for m in modes}
        for _ in range(a.calls):
            for m in modes:
                us[m].append(1000.0 * run(m) / STEPS)
        head = {m: {"median": float(np.median(v)), "min": min(v), "max": max(v)} for m, v in us.items()}
        # the top-M pass alone, on the head's rows and on the ranker's
        N = rows * BEAM
        xr = peaked_rows([rows, n, 2], N, n)
        tk = {"lm_topk": [], "beam_topk": [], "slow_rows": 0}
        for i in range(a.calls + 1):
            st = probe.lm_topk(xr, TOPK, iters=ITERS)
            tk["slow_rows"] += st["slow_rows"]
            if i:
                tk["lm_topk"].append(1000.0 * st["ms_lm_topk"] / ITERS); tk["beam_topk"].append(1000.0 * st["ms_beam_topk"] / ITERS)
        slow_head = probe.lm_topk(x[0], TOPK)["slow_rows"]
        # the ranker: rows x BEAM hypothesis rows somewhere inside phrases, states spread over the image
        ph = phrases(n, 1)
        z = np.zeros(N, np.int32)
        tab = np.zeros((N, 4), np.int32) + (np.arange(N)[:, None] // BEAM) * BEAM
        node = (np.arange(N) % 50 + 1).astype(np.int32)
        n_nodes = int(lm["image"][1])
        state = (np.arange(N) * 7919 % n_nodes).astype(np.int32)
        rk = {"plain": [], "lm": []}
        for i in range(a.calls + 1):
            st = probe.hotword_rank(xr, ph, 2.0, BEAM, 1, np.zeros(N, np.float32), z, z + 1, z, np.zeros(rows, np.int32), tab, tab, node, iters=ITERS, lm=lm,
                                    state_in=state)
            if i:                                                 # (the first call warms up)
                rk["plain"].append(1000.0 * st["ms_topk"] / ITERS); rk["lm"].append(1000.0 * st["ms_rerank"] / ITERS)
        med = lambda v: float(np.median(v))
        results.append({"rows": rows, "n_valid": n, "topk": TOPK, "image_words": int(lm["image"].size), "steps_per_call": STEPS, "calls_per_mode": a.calls,
                        "head_us_per_step": head,
                        "lm_minus_plain_us": head["lm"]["median"] - head["plain"]["median"],
                        "lm_minus_scores_us": head["scores + lm"]["median"] - head["scores"]["median"],
                        "top_m": {"rows": N, "M": TOPK, "lm_topk_us": med(tk["lm_topk"]), "beam_topk_k8_us": med(tk["beam_topk"]),
                                  "ratio": med(tk["lm_topk"]) / med(tk["beam_topk"]), "strict_order_rows": int(tk["slow_rows"]),
                                  "strict_order_rows_head": int(slow_head)},
                        "beam": {"width": BEAM, "rows": N, "phrases": len(ph), "topk_lse_hotword_rerank_us": med(rk["plain"]),
                                 "lm_topk_lm_rerank_us": med(rk["lm"]), "difference_us": med(rk["lm"]) - med(rk["plain"])}})
        print(json.dumps(results[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"what": "TokenHead steps without / with an n-gram model (order 3, topk 16), launches back to back between two device events; top_m: "
                           "launch_lm_topk against launch_beam_topk (K = 8, lse_out) on the ranker's rows; beam: launch_beam_topk (K = 5, lse_out) + "
                           "launch_hotword_rerank against launch_lm_topk + launch_lm_rerank at width 5", "shapes": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
