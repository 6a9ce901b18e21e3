"""What the device VAD (engine.op_vad, csrc/vad.hip) costs: one 1 h int16 mono file, and 64 x 30 s, each HBM-resident and from the host.

  call legs      a host clock around the synchronous op (its own allocations, the plan upload, the memset, the three launches, the result copies; from the host
                 also the H2D copy of the audio), medians and min / max over --iters calls after --warmup, the four legs interleaved
  kernel leg     --stats-csv FILE: read a `rocprofv3 --kernel-trace --stats` kernel-stats CSV taken in a run of its own (this script with --case hour --iters N
                 under the profiler) and print the stage-1 kernel's mean time, the bytes it has to read (every sample once) and write (e and q, 8 bytes per
                 analysis frame), and that traffic over the kernel time as a fraction of the 8.0 TB/s HBM peak; stage 2 and the pack are listed beside it

Prints one JSON line per invocation.
    python tools/probes/vad_cost.py [--iters 20 --warmup 3] [--case all|hour|batch]
    python tools/probes/vad_cost.py --stats-csv kernel_stats.csv --case hour"""
import argparse
import csv
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

PKG = "automatic-speech-recognition-asr-onnx_amd"
RATE = 16000
HBM_PEAK = 8.0e12
CASES = {"hour": (1, 3600), "batch": (64, 30)}


def traffic(batch, seconds):
    """Bytes stage 1 has to move for int16 mono at 16 kHz: the samples once, e and q once."""
    n = batch * seconds * RATE
    frames = batch * (-(-seconds * RATE // 160))
    return {"read": 2 * n, "write": 8 * frames, "analysis_frames": frames}


def from_stats(path, case):
    rows = list(csv.DictReader(open(path, newline="")))
    out = {"probe": "vad_cost", "leg": "kernels", "case": case, "source": "rocprofv3 --kernel-trace --stats"}
    for key, name in (("stage1", "vad_energy_kernel"), ("stage2", "vad_segment_kernel"), ("pack", "vad_pack_kernel")):
        r = [x for x in rows if name in x["Name"]]
        if not r:
            raise SystemExit(f"{path}: no kernel named {name}")
        out[key + "_us"] = {"mean": round(float(r[0]["AverageNs"]) / 1e3, 2), "min": round(float(r[0]["MinNs"]) / 1e3, 2), "max": round(float(r[0]["MaxNs"]) / 1e3, 2),
                            "calls": int(r[0]["Calls"])}
    t = traffic(*CASES[case])
    rate = (t["read"] + t["write"]) / (out["stage1_us"]["mean"] * 1e-6)
    out.update(stage1_bytes=t, stage1_bytes_per_s=round(rate, 0), stage1_fraction_of_hbm_peak=round(rate / HBM_PEAK, 4), hbm_peak_bytes_per_s=HBM_PEAK)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", default="all", choices=("all", "hour", "batch"))
    ap.add_argument("--stats-csv")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    a = ap.parse_args()
    if a.stats_csv:
        return from_stats(a.stats_csv, a.case)
    sys.path.insert(0, os.path.abspath(a.root))
    eng, _lib = (importlib.import_module(f"{PKG}.{m}") for m in ("engine", "_lib"))
    lib = _lib.load()
    rng = np.random.default_rng(5)
    legs, keep, segs = {}, [], {}
    for case in (("hour", "batch") if a.case == "all" else (a.case,)):
        batch, seconds = CASES[case]
        n = seconds * RATE
        # speech-like: 3 s loud, 1 s of low noise, so that the segment stage has runs to work on
        env = np.where((np.arange(n) // RATE) % 4 < 3, 3000.0, 8.0)
        audio = np.concatenate([np.round(rng.standard_normal(n) * env) for _ in range(batch)]).astype(np.int16)
        offs = np.arange(batch + 1, dtype=np.int64) * n
        dptr = C.c_void_p(None)
        _lib.check(lib.asr_mem_alloc(0, audio.nbytes, C.byref(dptr)))
        _lib.check(lib.asr_mem_copy(0, dptr, audio.ctypes.data_as(C.c_void_p), audio.nbytes, 0))
        keep.append((audio, offs, dptr))
        legs[case + "_resident"] = lambda audio=audio, offs=offs, dptr=dptr: eng.op_vad(audio, offs, rate=RATE, audio_device_ptr=dptr.value)
        legs[case + "_host"] = lambda audio=audio, offs=offs: eng.op_vad(audio, offs, rate=RATE)
    for _ in range(a.warmup):
        for name, fn in legs.items():
            segs[name] = int(fn()[2].sum())
    times = {k: [] for k in legs}
    for _ in range(a.iters):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    out = {"probe": "vad_cost", "leg": "calls", "root": os.path.abspath(a.root), "iters": a.iters, "audio": "int16 mono 16 kHz",
           "audio_mb": {k: CASES[k][0] * CASES[k][1] * RATE * 2 / 1e6 for k in CASES}, "segments": segs}
    for k, v in times.items():
        out[k + "_ms"] = {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}
    for _, _, dptr in keep:
        _lib.check(lib.asr_mem_free(0, dptr))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
