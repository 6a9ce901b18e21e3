"""What the device resampler costs next to the step: SenseVoice-small bf16, 64 x 8 s, one session, a plain timing loop in a fresh process.

  mono16k_f32 leg     the default format: 16 kHz mono float32 from the host (32.8 MB H2D + step) -- the call every earlier commit makes
  stereo48k leg       the same 8 s as 48 kHz stereo int16 from the host: set_input_format(48000, 2), 98.3 MB H2D + resampler + step
  resident48k leg     the 48 kHz stereo int16 frames already in HBM (asr_mem_alloc / asr_mem_copy): resampler + step
  resampler alone     the session profiler's "resample" class over the resident leg (HIP events around the plan upload and the one launch; the
                      profiler runs the step eagerly, so only that class is read from those calls)

Prints one JSON line (medians and min / max over --iters timed calls per leg, after --warmup calls each; the legs are interleaved so that clock and
co-tenant drift hit them alike). --root names another checkout of this repository whose built library is measured instead (one without
set_input_format runs the default leg only): the parent commit's figure comes from the same script on the same box.
    python tools/probes/resample_cost.py [--batch 64 --seconds 8 --iters 30 --warmup 5] [--root PATH]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

PKG = "automatic-speech-recognition-asr-onnx_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=8.0)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    cfgm, ckm, eng, _lib = (importlib.import_module(f"{PKG}.{m}") for m in ("config", "checkpoints", "engine", "_lib"))
    cfg = cfgm.sensevoice_small()
    arena = importlib.import_module(f"{PKG}.arena").build_sensevoice_arena(cfg, ckm.synth_sensevoice_checkpoint(cfg, 0), 0)
    can_resample = hasattr(eng.SenseVoiceSession, "set_input_format")
    # one session per leg: a session keeps ONE captured step per run form, so legs that alternate in one session would all run eagerly
    plain = eng.SenseVoiceSession(cfg, arena, 0)
    sess = eng.SenseVoiceSession(cfg, arena, 0, audio_dtype=np.int16) if can_resample else None
    resident = eng.SenseVoiceSession(cfg, arena, 0, audio_dtype=np.int16) if can_resample else None
    n = int(a.seconds * cfg.sample_rate)
    mono = ckm.synth_audio("kaldi", a.batch, n, seed=5).astype(np.float32).reshape(-1)
    offs = np.arange(a.batch + 1, dtype=np.int64) * n
    lang = np.zeros(a.batch, np.int32)
    rng = np.random.default_rng(5)
    stereo = rng.integers(-8000, 8000, size=a.batch * 3 * n * 2).astype(np.int16)       # 48 kHz, two interleaved channels
    offs48 = offs * 3
    lib, dptr = _lib.load(), C.c_void_p(None)

    def leg_default():
        return plain.run_packed(mono, offs, lang)

    def leg_stereo():
        return sess.run_packed(stereo, offs48, lang)

    def leg_resident():
        return resident.run_packed(None, offs48, lang, audio_device_ptr=dptr.value)

    legs = {"mono16k_f32_host": leg_default}
    if can_resample:
        sess.set_input_format(48000, 2)
        resident.set_input_format(48000, 2)
        _lib.check(lib.asr_mem_alloc(0, stereo.nbytes, C.byref(dptr)))
        _lib.check(lib.asr_mem_copy(0, dptr, stereo.ctypes.data_as(C.c_void_p), stereo.nbytes, 0))
        legs.update({"stereo48k_int16_host": leg_stereo, "stereo48k_int16_resident": leg_resident})
    for _ in range(a.warmup):
        for fn in legs.values():
            fn()
    times = {k: [] for k in legs}
    for _ in range(a.iters):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    out = {"probe": "resample_cost", "root": os.path.abspath(a.root), "model": "sensevoice_small", "precision": "bf16", "batch": a.batch, "seconds": a.seconds,
           "iters": a.iters, "audio_mb": {"mono16k_f32": mono.nbytes / 1e6, "stereo48k_int16": stereo.nbytes / 1e6}}
    for k, v in times.items():
        out[k + "_ms"] = {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}
    if can_resample:
        resident.profile(True)
        for _ in range(3):
            leg_resident()
        resident.profile_reset()
        for _ in range(a.iters):
            leg_resident()
        prof = resident.profile_read()["resample"]
        resident.profile(False)
        out["resampler_alone_ms"] = round(prof["total_ms"] / prof["launches"], 4)
        out["resampler_outputs"] = int(a.batch * n)
        _lib.check(lib.asr_mem_free(0, dptr))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
