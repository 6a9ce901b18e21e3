"""What int16 ingest is worth next to the step: SenseVoice-small bf16, 64 x 8 s, one session, a plain timing loop in a fresh process.

  f32 leg      the caller holds int16 PCM (what an audio decoder yields) and must widen it to float32 before the call: widening pass + 32.8 MB H2D + step
  int16 leg    the PCM goes in as it is: 16.4 MB H2D + step (the widening happens at the fbank kernel's load)
  resident leg the int16 audio already sits in HBM (asr_mem_alloc / asr_mem_copy): the step alone, for scale

Prints one JSON line (medians and min / max over --iters timed calls per leg, after --warmup calls each; the legs are interleaved so that clock and
co-tenant drift hit them alike).   python tools/probes/pcm_ingest_probe.py [--batch 64 --seconds 8 --iters 30 --warmup 5]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
PKG = "automatic-speech-recognition-asr-onnx_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=8.0)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    cfgm, ckm, eng, _lib = (importlib.import_module(f"{PKG}.{m}") for m in ("config", "checkpoints", "engine", "_lib"))
    cfg = cfgm.sensevoice_small()
    sess = eng.SenseVoiceSession.from_checkpoint(cfg, ckm.synth_sensevoice_checkpoint(cfg, 0), precision=0)
    n = int(a.seconds * cfg.sample_rate)
    pcm = ckm.synth_audio("kaldi", a.batch, n, seed=5).astype(np.int16).reshape(-1)
    offs = np.arange(a.batch + 1, dtype=np.int64) * n
    lang = np.zeros(a.batch, np.int32)
    lib, dptr = _lib.load(), C.c_void_p(None)
    _lib.check(lib.asr_mem_alloc(0, pcm.nbytes, C.byref(dptr)))
    _lib.check(lib.asr_mem_copy(0, dptr, pcm.ctypes.data_as(C.c_void_p), pcm.nbytes, 0))

    def leg_f32():
        sess.audio_dtype = np.float32
        return sess.run_packed(pcm.astype(np.float32), offs, lang)          # the widening pass is part of the leg

    def leg_i16():
        sess.audio_dtype = np.int16
        return sess.run_packed(pcm, offs, lang)

    def leg_resident():
        sess.audio_dtype = np.int16
        return sess.run_packed(None, offs, lang, audio_device_ptr=dptr.value)

    legs = {"f32_host_incl_widening": leg_f32, "int16_host": leg_i16, "int16_resident": leg_resident}
    ref = None
    for _ in range(a.warmup):
        for name, fn in legs.items():
            tok, num = fn()
            ref = (tok, num) if ref is None else ref
            assert np.array_equal(num, ref[1]) and np.array_equal(tok, ref[0]), name
    times = {k: [] for k in legs}
    widen = []
    for _ in range(a.iters):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        pcm.astype(np.float32)
        widen.append((time.perf_counter() - t0) * 1e3)
    _lib.check(lib.asr_mem_free(0, dptr))
    out = {"probe": "pcm_ingest", "model": "sensevoice_small", "precision": "bf16", "batch": a.batch, "seconds": a.seconds, "iters": a.iters,
           "audio_mb": {"f32": pcm.size * 4 / 1e6, "int16": pcm.nbytes / 1e6}}
    for k, v in list(times.items()) + [("host_widening_pass_alone", widen)]:
        out[k + "_ms"] = {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
