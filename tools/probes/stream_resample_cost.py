"""What the streaming input format costs (asr_session_set_input_format on a streaming Paraformer session, csrc/resample.hip launch_resample_stream): one
Paraformer-large session, 64 streams, chunk 8000 (0.5 s), bf16, int16 audio -- a chunk step with the default format against the same step with 48 kHz stereo
rows (64 x 24100 x 2 int16 = 6.2 MB per step instead of 1.0 MB), each from host memory and HBM-resident.

  step legs   a host clock around the synchronous ParaformerStreamSession.step (the staging copy, the captured step, the result copies), medians and min / max
              over --iters steps after --warmup. The four legs take turns in ONE session; a full reset in front of every turn lets the format change (a format
              is accepted only while no stream carries frames)

The default-format figures are what the parent commit's step costs: the default format launches what it launched. Prints one JSON line.
    python tools/probes/stream_resample_cost.py [--iters 20 --warmup 4 --streams 64]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

PKG = "automatic-speech-recognition-asr-onnx_amd"
CHUNK, RATE, CHANNELS = 8000, 48000, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    eng, _lib, cfgm, ckm, fmt = (importlib.import_module(f"{PKG}.{m}") for m in ("engine", "_lib", "config", "checkpoints", "input_format"))
    lib = _lib.load()
    cfg = cfgm.paraformer_large()
    n = a.streams
    sess = eng.ParaformerStreamSession(cfg, ckm.synth_paraformer_checkpoint(cfg, 0), precision=0, chunk=CHUNK, max_streams=n, audio_dtype=np.int16)
    ids = np.arange(n, dtype=np.int32)
    rng = np.random.default_rng(5)
    pitch = fmt.stream_pitch(CHUNK, RATE, cfg.sample_rate)
    audio = {"default": np.round(rng.standard_normal((n, CHUNK)) * 3000.0).astype(np.int16),
             "48k_stereo": np.round(rng.standard_normal((n, pitch, CHANNELS)) * 3000.0).astype(np.int16)}
    dptr = {}
    for k, v in audio.items():
        dptr[k] = C.c_void_p(None)
        _lib.check(lib.asr_mem_alloc(0, v.nbytes, C.byref(dptr[k])))
        _lib.check(lib.asr_mem_copy(0, dptr[k], v.ctypes.data_as(C.c_void_p), v.nbytes, 0))
    legs = [(k, where) for k in audio for where in ("host", "resident")]
    times = {f"{k}_{where}": [] for k, where in legs}
    per_turn = a.warmup + a.iters
    for k, where in legs:                                   # one turn per leg: reset, format, warm-up steps (eager, capture), timed replays
        sess.reset(-1)
        sess.set_input_format(*((RATE, CHANNELS) if k == "48k_stereo" else (cfg.sample_rate, 1)))
        for it in range(per_turn):
            t0 = time.perf_counter()
            if where == "host":
                sess.step(audio[k], ids)
            else:
                sess.step(None, ids, audio_device_ptr=dptr[k].value)
            if it >= a.warmup:
                times[f"{k}_{where}"].append((time.perf_counter() - t0) * 1e3)
    out = {"probe": "stream_resample_cost", "streams": n, "chunk": CHUNK, "precision": "bf16", "audio": "int16", "format": [RATE, CHANNELS], "pitch": pitch,
           "iters": a.iters, "step_mb": {k: round(v.nbytes / 1e6, 3) for k, v in audio.items()}}
    for k, v in times.items():
        out[k + "_ms"] = {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}
    for p in dptr.values():
        _lib.check(lib.asr_mem_free(0, p))
    sess.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
