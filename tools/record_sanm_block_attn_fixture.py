"""Record tests/golden/sanm_block_attn_parent.npz: the block kernel's results on the window lengths at which its attention half takes another path.

Run on an MI355X from the commit whose results are to be pinned (the parent of a change to phase A of csrc/sanm_block8.hip):

    python tools/record_sanm_block_attn_fixture.py --commit $(git rev-parse HEAD)

sensevoice_small with the seeded checkpoint of tests/helpers.py, bf16, ASR_SANM_BLOCK=1 and ASR_SANM_BLOCK_MIN=1, one ragged batch whose windows
have T = 128 (no shared ninth tile), 129 (one valid row in it), 130, 137, 143, 144 (a full ninth tile), 113 / 97 / 33 (4 / 3 / 2 sub-tiles of 32 keys)
and 5 (a single tile). Stored: the `enc_out` tap (f32) of the first 16 and the last 16 rows of every window, all token ids, and what
tests/test_sanm_block_attn_gpu.py needs to rebuild the batch (lengths, seeds, languages).
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "automatic-speech-recognition-asr-onnx_amd"
WINDOW_ROWS = (128, 129, 130, 137, 143, 144, 113, 97, 33, 5)
SEED0 = 700


def samples_for_rows(T: int) -> int:
    """Audio length of a window of T encoder rows: 4 prompt rows + n_lfr frames of 6 fbank frames (25 ms window, 10 ms hop at 16 kHz)."""
    n_frames = 6 * (T - 4)
    return 400 + 160 * (n_frames - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit this library was built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "sanm_block_attn_parent.npz"))
    args = ap.parse_args()
    os.environ["ASR_SANM_BLOCK"] = "1"
    os.environ["ASR_SANM_BLOCK_MIN"] = "1"
    os.environ.pop("ASR_SANM_BLOCK_SCATTER", None)
    cfgm, ckm, eng = (importlib.import_module(f"{PKG}.{m}") for m in ("config", "checkpoints", "engine"))
    cfg = cfgm.sensevoice_small()
    ck = ckm.synth_sensevoice_checkpoint(cfg, 0)
    lens = [samples_for_rows(T) for T in WINDOW_ROWS]
    assert samples_for_rows(144) == 134640
    seeds = [SEED0 + i for i in range(len(lens))]
    langs = [i % 7 for i in range(len(lens))]
    audios = [ckm.synth_audio("kaldi", 1, n, seed=s)[0, 0] for s, n in zip(seeds, lens)]
    sess = eng.SenseVoiceSession.from_checkpoint(cfg, ck, precision=0)
    rows = sess.utterance_rows(lens)
    assert [T for _, T in rows] == list(WINDOW_ROWS), rows
    sess.taps(True)
    toks = sess.run(audios, langs)
    enc = sess.tap("enc_out")
    sess.profile(True)
    sess.profile_reset()
    again = sess.run(audios, langs)
    assert "sanm_block" in set(sess.profile_read()), "the batch did not take the block kernel"
    assert all(np.array_equal(x, y) for x, y in zip(toks, again))
    out = {"commit": np.array(args.commit), "window_rows": np.array(WINDOW_ROWS, np.int32), "lens": np.array(lens, np.int64),
           "seeds": np.array(seeds, np.int32), "langs": np.array(langs, np.int32)}
    for i, ((r0, T), tok) in enumerate(zip(rows, toks)):
        out[f"w{i}_head"] = np.ascontiguousarray(enc[r0:r0 + min(16, T)], np.float32)
        out[f"w{i}_tail"] = np.ascontiguousarray(enc[r0 + max(0, T - 16):r0 + T], np.float32)
        out[f"w{i}_tokens"] = np.asarray(tok, np.int32)
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes; tokens per window:", [len(t) for t in toks])


if __name__ == "__main__":
    main()
