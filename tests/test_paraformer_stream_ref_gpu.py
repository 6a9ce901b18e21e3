"""Every path of the streaming Paraformer chunk step against the float64 reference of the step (tests/paraformer_stream_ref.py), per stream and per step.

One ParaformerStreamSession per (case, path) -- the dispatch switches are read at session creation -- on 1 + 3 encoder layers, 2 + 1 decoder blocks with
sharpened and planted attention, twelve stream slots, nine streams whose ids are neither dense nor in slot order, eight chunk steps (R.SCHEDULE): empty and
partial histories, a subset step, full histories beside partial ones, a reset stream (length 0) beside full ones in another subset, rolling histories. The run
is eager with taps and the profile on. Per step and active stream:

    encoder   encoder_exact on the session's OWN `enc_in` rows, the reference keeping its own K/V histories        stat(enc_out - exact) <= 3 x E_round
    decoder   decoder_exact on the session's OWN `enc_out` rows and its first n `list_frame` rows (n = the tokens   stat(logits - exact)  <= 3 x E_round
              the session returned; n = 0 advances no decoder state), the reference keeping carry and cache

with E_round = stat(exact - rounded) from the two references alone (the rounding points of the path: R.PATH_ROUNDINGS), both statistics (worst row's RMS, max
abs). The reference follows the session's fire decisions, so no (stream, step) is left out and no share of mismatches is tolerated. The f32 session has no
rounding model: it is held to TOL_F32 = 1e-3 of tests/test_paraformer_streaming_gpu.py (set against the reference goldens) in max abs. Also asserted: the history
lengths the kernels found (tap `s0_len`) are the reference's, 0 sits beside 36 in one launch, the fire counts cover 0 and 1 (sparse) / 2..8 and >= 9 (dense), the
tokens are the arg-max of the logits rows, the launch counts of the path in the profile of EVERY step (stream_dec is launched on a step where nothing fired as
well: its workgroups leave at once), no give-up, and the reset: behind its reset the stream's rows meet the reference restarted from empty state (it is one of
the (stream, step) above) and equal, bit for bit, the rows a fresh session gives for the same step.

The margin of 3 covers what the rounded twins do not model (f32 summation order, the hardware exp, statistics from rounded sums, flips of single roundings).
Measured stat / E_round on an MI355X, worst (stream, step) of each class (RMS ratio, then max-abs ratio); "mixed" = the steps whose launch holds more than one
history length (4 .. 7). No path needed a rounding point beyond those its kernels document (the encoder cluster launch sits at 1.7 where the per-launch layers
sit at 1.2 .. 1.6), the two workgroup-to-cluster maps give the same figures, and the steps with mixed lengths, the reset stream and the subset steps do not stand
out:

    case   path                     encoder        encoder mixed   decoder        decoder mixed
    sparse per_launch_separate_ln   1.22 1.39      1.22 1.26       1.08 1.15      1.05 1.15
    sparse per_launch_folded_ln     1.32 1.58      1.27 1.56       1.03 1.15      1.03 1.15
    sparse fused_encoder            1.72 1.65      1.72 1.65       1.01 1.05      1.01 1.04
    sparse fused_both               1.72 1.65      1.72 1.65       1.07 1.39      1.07 1.39
    sparse fused_old_placement      1.72 1.65      1.72 1.65       1.07 1.39      1.07 1.39
    dense  per_launch_separate_ln   1.22 1.39      1.22 1.26       1.07 1.21      1.07 1.21
    dense  per_launch_folded_ln     1.32 1.58      1.27 1.56       1.10 1.20      1.10 1.18
    dense  fused_encoder            1.72 1.65      1.72 1.65       1.06 1.31      1.06 1.31
    dense  fused_both               1.72 1.65      1.72 1.65       1.10 1.24      1.10 1.24
    dense  fused_old_placement      1.72 1.65      1.72 1.65       1.10 1.24      1.10 1.24
    f32_per_launch, max abs against the exact reference (bar 1e-3): sparse enc_out 3.81e-06 logits 2.32e-06; dense enc_out 3.81e-06 logits 3.25e-06

The planted mistakes this comparison catches, and by how much, are in tests/test_paraformer_stream_ref_cpu.py (there the rounded twin stands in for a kernel).
Once, off the GPU, on the rows recorded from the fused_both and per_launch_separate_ln sessions of both cases, with the mistake on the reference side: every
one of the thirteen made the comparison fail on every (stream, step) it applies to; the smallest failing statistic was 3.5 x E_round (cache_on_empty, sparse),
3.9 (mask_oldest, per-launch), 4.3 (hist_shift), 7.4 (no_roll) and above 10 for the other nine.
"""
import numpy as np
import pytest

import paraformer_stream_ref as R
from conftest import sub
from test_paraformer_streaming_gpu import TOL_F32

pytestmark = pytest.mark.gpu

BF16, F32 = 0, 1
# every dispatch switch of the streaming session, at its default; a path overrides some
DEFAULTS = {"ASR_STREAM_FUSED": "2", "ASR_LN_FUSED": "1", "ASR_STREAM_OPT": "0", "ASR_STREAM_SHARE": "0"}
UNSET = ("ASR_STREAM_FAULT", "ASR_STREAM_SNAPSHOT", "ASR_STREAM_TIMES", "ASR_NO_GRAPH", "ASR_STREAM_FUSED_MAX")
# name -> (precision, environment, stream_layers / stream_dec launches per step)
PATHS = {
    "per_launch_separate_ln": (BF16, {"ASR_STREAM_FUSED": "0", "ASR_LN_FUSED": "0"}, (0, 0)),
    "per_launch_folded_ln": (BF16, {"ASR_STREAM_FUSED": "0", "ASR_LN_FUSED": "1"}, (0, 0)),
    "fused_encoder": (BF16, {"ASR_STREAM_FUSED": "1"}, (1, 0)),
    "fused_both": (BF16, {"ASR_STREAM_FUSED": "2"}, (1, 1)),
    "fused_old_placement": (BF16, {"ASR_STREAM_FUSED": "2", "ASR_STREAM_OPT": "8"}, (1, 1)),
    "f32_per_launch": (F32, {}, (0, 0)),
}
BF16_PATHS = [p for p in PATHS if PATHS[p][0] == BF16]
ROWS = 13                                                        # live rows of a 16-row slot


def _session(monkeypatch, case, path, max_streams=R.MAX_STREAMS):
    for k in UNSET:
        monkeypatch.delenv(k, raising=False)
    for k, v in {**DEFAULTS, **PATHS[path][1]}.items():
        monkeypatch.setenv(k, v)
    cfg, ck, chunk = R.case(case)
    return sub("engine").ParaformerStreamSession(cfg, ck, precision=PATHS[path][0], chunk=chunk, max_streams=max_streams)


def _step(sess, sids, chunks):
    """One eager chunk step with taps and the profile on: ({stream: its rows of the taps}, the history lengths the step found, the profile of this step)."""
    sess.profile_reset()
    toks = sess.step(chunks, list(sids))
    prof = sess.profile_read()
    enc_in, enc_out, frames, logits = (sess.tap(n) for n in ("enc_in", "enc_out", "list_frame", "logits"))
    lens = sess.tap("s0_len", dtype=np.int32)[:, 0]
    out = {}
    for slot, s in enumerate(sids):
        r0, n = 16 * slot, int(toks[slot].size)
        out[s] = dict(enc_in=enc_in[r0:r0 + ROWS].copy(), enc_out=enc_out[r0:r0 + ROWS].copy(), frames=frames[r0:r0 + n].copy(), logits=logits[r0:r0 + n].copy(),
                      tokens=toks[slot], len=int(lens[s]))
    return out, prof


def _run(sess, chunk):
    sess.taps(True)
    sess.profile(True)
    record, profs = [], []
    for resets, sids, chunks in R.schedule_chunks(chunk):
        for s in resets:
            sess.reset(s)
        rows, prof = _step(sess, sids, chunks)
        record.append(rows)
        profs.append(prof)
    return record, profs


def _check_launches(cfg, path, profs):
    """The cluster launches of the path ran on every step (and only there); the per-launch attention kernel ran the layers they did not."""
    layers, dec = PATHS[path][2]
    n_blocks = cfg.n_enc0 + cfg.n_enc
    for k, prof in enumerate(profs):
        n = lambda name: prof.get(name, {}).get("launches", 0)
        assert (n("stream_layers"), n("stream_dec")) == (layers, dec), (path, k, prof)
        assert n("attention") == (1 if layers else n_blocks) + (0 if dec else cfg.n_dec), (path, k, prof)
        assert n("gemm_qkv") == (1 if layers else n_blocks), (path, k, prof)


def _check_state_and_coverage(case, record, enc):
    for k, rows in enumerate(record):
        for s, r in rows.items():
            assert r["len"] == enc[(k, s)]["len"], (k, s)                                                # the kernels found the history length the reference holds
            assert np.array_equal(r["tokens"], r["logits"].argmax(axis=1)), (k, s)
            assert all(np.isfinite(r[f]).all() for f in ("enc_out", "frames", "logits")), (k, s)
    lens5 = {r["len"] for r in record[5].values()}
    assert record[5][R.RESET_STREAM]["len"] == 0 and 36 in lens5, lens5
    assert all(len({r["len"] for r in record[k].values()}) > 1 for k in R.MIXED_STEPS)
    counts = {int(r["tokens"].size) for rows in record for r in rows.values()}
    if case == "sparse":
        assert 0 in counts and 1 in counts, counts
    else:
        assert any(2 <= n <= 8 for n in counts) and any(n >= 9 for n in counts), counts


def _worst(entries, steps=None):
    """Worst (RMS ratio, max-abs ratio) over the entries (of the given steps), each with its (step, stream)."""
    out = []
    for i in (0, 1):
        c = [(e["ratio"][i], key) for key, e in entries.items() if steps is None or key[0] in steps]
        out.append(max(c) if c else (float("nan"), None))
    return out


def _against_the_reference(monkeypatch, case, path):
    cfg, ck, chunk = R.case(case)
    sess = _session(monkeypatch, case, path)
    record, profs = _run(sess, chunk)
    st = sess.stream_stats()
    assert st["giveups"] == 0 and st["shared_steps"] == 0 and st["can_fuse"] == (PATHS[path][2][0] == 1), st
    _check_launches(cfg, path, profs)
    rnd = R.PATH_ROUNDINGS.get(path, R.BASE_ROUNDINGS)
    enc, dec = R.encoder_runs(cfg, ck, record, rnd), R.decoder_runs(cfg, ck, record, rnd)
    _check_state_and_coverage(case, record, enc)
    assert set(dec) == {(k, s) for k, rows in enumerate(record) for s, r in rows.items() if r["tokens"].size}
    for entries, field in ((enc, "enc_out"), (dec, "logits")):
        for (k, s), e in entries.items():
            e = entries[(k, s)] = dict(e)                                                                 # (the encoder's entries are cached across paths)
            e["stat"] = R.stat(record[k][s][field].astype(np.float64) - e["exact"])
            e["ratio"] = (e["stat"][0] / e["e_round"][0], e["stat"][1] / e["e_round"][1])
    # the reset: a fresh session on the same step (same launch shapes; every other stream empty instead of full) gives the reset stream's rows bit for bit
    fresh = _session(monkeypatch, case, path)
    fresh.taps(True)
    fresh.profile(True)
    resets, sids, chunks = R.schedule_chunks(chunk)[5]
    assert sids[0] == R.RESET_STREAM and resets == (R.RESET_STREAM,)
    again, _ = _step(fresh, sids, chunks)
    for f in ("enc_in", "enc_out", "frames", "logits"):
        assert np.array_equal(again[R.RESET_STREAM][f], record[5][R.RESET_STREAM][f]), (path, f)
    return enc, dec


def _fmt(w):
    return f"{w[0][0]:.2f} {w[1][0]:.2f}"


@pytest.mark.parametrize("path", BF16_PATHS)
@pytest.mark.parametrize("case", ["sparse", "dense"])
def test_chunk_steps_against_the_float64_reference(monkeypatch, case, path):
    enc, dec = _against_the_reference(monkeypatch, case, path)
    print(f"\n    {case:6s} {path:24s} {_fmt(_worst(enc)):14s} {_fmt(_worst(enc, R.MIXED_STEPS)):15s} {_fmt(_worst(dec)):14s} {_fmt(_worst(dec, R.MIXED_STEPS))}")
    print("      worst at (step, stream): encoder", [w[1] for w in _worst(enc)], "decoder", [w[1] for w in _worst(dec)])
    over = [(name, key, e["stat"], e["e_round"]) for name, entries in (("encoder", enc), ("decoder", dec)) for key, e in sorted(entries.items())
            if e["ratio"][0] > R.MARGIN or e["ratio"][1] > R.MARGIN]
    assert not over, (case, path, len(over), over[:6])


@pytest.mark.parametrize("case", ["sparse", "dense"])
def test_f32_chunk_steps_against_the_float64_reference(monkeypatch, case):
    enc, dec = _against_the_reference(monkeypatch, case, "f32_per_launch")
    worst = [max(e["stat"][1] for e in entries.values()) for entries in (enc, dec)]
    print(f"\n    {case} f32_per_launch max abs: enc_out {worst[0]:.2e}, logits {worst[1]:.2e}")
    over = [(name, key, e["stat"]) for name, entries in (("encoder", enc), ("decoder", dec)) for key, e in sorted(entries.items()) if not e["stat"][1] < TOL_F32]
    assert not over, (case, len(over), over[:6])
