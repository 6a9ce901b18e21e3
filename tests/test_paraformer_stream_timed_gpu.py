"""GPU, session level: ParaformerStreamSession.step_timed / asr_paraformer_stream_step_timed -- ids equal a twin session's `step`, the fire steps equal the
f32 restatement of the integrate-and-fire on the tapped alphas (with the carried weight the test tracks itself), the log-probabilities match the float64
statement of the tapped logits within launch_argmax_logprob_rows' budget, and the session's chunk counting gives non-decreasing absolute rows."""
import numpy as np
import pytest

import paraformer_timing_ref as R
import token_scores_ref as S
from conftest import sub
from helpers import kaldi_audio, load_golden
from test_oracle_paraformer_streaming import streaming_setup

pytestmark = pytest.mark.gpu

BF16, F32 = 0, 1


def _setup(fixture):
    g = load_golden(fixture)
    cfg, ck = streaming_setup(g)
    return cfg, ck, int(g["chunk"])


@pytest.mark.parametrize("fixture,prec", [("paraformer_streaming_tiny", F32), ("paraformer_streaming_large", BF16)])
def test_timed_steps_equal_a_twin_session_and_the_reference(fixture, prec, monkeypatch):
    monkeypatch.setenv("ASR_STREAM_SHARE", "0")          # the twins alternate on this GPU: the co-tenancy rule would move one of them to the per-launch path
    cfg, ck, chunk = _setup(fixture)
    eng = sub("engine")
    n_chunks = [5, 4, 3]                                  # three streams of unequal length: the active set shrinks
    sids = [2, 0, 1]                                      # slots != stream ids
    audio = [kaldi_audio(7300 + i, n * chunk) for i, n in enumerate(n_chunks)]
    timed = eng.ParaformerStreamSession(cfg, ck, precision=prec, chunk=chunk, max_streams=3)
    twin = eng.ParaformerStreamSession(cfg, ck, precision=prec, chunk=chunk, max_streams=3)
    timed.taps(True)
    B, Cr = timed.rows_per_chunk, timed.rows_carried
    assert (B, Cr) == (9, 4)
    carried = {s: np.float32(0.0) for s in sids}
    last_row = {s: 0 for s in sids}
    total = 0
    worst = 0.0
    for k in range(max(n_chunks)):
        live = [i for i, n in enumerate(n_chunks) if k < n]
        block = np.stack([audio[i][k * chunk:(k + 1) * chunk] for i in live])
        ids_live = [sids[i] for i in live]
        recs = timed.step_timed(block, ids_live)
        plain = twin.step(block, ids_live)
        alphas, logits = timed.tap("alphas")[:, 0], timed.tap("logits")
        fire_tap, lp_tap = timed.tap("fire_frames", dtype=np.int32), timed.tap("token_logprob")
        for slot, (sid, rec, u) in enumerate(zip(ids_live, recs, plain)):
            assert np.array_equal(rec["ids"], u), (k, sid)
            n = len(rec["ids"])
            steps, carried[sid] = R.stream_fire_steps(alphas[16 * slot:16 * slot + B], carried[sid])
            assert np.array_equal(rec["fire_step"], steps), (k, sid, rec["fire_step"], steps)
            assert (rec["fire_step"] >= -1).all() and (rec["fire_step"] < B).all() and (np.diff(rec["fire_step"]) > 0).all()
            assert np.array_equal(rec["row"], R.absolute_rows(steps, k, B, Cr))
            assert np.array_equal(fire_tap[slot, :n], steps) and np.array_equal(lp_tap[slot, :n].view(np.uint32), rec["logprob"].view(np.uint32))
            if n:
                assert rec["row"][0] >= last_row[sid] and (np.diff(rec["row"]) >= 0).all()
                last_row[sid] = int(rec["row"][-1])
                ref_ids, score, M, lse = S.argmax_scores(logits[16 * slot:16 * slot + n])
                assert np.array_equal(rec["ids"], ref_ids)
                worst = max(worst, S.over_budget(rec["logprob"], score, S.fused_budget(cfg.vocab, M, lse)))
                assert (rec["logprob"] <= 0).all() and np.isfinite(rec["logprob"]).all()
            total += n
    print(f"streaming token logprob vs the float64 log soft-max of the logits tap: max err / budget {worst:.3f} over {total} tokens")
    assert total > 0 and worst <= 1.0
    assert timed.chunks_done.tolist() == [4, 3, 5]       # indexed by stream id
    # reset restarts the chunk count of that stream only; the reset stream steps like a fresh session
    timed.reset(2)
    assert timed.chunks_done.tolist() == [4, 3, 0]
    first = timed.step_timed(audio[0][:chunk][None], [2])[0]
    fresh = eng.ParaformerStreamSession(cfg, ck, precision=prec, chunk=chunk, max_streams=1)
    want = fresh.step_timed(audio[0][:chunk][None], [0])[0]
    for key in ("ids", "fire_step", "row"):
        assert np.array_equal(first[key], want[key]), key
    assert np.array_equal(first["logprob"].view(np.uint32), want["logprob"].view(np.uint32))
    assert (first["row"] <= B - 1 - Cr).all() and timed.chunks_done[2] == 1
    for s in (timed, twin, fresh):
        s.close()


@pytest.mark.parametrize("snapshot", ["0", "1"])
def test_step_and_step_timed_interleaved(snapshot, monkeypatch):
    """One bf16 session alternating the two forms (captured graphs of both, fused launches; with ASR_STREAM_SNAPSHOT=1 the fused step behind a state
    snapshot) gives the ids of an all-`step` session, and its timed chunks give what an all-`step_timed` session gives."""
    monkeypatch.setenv("ASR_STREAM_SHARE", "0")
    monkeypatch.setenv("ASR_STREAM_SNAPSHOT", snapshot)
    cfg, ck, chunk = _setup("paraformer_streaming_large")
    eng = sub("engine")
    audio = [kaldi_audio(7400 + i, 6 * chunk) for i in range(2)]
    mixed, plain, timed = (eng.ParaformerStreamSession(cfg, ck, precision=BF16, chunk=chunk, max_streams=2) for _ in range(3))
    total = 0
    for k in range(6):
        block = np.stack([a[k * chunk:(k + 1) * chunk] for a in audio])
        want = plain.step(block, [0, 1])
        full = timed.step_timed(block, [0, 1])
        if k in (1, 2, 4):
            recs = mixed.step_timed(block, [0, 1])
            got = [r["ids"] for r in recs]
            for r, f in zip(recs, full):
                assert np.array_equal(r["fire_step"], f["fire_step"]) and np.array_equal(r["row"], f["row"])
                assert np.array_equal(r["logprob"].view(np.uint32), f["logprob"].view(np.uint32))
        else:
            got = mixed.step(block, [0, 1])
        for g, w, f in zip(got, want, full):
            assert np.array_equal(g, w) and np.array_equal(f["ids"], w), k
            total += len(w)
    assert total > 0
    stats = mixed.stream_stats()
    assert stats["can_fuse"] and (stats["snapshots"] == 6) == (snapshot == "1")
    for s in (mixed, plain, timed):
        s.close()


def test_stream_transcriber_timestamps():
    """transcribe_many(timestamps=True): the ids and the text of the untimed loop, one record per kept token, spans in seconds of the clip."""
    from test_oracle_paraformer_streaming import streaming_cases
    g = load_golden("paraformer_streaming_tiny")
    cfg, ck = streaming_setup(g)
    chunk = int(g["chunk"])
    vocab = [f"t{i}" for i in range(cfg.vocab)]
    vocab[2] = "</s>"
    sess = sub("engine").ParaformerStreamSession(cfg, ck, precision=F32, chunk=chunk, max_streams=2)
    tr = sub("paraformer_streaming").ParaformerStreamTranscriber(sess, vocab, stop_token_ids=[2], decode_mode="zh")
    cases = [c for _, c in streaming_cases(g)][:2]
    clips = [kaldi_audio(c["audio_seed"], int(c["n_chunks"]) * chunk).astype(np.int16) for c in cases]
    plain, _ = tr.transcribe_many(clips)
    timed, _ = tr.transcribe_many(clips, timestamps=True)
    again, _ = tr.transcribe_many(clips)
    row_s = cfg.lfr_n * cfg.hop_length / cfg.sample_rate
    total = 0
    for p, t, a, clip in zip(plain, timed, again, clips):
        assert set(t) == set(p) | {"tokens"} and "tokens" not in a
        assert np.array_equal(p["token_ids"], t["token_ids"]) and np.array_equal(p["token_ids"], a["token_ids"]) and p["text"] == t["text"] == a["text"]
        toks, dur = t["tokens"], clip.size / cfg.sample_rate
        assert [k["id"] for k in toks] == t["token_ids"].tolist()             # stop ids dropped with their records
        assert all(set(k) == {"id", "text", "start", "end", "logprob"} and k["text"] == vocab[k["id"]] and k["logprob"] <= 0 for k in toks)
        assert all(0.0 <= k["start"] <= k["end"] <= dur and k["end"] - k["start"] <= 4 * row_s + 1e-9 for k in toks)
        assert all(x["end"] <= y["start"] for x, y in zip(toks, toks[1:]))        # in order, no overlap
        total += len(toks)
    assert total > 0
    sess.close()
