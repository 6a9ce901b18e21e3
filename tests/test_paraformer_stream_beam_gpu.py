"""GPU, session level: ParaformerStreamSession.step_beam / finish_beam (asr_paraformer_stream_step_beam / _finish_beam) on the tiny streaming fixture, f32
and bf16. The tiny geometry (d_model 256, two heads) has no cluster launches -- stream_stats, printed by the fixture, says can_fuse False -- so both
precisions run the per-launch path; the cluster-launch path ran under the mode in tools/probes/paraformer_stream_beam_probe.py (Paraformer-large).

Without hotwords and model the step's greedy outputs are step_timed's bytes and the committed tokens followed by the finish's best tail are the
concatenation of `step`'s ids; the session's search outputs equal engine.op_nar_stream_beam on the tapped candidates byte for byte and the float64
statement (tests/nar_stream_beam_ref.py) where its decisions are clear; a hotword phrase and a bigram of second-best tokens that straddle a chunk border
come to the front; reset and the setters treat the search state as the issue of history it is; and the other step forms launch what they launched."""
import ctypes

import numpy as np
import pytest

import ctc_lm_ref as L
import nar_stream_beam_ref as S
from conftest import sub
from helpers import kaldi_audio, load_golden
from test_oracle_paraformer_streaming import streaming_setup
from test_paraformer_beam_gpu import _launches, _pairs, _smallest

pytestmark = pytest.mark.gpu

BF16, F32 = 0, 1
GAP, TOL = L.GAP, min(6 * 1.7e-5, L.GAP / 4)             # test_nar_stream_beam_gpu.py's bound
CHUNKS = {0: 8, 2: 5, 3: 6}                              # stream id -> chunks of its clip: the streams end at different chunks
BEAM, TOPK, NBEST, CAP = 4, 4, 2, 3
HOT_CAP = 4                                              # the hotword / bigram test: the longest clip fires 13 tokens, so its stream saturates


@pytest.fixture(scope="module", params=[F32, BF16], ids=["f32", "bf16"])
def tiny(request):
    g = load_golden("paraformer_streaming_tiny")
    cfg, ck = streaming_setup(g)
    chunk = int(g["chunk"])
    eng = sub("engine")
    make = lambda: eng.ParaformerStreamSession(cfg, ck, precision=request.param, chunk=chunk, max_streams=4)
    mp = pytest.MonkeyPatch()
    mp.setenv("ASR_STREAM_SHARE", "0")                     # (the two sessions alternate on this GPU: the co-tenancy rule would move one of them to the per-launch path)
    try:
        beam, twin = make(), make()
    finally:
        mp.undo()
    audio = {s: kaldi_audio(3600 + s, n * chunk) for s, n in CHUNKS.items()}
    print(f"precision {request.param}: stream_stats {beam.stream_stats()}")
    yield cfg, chunk, beam, twin, audio
    beam.close()
    twin.close()


def _live(k):
    return [s for s, n in CHUNKS.items() if k < n]


def _chunks(audio, chunk, k, sids):
    return np.stack([audio[s][k * chunk:(k + 1) * chunk] for s in sids])


def _run_all(sess, audio, chunk, tap=False):
    """Every clip through step_beam, each stream finished behind its last chunk. Returns per stream (greedy records, committed ids, committed logprob,
    committed rows, finish record, per-step results) and, with `tap`, the candidates of every step's token rows."""
    sess.reset()
    out = {s: {"greedy": [], "ids": [], "lp": [], "row": [], "steps": [], "cand": []} for s in CHUNKS}
    for k in range(max(CHUNKS.values())):
        sids = _live(k)
        recs = sess.step_beam(_chunks(audio, chunk, k, sids), sids)
        if tap:
            cid, clp = sess.tap("cand_ids", dtype=np.int32), sess.tap("cand_logprob")
        for slot, (s, r) in enumerate(zip(sids, recs)):
            o = out[s]
            o["greedy"].append(r)
            o["steps"].append(r)
            o["ids"] += r["committed"]["ids"].tolist(); o["lp"] += r["committed"]["logprob"].tolist(); o["row"] += r["committed"]["row"].tolist()
            if tap:
                n = len(r["ids"])
                o["cand"].append((cid[16 * slot:16 * slot + n].copy(), clp[16 * slot:16 * slot + n].copy()))
        done = [s for s in sids if k == CHUNKS[s] - 1]
        if done:
            for s, f in zip(done, sess.finish_beam(done)):
                o = out[s]
                o["finish"] = f
                o["ids"] += f["committed"]["ids"].tolist(); o["lp"] += f["committed"]["logprob"].tolist(); o["row"] += f["committed"]["row"].tolist()
    return out


def test_plain_search_is_the_greedy_stream_and_the_timed_steps_bytes(tiny):
    cfg, chunk, beam, twin, audio = tiny
    beam.set_beam(BEAM, TOPK, NBEST, CAP)
    got = _run_all(beam, audio, chunk)
    twin.reset()
    timed = {s: [] for s in CHUNKS}
    for k in range(max(CHUNKS.values())):
        sids = _live(k)
        for s, r in zip(sids, twin.step_timed(_chunks(audio, chunk, k, sids), sids)):
            timed[s].append(r)
    twin.reset()
    plain = {s: [] for s in CHUNKS}
    for k in range(max(CHUNKS.values())):
        sids = _live(k)
        for s, ids in zip(sids, twin.step(_chunks(audio, chunk, k, sids), sids)):
            plain[s] += ids.tolist()
    saturated = 0
    for s in CHUNKS:
        for a, b in zip(got[s]["greedy"], timed[s]):
            for key in ("ids", "fire_step", "row", "logprob"):
                assert a[key].tobytes() == b[key].tobytes(), (s, key)
        want_lp = np.concatenate([r["logprob"] for r in timed[s]]).tolist()
        want_row = np.concatenate([r["row"] for r in timed[s]]).tolist()
        assert got[s]["ids"] == plain[s] and len(plain[s]) > CAP, s             # committed tokens, then the finish's tail 0: the greedy stream
        # ... with the greedy picks' fire rows, and their scores up to the rounding of a second log soft-max (the candidate kernel sums the row in another order
        # than the timed head: a few ulps of a value near 4)
        assert got[s]["row"] == want_row and np.allclose(got[s]["lp"], want_lp, rtol=0.0, atol=1e-5)
        f = got[s]["finish"]
        assert f["total"] == len(plain[s]) and len(f["committed"]["ids"]) == min(CAP, len(plain[s]))
        assert f["pending"][0]["ids"].tolist() == f["committed"]["ids"].tolist() and f["pending"][0]["score"] == f["pending"][0]["am_score"]
        saturated += sum(len(r["committed"]["ids"]) for r in got[s]["steps"])
        for r in got[s]["steps"]:                            # every report: at most CAP pending, best first, totals add up
            assert all(len(p["ids"]) == min(r["total"], CAP) for p in r["pending"]) and len(r["pending"]) <= NBEST
            assert all(x["score"] >= y["score"] for x, y in zip(r["pending"][:-1], r["pending"][1:]))
    assert saturated > 0                                     # forced commits happened inside steps


def test_search_on_the_tapped_candidates_is_the_op_and_the_float64_statement(tiny):
    cfg, chunk, beam, twin, audio = tiny
    eng = sub("engine")
    beam.set_beam(BEAM, TOPK, NBEST, CAP)
    beam.taps(True)
    try:
        got = _run_all(beam, audio, chunk, tap=True)
    finally:
        beam.taps(False)
    clear = 0
    for s in CHUNKS:
        cand = got[s]["cand"]
        assert all(c[0].shape == (len(r["ids"]), TOPK) for c, r in zip(cand, got[s]["steps"]))
        for (cid, clp), r in zip(cand, got[s]["steps"]):      # column 0 is the greedy pick with its score; columns in descending order, ids distinct
            assert cid[:, 0].tolist() == r["ids"].tolist() and np.allclose(clp[:, 0], r["logprob"], atol=1e-5)
            assert np.all(np.diff(clp, axis=1) <= 0) and all(len(set(row)) == TOPK for row in cid.tolist())
        steps = [[(0, cid, clp, False)] for cid, clp in cand] + [[(0, cand[0][0][:0], cand[0][1][:0], True)]]
        op = eng.op_nar_stream_beam(steps, 1, BEAM, NBEST, CAP)
        ref = S.NarStreamBeam(BEAM, NBEST, CAP)
        refs = [ref.step(cid, clp) for cid, clp in cand] + [ref.finish()]
        for k, (o, r) in enumerate(zip(op, got[s]["steps"] + [got[s]["finish"]])):
            nc = int(o["commit_num"][0])
            assert o["commit_ids"][0, :nc].tobytes() == r["committed"]["ids"].tobytes() and o["commit_logprob"][0, :nc].tobytes() == r["committed"]["logprob"].tobytes()
            assert int(o["total"][0]) == r["total"] and len(r["pending"]) == int(np.isfinite(o["pend_score"][0]).sum())
            for m, p in enumerate(r["pending"]):
                n = int(o["pend_num"][0, m])
                assert o["pend_ids"][0, m, :n].tobytes() == p["ids"].tobytes() and o["pend_logprob"][0, m, :n].tobytes() == p["logprob"].tobytes()
                assert np.float32(p["score"]) == o["pend_score"][0, m] and np.float32(p["am_score"]) == o["pend_am"][0, m]
        print(f"stream {s}: {len(got[s]['ids'])} tokens, decision gap {ref.gap:.2e}")
        if ref.gap >= GAP:
            clear += 1
            for w, r in zip(refs, got[s]["steps"] + [got[s]["finish"]]):
                assert r["committed"]["ids"].tolist() == [c for c, _ in w["commit"]] and r["total"] == w["total"]
                assert [p["ids"].tolist() for p in r["pending"]] == [p["tokens"] for p in w["pending"]]
                assert all(max(abs(p["score"] - q["score"]), abs(p["am_score"] - q["am_score"])) <= TOL for p, q in zip(r["pending"], w["pending"]))
    assert clear >= 1


def _border_pairs(cand):
    """_pairs of test_paraformer_beam_gpu.py over the stream's rows, the pairs that straddle a chunk border only"""
    cid, clp = np.concatenate([c[0] for c in cand]), np.concatenate([c[1] for c in cand])
    borders = set(np.cumsum([len(c[0]) for c in cand])[:-1].tolist())
    return cid, clp, [p for p in _pairs(cid, clp) if p[0] + 1 in borders]


def _flip(pairs, base, make_search, hi_of):
    for k, phrase, loss in pairs:
        made, search = make_search(phrase)
        changes = lambda x: search(x)[0] != base
        if not changes(hi_of(loss)):
            continue
        least = _smallest(changes, hi_of(loss))
        want, gap = search(1.5 * least)
        if want[k:k + 2] == phrase:
            return k, phrase, made, least, want, gap
    raise AssertionError("no pair of second-best tokens across a chunk border that the reference brings to the front")


def _reference(cand, **kw):
    ref = S.NarStreamBeam(8, 1, HOT_CAP, **kw)
    res = [ref.step(cid, clp) for cid, clp in cand] + [ref.finish()]
    return [c for r in res for c, _ in r["commit"]], ref.gap


def test_a_hotword_phrase_and_a_bigram_across_a_chunk_border_come_to_the_front(tiny):
    cfg, chunk, beam, twin, audio = tiny
    beam.set_beam(8, 4, 1, HOT_CAP)
    beam.taps(True)
    try:
        cand = _run_all(beam, audio, chunk, tap=True)[0]["cand"]
    finally:
        beam.taps(False)
    cid, clp, pairs = _border_pairs(cand)
    base, _ = _reference(cand)
    assert base == cid[:, 0].tolist() and pairs and len(base) > HOT_CAP                    # (the stream saturates: the phrase also straddles forced commits)

    def hot_search(phrase):
        trie = S.build_trie([phrase])
        return trie, lambda x: _reference(cand, trie=trie, boost=x)
    k, phrase, _, least, want, gap = _flip(pairs, base, hot_search, lambda loss: loss + 1.0)
    print(f"rows {k}, {k + 1}: phrase {phrase}, least boost {least:.4f}, gap at 1.5 x {gap:.2e}")
    try:
        beam.set_hotwords([phrase], 1.5 * least)
        hot = _run_all(beam, audio, chunk)[0]
        assert hot["ids"][k:k + 2] == phrase and hot["ids"] != base
        if gap >= GAP:
            assert hot["ids"] == want
    finally:
        beam.set_hotwords([], 0.0)

    def lm_search(phrase):
        ngrams = {(c,): (-3.0, 0.0) for c in range(cfg.vocab)}
        ngrams[tuple(phrase)] = (-0.25, 0.0)
        image = L.build_image(ngrams, cfg.vocab)
        return image, lambda a: _reference(cand, image=image, alpha=a, beta=0.0, oov=0.0)
    k, phrase, image, least, want, gap = _flip(pairs, base, lm_search, lambda loss: loss / 2.75 + 1.0)
    print(f"rows {k}, {k + 1}: bigram {phrase}, least weight {least:.4f}, gap at 1.5 x {gap:.2e}")
    try:
        beam.set_lm(image, alpha=1.5 * least, beta=0.0, oov_logprob=0.0)
        hot = _run_all(beam, audio, chunk)[0]
        assert hot["ids"][k:k + 2] == phrase and hot["ids"] != base
        if gap >= GAP:
            assert hot["ids"] == want
    finally:
        beam.set_lm(None)
    assert _run_all(beam, audio, chunk)[0]["ids"] == base


def test_reset_clears_one_streams_search_and_the_setters_wait_for_history_to_end(tiny):
    cfg, chunk, beam, twin, audio = tiny
    lib = sub("_lib")
    beam.reset()
    beam.set_beam(BEAM, TOPK, NBEST, CAP)
    totals = {0: 0, 3: 0}
    for k in range(3):
        for s, r in zip((0, 3), beam.step_beam(_chunks(audio, chunk, k, (0, 3)), (0, 3))):
            totals[s] += len(r["ids"])
            assert r["total"] == totals[s]
    assert min(totals.values()) > 0
    for call in (lambda: beam.set_beam(BEAM, TOPK, NBEST, CAP + 1), lambda: beam.set_hotwords([[3, 4]], 1.0), lambda: beam.set_lm(None), lambda: beam.set_beam(0)):
        with pytest.raises(lib.AsrError, match="history"):
            call()
    beam.reset(0)                                          # stream 0 starts over, acoustically and in the search; stream 3 goes on
    r0, r3 = beam.step_beam(_chunks(audio, chunk, 0, (0, 3)), (0, 3))
    twin.reset()
    fresh = twin.step_timed(audio[0][:chunk][None], [1])[0]
    twin.reset()
    assert r0["total"] == len(r0["ids"]) == len(fresh["ids"]) and r0["ids"].tobytes() == fresh["ids"].tobytes() and len(r0["committed"]["ids"]) == 0
    assert r3["total"] == totals[3] + len(r3["ids"])
    with pytest.raises(lib.AsrError, match="history"):
        beam.set_hotwords([[3, 4]], 1.0)
    beam.finish_beam([3])
    beam.reset(0)
    beam.set_hotwords([[3, 4]], 1.0)                       # no stream holds history: all three succeed
    beam.set_lm(None)
    beam.set_hotwords([], 0.0)
    beam.set_beam(BEAM, TOPK, NBEST, CAP + 1)
    empty = beam.finish_beam([1])[0]                       # a stream that was never stepped: the one empty hypothesis
    assert empty["total"] == 0 and len(empty["committed"]["ids"]) == 0 and len(empty["pending"]) == 1 and empty["pending"][0]["score"] == 0.0
    beam.set_beam(0)
    with pytest.raises(Exception):
        beam.step_beam(_chunks(audio, chunk, 0, (0,)), (0,))
    beam.reset()
    ids, offs = np.array([3, 4], np.int32), np.array([0, 2], np.int32)
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    with pytest.raises(lib.AsrError):                      # the offline setters keep rejecting the streaming session
        lib.check(lib.load().asr_paraformer_set_hotwords(beam._h, ip(ids), ip(offs), 1, 1.0))
    with pytest.raises(lib.AsrError):
        lib.check(lib.load().asr_paraformer_set_lm(beam._h, None, 0, 0.0, 0.0, 0.0))


def test_with_the_mode_on_step_and_step_timed_are_the_twins_bytes_and_launches(tiny):
    cfg, chunk, beam, twin, audio = tiny
    beam.reset()
    twin.reset()
    beam.set_beam(BEAM, TOPK, NBEST, CAP)
    sids = (0, 2, 3)
    counts = {}
    for sess in (twin, beam):
        sess.profile(True)
    try:
        for k in range(4):
            a = _chunks(audio, chunk, k, sids)
            form = ("step", "step_timed", "step_beam", "step")[k]
            for sess in (twin, beam):
                sess.profile_reset()
            if form == "step":
                x, y = twin.step(a, sids), beam.step(a, sids)
                assert [i.tobytes() for i in x] == [i.tobytes() for i in y]
            else:
                x, y = twin.step_timed(a, sids), getattr(beam, form)(a, sids)
                assert all(p[key].tobytes() == q[key].tobytes() for p, q in zip(x, y) for key in ("ids", "fire_step", "row", "logprob"))
            counts[k] = (_launches(twin), _launches(beam))
    finally:
        for sess in (twin, beam):
            sess.profile(False)
    assert counts[0][0] == counts[0][1] and counts[1][0] == counts[1][1] and counts[3][0] == counts[3][1]          # step, step_timed: what they were
    assert counts[0][0] == counts[3][0] and "nar_stream_beam" not in counts[1][1] and "beam_topk" not in counts[0][1]
    extra = dict(counts[2][1])
    assert extra.pop("beam_topk") == 1 and extra.pop("nar_stream_beam") == 1 and extra == counts[2][0]                 # step_beam: the timed step + two launches
    beam.finish_beam(list(sids))
    beam.set_beam(0)
    beam.reset()
    twin.reset()


def test_the_transcriber_with_a_beam_returns_the_committed_stream_and_the_nbest(tiny):
    cfg, chunk, beam, twin, audio = tiny
    ps = sub("paraformer_streaming")
    vocab = [f"t{i}" for i in range(cfg.vocab)]
    vocab[2] = "</s>"
    tr = ps.ParaformerStreamTranscriber(beam, vocab, stop_token_ids=[2], decode_mode="zh")
    clips = [audio[s].astype(np.int16) for s in CHUNKS]
    plain, _ = tr.transcribe_many(clips, timestamps=True)
    assert all("nbest" not in o for o in plain)                                # without the arguments: the call it was
    got, stats = tr.transcribe_many(clips, timestamps=True, beam_size=4, nbest=2, revise_tokens=3)
    assert stats["chunks"] == max(CHUNKS.values())
    for o, p in zip(got, plain):                             # no hotwords, no model: the committed stream is the greedy one, with its times
        assert np.array_equal(o["token_ids"], p["token_ids"]) and o["text"] == p["text"] and len(o["nbest"]) == 2
        assert np.array_equal(o["nbest"][0]["token_ids"], o["token_ids"]) and o["nbest"][0]["score"] >= o["nbest"][1]["score"]
        assert [(t["id"], t["start"], t["end"]) for t in o["tokens"]] == [(t["id"], t["start"], t["end"]) for t in p["tokens"]]
    best, second = got[0]["nbest"][0]["token_ids"], got[0]["nbest"][1]["token_ids"]
    at = next(j for j in range(len(best)) if best[j] != second[j])             # (same length: neither holds the stop id here)
    assert len(best) == len(second) and int(second[at]) != 2
    hot, _ = tr.transcribe_many(clips[:1], beam_size=4, hotwords=[[int(second[at])]], hotword_boost=50.0, revise_tokens=3)     # a boost no acoustic score outweighs
    assert not np.array_equal(hot[0]["token_ids"], plain[0]["token_ids"]) and int(second[at]) in hot[0]["token_ids"].tolist()
    back, _ = tr.transcribe_many(clips[:1], beam_size=4)                       # the call sets exactly its own list
    assert np.array_equal(back[0]["token_ids"], plain[0]["token_ids"])
    beam.set_beam(0)
