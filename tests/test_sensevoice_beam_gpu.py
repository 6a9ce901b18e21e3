"""GPU, session level: SenseVoiceSession.run_beam / asr_sensevoice_run_beam on the tiny golden configuration -- beam 1 is the plain (not circular) collapse
of the arg-max with the frame log-probabilities as its score, wider beams return ordered distinct hypotheses, hotwords re-rank them, and the other run forms
are untouched by a beam call."""
import numpy as np
import pytest

import ctc_beam_ref as R
from conftest import sub
from helpers import kaldi_audio, sensevoice_setup

pytestmark = pytest.mark.gpu

BF16, F32 = 0, 1


def _audios(cfg):
    return [kaldi_audio(31, 32000), kaldi_audio(32, cfg.win_length), kaldi_audio(33, 9000), kaldi_audio(34, 20000)], [2, 0, 4, 1]


@pytest.fixture(scope="module")
def tiny():
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    sess = sub("engine").SenseVoiceSession.from_checkpoint(cfg, ck, precision=F32)
    yield cfg, sess
    sess.close()


@pytest.mark.parametrize("prec", [F32, BF16])
def test_beam_1_is_the_argmax_collapse_with_its_score(prec):
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    sess = sub("engine").SenseVoiceSession.from_checkpoint(cfg, ck, precision=prec)
    audios, langs = _audios(cfg)
    plain = sess.run(audios, langs)
    sess.taps(True)
    sess.run_timed(audios, langs)
    ids, flp = sess.tap("frame_ids", dtype=np.int32)[:, 0].copy(), sess.tap("frame_logprob")[:, 0].copy()
    sess.taps(False)
    got = sess.run_beam(audios, langs, beam=1, topk=1, nbest=1)
    compared = 0
    for (r0, T), hyps, u in zip(sess.utterance_rows([a.size for a in audios]), got, plain):
        assert len(hyps) == 1
        h = hyps[0]
        assert h["tokens"].tolist() == R.collapse(ids[r0:r0 + T], cfg.blank_id)
        if ids[r0 + T - 1] == cfg.blank_id or ids[r0 + T - 1] != ids[r0]:         # the only place the circular rule differs
            assert np.array_equal(h["tokens"], u)
            compared += 1
        want = float(flp[r0:r0 + T].astype(np.float64).sum())
        assert abs(h["ctc_score"] - want) <= 1e-4 * abs(want), (h["ctc_score"], want)
        assert h["score"] == h["ctc_score"]
    assert compared >= 2
    sess.close()


def test_nbest_is_ordered_distinct_and_batching_changes_nothing(tiny):
    cfg, sess = tiny
    audios, langs = _audios(cfg)
    audios, langs = audios[:3], langs[:3]
    greedy = sess.run_beam(audios, langs, beam=1, topk=1, nbest=1)
    batch = sess.run_beam(audios, langs, beam=4, nbest=4)
    again = sess.run_beam(audios, langs, beam=4, nbest=4)
    for b, (hyps, g) in enumerate(zip(batch, greedy)):
        assert 1 <= len(hyps) <= 4
        assert hyps[0]["ctc_score"] >= g[0]["ctc_score"] - 1e-4 * abs(g[0]["ctc_score"])        # the greedy path is one alignment of a prefix the beam scored
        assert all(x["score"] >= y["score"] for x, y in zip(hyps[:-1], hyps[1:]))
        assert len({tuple(h["tokens"].tolist()) for h in hyps}) == len(hyps)
        assert all(h["score"] == h["ctc_score"] and h["score"] <= 0 for h in hyps)
        for x, y in zip(hyps, again[b]):                                                       # the replayed step returns the same bytes
            assert np.array_equal(x["tokens"], y["tokens"]) and x["score"] == y["score"] and x["ctc_score"] == y["ctc_score"]
        single = sess.run_beam([audios[b]], [langs[b]], beam=4, nbest=4)[0]
        assert len(single) == len(hyps)
        for x, y in zip(hyps, single):                     # f32 session: the same rows through the same kernels, in another batch
            assert np.array_equal(x["tokens"], y["tokens"]), b
            assert abs(x["score"] - y["score"]) <= 1e-3 and abs(x["ctc_score"] - y["ctc_score"]) <= 1e-3


def test_session_search_equals_the_reference_on_the_tapped_candidates(tiny):
    cfg, sess = tiny
    audios, langs = _audios(cfg)
    sess.taps(True)
    got = sess.run_beam(audios, langs, beam=4, topk=4, nbest=4)
    cid, clp, logits = sess.tap("cand_ids", dtype=np.int32), sess.tap("cand_logprob"), sess.tap("logits")
    sess.taps(False)
    clear = 0
    for (r0, T), hyps in zip(sess.utterance_rows([a.size for a in audios]), got):
        lo = logits[r0:r0 + T].astype(np.float64)
        ref_lp = lo - np.logaddexp.reduce(lo, axis=1, keepdims=True)
        order = np.argsort(-lo, axis=1, kind="stable")[:, :5]
        gaps = -np.diff(np.take_along_axis(lo, order, axis=1), axis=1)
        err = np.abs(clp[r0:r0 + T] - np.take_along_axis(ref_lp, cid[r0:r0 + T].astype(np.int64), axis=1)).max()
        assert err <= 1e-3, err
        safe = (gaps > 2 * err).all(axis=1)
        assert np.array_equal(cid[r0:r0 + T][safe], order[safe, :4]) and safe.mean() >= 0.9
        want, gap = R.prefix_beam(cid[r0:r0 + T], clp[r0:r0 + T], cfg.blank_id, 4, 4)
        if gap >= 1e-3:
            clear += 1
            assert [h["tokens"].tolist() for h in hyps] == [h["tokens"] for h in want]
            assert max(abs(h["score"] - w["score"]) for h, w in zip(hyps, want)) <= 2.5e-4
    assert clear >= 2


def test_hotword_brings_the_second_hypothesis_to_the_front_and_clearing_restores(tiny):
    cfg, sess = tiny
    audios, langs = _audios(cfg)
    audio, lang = [audios[0]], [langs[0]]
    sess.set_hotwords([], 0.0)
    first = sess.run_beam(audio, lang, beam=8, nbest=8)[0]
    assert len(first) >= 2
    top = first[0]["tokens"].tolist()
    pick = next((h for h in first[1:] if any(t not in top for t in h["tokens"].tolist())), None)
    assert pick is not None, "no hypothesis with a token of its own"
    own = [t for t in pick["tokens"].tolist() if t not in top]
    phrase = [own[0]]
    boost = (first[0]["score"] - pick["score"]) + 0.5
    sess.set_hotwords([phrase], boost)
    hot = sess.run_beam(audio, lang, beam=8, nbest=8)[0]
    assert phrase[0] in hot[0]["tokens"].tolist() and hot[0]["tokens"].tolist() != top
    assert hot[0]["score"] > hot[0]["ctc_score"] and abs(hot[0]["score"] - hot[0]["ctc_score"] - boost * hot[0]["tokens"].tolist().count(phrase[0])) <= 1e-3
    by_tokens = {tuple(h["tokens"].tolist()): h for h in hot}
    if tuple(top) in by_tokens and tuple(pick["tokens"].tolist()) in by_tokens:
        assert by_tokens[tuple(pick["tokens"].tolist())]["score"] > by_tokens[tuple(top)]["score"]
    if pick["tokens"].tolist().count(phrase[0]) == 1 and pick is first[1]:
        assert abs(by_tokens[tuple(pick["tokens"].tolist())]["ctc_score"] - pick["ctc_score"]) <= 1e-4
    sess.set_hotwords([], 0.0)
    back = sess.run_beam(audio, lang, beam=8, nbest=8)[0]
    assert len(back) == len(first)
    for x, y in zip(first, back):
        assert np.array_equal(x["tokens"], y["tokens"]) and x["score"] == y["score"] and x["ctc_score"] == y["ctc_score"]


def test_other_run_forms_are_untouched_by_a_beam_call(tiny):
    cfg, sess = tiny
    audios, langs = _audios(cfg)
    before, before_t = sess.run(audios, langs), sess.run_timed(audios, langs)
    sess.run(audios, langs); sess.run_timed(audios, langs)                    # (their captured steps exist now)
    sess.set_hotwords([[3, 4]], 1.0)
    sess.run_beam(audios, langs, beam=16, topk=16, nbest=2)
    sess.set_hotwords([], 0.0)
    after, after_t = sess.run(audios, langs), sess.run_timed(audios, langs)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    for x, y in zip(before_t, after_t):
        assert all(np.array_equal(x[k], y[k]) for k in ("ids", "first_frame", "last_frame"))
        assert np.array_equal(x["logprob"].view(np.uint32), y["logprob"].view(np.uint32))


def test_argument_errors_leave_the_hotword_list_alone(tiny):
    cfg, sess = tiny
    lib = sub("_lib")
    audios, langs = _audios(cfg)
    for bad in ([[cfg.blank_id]], [[3], []], [[cfg.vocab]], [[-1]]):
        with pytest.raises(lib.AsrError):
            sess.set_hotwords(bad, 1.0)
    for kw in (dict(beam=17), dict(beam=0), dict(beam=2, nbest=3), dict(beam=2, topk=17)):
        with pytest.raises(lib.AsrError):
            sess.run_beam(audios[:1], langs[:1], **kw)
    assert len(sess.run_beam(audios[:1], langs[:1], beam=2)[0]) >= 1
