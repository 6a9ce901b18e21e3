"""GPU, session level: ParaformerSession.run_beam / asr_paraformer_run_beam on paraformer_tiny, f32 and bf16 -- without hotwords and model hypothesis 0 is the
arg-max run with the timed run's fire rows and scores, the tapped candidates are the float64 top-k of the tapped logits, the search on them is the float64
statement's (tests/nar_beam_ref.py), a hotword phrase and a language model each bring a chosen second-best pair to the front, and the other run forms are
untouched by beam calls."""
import ctypes

import numpy as np
import pytest

import ctc_lm_ref as L
import ctc_timing_ref as C
import nar_beam_ref as N
from conftest import sub
from helpers import golden_cases, kaldi_audio, load_golden
from test_oracle_paraformer import paraformer_setup

pytestmark = pytest.mark.gpu

BF16, F32 = 0, 1
GAP, TOL = L.GAP, min(6 * 4.1e-5, L.GAP / 4)             # test_nar_beam_gpu.py's bound
COUNTS = [9, 0, 2, 31]


def _batch():
    """The three-clip batch of test_paraformer_timed_gpu.py (the middle clip yields no token) with golden case 1 added."""
    cases = [c for _, c in golden_cases(load_golden("paraformer_tiny"))]
    return [kaldi_audio(c["audio_seed"], c["n_samples"]) for c in (cases[0], cases[2], cases[3], cases[1])]


@pytest.fixture(scope="module", params=[F32, BF16], ids=["f32", "bf16"])
def tiny(request):
    cfg, ck = paraformer_setup("paraformer_tiny")
    sess = sub("engine").ParaformerSession.from_checkpoint(cfg, ck, precision=request.param)
    audios = _batch()
    plain = sess.run(audios)
    assert [len(p) for p in plain] == COUNTS
    yield cfg, sess, audios, plain
    sess.close()


def _abs_dot(cfg, prec, dec, ids):
    """sum_k |h_k| |w_nk| of every row's column ids[row] in the decoder head: h the affine-free LayerNorm of the last decoder layer's output (the `dec` tap),
    w the output layer with after_norm's affine folded in, both rounded to bf16 in a bf16 session."""
    _, ck = paraformer_setup("paraformer_tiny")
    w, _ = sub("arena")._fold64(ck["decoder.after_norm.weight"], ck["decoder.after_norm.bias"], ck["decoder.output_layer.weight"], ck["decoder.output_layer.bias"])
    x = dec.astype(np.float64)
    h = (x - x.mean(axis=1, keepdims=True)) / np.sqrt(x.var(axis=1, keepdims=True) + 1e-5)
    w = w[np.asarray(ids, np.int64)]
    if prec == BF16:
        h, w = C.bf16_round(h), C.bf16_round(w)
    return (np.abs(h.astype(np.float64)) * np.abs(w.astype(np.float64))).sum(axis=1)


def _tapped(sess, audios, beam, topk, nbest):
    """(result, per utterance (cand ids, cand logprob, logits) over its token rows) of one beam call with the taps on."""
    sess.taps(True)
    got = sess.run_beam(audios, beam=beam, topk=topk, nbest=nbest)
    cid, clp, logits = sess.tap("cand_ids", dtype=np.int32), sess.tap("cand_logprob"), sess.tap("logits")
    dec = sess.tap(f"dec{sess.cfg.n_dec + sess.cfg.n_dec3 - 1}")
    sess.taps(False)
    rows = []
    for t0, (hyps, fire) in zip(sess.token_rows([len(f) for _, f in got]), got):
        n = len(fire)
        rows.append((cid[t0:t0 + n].copy(), clp[t0:t0 + n].copy(), logits[t0:t0 + n].astype(np.float64), dec[t0:t0 + n].copy()))
    return got, rows


@pytest.mark.parametrize("beam", [1, 4, 16])
def test_the_plain_search_is_the_argmax_run_with_the_timed_runs_fire_rows(tiny, beam):
    cfg, sess, audios, plain = tiny
    timed = sess.run_timed(audios)
    got, rows = _tapped(sess, audios, beam, beam, min(beam, 4))
    worst = 0.0
    for b, ((hyps, fire), u, t, (cid, clp, lo, dec)) in enumerate(zip(got, plain, timed, rows)):
        assert 1 <= len(hyps) <= min(beam, 4)
        h = hyps[0]
        assert np.array_equal(h["tokens"], u), b
        assert np.array_equal(fire, t["fire_frame"]) and fire.dtype == np.int32
        assert all(len(x["tokens"]) == len(u) == len(x["logprob"]) for x in hyps)                      # every hypothesis has the fire count as its length
        assert all(x["score"] >= y["score"] for x, y in zip(hyps[:-1], hyps[1:])) and all(x["score"] == x["am_score"] for x in hyps)
        assert len({tuple(x["tokens"].tolist()) for x in hyps}) == len(hyps)
        if len(u) == 0:
            assert len(hyps) == 1 and h["score"] == 0.0 and h["am_score"] == 0.0
            continue
        assert len(hyps) == min(beam, 4)
        ref_ids, ref_lp, spread = C.frame_logprob(lo)
        # The row's log-sum-exp is the timed head's, from the logits the tap holds; the candidate's own logit is recomputed by ctc_topk_kernel (the logits are
        # not stored in a run without taps), so it differs from the tapped one by two f32 accumulations of K = d_model terms: budget's K term, twice one
        # logit's bound, with abs_dot of the chosen column. ctc_logit's chain is K / 16 + 10 roundings deep (K / 16 adds per partial sum, 8 fmas inside a
        # dot8, the two partial sums, the bias) where budget counts K // 16 + 5: K + 80 is passed.
        bud0 = C.budget(cfg.vocab, ref_lp, spread)
        bud = C.budget(cfg.vocab, ref_lp, spread, K=cfg.d_model + 80, abs_dot=_abs_dot(cfg, sess.precision, dec, u), vmax=np.abs(lo).max(axis=1))
        err = np.abs(h["logprob"].astype(np.float64) - ref_lp)
        print(f"utterance {b}: logprob error {err.max():.2e}; budget of a stored logit {bud0.min():.2e} (max err / that {float((err / bud0).max()):.2f})")
        worst = max(worst, float((err / bud).max()))
        print(f"utterance {b}: logprob error {err.max():.2e}, budget {bud.min():.2e}, am_score {h['am_score']:.6f} against {ref_lp.sum():.6f}")
        assert np.array_equal(ref_ids, u)
        assert (err <= bud).all(), (b, err.max(), bud.min())
        assert abs(h["am_score"] - ref_lp.sum()) <= 1e-4 * abs(ref_lp.sum())
        full = lo - np.logaddexp.reduce(lo, axis=1, keepdims=True)
        for x in hyps[1:]:                                                                             # the others' scores are their own tokens' log soft-max
            want = full[np.arange(len(u)), x["tokens"]]
            assert np.abs(x["logprob"] - want).max() <= 1e-3 and abs(x["am_score"] - want.sum()) <= 1e-3
    print(f"beam {beam}: hypothesis 0 logprob vs the float64 log soft-max of the logits tap: max err / budget {worst:.3f}")


def test_tapped_candidates_are_the_top_k_and_the_search_is_the_reference_on_them(tiny):
    cfg, sess, audios, plain = tiny
    got, rows = _tapped(sess, audios, 4, 4, 4)
    clear = 0
    for b, ((hyps, fire), (cid, clp, lo, _)) in enumerate(zip(got, rows)):
        if len(fire) == 0:
            continue
        ref_lp = lo - np.logaddexp.reduce(lo, axis=1, keepdims=True)
        order = np.argsort(-lo, axis=1, kind="stable")[:, :5]
        gaps = -np.diff(np.take_along_axis(lo, order, axis=1), axis=1)
        err = np.abs(clp - np.take_along_axis(ref_lp, cid.astype(np.int64), axis=1)).max()
        assert err <= 1e-3, err
        assert all(len(set(r)) == 4 for r in cid.tolist()) and (np.diff(clp, axis=1) <= 0).all()
        safe = (gaps > 2 * err).all(axis=1)
        print(f"utterance {b}: candidate logprob error {err:.2e}, {int(safe.sum())} of {len(safe)} rows with clear gaps")
        assert np.array_equal(cid[safe], order[safe, :4]) and safe.mean() >= 0.9
        want, gap = N.nar_beam(cid, clp, 4, 4)
        print(f"utterance {b}: decision gap {gap:.2e}")
        if gap >= GAP:
            clear += 1
            assert [h["tokens"].tolist() for h in hyps] == [h["tokens"] for h in want]
            assert [h["logprob"].tolist() for h in hyps] == [[float(np.float32(x)) for x in h["logprob"]] for h in want]
            worst = max(max(abs(h["score"] - w["score"]), abs(h["am_score"] - w["am_score"])) for h, w in zip(hyps, want))
            print(f"utterance {b}: largest score error {worst:.2e}")
            assert worst <= TOL
    assert clear >= 2


def _pairs(cid, clp):
    """The adjacent rows whose best two tokens are four distinct ids, the pair of second-best tokens that costs least against the best ones first:
    [(row, phrase, loss)]."""
    out = []
    for k in range(len(cid) - 1):
        if len({int(cid[k, 0]), int(cid[k, 1]), int(cid[k + 1, 0]), int(cid[k + 1, 1])}) == 4:
            out.append((k, [int(cid[k, 1]), int(cid[k + 1, 1])], float(clp[k, 0] - clp[k, 1]) + float(clp[k + 1, 0] - clp[k + 1, 1])))
    return sorted(out, key=lambda p: p[2])


def _smallest(changes, hi):
    """The smallest x in (0, hi] with changes(x), by bisection (changes(hi) holds, changes(0) does not)."""
    assert changes(hi) and not changes(0.0)
    lo = 0.0
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if changes(mid) else (mid, hi)
    return hi


def _flip(cid, clp, base, make_search, hi_of):
    """The cheapest pair that the reference brings to the front, at 1.5 x the smallest weight that changes the reference's best hypothesis: (row, phrase, loss,
    what make_search made, least weight, the reference's result and gap at 1.5 x). Not every pair can come to the front: a beam of 8 may drop the path
    through a row's second-best token before the next row completes the pair, whatever the weight, and the same tokens may match elsewhere."""
    for k, phrase, loss in _pairs(cid, clp):
        made, search = make_search(phrase)
        changes = lambda x: search(x)[0][0]["tokens"] != base
        if not changes(hi_of(loss)):
            continue
        least = _smallest(changes, hi_of(loss))
        want, gap = search(1.5 * least)
        if want[0]["tokens"][k:k + 2] == phrase:
            return k, phrase, loss, made, least, want, gap
    raise AssertionError("no adjacent pair of second-best tokens that the reference brings to the front")


def test_a_hotword_phrase_of_second_best_tokens_comes_to_the_front(tiny):
    cfg, sess, audios, plain = tiny
    audio = [audios[3]]                                    # golden case 1: 31 tokens
    got, rows = _tapped(sess, audio, 8, 4, 1)
    cid, clp = rows[0][:2]
    base = N.nar_beam(cid, clp, 8, 1)[0][0]["tokens"]
    assert base == got[0][0][0]["tokens"].tolist() == plain[3].tolist()

    def make_search(phrase):
        trie = N.build_trie([phrase])
        return trie, lambda x: N.nar_beam(cid, clp, 8, 1, trie, x)
    k, phrase, loss, _, least, want, gap = _flip(cid, clp, base, make_search, lambda loss: loss + 1.0)      # (two matched tokens earn 2 x boost)
    boost = 1.5 * least
    print(f"rows {k}, {k + 1}: phrase {phrase}, loss {loss:.4f}, least boost {least:.4f}, gap at 1.5 x {gap:.2e}")
    assert base[k:k + 2] != phrase
    try:
        sess.set_hotwords([phrase], boost)
        hot = sess.run_beam(audio, beam=8, topk=4, nbest=1)[0][0][0]
        assert hot["tokens"][k:k + 2].tolist() == phrase and hot["tokens"].tolist() != base
        if gap >= GAP:
            assert hot["tokens"].tolist() == want[0]["tokens"] and abs(hot["score"] - want[0]["score"]) <= TOL
        assert hot["score"] > hot["am_score"]
    finally:
        sess.set_hotwords([], 0.0)
    back = sess.run_beam(audio, beam=8, topk=4, nbest=1)[0][0][0]
    assert back["tokens"].tolist() == base and back["score"] == got[0][0][0]["score"]


def test_a_language_model_brings_its_bigram_to_the_front(tiny):
    """A bigram model over the 500 ids: every token has the same unigram, the one listed bigram is the pair of second-best tokens of two adjacent rows."""
    cfg, sess, audios, plain = tiny
    audio = [audios[3]]
    got, rows = _tapped(sess, audio, 8, 4, 1)
    cid, clp = rows[0][:2]
    base = N.nar_beam(cid, clp, 8, 1)[0][0]["tokens"]
    assert base == plain[3].tolist()

    def make_search(phrase):
        ngrams = {(c,): (-3.0, 0.0) for c in range(cfg.vocab)}
        ngrams[tuple(phrase)] = (-0.25, 0.0)
        image = L.build_image(ngrams, cfg.vocab)
        return image, lambda a: N.nar_beam(cid, clp, 8, 1, image=image, alpha=a, beta=0.0, oov=0.0)
    k, phrase, loss, image, least, want, gap = _flip(cid, clp, base, make_search, lambda loss: loss / 2.75 + 1.0)      # (the bigram earns 2.75 x the weight)
    alpha = 1.5 * least
    print(f"rows {k}, {k + 1}: bigram {phrase}, loss {loss:.4f}, least weight {least:.4f}, gap at 1.5 x {gap:.2e}")
    assert base[k:k + 2] != phrase
    try:
        sess.set_lm(image, alpha=alpha, beta=0.0, oov_logprob=0.0)
        hot = sess.run_beam(audio, beam=8, topk=4, nbest=1)[0][0][0]
        assert hot["tokens"][k:k + 2].tolist() == phrase and hot["tokens"].tolist() != base
        if gap >= GAP:
            assert hot["tokens"].tolist() == want[0]["tokens"] and abs(hot["score"] - want[0]["score"]) <= TOL
        lm = hot["score"] - hot["am_score"]
        toks = hot["tokens"].tolist()
        hits = sum(toks[i:i + 2] == phrase for i in range(len(toks) - 1))
        assert hits >= 1 and abs(lm - alpha * (-3.0 * (len(toks) - hits) - 0.25 * hits)) <= 1e-3
        with pytest.raises(sub("_lib").AsrError):          # a rejected image leaves the model in force
            sess.set_lm(image[:-3].copy(), alpha=alpha)
        again = sess.run_beam(audio, beam=8, topk=4, nbest=1)[0][0][0]
        assert again["tokens"].tolist() == hot["tokens"].tolist() and again["score"] == hot["score"]
    finally:
        sess.set_lm(None)
    back = sess.run_beam(audio, beam=8, topk=4, nbest=1)[0][0][0]
    assert back["tokens"].tolist() == base and back["score"] == got[0][0][0]["score"]


def _launches(sess):
    """launches per profile scope since the last reset (a scope another form opened earlier stays listed with none: dropped)"""
    return {k: v["launches"] for k, v in sess.profile_read().items() if v["launches"]}


def _bytes(x):
    return [np.ascontiguousarray(a).tobytes() for a in x]


def test_the_other_forms_are_untouched_and_the_three_interleave(tiny):
    cfg, sess, audios, plain = tiny
    packed = np.concatenate(audios)
    offs = np.concatenate([[0], np.cumsum([a.size for a in audios])])
    counts = {}
    sess.profile(True)
    for name, call in (("run", lambda: sess.run_packed(packed, offs)), ("timed", lambda: sess.run_packed_timed(packed, offs))):
        sess.profile_reset()
        call()
        counts[name] = _launches(sess)
    sess.profile_reset()
    sess.run_packed_beam(packed, offs, 8, 8, 2)
    beam_counts = _launches(sess)
    sess.profile(False)
    assert beam_counts.get("ctc_topk") == 1 and beam_counts.get("nar_beam") == 1 and "nar_beam" not in counts["run"] and "ctc_topk" not in counts["timed"]
    forms = (lambda: sess.run_packed(packed, offs), lambda: sess.run_packed_timed(packed, offs), lambda: sess.run_packed_beam(packed, offs, 8, 8, 2))
    rounds = [[_bytes(f()) for f in forms] for _ in range(3)]            # eager, capture, replay -- each form its own graph
    assert rounds[0] == rounds[1] == rounds[2]
    sess.set_hotwords([[3, 4]], 1.0)
    sess.run_packed_beam(packed, offs, 16, 16, 2)
    sess.set_hotwords([], 0.0)
    assert [_bytes(f()) for f in forms] == rounds[0]
    sess.profile(True)
    for name, call in (("run", forms[0]), ("timed", forms[1])):
        sess.profile_reset()
        call()
        assert _launches(sess) == counts[name], name
    sess.profile(False)
    tok, num = sess.run_packed(packed, offs)
    assert [tok[b, :num[b]].tolist() for b in range(4)] == [p.tolist() for p in plain]


def test_rejections(tiny):
    cfg, sess, audios, plain = tiny
    lib = sub("_lib")
    ids, offs = np.array([3, 4], np.int32), np.array([0, 2], np.int32)
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    with pytest.raises(lib.AsrError):                      # the SenseVoice setters keep rejecting this family
        lib.check(lib.load().asr_sensevoice_set_hotwords(sess._h, ip(ids), ip(offs), 1, 1.0))
    with pytest.raises(lib.AsrError):
        lib.check(lib.load().asr_sensevoice_set_lm(sess._h, None, 0, 0.0, 0.0, 0.0))
    audio = [audios[0]]
    base = sess.run_beam(audio, beam=4, nbest=2)[0][0]
    try:
        sess.set_hotwords([[0, int(base[1]["tokens"][0])]], 0.25)                # id 0 is a token like any other here: no blank
        kept = sess.run_beam(audio, beam=4, nbest=2)[0][0]
        for bad in ([[3], []], [[cfg.vocab]], [[-1]]):
            with pytest.raises(lib.AsrError):
                sess.set_hotwords(bad, 1.0)
        after = sess.run_beam(audio, beam=4, nbest=2)[0][0]                      # a rejected list leaves the one in force
        assert [(h["tokens"].tolist(), h["score"]) for h in after] == [(h["tokens"].tolist(), h["score"]) for h in kept]
    finally:
        sess.set_hotwords([], 0.0)
    for kw in (dict(beam=17), dict(beam=0), dict(beam=2, nbest=3), dict(beam=2, topk=17)):
        with pytest.raises(lib.AsrError):
            sess.run_beam(audio, **kw)
    assert len(sess.run_beam(audio, beam=2)[0][0]) == 1
