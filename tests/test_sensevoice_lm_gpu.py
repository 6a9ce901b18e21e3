"""GPU, session level: SenseVoiceSession.set_lm / asr_sensevoice_set_lm on the tiny golden configuration -- run_beam under a language model equals the float64
statement (tests/ctc_lm_ref.py) on the tapped candidates, a changed or cleared model never meets a stale captured step, the other run forms do not see the
model, and a rejected model leaves the one in force."""
import functools

import numpy as np
import pytest

import ctc_lm_ref as L
from conftest import sub
from helpers import kaldi_audio, sensevoice_setup

pytestmark = pytest.mark.gpu

BF16, F32 = 0, 1
GAP, TOL = 1e-3, 2.5e-4                # as test_ctc_lm_beam_gpu.py derives it (the utterances here have at most 37 rows)
BEAM = dict(beam=4, topk=4, nbest=4)


def _audios(cfg):
    return [kaldi_audio(31, 32000), kaldi_audio(32, cfg.win_length), kaldi_audio(33, 9000), kaldi_audio(34, 20000)], [2, 0, 4, 1]


@functools.lru_cache(maxsize=None)
def _model(vocab, blank, which):
    """Two models over the session's vocabulary: A a bigram with </s>, B a trigram without; (image, alpha, beta, oov)."""
    if which == "A":
        return L.build_image(L.random_arpa(1, vocab, 2, 8.0 / vocab, blank=blank), vocab), 0.5, 0.3, -0.7
    return L.build_image(L.random_arpa(2, vocab, 3, 4.0 / vocab, blank=blank, eos=False), vocab), 0.8, -0.2, 0.0


def _candidates(sess, audios, langs):
    """The tapped candidates of a beam run (they do not depend on the model), per utterance."""
    sess.taps(True)
    sess.run_beam(audios, langs, **BEAM)
    cid, clp = sess.tap("cand_ids", dtype=np.int32).copy(), sess.tap("cand_logprob").copy()
    sess.taps(False)
    return [(cid[r0:r0 + T], clp[r0:r0 + T]) for r0, T in sess.utterance_rows([a.size for a in audios])]


def _check(got, cands, blank, model, need=2):
    image, alpha, beta, oov = model
    clear = 0
    for hyps, (cid, clp) in zip(got, cands):
        want, gap = L.prefix_beam_lm(cid, clp, blank, BEAM["beam"], BEAM["nbest"], image, alpha, beta, oov)
        if gap < GAP:
            continue
        clear += 1
        assert [h["tokens"].tolist() for h in hyps] == [h["tokens"] for h in want]
        err = max(max(abs(h["score"] - w["score"]), abs(h["ctc_score"] - w["ctc_score"])) for h, w in zip(hyps, want))
        print(f"  {len(hyps)} hypotheses, gap {gap:.2e}, score error {err:.2e}, LM term of the best {want[0]['lm']:.3f}")
        assert err <= TOL
    assert clear >= need, f"{clear} utterances with a decision gap >= {GAP}"


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert len(x) == len(y)
        for h, g in zip(x, y):
            assert np.array_equal(h["tokens"], g["tokens"]) and h["score"] == g["score"] and h["ctc_score"] == g["ctc_score"]


@pytest.fixture(scope="module")
def tiny():
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    sess = sub("engine").SenseVoiceSession.from_checkpoint(cfg, ck, precision=F32)
    yield cfg, sess
    sess.close()


@pytest.mark.parametrize("prec", [F32, BF16], ids=["f32", "bf16"])
def test_run_beam_under_a_model_equals_the_reference_on_the_tapped_candidates(prec):
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    sess = sub("engine").SenseVoiceSession.from_checkpoint(cfg, ck, precision=prec)
    audios, langs = _audios(cfg)
    model = _model(cfg.vocab, cfg.blank_id, "A")
    sess.set_lm(model[0], *model[1:])
    sess.taps(True)
    got = sess.run_beam(audios, langs, **BEAM)
    cid, clp = sess.tap("cand_ids", dtype=np.int32), sess.tap("cand_logprob")
    sess.taps(False)
    cands = [(cid[r0:r0 + T], clp[r0:r0 + T]) for r0, T in sess.utterance_rows([a.size for a in audios])]
    _check(got, cands, cfg.blank_id, model)
    assert any(h["score"] != h["ctc_score"] for hyps in got for h in hyps)
    sess.close()


def test_a_changed_or_cleared_model_never_meets_a_stale_captured_step(tiny):
    cfg, sess = tiny
    audios, langs = _audios(cfg)
    A, B = _model(cfg.vocab, cfg.blank_id, "A"), _model(cfg.vocab, cfg.blank_id, "B")
    sess.set_lm(None)
    cands = _candidates(sess, audios, langs)
    before = [sess.run_beam(audios, langs, **BEAM) for _ in range(3)]            # (eager, captured, replayed)
    _same(before[0], before[2])
    sess.set_lm(A[0], *A[1:])
    with_a = [sess.run_beam(audios, langs, **BEAM) for _ in range(3)]
    _same(with_a[0], with_a[2])
    _check(with_a[2], cands, cfg.blank_id, A)
    sess.set_lm(B[0], *B[1:])
    with_b = [sess.run_beam(audios, langs, **BEAM) for _ in range(3)]
    _same(with_b[0], with_b[2])
    _check(with_b[2], cands, cfg.blank_id, B)
    assert any(x["score"] != y["score"] for hx, hy in zip(with_a[2], with_b[2]) for x, y in zip(hx, hy))
    sess.set_lm(A[0], 0.25, *A[2:])                                              # the same image under another weight is another step too
    _check(sess.run_beam(audios, langs, **BEAM), cands, cfg.blank_id, (A[0], 0.25) + A[2:], need=1)
    sess.set_lm(None)
    for _ in range(3):
        _same(sess.run_beam(audios, langs, **BEAM), before[0])


def test_the_other_run_forms_do_not_see_the_model(tiny):
    cfg, sess = tiny
    audios, langs = _audios(cfg)
    sess.set_lm(None)
    targets = [t[:6] for t in sess.run(audios, langs)]
    plain, timed, aligned = sess.run(audios, langs), sess.run_timed(audios, langs), sess.align(audios, langs, targets)
    A = _model(cfg.vocab, cfg.blank_id, "A")
    sess.set_lm(A[0], *A[1:])
    sess.run_beam(audios, langs, **BEAM)
    plain2, timed2, aligned2 = sess.run(audios, langs), sess.run_timed(audios, langs), sess.align(audios, langs, targets)
    sess.set_lm(None)
    for x, y in zip(plain, plain2):
        assert x.tobytes() == y.tobytes()
    for x, y in zip(timed, timed2):
        assert all(x[k].tobytes() == y[k].tobytes() for k in ("ids", "first_frame", "last_frame", "logprob"))
    for x, y in zip(aligned, aligned2):
        assert x["aligned"] == y["aligned"] and all(np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes() for k in ("first_frame", "last_frame", "logprob", "path_score", "loglik"))


def test_a_rejected_model_leaves_the_one_in_force(tiny):
    cfg, sess = tiny
    lib = sub("_lib")
    audios, langs = _audios(cfg)
    A = _model(cfg.vocab, cfg.blank_id, "A")
    sess.set_lm(A[0], *A[1:])
    want = sess.run_beam(audios, langs, **BEAM)
    other = L.build_image(L.random_arpa(1, cfg.vocab + 1, 2, 0.01, blank=cfg.blank_id), cfg.vocab + 1)        # a model over another vocabulary
    broken = A[0].copy()
    broken[-3] = cfg.vocab + 5                                                   # a uni entry past the root's edges
    on_blank = L.build_image({(cfg.blank_id,): (-1.0, 0.0), (5,): (-1.0, 0.0)}, cfg.vocab)
    for image, kw in ((other, {}), (broken, {}), (on_blank, {}), (A[0][:-1], {}), (A[0], dict(alpha=-0.5)), (A[0], dict(beta=np.nan)), (A[0], dict(oov_logprob=1.0))):
        with pytest.raises(lib.AsrError):
            sess.set_lm(image, **{**dict(alpha=A[1], beta=A[2], oov_logprob=A[3]), **kw})
        _same(sess.run_beam(audios, langs, **BEAM), want)
    sess.set_lm(None)
