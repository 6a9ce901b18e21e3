"""n-gram LM fusion end to end (asr_whisper_set_lm / asr_qwen_set_lm; tiny synthetic checkpoints, F32), after tests/test_hotword_sessions_gpu.py: the expected
tokens are tests/decoder_lm_ref.py's greedy walk and beam search over the CPU oracle's logits. A clip is compared when every decision margin of its walk --
the fused gaps, and the top-M boundary where the column outside could matter -- exceeds 10 x LOGIT_TOL_F32, the project's rule; the clips and the models
(order 3 on the 2^-6 grid, a fifth of the vocabulary without a unigram) were chosen on the CPU so that at least three qualify for every check."""
import numpy as np
import pytest

import ctc_lm_ref as clr
import decoder_lm_ref as dl
import hotword_heads_ref as hw
from conftest import sub
from helpers import load_golden
from oracle.qwen_asr_oracle import QwenAsrOracle
from oracle.whisper_oracle import WhisperOracle
from test_hotword_sessions_gpu import QW_BOOST, QW_PHRASES, WH_BOOST, WH_PHRASES
from test_oracle_qwen_asr import qwen_setup
from test_oracle_qwen_asr import unit_audio as qwen_audio
from test_oracle_whisper import unit_audio, whisper_setup
from whisper_beam_ref import as_lists

pytestmark = pytest.mark.gpu

F32 = 1
LOGIT_TOL_F32 = 1e-3
MAX_NEW, WIDTH = 7, 3
ALPHA, BETA, OOV, TOPK = 0.5, 0.25, -1.0, 16
WH_CLIPS, WH_SEED = [(601, 29920), (602, 12640), (603, 26240), (604, 29920), (607, 29920)], 2
QW_CLIPS, QW_SEED = [(7017, 30000), (7021, 30000), (7025, 30000), (7003, 48000), (7010, 9000)], 0


def _model(vocab, seed, end_ids):
    rng = np.random.default_rng([seed, vocab])
    words = sorted(int(c) for c in np.nonzero(rng.random(vocab) < 0.8)[0])
    return dl.model(clr.build_image(dl.grid_ngrams(30 + seed, vocab, 3, words), vocab), ALPHA, BETA, oov=OOV, topk=TOPK, end_ids=end_ids)


def _set(sess, lm, **kw):
    a = dict(alpha=lm["alpha"], beta=lm["beta"], oov_logprob=lm["oov"], topk=lm["topk"], end_ids=lm["end_ids"])
    a.update(kw)
    sess.set_lm(a.pop("image", lm["image"]), a.pop("alpha"), a.pop("beta"), **a)


def _expect(runs, lm, phrases, boost):
    out = []
    tol = 10 * LOGIT_TOL_F32
    for first, state, step in runs:
        toks, mg = dl.greedy_lm(first, state, step, MAX_NEW, [], 0.0, lm)
        plain, _ = hw.greedy_hot(first, state, step, MAX_NEW, [], 0.0)
        m = []
        beam = dl.beam_search_core_lm(first, state, step, WIDTH, MAX_NEW, [], 0.0, lm, margins=m)
        hot, mh = dl.greedy_lm(first, state, step, MAX_NEW, phrases, boost, lm)
        m2 = []
        hot_beam = dl.beam_search_core_lm(first, state, step, WIDTH, MAX_NEW, phrases, boost, lm, margins=m2)
        out.append(dict(toks=toks, plain=plain, ok=min(mg) > tol, beam=beam, beam_ok=min(m) > tol, hot=hot, hot_ok=min(mh) > tol, hot_beam=hot_beam,
                        hot_beam_ok=min(m2) > tol, margins=(min(mg), min(m), min(mh), min(m2))))
    return out


def _check_tokens(got, exp, key="toks", ok="ok"):
    good = [b for b, e in enumerate(exp) if e[ok]]
    assert len(good) >= 3, [e["margins"] for e in exp]
    for b in good:
        assert got[b] == exp[b][key], (b, got[b], exp[b][key])
    return good


def _check_beam(got, exp, key="beam", ok="beam_ok"):
    good = [b for b, e in enumerate(exp) if e[ok]]
    assert len(good) >= 3, [e["margins"] for e in exp]
    for b in good:
        t_ref, s_ref = as_lists(exp[b][key])
        t_got, s_got = as_lists(got[b])
        assert t_got == t_ref, b
        assert np.abs(s_got - s_ref).max() < LOGIT_TOL_F32 * MAX_NEW, b
    return good


# ------------------------------------------------------------------------------------------------ Whisper
@pytest.fixture(scope="module")
def wh():
    cfg, ck, sup, beg = whisper_setup("whisper_tiny_test")
    sess = sub("engine").WhisperSession.from_checkpoint(cfg, ck, precision=F32, suppress_tokens=sup, begin_suppress_tokens=beg)
    orc = WhisperOracle(cfg, ck, sup, beg)
    audios = [unit_audio(s, n) for s, n in WH_CLIPS]
    prompt = [cfg.sot_id, cfg.first_language_id, cfg.transcribe_id, cfg.no_timestamps_id]
    lm = _model(cfg.vocab, WH_SEED, (cfg.eot_id,))
    exp = _expect([hw.whisper_runs(orc, a, prompt) for a in audios], lm, WH_PHRASES, WH_BOOST)
    sess.encode(audios)
    return dict(cfg=cfg, sup=sup, sess=sess, audios=audios, prompts=np.array([prompt] * len(audios), np.int32), exp=exp, lm=lm)


def _wh_generate(w):
    w["sess"].prefill(w["prompts"], want_logits=False)
    return [t.tolist() for t in w["sess"].generate(MAX_NEW, eos_id=-1)]


def test_whisper_generate_follows_the_fused_walk_and_clearing_restores(wh):
    sess = wh["sess"]
    before = _wh_generate(wh)
    _set(sess, wh["lm"])
    try:
        got = _wh_generate(wh)
        good = _check_tokens(got, wh["exp"])
        assert any(wh["exp"][b]["toks"] != wh["exp"][b]["plain"] for b in good)          # a qualifying clip decodes differently from its plain run
        assert got == _wh_generate(wh)                                                   # the captured step replays with the model on
    finally:
        sess.set_lm(None)
    assert _wh_generate(wh) == before


def test_whisper_beam_search_scores_the_fused_sum(wh):
    sess = wh["sess"]
    sess.prefill(wh["prompts"], want_logits=False)
    _set(sess, wh["lm"])                                                                 # a model set between the prefill and the search is accepted
    try:
        got = sess.beam_search(WIDTH, MAX_NEW, -1)
    finally:
        sess.set_lm(None)
    good = _check_beam(got, wh["exp"])
    sess.prefill(wh["prompts"], want_logits=False)
    plain = sess.beam_search(WIDTH, MAX_NEW, -1)
    assert any(as_lists(plain[b])[0] != as_lists(got[b])[0] for b in good)


def test_whisper_model_and_hotwords_together(wh):
    sess = wh["sess"]
    sess.set_hotwords(WH_PHRASES, WH_BOOST)
    _set(sess, wh["lm"])
    try:
        _check_tokens(_wh_generate(wh), wh["exp"], "hot", "hot_ok")
        sess.prefill(wh["prompts"], want_logits=False)
        _check_beam(sess.beam_search(WIDTH, MAX_NEW, -1), wh["exp"], "hot_beam", "hot_beam_ok")
    finally:
        sess.set_lm(None)
        sess.set_hotwords([])


def test_whisper_zero_weights_give_the_plain_tokens(wh):
    sess = wh["sess"]
    before = _wh_generate(wh)
    _set(sess, wh["lm"], alpha=0.0, beta=0.0, oov_logprob=0.0)
    try:
        assert _wh_generate(wh) == before
    finally:
        sess.set_lm(None)


def test_whisper_refusals_leave_the_model_in_force(wh):
    sess, cfg, lm = wh["sess"], wh["cfg"], wh["lm"]
    err = sub("_lib").AsrError
    other = _model(cfg.vocab + 1, 1, ())
    _set(sess, lm)
    try:
        with pytest.raises(err, match="vocabulary"):
            _set(sess, lm, image=other["image"])
        with pytest.raises(err, match="topk 33"):
            _set(sess, lm, topk=33)
        with pytest.raises(err, match="9 end ids"):
            _set(sess, lm, end_ids=tuple(range(9)))
        with pytest.raises(err, match="whisper_set_lm"):
            _set(sess, lm, end_ids=(cfg.vocab,))
        with pytest.raises(err, match="whisper_set_lm"):
            _set(sess, lm, alpha=-1.0)
        _check_tokens(_wh_generate(wh), wh["exp"])                                       # each refusal left the model in force
        _set(sess, lm, topk=2)
        sess.prefill(wh["prompts"], want_logits=False)
        with pytest.raises(err, match="topk 2 is below the beam width 3"):
            sess.beam_search(WIDTH, MAX_NEW, -1)
        _set(sess, lm)
        _check_tokens(_wh_generate(wh), wh["exp"])
    finally:
        sess.set_lm(None)


def test_whisper_cleared_model_launches_nothing_new(wh):
    sess = wh["sess"]

    def launches(beam):
        sess.profile_reset()
        sess.prefill(wh["prompts"], want_logits=False)
        sess.beam_search(WIDTH, 4, -1) if beam else sess.generate(4, eos_id=-1)
        return {k: v["launches"] for k, v in sess.profile_read().items() if v["launches"] > 0}

    sess.profile(True)
    try:
        off = [launches(False), launches(True)]
        _set(sess, wh["lm"])
        on = [launches(False), launches(True)]
        sess.set_lm(None)
        off_again = [launches(False), launches(True)]
    finally:
        sess.profile(False)
        sess.set_lm(None)
    assert all("lm" not in o for o in off) and off_again == off
    assert on[0]["lm"] == 4                                                              # the prefill's pick and three decode steps: one scope (top-M pass + pick) each
    assert on[1]["lm"] == 1 + 4                                                          # the prefill's pick, the first ranking and three passes (top-M pass + re-rank each)


def test_whisper_transcriber_takes_the_model(wh):
    sess, cfg = wh["sess"], wh["cfg"]
    mod = sub("whisper")
    pcm = [(a * 32767.0).astype(np.int16) for a in wh["audios"]]
    kw = dict(suppress_tokens=wh["sup"], no_speech_threshold=2.0, remove_repeats=False)
    plain, _ = mod.WhisperTranscriber(cfg, sess, **kw).transcribe(pcm, max_new=MAX_NEW)
    fused, _ = mod.WhisperTranscriber(cfg, sess, lm=wh["lm"]["image"], lm_weight=ALPHA, length_bonus=BETA, lm_topk=TOPK, **kw).transcribe(pcm, max_new=MAX_NEW)
    for p, f in zip(plain, fused):
        assert p["language_id"] == f["language_id"] and p["no_speech_prob"] == f["no_speech_prob"]
    assert any(not np.array_equal(p["tokens"], f["tokens"]) for p, f in zip(plain, fused))
    again, _ = mod.WhisperTranscriber(cfg, sess, **kw).transcribe(pcm, max_new=MAX_NEW)        # the model does not outlive the call
    for p, a in zip(plain, again):
        assert np.array_equal(p["tokens"], a["tokens"])
    sess.encode(wh["audios"])                                                            # (the fixture's batch, for the tests that follow)


# ------------------------------------------------------------------------------------------------ Qwen3-ASR
@pytest.fixture(scope="module")
def qw():
    g = load_golden("qwen_asr_tiny")
    cfg, ck = qwen_setup(g)
    head, tail, suffix = g["head_ids"].tolist(), g["tail_ids"].tolist(), g["suffix_ids"].tolist()
    orc = QwenAsrOracle(cfg, ck, head, tail, suffix)
    sess = sub("engine").QwenAsrSession.from_checkpoint(cfg, ck, precision=F32)
    audios = [qwen_audio(s, n) for s, n in QW_CLIPS]
    lm = _model(cfg.vocab, QW_SEED, (0,))
    exp = _expect([hw.qwen_runs(orc, a) for a in audios], lm, QW_PHRASES, QW_BOOST)
    return dict(cfg=cfg, ck=ck, sess=sess, audios=audios, pre=[head + suffix], post=[tail], exp=exp, lm=lm)


def _qw_generate(q):
    q["sess"].prefill(q["audios"], q["pre"], q["post"], want_logits=False)
    return [t.tolist() for t in q["sess"].generate(MAX_NEW, stop_ids=())]


def test_qwen_generate_beam_and_clearing(qw):
    sess = qw["sess"]
    before = _qw_generate(qw)
    _set(sess, qw["lm"])
    try:
        got = _qw_generate(qw)
        good = _check_tokens(got, qw["exp"])
        assert any(qw["exp"][b]["toks"] != qw["exp"][b]["plain"] for b in good)
        assert got == _qw_generate(qw)
        sess.prefill(qw["audios"], qw["pre"], qw["post"], want_logits=False)
        _check_beam(sess.beam_search(WIDTH, MAX_NEW, ()), qw["exp"])
        sess.set_hotwords(QW_PHRASES, QW_BOOST)
        _check_tokens(_qw_generate(qw), qw["exp"], "hot", "hot_ok")
    finally:
        sess.set_hotwords([])
        sess.set_lm(None)
    assert _qw_generate(qw) == before


def test_qwen_refusals_and_the_aligner(qw):
    sess, cfg, lm = qw["sess"], qw["cfg"], qw["lm"]
    err = sub("_lib").AsrError
    _set(sess, lm)
    try:
        with pytest.raises(err, match="vocabulary"):
            _set(sess, lm, image=_model(cfg.vocab + 1, 1, ())["image"])
        with pytest.raises(err, match="topk 33"):
            _set(sess, lm, topk=33)
        with pytest.raises(err, match="9 end ids"):
            _set(sess, lm, end_ids=tuple(range(9)))
        _set(sess, lm, topk=2)
        sess.prefill(qw["audios"], qw["pre"], qw["post"], want_logits=False)
        with pytest.raises(err, match="topk 2 is below the beam width 3"):
            sess.beam_search(WIDTH, MAX_NEW, ())
        _set(sess, lm)
        _check_tokens(_qw_generate(qw), qw["exp"])
    finally:
        sess.set_lm(None)


def test_an_aligner_session_refuses_the_model(qw):
    from test_qwen_aligner_gpu import _golden, _session
    _, cfg, ck, _, _ = _golden()
    al = _session(cfg, ck, F32)
    with pytest.raises(sub("_lib").AsrError, match="forced-aligner"):
        _set(al, qw["lm"])
