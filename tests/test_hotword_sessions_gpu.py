"""Hotword boosting end to end (asr_whisper_set_hotwords / asr_qwen_set_hotwords; tiny synthetic checkpoints, F32): the expected tokens are a greedy loop
(and tests/hotword_heads_ref.py: beam_search_core_hot) over the CPU oracle's logits with the float64 bias, the pattern of tests/test_whisper_beam_gpu.py.
A clip is compared when every decision margin of its walk exceeds 10 x LOGIT_TOL_F32, the project's rule; the clips and the phrase lists (ids from the
oracles' ranks 1..3, so a boost flips picks, matches complete and partial matches are abandoned) were chosen on the CPU so that all five qualify."""
import numpy as np
import pytest

import hotword_heads_ref as hw
import token_scores_ref as R
from conftest import sub
from helpers import load_golden
from oracle.qwen_asr_oracle import QwenAsrOracle
from oracle.whisper_oracle import WhisperOracle
from test_oracle_qwen_asr import qwen_setup
from test_oracle_qwen_asr import unit_audio as qwen_audio
from test_oracle_whisper import unit_audio, whisper_setup
from whisper_beam_ref import as_lists

pytestmark = pytest.mark.gpu

F32 = 1
LOGIT_TOL_F32 = 1e-3
MAX_NEW, WIDTH = 7, 3
WH_CLIPS = [(600, 26240), (606, 29920), (611, 29920), (622, 12640), (610, 26240)]
WH_PHRASES, WH_BOOST = [[344, 555], [344, 393, 344], [393, 344], [555, 555, 555], [135, 198], [198, 532], [555, 393, 135]], 0.5
QW_CLIPS = [(7000, 16000), (7001, 30000), (7002, 9000), (7003, 48000), (7005, 16000)]
QW_PHRASES, QW_BOOST = [[152, 344], [152, 258, 152], [258, 310], [310, 310, 310], [242, 217], [196, 446], [344, 152, 217]], 1.0


def _expect(runs, phrases, boost):
    """Per clip: the hot and the plain greedy walk of the oracle, the beam reference, and whether the margins let the clip be compared."""
    out = []
    for first, state, step in runs:
        toks, mg = hw.greedy_hot(first, state, step, MAX_NEW, phrases, boost)
        plain, _ = hw.greedy_hot(first, state, step, MAX_NEW, [], boost)
        m = []
        beam = hw.beam_search_core_hot(first, state, step, WIDTH, MAX_NEW, phrases, boost, margins=m)
        out.append(dict(toks=toks, plain=plain, ok=min(mg) > 10 * LOGIT_TOL_F32, beam=beam, beam_ok=min(m) > 10 * LOGIT_TOL_F32, margins=(min(mg), min(m))))
    return out


@pytest.fixture(scope="module")
def wh():
    cfg, ck, sup, beg = whisper_setup("whisper_tiny_test")
    sess = sub("engine").WhisperSession.from_checkpoint(cfg, ck, precision=F32, suppress_tokens=sup, begin_suppress_tokens=beg)
    orc = WhisperOracle(cfg, ck, sup, beg)
    audios = [unit_audio(s, n) for s, n in WH_CLIPS]
    prompt = [cfg.sot_id, cfg.first_language_id, cfg.transcribe_id, cfg.no_timestamps_id]
    exp = _expect([hw.whisper_runs(orc, a, prompt) for a in audios], WH_PHRASES, WH_BOOST)
    sess.encode(audios)
    bias = np.zeros(cfg.vocab, np.float32)
    bias[list(beg)] = -np.inf
    return dict(cfg=cfg, sup=sup, sess=sess, audios=audios, prompts=np.array([prompt] * len(audios), np.int32), exp=exp, bias=bias)


def _wh_generate(w):
    w["sess"].prefill(w["prompts"], want_logits=False)
    return [t.tolist() for t in w["sess"].generate(MAX_NEW, eos_id=-1)]


def _check_tokens(got, exp, key="toks", ok="ok"):
    good = [b for b, e in enumerate(exp) if e[ok]]
    assert len(good) >= 3, [e["margins"] for e in exp]
    for b in good:
        assert got[b] == exp[b][key], (b, got[b], exp[b][key])
    return good


def test_whisper_generate_follows_the_biased_oracle_and_clearing_restores(wh):
    sess = wh["sess"]
    before = _wh_generate(wh)
    sess.set_hotwords(WH_PHRASES, WH_BOOST)
    try:
        hot = _wh_generate(wh)
        good = _check_tokens(hot, wh["exp"])
        assert any(wh["exp"][b]["toks"] != wh["exp"][b]["plain"] for b in good)          # a qualifying clip decodes differently from its unbiased run
        assert hot == _wh_generate(wh)                                                   # the captured step replays with the mode on
    finally:
        sess.set_hotwords([])
    assert _wh_generate(wh) == before


def test_whisper_beam_search_scores_log_prob_plus_delta(wh):
    sess = wh["sess"]
    sess.set_hotwords(WH_PHRASES, WH_BOOST)
    try:
        sess.prefill(wh["prompts"], want_logits=False)
        got = sess.beam_search(WIDTH, MAX_NEW, -1)
    finally:
        sess.set_hotwords([])
    good = [b for b, e in enumerate(wh["exp"]) if e["beam_ok"]]
    assert len(good) >= 3, [e["margins"] for e in wh["exp"]]
    for b in good:
        t_ref, s_ref = as_lists(wh["exp"][b]["beam"])
        t_got, s_got = as_lists(got[b])
        assert t_got == t_ref, b
        assert np.abs(s_got - s_ref).max() < LOGIT_TOL_F32 * MAX_NEW, b
    sess.prefill(wh["prompts"], want_logits=False)                                       # off again: the plain search, and a list set after the prefill is refused
    plain = sess.beam_search(WIDTH, MAX_NEW, -1)
    assert any(as_lists(plain[b])[0] != as_lists(got[b])[0] for b in good)
    sess.set_hotwords(WH_PHRASES, WH_BOOST)
    try:
        sess.prefill(wh["prompts"], want_logits=False)
        sess.set_hotwords(WH_PHRASES[:2], WH_BOOST)
        with pytest.raises(sub("_lib").AsrError, match="changed since the prefill"):
            sess.beam_search(WIDTH, MAX_NEW, -1)
    finally:
        sess.set_hotwords([])


def test_whisper_profile_class_and_launch_counts(wh):
    sess = wh["sess"]

    def launches():
        sess.profile_reset()
        sess.prefill(wh["prompts"], want_logits=False)
        sess.generate(4, eos_id=-1)
        return {k: v["launches"] for k, v in sess.profile_read().items() if v["launches"] > 0}

    sess.profile(True)
    try:
        off = launches()
        sess.set_hotwords(WH_PHRASES, WH_BOOST)
        on = launches()
        sess.set_hotwords([])
        off_again = launches()
    finally:
        sess.profile(False)
        sess.set_hotwords([])
    assert "hotwords" not in off and off_again == off
    assert on.pop("hotwords") == 2 * 4                                                   # the bias and the advance of the prefill and of three decode steps
    assert {k: v for k, v in on.items() if k in off} == {k: v for k, v in off.items() if k in on}


def test_whisper_token_scores_and_logits_are_the_biased_rows(wh):
    sess, cfg = wh["sess"], wh["cfg"]
    plain_nxt, plain_lg = sess.prefill(wh["prompts"])
    sess.set_hotwords(WH_PHRASES, WH_BOOST)
    sess.set_token_scores(True)
    try:
        nxt, lg = sess.prefill(wh["prompts"])
        picks, logits = [nxt.copy()], [lg.copy()]
        for _ in range(1, MAX_NEW):
            nxt, lg = sess.decode(None, want_logits=True)
            picks.append(nxt.copy()); logits.append(lg.copy())
        got = sess.token_scores()
    finally:
        sess.set_token_scores(False)
        sess.set_hotwords([])
    roots = sorted({p[0] for p in WH_PHRASES})
    want0 = plain_lg.copy()
    want0[:, roots] = (plain_lg[:, roots] + np.float32(WH_BOOST)).astype(np.float32)
    assert np.array_equal(logits[0], want0)                                              # logits_out shows the biased row: + boost on the root's children, nothing else
    assert [np.asarray(picks)[:, b].tolist() for b in range(len(WH_CLIPS)) if wh["exp"][b]["ok"]] == [e["toks"] for e in wh["exp"] if e["ok"]]
    worst = 0.0
    for t in range(MAX_NEW):
        want, M, lse = R.scores_at(logits[t], picks[t], wh["bias"] if t == 0 else None)
        worst = max(worst, R.over_budget(got[:, t], want, R.fused_budget(cfg.vocab, M, lse)))
    print(f"token scores under hotwords: largest error {worst:.4f} of the budget")
    assert worst <= 1.0


def test_whisper_argument_errors_leave_the_list_alone(wh):
    sess, cfg = wh["sess"], wh["cfg"]
    err = sub("_lib").AsrError
    sess.set_hotwords(WH_PHRASES, WH_BOOST)
    try:
        for bad, boost in (([[cfg.vocab]], 1.0), ([[3], []], 1.0), ([[-1]], 1.0), ([[3]], float("nan")), ([[3]], float("inf"))):
            with pytest.raises(err, match="whisper_set_hotwords"):
                sess.set_hotwords(bad, boost)
        _check_tokens(_wh_generate(wh), wh["exp"])
    finally:
        sess.set_hotwords([])


def test_whisper_transcriber_probe_is_unbiased_and_the_decode_is_not(wh):
    sess, cfg = wh["sess"], wh["cfg"]
    mod = sub("whisper")
    pcm = [(a * 32767.0).astype(np.int16) for a in wh["audios"]]
    kw = dict(suppress_tokens=wh["sup"], no_speech_threshold=2.0, remove_repeats=False)
    plain, _ = mod.WhisperTranscriber(cfg, sess, **kw).transcribe(pcm, max_new=MAX_NEW)
    hot, _ = mod.WhisperTranscriber(cfg, sess, hotwords=WH_PHRASES, hotword_boost=WH_BOOST, **kw).transcribe(pcm, max_new=MAX_NEW)
    for p, h in zip(plain, hot):
        assert p["language_id"] == h["language_id"] and p["no_speech_prob"] == h["no_speech_prob"]
    assert any(not np.array_equal(p["tokens"], h["tokens"]) for p, h in zip(plain, hot))
    beam, _ = mod.WhisperTranscriber(cfg, sess, hotwords=WH_PHRASES, hotword_boost=WH_BOOST, beam_size=WIDTH, **kw).transcribe(pcm, max_new=MAX_NEW)
    assert all(len(r["tokens"]) > 0 for r in beam)
    again, _ = mod.WhisperTranscriber(cfg, sess, **kw).transcribe(pcm, max_new=MAX_NEW)        # the list does not outlive the call
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
    exp = _expect([hw.qwen_runs(orc, a) for a in audios], QW_PHRASES, QW_BOOST)
    return dict(cfg=cfg, sess=sess, audios=audios, pre=[head + suffix], post=[tail], exp=exp)


def _qw_generate(q):
    q["sess"].prefill(q["audios"], q["pre"], q["post"], want_logits=False)
    return [t.tolist() for t in q["sess"].generate(MAX_NEW, stop_ids=())]


def test_qwen_generate_beam_and_clearing(qw):
    sess = qw["sess"]
    before = _qw_generate(qw)
    sess.set_hotwords(QW_PHRASES, QW_BOOST)
    try:
        hot = _qw_generate(qw)
        good = _check_tokens(hot, qw["exp"])
        assert any(qw["exp"][b]["toks"] != qw["exp"][b]["plain"] for b in good)
        sess.prefill(qw["audios"], qw["pre"], qw["post"], want_logits=False)
        got = sess.beam_search(WIDTH, MAX_NEW, ())
    finally:
        sess.set_hotwords([])
    good = [b for b, e in enumerate(qw["exp"]) if e["beam_ok"]]
    assert len(good) >= 3, [e["margins"] for e in qw["exp"]]
    for b in good:
        t_ref, s_ref = as_lists(qw["exp"][b]["beam"])
        t_got, s_got = as_lists(got[b])
        assert t_got == t_ref, b
        assert np.abs(s_got - s_ref).max() < LOGIT_TOL_F32 * MAX_NEW, b
    assert _qw_generate(qw) == before
    with pytest.raises(sub("_lib").AsrError, match="qwen_set_hotwords"):
        sess.set_hotwords([[qw["cfg"].vocab + 1]], 1.0)
