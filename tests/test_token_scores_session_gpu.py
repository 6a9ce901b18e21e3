"""Token scores end to end (asr_whisper_set_token_scores / asr_qwen_set_token_scores; tiny synthetic checkpoints): the scores of a session's picks against
the float64 log-soft-max of that step's own returned logits (tests/token_scores_ref.py, within the kernels' derived budget), the picks against the same
run with the mode off, the captured step across on / off / on, the profile class, the transcribers' fields and Whisper's temperature fallback.

Nothing here is decided by a margin: every comparison is a score against the float64 value of the same f32 logits, or an exact equality of ids."""
import numpy as np
import pytest

import token_scores_ref as R
from conftest import sub
from helpers import golden_cases, load_golden
from test_oracle_qwen_asr import qwen_setup
from test_oracle_qwen_asr import unit_audio as qwen_audio
from test_oracle_whisper import unit_audio, whisper_setup

pytestmark = pytest.mark.gpu

BF16, F32 = 0, 1
B, MAX_NEW = 3, 24
LENGTHS = [26240, 12640, 18080]
HEADS = {"greedy": dict(), "penalty-greedy": dict(penalty=(0.8, 4)), "seeded sampling": dict(sampling=(0.7, 10, 0.95, 1.3, 20241019))}


def _configure(sess, penalty=(1.0, 20), sampling=None):
    sess.set_penalty(*penalty)
    if sampling is None:
        sess.set_sampling(False)
    else:
        sess.set_sampling(True, *sampling)


def _prompt(cfg):
    return np.array([[cfg.sot_id, cfg.first_language_id, cfg.transcribe_id, cfg.no_timestamps_id]] * B, np.int32)


def _replay(sess, prompt, n):
    """Prefill + n - 1 decode steps fed from the host with the session's own picks: (picks [n][B], logits [n][B][vocab])."""
    nxt, lg = sess.prefill(prompt)
    picks, logits = [nxt.copy()], [lg.copy()]
    for _ in range(1, n):
        nxt, lg = sess.decode(picks[-1], want_logits=True)
        picks.append(nxt.copy()); logits.append(lg.copy())
    return np.stack(picks), np.stack(logits)


def _check_scores(got, picks, logits, bias, sampled, label):
    """got [B][n] against the reference on each step's returned logits (+ bias on the prefill step) at that step's pick"""
    n, vocab = len(picks), logits.shape[2]
    worst = 0.0
    for t in range(n):
        want, M, lse = R.scores_at(logits[t], picks[t], bias if t == 0 else None)
        budget = R.at_id_budget(vocab, M, lse, want) if sampled else R.fused_budget(vocab, M, lse)
        assert np.isfinite(want).all(), (label, t)
        worst = max(worst, R.over_budget(got[:, t], want, budget))
    print(f"session scores, {label}: largest error {worst:.4f} of the budget over {n} steps x {got.shape[0]} sequences")
    assert worst <= 1.0, label


@pytest.fixture(scope="module", params=[F32, BF16], ids=["f32", "bf16"])
def run(request):
    cfg, ck, sup, beg = whisper_setup("whisper_tiny_test")
    sess = sub("engine").WhisperSession.from_checkpoint(cfg, ck, precision=request.param, suppress_tokens=sup, begin_suppress_tokens=beg)
    audios = [unit_audio(600 + i, n) for i, n in enumerate(LENGTHS)]
    sess.encode(audios)
    bias = np.zeros(cfg.vocab, np.float32)
    bias[list(beg)] = -np.inf
    return dict(cfg=cfg, sup=sup, sess=sess, audios=audios, bias=bias, prec=request.param)


@pytest.mark.parametrize("head", list(HEADS))
def test_replayed_scores_are_the_log_softmax_of_the_returned_logits(run, head):
    cfg, sess = run["cfg"], run["sess"]
    _configure(sess, **HEADS[head])
    sess.set_token_scores(True)
    try:
        picks, logits = _replay(sess, _prompt(cfg), MAX_NEW)
        got = sess.token_scores()
        assert got.shape == (B, MAX_NEW) and got.dtype == np.float32
        _check_scores(got, picks, logits, run["bias"], "sampling" in head, f"whisper {head}")
        sess.set_token_scores(False)
        _configure(sess, **HEADS[head])
        off, _ = _replay(sess, _prompt(cfg), MAX_NEW)            # the mode changes no pick
        assert np.array_equal(off, picks), head
    finally:
        sess.set_token_scores(False)
        _configure(sess)


def _generate(sess, cfg, on, eos=-1):
    sess.set_token_scores(on)
    sess.prefill(_prompt(cfg), want_logits=False)
    toks = [t.tolist() for t in sess.generate(MAX_NEW, eos_id=eos)]
    return toks, (sess.token_scores() if on else None)


@pytest.mark.parametrize("head", list(HEADS))
def test_generate_is_unchanged_and_the_step_graph_follows_the_mode(run, head):
    cfg, sess = run["cfg"], run["sess"]
    _configure(sess, **HEADS[head])
    try:
        on1, s1 = _generate(sess, cfg, True)
        off, _ = _generate(sess, cfg, False)
        on2, s2 = _generate(sess, cfg, True)
        assert on1 == off == on2, head                            # the captured step, fed from the device
        assert s1.shape == (B, MAX_NEW) and np.array_equal(s1, s2) and np.isfinite(s1).all() and (s1 <= 0).all(), head
        sess.set_token_scores(True)
        picks, logits = _replay(sess, _prompt(cfg), MAX_NEW)      # the same steps outside the graph, with their logits
        assert [picks[:, b].tolist() for b in range(B)] == on1
        _check_scores(s1, picks, logits, run["bias"], "sampling" in head, f"whisper generate, {head}")
    finally:
        sess.set_token_scores(False)
        _configure(sess)


def test_count_after_generate_and_the_transcribers_avg_logprob(run):
    cfg, sess = run["cfg"], run["sess"]
    wh = sub("whisper")
    _configure(sess)
    try:
        free, _ = _generate(sess, cfg, True)
        eos = free[0][5]                                          # a stop id that sequence 0 meets at step 5: the others go on
        toks, scores = _generate(sess, cfg, True, eos=eos)
        longest = max(len(t) + (len(t) < MAX_NEW) for t in toks)
        assert scores.shape == (B, min(longest, MAX_NEW)), (scores.shape, [len(t) for t in toks])      # the picks made: the prefill's and one per decode step
        assert len(toks[0]) == free[0].index(eos)
    finally:
        sess.set_token_scores(False)
    pcm = [(a * 32767.0).astype(np.int16) for a in run["audios"]]
    kw = dict(suppress_tokens=run["sup"], no_speech_threshold=2.0, detect_language=False)
    tr = wh.WhisperTranscriber(cfg, sess, token_scores=True, **kw)
    out, _ = tr.transcribe(pcm, max_new=MAX_NEW)
    plain, _ = wh.WhisperTranscriber(cfg, sess, remove_repeats=False, **kw).transcribe(pcm, max_new=MAX_NEW)
    sess.set_token_scores(True)
    try:
        sess.prefill(_prompt(cfg), want_logits=False)
        ids = sess.generate(MAX_NEW, eos_id=cfg.eot_id)
        scores = sess.token_scores()
    finally:
        sess.set_token_scores(False)
    for b, (r, q) in enumerate(zip(out, plain)):
        assert np.array_equal(r["tokens"], q["tokens"]) and np.array_equal(r["tokens"], ids[b]), b
        assert len(r["token_logprobs"]) == len(r["tokens"]) and np.array_equal(r["token_logprobs"], scores[b, :len(ids[b])]), b
        assert r["avg_logprob"] == pytest.approx(wh.avg_logprob(scores[b], len(ids[b]), len(ids[b]) < MAX_NEW), abs=1e-12), b
        assert r["temperature"] == 0.0 and r["compression_ratio"] is None


def test_profile_class_and_the_refusals(run):
    cfg, sess = run["cfg"], run["sess"]
    lib = sub("_lib")
    _configure(sess)
    sess.profile(True)
    try:
        for on in (False, True):
            for head in HEADS:
                _configure(sess, **HEADS[head])
                sess.profile_reset()
                sess.set_token_scores(on)
                sess.prefill(_prompt(cfg), want_logits=False)
                sess.generate(4, eos_id=-1)
                prof = {k: v["launches"] for k, v in sess.profile_read().items() if v["launches"] > 0}
                assert ("token_scores" in prof) == on, (on, head, prof)
                if on:
                    assert prof["token_scores"] == 4, (head, prof)       # the prefill and three decode steps, one launch each
    finally:
        sess.profile(False)
        sess.set_token_scores(False)
        _configure(sess)
    with pytest.raises(lib.AsrError, match="whisper_token_scores"):
        sess.token_scores()                                       # the mode is off
    sess.set_token_scores(True)
    try:
        with pytest.raises(lib.AsrError, match="whisper_token_scores"):
            sess.token_scores()                                   # on, but no prefill since
        sess.prefill(_prompt(cfg), want_logits=False)
        assert sess.token_scores().shape == (B, 1)
    finally:
        sess.set_token_scores(False)


def test_word_probabilities_and_token_logprobs_pair_with_the_tokens(run):
    cfg, sess = run["cfg"], run["sess"]
    wh = sub("whisper")
    pcm = [(a * 32767.0).astype(np.int16) for a in run["audios"]]
    kw = dict(suppress_tokens=run["sup"], no_speech_threshold=2.0, detect_language=False)
    decode = lambda ids: "".join(" t%d" % t for t in ids)
    tr = wh.WhisperTranscriber(cfg, sess, token_scores=True, word_timestamps=True, piece_decoder=decode, **kw)
    out, _ = tr.transcribe(pcm, max_new=MAX_NEW)
    plain, _ = wh.WhisperTranscriber(cfg, sess, remove_repeats=False, **kw).transcribe(pcm, max_new=MAX_NEW)
    for b, (r, q) in enumerate(zip(out, plain)):
        assert np.array_equal(r["tokens"], q["tokens"]) and len(r["tokens"]) > 0, b
        assert len(r["token_logprobs"]) == len(r["tokens"]) == len(r["token_times"]) == len(r["words"]), b
        for w, lp in zip(r["words"], r["token_logprobs"]):       # one token per word under this decoder
            assert 0.0 < w["probability"] <= 1.0 and w["probability"] == pytest.approx(float(np.exp(np.float64(lp)))), (b, w)
        assert r["compression_ratio"] == pytest.approx(wh.compression_ratio(decode(r["tokens"].tolist())))
    # timestamp mode: token_logprobs are the text ids' only, avg_logprob counts every pick
    ts = wh.WhisperTranscriber(cfg, sess, token_scores=True, timestamps=True, **kw)
    out, _ = ts.transcribe(pcm, max_new=MAX_NEW)
    for b, r in enumerate(out):
        assert len(r["token_logprobs"]) == len(r["tokens"]) and (r["tokens"] < cfg.no_timestamps_id).all() and np.isfinite(r["avg_logprob"]), b


@pytest.mark.parametrize("threshold,attempts", [(0.0, 3), (-np.inf, 1)])
def test_temperature_fallback_runs_every_attempt_or_one(run, threshold, attempts):
    cfg, sess = run["cfg"], run["sess"]
    wh = sub("whisper")
    pcm = [(a * 32767.0).astype(np.int16) for a in run["audios"]]
    temps, seed = (0.4, 0.9), 77
    kw = dict(suppress_tokens=run["sup"], no_speech_threshold=2.0, detect_language=False, top_k=10, top_p=0.95, seed=seed)
    tr = wh.WhisperTranscriber(cfg, sess, temperature_fallback=temps, logprob_threshold=threshold, **kw)
    out, _ = tr.transcribe(pcm, max_new=MAX_NEW)
    last = attempts - 1
    # that attempt alone, replayed by hand with its seed
    if last == 0:
        _configure(sess)
    else:
        _configure(sess, sampling=(temps[last - 1], 10, 0.95, 1.0, seed + last))
    sess.set_token_scores(True)
    try:
        sess.prefill(_prompt(cfg), want_logits=False)
        ids = sess.generate(MAX_NEW, eos_id=cfg.eot_id)
        scores = sess.token_scores()
    finally:
        sess.set_token_scores(False)
        _configure(sess)
    for b, r in enumerate(out):
        assert r["temperature"] == (0.0 if last == 0 else temps[last - 1]), b       # an unreachable threshold keeps the last attempt, -inf the first
        assert np.array_equal(r["tokens"], ids[b]) and np.array_equal(r["token_logprobs"], scores[b, :len(ids[b])]), b
        assert r["avg_logprob"] == pytest.approx(wh.avg_logprob(scores[b], len(ids[b]), len(ids[b]) < MAX_NEW), abs=1e-12), b


# ------------------------------------------------------------------------------------------------ Qwen3-ASR
@pytest.mark.parametrize("prec", [F32, BF16], ids=["f32", "bf16"])
def test_qwen_replay_and_on_off_on(prec):
    g = load_golden("qwen_asr_tiny")
    cfg, ck = qwen_setup(g)
    lib = sub("_lib")
    sess = sub("engine").QwenAsrSession.from_checkpoint(cfg, ck, precision=prec)
    cases = [c for _, c in golden_cases(g)][:3]
    audios = [qwen_audio(c["audio_seed"], c["n_samples"]) for c in cases]
    head, tail, suffix = g["head_ids"].tolist(), g["tail_ids"].tolist(), g["suffix_ids"].tolist()
    pre = [head + c["query_ids"].tolist() + suffix for c in cases]
    post = [tail + c["language_tail_ids"].tolist() for c in cases]
    n = 12

    def stepwise():
        nxt, lg, _ = sess.prefill(audios, pre, post)
        picks, logits = [nxt.copy()], [lg.copy()]
        for _ in range(n - 1):
            nxt, lg = sess.decode(None, want_logits=True)
            picks.append(nxt.copy()); logits.append(lg.copy())
        return np.stack(picks), np.stack(logits)

    def generate(on):
        sess.set_token_scores(on)
        sess.prefill(audios, pre, post, want_logits=False)
        toks = [t.tolist() for t in sess.generate(n, stop_ids=())]
        return toks, (sess.token_scores() if on else None)

    with pytest.raises(lib.AsrError, match="qwen_token_scores"):
        sess.token_scores()
    for label, kw in HEADS.items():
        _configure(sess, **({"penalty": (0.8, 4)} if "penalty" in kw else kw))
        sess.set_token_scores(True)
        picks, logits = stepwise()
        got = sess.token_scores()
        assert got.shape == (len(cases), n)
        _check_scores(got, picks, logits, None, "sampling" in label, f"qwen {label}")
        on1, s1 = generate(True)
        off, _ = generate(False)
        on2, s2 = generate(True)
        assert on1 == off == on2 == [picks[:, b].tolist() for b in range(len(cases))], label
        assert np.array_equal(s1, s2) and s1.shape == (len(cases), n), label
        _check_scores(s1, picks, logits, None, "sampling" in label, f"qwen generate, {label}")
        sess.set_token_scores(False)
    _configure(sess)
    # the transcriber: token_logprobs pair with tokens, avg_logprob includes the stop pick of an utterance that ended
    special = {"stop": [1, 521], "asr_text": [540], "audio_start": 524, "audio_end": 520, "audio_pad": 525, "im_start": 510, "im_end": 521,
               "system": 511, "user": 523, "assistant": 522, "newline": 512, "language_prefix": [530, 531]}
    meta = {"audio_pcm_scale": "32768", "max_seq_len": str(cfg.max_seq_len), "sample_rate": "16000", "special_token_ids": special, "supported_languages": {}}
    q = sub("qwen_asr")
    clips = [np.round(a * 32768.0).astype(np.int16) for a in audios]
    plain, _ = q.QwenAsrTranscriber(cfg, sess, meta).transcribe(clips, max_new=n)
    out, _ = q.QwenAsrTranscriber(cfg, sess, meta, token_scores=True).transcribe(clips, max_new=n)
    for b, (r, p) in enumerate(zip(out, plain)):
        assert np.array_equal(r["tokens"], p["tokens"]) and "token_logprobs" not in p, b
        assert len(r["token_logprobs"]) == len(r["tokens"]) and np.isfinite(r["token_logprobs"]).all() and (r["token_logprobs"] <= 0).all(), b
        assert np.isfinite(r["avg_logprob"]) and r["avg_logprob"] <= 0.0, b
    with pytest.raises(ValueError):
        q.QwenAsrTranscriber(cfg, sess, meta, token_scores=True, beam_size=2)


def test_qwen_mode_switched_on_after_a_larger_batch_was_prefilled():
    """on, prefill 1 clip; off; prefill 3 clips; on; decode: the step scores three rows, so the score history must cover three before anything is launched
    (the decode step reserves it, and the head refuses a step with more rows than the history holds). The run is a correct one: the picks are those of
    the mode-off run, the scores of a run that no prefill started are not handed out, and the next prefill's scores are right at the larger batch."""
    g = load_golden("qwen_asr_tiny")
    cfg, ck = qwen_setup(g)
    lib = sub("_lib")
    sess = sub("engine").QwenAsrSession.from_checkpoint(cfg, ck, precision=F32)
    cases = [c for _, c in golden_cases(g)][:3]
    audios = [qwen_audio(c["audio_seed"], c["n_samples"]) for c in cases]
    head, tail, suffix = g["head_ids"].tolist(), g["tail_ids"].tolist(), g["suffix_ids"].tolist()
    pre = [head + c["query_ids"].tolist() + suffix for c in cases]
    post = [tail + c["language_tail_ids"].tolist() for c in cases]
    n = 6

    def steps(k):
        out = []
        for _ in range(k):
            nxt, lg = sess.decode(None, want_logits=True)
            out.append((nxt.copy(), lg.copy()))
        return out

    first, _, _ = sess.prefill(audios, pre, post)                # the mode never on: the picks to compare with
    want = [first.copy()] + [p for p, _ in steps(n - 1)]
    sess.set_token_scores(True)
    sess.prefill(audios[:1], pre[:1], post[:1])
    assert sess.token_scores().shape == (1, 1)
    sess.set_token_scores(False)
    first, _, _ = sess.prefill(audios, pre, post)
    sess.set_token_scores(True)
    got = [first.copy()] + [p for p, _ in steps(n - 1)]          # scored steps at batch 3 on a history last sized for batch 1
    assert np.array_equal(np.stack(got), np.stack(want))
    with pytest.raises(lib.AsrError, match="qwen_token_scores"):
        sess.token_scores()                                       # no prefill since the switch: whose picks these columns are is not defined
    nxt, lg, _ = sess.prefill(audios, pre, post)
    rest = steps(n - 1)
    picks, logits = np.stack([nxt] + [p for p, _ in rest]), np.stack([lg] + [l for _, l in rest])
    assert np.array_equal(picks, np.stack(want))
    scores = sess.token_scores()
    assert scores.shape == (3, n)
    _check_scores(scores, picks, logits, None, False, "qwen, batch grown while the mode was off")
    sess.set_token_scores(False)


def test_whisper_mode_switched_on_after_a_larger_batch_was_prefilled(run):
    """The same order on Whisper, whose step has always reserved the head's buffers: encode 1, on, prefill; off; encode 3, prefill; on; decode."""
    cfg, sess, lib = run["cfg"], run["sess"], sub("_lib")
    _configure(sess)
    try:
        sess.encode(run["audios"][:1])
        sess.set_token_scores(True)
        sess.prefill(_prompt(cfg)[:1], want_logits=False)
        assert sess.token_scores().shape == (1, 1)
        sess.set_token_scores(False)
        sess.encode(run["audios"])
        want, _ = _replay(sess, _prompt(cfg), 6)
        nxt, _ = sess.prefill(_prompt(cfg))
        sess.set_token_scores(True)
        got = [nxt.copy()]
        for _ in range(5):
            got.append(sess.decode(got[-1], want_logits=False)[0].copy())
        assert np.array_equal(np.stack(got), want)
        with pytest.raises(lib.AsrError, match="whisper_token_scores"):
            sess.token_scores()
        picks, logits = _replay(sess, _prompt(cfg), 6)
        assert np.array_equal(picks, want)
        _check_scores(sess.token_scores(), picks, logits, run["bias"], False, "whisper, batch grown while the mode was off")
    finally:
        sess.set_token_scores(False)
        sess.encode(run["audios"])
