"""asr_whisper_beam_search: the device beam search of the Whisper decoder against its restatement (tests/whisper_beam_ref.py =
oracle/qwen_asr_oracle.py:beam_search_core over WhisperOracle.decoder), its width-1 / width-5 properties, row counts on both sides of the
decode GEMM's 64-row limit, cache layouts and precisions, argument errors and the transcriber's beam mode."""
import os

import numpy as np
import pytest

from conftest import sub
from oracle.whisper_oracle import WhisperOracle
from test_oracle_whisper import unit_audio, whisper_setup
from whisper_beam_ref import as_lists, beam_reference

pytestmark = pytest.mark.gpu

BF16, F32, FP8W = 0, 1, 2
LOGIT_TOL_F32 = 1e-3


def _session(cfg_name, prec, env=None):
    cfg, ck, sup, beg = whisper_setup(cfg_name)
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        sess = sub("engine").WhisperSession.from_checkpoint(cfg, ck, precision=prec, suppress_tokens=sup, begin_suppress_tokens=beg)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return cfg, ck, sup, beg, sess


def _prompt(cfg, B):
    return np.array([[cfg.sot_id, cfg.first_language_id, cfg.transcribe_id, cfg.no_timestamps_id]] * B, np.int32)


def _clips(seed0, lengths):
    return [unit_audio(seed0 + i, n) for i, n in enumerate(lengths)]


def _beam(sess, audios, prompts, width, max_new, eos_id=-1):
    sess.encode(audios)
    sess.prefill(prompts, want_logits=False)
    return sess.beam_search(width, max_new, eos_id)


# ragged clips (audio seed, samples) whose searches on the synthetic checkpoints keep every ranking gap above 10 x LOGIT_TOL_F32 (most clips of
# these checkpoints come within 0.01 of a flip somewhere: their logits are nearly flat); the test still only compares clips that qualify
CLIPS = {"whisper_tiny_test": ([(601, 26240), (602, 29920), (619, 12640), (624, 31040), (653, 18080)], 6),
         "whisper_mid_test": ([(609, 15680), (618, 8960), (630, 13280), (656, 29280), (619, 12640)], 4)}


@pytest.mark.parametrize("cfg_name", ["whisper_tiny_test", "whisper_mid_test"])
def test_f32_matches_the_restatement(cfg_name):
    cfg, ck, sup, beg, sess = _session(cfg_name, F32)
    orc = WhisperOracle(cfg, ck, sup, beg)
    clips, max_new = CLIPS[cfg_name]
    audios = [unit_audio(s, n) for s, n in clips]
    B, width = len(audios), 3
    prompts = _prompt(cfg, B)
    refs, margins = [], []
    for a, p in zip(audios, prompts):
        m = []
        refs.append(beam_reference(orc, a, p.tolist(), width, max_new, margins=m))
        margins.append(min(m))
    ok = [b for b in range(B) if margins[b] > 10 * LOGIT_TOL_F32]
    assert len(ok) >= 3, margins
    got = _beam(sess, audios, prompts, width, max_new)
    for b in ok:
        t_ref, s_ref = as_lists(refs[b])
        t_got, s_got = as_lists(got[b])
        assert t_got == t_ref, b
        assert np.abs(s_got - s_ref).max() < LOGIT_TOL_F32 * max_new, b
    # a stop id from the restatement's second hypothesis of the first qualifying clip: hypotheses end mid-search
    eos = as_lists(refs[ok[0]])[0][1][1]
    refs_e, ok_e = [], []
    for b, (a, p) in enumerate(zip(audios, prompts)):
        m = []
        refs_e.append(beam_reference(orc, a, p.tolist(), width, max_new, eos_id=eos, margins=m))
        if min(m) > 10 * LOGIT_TOL_F32:
            ok_e.append(b)
    got_e = _beam(sess, audios, prompts, width, max_new, eos_id=eos)
    assert ok_e and any(len(t) < max_new for b in ok_e for t in as_lists(refs_e[b])[0]), margins
    for b in ok_e:
        t_ref, s_ref = as_lists(refs_e[b])
        t_got, s_got = as_lists(got_e[b])
        assert t_got == t_ref and all(eos not in t for t in t_got), b
        assert np.abs(s_got - s_ref).max() < LOGIT_TOL_F32 * max_new, b
    # the session's greedy state is the prefill's: generate() after a search continues it
    after = sess.generate(max_new, eos_id=-1)
    sess.prefill(prompts, want_logits=False)
    fresh = sess.generate(max_new, eos_id=-1)
    for b in range(B):
        assert np.array_equal(after[b], fresh[b]), b


def _greedy_with_gaps(sess, audios, prompts, n):
    sess.encode(audios)
    nxt, logits = sess.prefill(prompts)
    ids, gaps = [nxt.copy()], []
    gaps.append(np.sort(logits, axis=1)[:, -1] - np.sort(logits, axis=1)[:, -2])
    for _ in range(n - 1):
        nxt, lg = sess.decode(None, want_logits=True)
        ids.append(nxt.copy())
        s = np.sort(lg, axis=1)
        gaps.append(s[:, -1] - s[:, -2])
    return np.stack(ids, 1), np.stack(gaps, 1)


@pytest.mark.parametrize("prec", [F32, BF16])
def test_width_one_is_greedy_width_five_is_sorted_and_batch_independent(prec):
    cfg, ck, sup, beg, sess = _session("whisper_mid_test", prec)
    audios = _clips(700, [24000, 40000, 9600, 16000, 56000, 12000])
    B, n = len(audios), 8
    prompts = _prompt(cfg, B)
    greedy, gaps = _greedy_with_gaps(sess, audios, prompts, n)
    w1 = _beam(sess, audios, prompts, 1, n)
    for b in range(B):
        toks = w1[b][0][0]
        if prec == F32:
            assert toks.tolist() == greedy[b].tolist(), b
        else:                                       # bf16: up to the first step whose greedy top-2 gap is below 0.05
            low = np.nonzero(gaps[b] < 0.05)[0]
            upto = int(low[0]) if low.size else n
            assert toks[:upto].tolist() == greedy[b][:upto].tolist(), b
        assert np.isfinite(w1[b][0][1])
    w5 = _beam(sess, audios, prompts, 5, n)
    for b in range(B):
        toks, scores = as_lists(w5[b])
        assert (np.diff(scores) <= 0).all() and np.isfinite(scores).all(), b
        assert len({tuple(t) for t in toks}) == 5, b
    if prec == F32:                                 # a pair alone == the same pair inside the batch of 6
        pair = [1, 4]
        alone = _beam(sess, [audios[i] for i in pair], prompts[:2], 5, n)
        for j, b in enumerate(pair):
            ta, sa = as_lists(alone[j])
            tb, sb = as_lists(w5[b])
            assert ta == tb and np.abs(sa - sb).max() < 1e-4, b


def _log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


@pytest.mark.parametrize("B,width", [(8, 8), (16, 5)])
def test_large_v3_rows_on_both_sides_of_64(B, width):
    """8 x 8 = 64 hypothesis rows take the decode GEMM, 16 x 5 = 80 the tiled path (bf16, large-v3 dimensions, synthetic weights). Every hypothesis's
    score is re-computed by teacher-forcing its ids through the greedy path of B rows (prefill logits + BEGIN_SUPPRESS, then decode steps fed from the
    host): a row mixed up on either GEMM path would score another row's context. Width 1 at the same 64 / 80 rows equals generate()."""
    cfg, ck, sup, beg, sess = _session("whisper_large_v3", BF16)
    probe = sub("_probe")
    audios = _clips(800, [16000 + 1600 * i for i in range(B)])
    prompts = _prompt(cfg, B)
    n = 5
    sess.encode(audios)
    sess.prefill(prompts, want_logits=False)
    probe.gemm_counts(reset=True)
    wide = sess.beam_search(width, n, -1)
    tiled = sum(probe.gemm_counts().values())        # launches of the generic GEMM dispatcher (eager passes and captures; replays do not count)
    for b in range(B):
        toks, scores = as_lists(wide[b])
        assert np.isfinite(scores).all() and (np.diff(scores) <= 0).all() and len({tuple(t) for t in toks}) == width, b
        assert all(len(t) == n for t in toks), b
    bias = np.zeros(cfg.vocab)
    bias[list(beg)] = -np.inf
    worst = 0.0
    for r in range(width):
        hyp = np.stack([np.asarray(wide[b][r][0], np.int32) for b in range(B)])       # (B, n)
        _, logits = sess.prefill(prompts)
        score = _log_softmax(logits + bias)[np.arange(B), hyp[:, 0]]
        for t in range(1, n):
            _, lg = sess.decode(hyp[:, t - 1], want_logits=True)
            score += _log_softmax(lg)[np.arange(B), hyp[:, t]]
        got = np.array([wide[b][r][1] for b in range(B)])
        worst = max(worst, float(np.abs(got - score).max()))
    print(f"{B} x {width}: largest |device score - teacher-forced score| {worst:.4f}")
    assert worst < 0.05 * n
    # the five other projections: the decode GEMM at 64 rows (only fc2 and the logits reach the generic dispatcher), the tiled path at 80 (all six)
    if B * width > 64:
        assert tiled >= 5 * 4 * (cfg.n_dec_layers + 1), tiled
    else:
        assert 0 < tiled <= 4 * (cfg.n_dec_layers + 1), tiled
    # width 1 over the same row count: the search's rows against greedy decoding
    R = B * width
    audios1 = _clips(850, [16000 + 400 * (i % 16) for i in range(R)])
    prompts1 = _prompt(cfg, R)
    sess.encode(audios1)
    sess.prefill(prompts1, want_logits=False)
    greedy = sess.generate(n, eos_id=-1)
    sess.prefill(prompts1, want_logits=False)
    w1 = sess.beam_search(1, n, -1)
    for b in range(R):
        assert w1[b][0][0].tolist() == greedy[b].tolist(), b


def _lists(cfg_name, prec, env, audios, width, n):
    cfg, _, _, _, sess = _session(cfg_name, prec, env)
    got = _beam(sess, audios, _prompt(cfg, len(audios)), width, n)
    return [as_lists(h) for h in got]


def _assert_same(a, b, score_tol=0.0):
    for x, y in zip(a, b):
        assert x[0] == y[0] and np.abs(x[1] - y[1]).max() <= score_tol


def test_cache_layouts_and_fp8_twin_give_the_same_lists():
    audios = _clips(900, [20000, 36000, 11200])
    base = _lists("whisper_mid_test", BF16, None, audios, 4, 7)
    _assert_same(base, _lists("whisper_mid_test", BF16, {"ASR_KV_PAGE_SHUFFLE": "1"}, audios, 4, 7))
    _assert_same(base, _lists("whisper_mid_test", BF16, {"ASR_KV_PAGED": "0"}, audios, 4, 7))
    # 32 and 64 rows (byte weights in the decode GEMM), 65 (the dequantised tiled path): the same lists, bit for bit at 32 and 65 rows. At 33..64 rows the
    # fake twin's fc2 runs on the tiled split-K GEMM while the byte weights stay on the decode GEMM (whisper.hip, enqueue_step), so the scores there agree
    # to summation order and bf16 rounding of the residual copies only
    for B, width, tol in ((4, 8, 0.0), (8, 8, 2e-3), (13, 5, 0.0)):
        clips = _clips(950, [12800 + 800 * i for i in range(B)])
        real = _lists("whisper_d256_test", FP8W, None, clips, width, 5)
        fake = _lists("whisper_d256_test", FP8W, {"ASR_FP8_FAKE": "1"}, clips, width, 5)
        _assert_same(real, fake, score_tol=tol)


def test_bad_arguments():
    cfg, ck, sup, beg, sess = _session("whisper_tiny_test", F32)
    audios = _clips(990, [16000, 9600])
    prompts = _prompt(cfg, 2)
    sess.encode(audios)
    with pytest.raises(RuntimeError, match="prefill first"):
        sess.beam_search(2, 4, -1)
    sess.prefill(prompts, want_logits=False)
    for w in (0, 9):
        with pytest.raises(RuntimeError, match="beam width"):
            sess.beam_search(w, 4, -1)
    with pytest.raises(RuntimeError, match="max_target_positions"):
        sess.beam_search(2, cfg.max_target_positions - 3, -1)
    sess.set_penalty(0.8, 20)
    with pytest.raises(RuntimeError, match="do not combine"):
        sess.beam_search(2, 4, -1)
    sess.set_penalty(1.0, 20)
    sess.set_sampling(True, 0.8, 10, 0.95, 1.0, 1)
    with pytest.raises(RuntimeError, match="do not combine"):
        sess.beam_search(2, 4, -1)
    sess.set_sampling(False)
    sess.beam_search(2, 4, -1)                      # the session is still right after its prefill
    sess.generate(4, eos_id=-1)
    with pytest.raises(RuntimeError, match="prefill first"):
        sess.beam_search(2, 4, -1)


def test_transcriber_beam_mode_returns_the_first_hypothesis():
    wmod = sub("whisper")
    cfg, ck, sup, beg, sess = _session("whisper_tiny_test", F32)
    clips = [(unit_audio(s, n) * 32767).astype(np.int16) for s, n in ((1001, 24000), (1002, 14400))]
    n = 10
    tr = wmod.WhisperTranscriber(cfg, sess, suppress_tokens=sup, beam_size=3, no_speech_detection=False)
    out, _ = tr.transcribe(clips, max_new=n)
    # the same steps by hand: probe prefill for the language, full-prompt prefill, first hypothesis, repeat guard
    audios = [wmod.prepare_audio_input(c) for c in clips]
    sess.encode(audios)
    _, logits = sess.prefill(np.full((2, 1), cfg.sot_id, np.int32))
    lang = tr.language_token_ids[np.argmax(logits[:, tr.language_token_ids], axis=1)]
    prompt = np.stack([[cfg.sot_id, int(l), cfg.transcribe_id, cfg.no_timestamps_id] for l in lang]).astype(np.int32)
    sess.prefill(prompt, want_logits=False)
    hyps = sess.beam_search(3, n, cfg.eot_id)
    for b in range(2):
        want = list(wmod.remove_repeated_parts(hyps[b][0][0].tolist(), 3, len(hyps[b][0][0])))
        assert out[b]["tokens"].tolist() == want, b
    with pytest.raises(ValueError):
        wmod.WhisperTranscriber(cfg, sess, suppress_tokens=sup, beam_size=3, repeat_penalty=0.8)
    with pytest.raises(ValueError):
        wmod.WhisperTranscriber(cfg, sess, suppress_tokens=sup, beam_size=3, use_sampling=True)
