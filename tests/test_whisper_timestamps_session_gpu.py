"""Whisper's timestamp mode end to end (asr_whisper_set_timestamps; tiny synthetic checkpoint, f32 and bf16): the rules inside the greedy step, the
captured graph, the beam search and the transcriber, against tests/whisper_timestamps_ref.py applied to the session's own raw logits.

The raw logits come from the GPU, so the margin |L - T| of a step cannot be planted: a row of a step whose float64 margin is below the kernel's derived
budget is undecidable and left out -- at most two such rows in the whole file (the last test counts them and prints the smallest margin met).
The specials between eot and the first timestamp carry the suppress penalty, as in every released Whisper vocabulary."""
import numpy as np
import pytest

import whisper_timestamps_ref as ref
from conftest import sub
from test_oracle_whisper import unit_audio, whisper_setup

pytestmark = pytest.mark.gpu

BF16, F32 = 0, 1
B, MAX_NEW = 3, 24
LENGTHS = [26240, 12640, 18080]
SKIPPED, MARGINS, KINDS = [], [], set()


def _session(prec):
    cfg, ck, sup, beg = whisper_setup("whisper_tiny_test")
    sup = sorted(set(sup) | set(range(cfg.eot_id + 1, cfg.no_timestamps_id + 1)))
    sess = sub("engine").WhisperSession.from_checkpoint(cfg, ck, precision=prec, suppress_tokens=sup, begin_suppress_tokens=beg)
    return cfg, sup, beg, sess


def _params(cfg, max_initial=50):
    return cfg.no_timestamps_id + 1, cfg.no_timestamps_id, cfg.eot_id, max_initial


def _audios(seed0=600):
    return [unit_audio(seed0 + i, n) for i, n in enumerate(LENGTHS)]


def _prompt(cfg, with_no_timestamps=False):
    p = [cfg.sot_id, cfg.first_language_id, cfg.transcribe_id] + ([cfg.no_timestamps_id] if with_no_timestamps else [])
    return np.array([p] * B, np.int32)


def _stream(ids, eot):
    ids = [int(t) for t in ids]
    return ids[:ids.index(eot)] if eot in ids else ids


def _replay(sess, prompt, n, feed=None):
    """Prefill + n - 1 decode steps fed from the host (`feed` [n][B], or the session's own picks): (picks [n][B], logits [n][B][vocab])."""
    nxt, lg = sess.prefill(prompt)
    picks, logits = [nxt.copy()], [lg.copy()]
    for t in range(1, n):
        nxt, lg = sess.decode(picks[-1] if feed is None else feed[t - 1], want_logits=True)
        picks.append(nxt.copy()); logits.append(lg.copy())
    return np.stack(picks), np.stack(logits)


@pytest.fixture(scope="module", params=[F32, BF16], ids=["f32", "bf16"])
def run(request):
    """One session per precision, and its teacher-forced replays: mode on (masked logits, picks), mode off on the same ids (raw logits)."""
    cfg, sup, beg, sess = _session(request.param)
    audios = _audios()
    sess.encode(audios)
    sess.set_timestamps(True, 50)
    picks, masked = _replay(sess, _prompt(cfg), MAX_NEW)
    sess.set_timestamps(False)
    picks_off, raw = _replay(sess, _prompt(cfg), MAX_NEW, feed=picks)
    return dict(cfg=cfg, sup=sup, beg=beg, sess=sess, audios=audios, prec=request.param, picks=picks, masked=masked, raw=raw)


def test_masked_logits_are_the_rule_applied_to_the_raw_ones(run):
    cfg, picks, masked, raw = run["cfg"], run["picks"], run["masked"], run["raw"]
    p = _params(cfg)
    bias = np.zeros(cfg.vocab, np.float32)
    bias[list(run["beg"])] = -np.inf
    for t in range(MAX_NEW):
        hists = [picks[:t, b].tolist() for b in range(B)]
        want, margins, budgets = ref.apply(raw[t], hists, p)
        first, _ = ref.thr.argmax_rows(masked[t], bias if t == 0 else None)
        for b in range(B):
            if np.isfinite(margins[b]):
                MARGINS.append(float(margins[b]))
            if margins[b] < budgets[b]:
                SKIPPED.append((run["prec"], t, b, float(margins[b]), float(budgets[b])))
                continue
            assert np.array_equal(masked[t, b].view(np.uint32), want[b].view(np.uint32)), (t, b, float(margins[b]), float(budgets[b]))
            assert picks[t, b] == first[b], (t, b)
            h = hists[b]
            last_ts, penult_ts = bool(h) and h[-1] >= p[0], len(h) < 2 or h[-2] >= p[0]
            KINDS.add("first" if not h else "pair" if last_ts and penult_ts else "closing" if last_ts else "text")
    print("timestamp rules, session steps: smallest |L - T| = %.6g over %d compared rows, %d undecidable" % (min(MARGINS), len(MARGINS), len(SKIPPED)))


def test_streams_are_grammatical_and_generate_equals_the_steps(run):
    cfg, sess, picks = run["cfg"], run["sess"], run["picks"]
    p = _params(cfg)
    for b in range(B):
        s = _stream(picks[:, b], cfg.eot_id)
        assert s and ref.grammatical(s, p[0], p[1], p[2]), s
    sess.set_timestamps(True, 50)
    sess.prefill(_prompt(cfg), want_logits=False)
    free = sess.generate(MAX_NEW, eos_id=-1)                   # the captured step, fed from the device
    for b in range(B):
        assert free[b].tolist() == picks[:, b].tolist(), b
    sess.prefill(_prompt(cfg), want_logits=False)
    stopped = sess.generate(MAX_NEW, eos_id=cfg.eot_id)
    for b in range(B):
        assert stopped[b].tolist() == _stream(picks[:, b], cfg.eot_id), b
    sess.set_timestamps(False)


def test_toggling_the_mode_recaptures_the_step(run):
    cfg, sess = run["cfg"], run["sess"]

    def gen(s, on):
        s.set_timestamps(on, 50)
        s.prefill(_prompt(cfg, with_no_timestamps=not on), want_logits=False)
        return [t.tolist() for t in s.generate(MAX_NEW, eos_id=-1)]

    on1, off1, on2, off2 = gen(sess, True), gen(sess, False), gen(sess, True), gen(sess, False)
    assert on1 == on2 and off1 == off2 and on1 != off1
    _, _, _, fresh = _session(run["prec"])
    fresh.encode(run["audios"])
    assert gen(fresh, False) == off1                            # a session that never saw the mode: the existing path
    assert gen(fresh, True) == on1
    assert on1 == [run["picks"][:, b].tolist() for b in range(B)]
    sess.set_timestamps(False)


def test_mode_off_launches_no_rule_kernel(run):
    cfg, sess = run["cfg"], run["sess"]
    sess.profile(True)
    try:
        for on, prompt in ((False, _prompt(cfg, True)), (True, _prompt(cfg))):
            sess.profile_reset()
            sess.set_timestamps(on, 50)
            sess.prefill(prompt, want_logits=False)
            sess.generate(4, eos_id=-1)
            names = {k for k, v in sess.profile_read().items() if v["launches"] > 0}
            assert ("timestamp_rules" in names) == on, names
            if on:
                assert sess.profile_read()["timestamp_rules"]["launches"] == 4      # the prefill and three decode steps
    finally:
        sess.profile(False)
        sess.set_timestamps(False)


def test_bad_ids_are_refused(run):
    lib, sess = sub("_lib"), run["sess"]
    cfg = run["cfg"]
    for args in [(cfg.vocab, cfg.no_timestamps_id, cfg.eot_id, 50), (cfg.no_timestamps_id, cfg.no_timestamps_id, cfg.eot_id, 50),
                 (cfg.no_timestamps_id + 1, cfg.eot_id, cfg.eot_id, 50), (cfg.no_timestamps_id + 1, cfg.no_timestamps_id, -1, 50),
                 (cfg.no_timestamps_id + 1, cfg.no_timestamps_id, cfg.eot_id, -2)]:
        with pytest.raises(lib.AsrError, match="whisper_set_timestamps"):
            lib.check(lib.load().asr_whisper_set_timestamps(sess._h, 1, *args))


def test_beam_search_in_timestamp_mode(run):
    cfg, sess, picks, prec = run["cfg"], run["sess"], run["picks"], run["prec"]
    p = _params(cfg)
    n = 12
    sess.set_timestamps(True, 50)
    try:
        sess.prefill(_prompt(cfg), want_logits=False)
        w1 = sess.beam_search(1, n, -1)
        top2 = np.sort(run["masked"][:n], axis=2)[:, :, -2:]
        gaps = top2[:, :, 1] - top2[:, :, 0]
        for b in range(B):
            toks = w1[b][0][0].tolist()
            if prec == F32:
                assert toks == picks[:n, b].tolist(), b
            else:                                               # bf16: up to the first step whose greedy top-2 gap is below 0.05, as test_whisper_beam_gpu does
                low = np.nonzero(gaps[:, b] < 0.05)[0]
                upto = int(low[0]) if low.size else n
                assert toks[:upto] == picks[:upto, b].tolist(), b
        sess.prefill(_prompt(cfg), want_logits=False)
        w3 = sess.beam_search(3, n, cfg.eot_id)
        for b in range(B):
            scores = [s for _, s in w3[b]]
            assert np.isfinite(scores).all() and (np.diff(scores) <= 0).all(), (b, scores)
            for toks, _ in w3[b]:
                assert len(toks) and cfg.eot_id not in toks.tolist() and ref.grammatical(toks.tolist(), p[0], p[1], p[2]), (b, toks.tolist())
    finally:
        sess.set_timestamps(False)


def test_transcriber_segments_and_window_offsets(run):
    cfg, sess = run["cfg"], run["sess"]
    wh = sub("whisper")
    ts_begin = cfg.no_timestamps_id + 1
    pcm = [(a * 32767.0).astype(np.int16) for a in run["audios"]]
    tr = wh.WhisperTranscriber(cfg, sess, suppress_tokens=run["sup"], timestamps=True, no_speech_threshold=2.0)
    plain = wh.WhisperTranscriber(cfg, sess, suppress_tokens=run["sup"], remove_repeats=False, no_speech_threshold=2.0)
    out, _ = tr.transcribe(pcm, max_new=MAX_NEW)
    ref_out, _ = plain.transcribe(pcm, max_new=MAX_NEW)
    for b, (r, q) in enumerate(zip(out, ref_out)):
        assert r["language_id"] == q["language_id"] and r["no_speech_prob"] == q["no_speech_prob"], b       # the probe never sees the mode
        assert (r["tokens"] < cfg.eot_id).all() and r["tokens"].tolist() == [t for s in r["segments"] for t in s["tokens"]], b
        assert r["segments"] and all(0.0 <= s["start"] <= s["end"] <= len(pcm[b]) / cfg.sample_rate + 1e-9 for s in r["segments"]), (b, r["segments"])
        assert all(a["end"] <= c["start"] + 1e-9 for a, c in zip(r["segments"], r["segments"][1:])), (b, r["segments"])
        assert r["segments"][0]["start"] <= 1.0                  # max_initial_timestamp
    again, _ = plain.transcribe(pcm, max_new=MAX_NEW)
    assert all(np.array_equal(a["tokens"], q["tokens"]) for a, q in zip(again, ref_out))                  # nothing of the mode is left on the session
    # two windows of one second: the second window's segments are offset by the stride
    long = np.concatenate([pcm[0][:16000], pcm[2][:14000]])
    res, _ = tr.transcribe_file(long, input_audio_length=16000, max_new=MAX_NEW)
    assert res["n_windows"] == 2 and res["stride"] == 16000
    want = [s for w in range(2) for s in wh.split_segments(res["windows"][w], ts_begin, float(w), 1.0)]
    assert res["segments"] == want and any(s["start"] >= 1.0 for s in want) and any(s["start"] < 1.0 for s in want)
    assert res["tokens"].tolist() == [t for w in res["windows"] for t in w if t < ts_begin]
    for w in range(2):
        assert ref.grammatical(_stream(res["windows"][w], cfg.eot_id), ts_begin, ts_begin - 1, cfg.eot_id), res["windows"][w]


def test_at_most_two_steps_were_undecidable():
    print("timestamp rules, session steps: smallest |L - T| = %.6g over %d compared rows; undecidable: %s; branches met: %s"
          % (min(MARGINS), len(MARGINS), SKIPPED, sorted(KINDS)))
    assert len(SKIPPED) <= 2, SKIPPED
