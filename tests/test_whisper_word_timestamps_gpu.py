"""Whisper's token / word timestamps end to end (asr_whisper_set_word_timestamps / asr_whisper_align; tiny synthetic checkpoint, f32 and bf16): the capture
inside the decoder step against the float64 oracle's cross-attention, the three capture paths against each other, the alignment against the float64
statement of tests/whisper_align_ref.py run on the session's own captured scores, the mode's cost when it is off, the refusals and the transcriber.

The audio is noise under a block envelope: under plain noise the tiny checkpoint's cross-attention is nearly uniform (every head within 1e-2 of every
other), and a capture of the wrong head could pass. With the envelope the (layer, head) pairs differ by 2e-2 and more in every utterance; the first test
asserts that on the oracle alone."""
import numpy as np
import pytest

import whisper_align_ref as ref
from conftest import sub
from test_oracle_whisper import unit_audio, whisper_setup

pytestmark = pytest.mark.gpu

BF16, F32 = 0, 1
B, MAX_NEW = 3, 24
LENGTHS = [26240, 12640, 18080]
SEEDS = [709, 710, 707]
PAIRS = [(1, 0), (0, 1)]
ALL_PAIRS = [(0, 0), (0, 1), (1, 0), (1, 1)]
_RUNS = {}


def burst_audio(seed, n, blk=1600):
    rng = np.random.default_rng(seed + 5000)
    env = np.repeat(rng.choice([0.002, 0.05, 1.0, 8.0], size=n // blk + 1), blk)[:n].astype(np.float32)
    return np.clip(unit_audio(seed, n) * env, -1.0, 1.0).astype(np.float32)


def _session(prec):
    cfg, ck, sup, beg = whisper_setup("whisper_tiny_test")
    sup = sorted(set(sup) | set(range(cfg.eot_id + 1, cfg.no_timestamps_id + 1)))
    sess = sub("engine").WhisperSession.from_checkpoint(cfg, ck, precision=prec, suppress_tokens=sup, begin_suppress_tokens=beg)
    return cfg, ck, sup, beg, sess


def _prompt(cfg):
    return np.array([[cfg.sot_id, cfg.first_language_id, cfg.transcribe_id, cfg.no_timestamps_id]] * B, np.int32)


def _generate(sess, cfg, n=MAX_NEW):
    sess.prefill(_prompt(cfg), want_logits=False)
    return np.stack(sess.generate(n, eos_id=-1))              # [B][n]: no stop id, every utterance runs to the limit


def _scores(sess):
    return [sess.align_read(0, b) for b in range(B)]


def _run(prec):
    """One session per precision; its ids and the rows captured while generate() produced them (the captured graph, fed from the device)."""
    if prec not in _RUNS:
        cfg, ck, sup, beg, sess = _session(prec)
        audios = [burst_audio(s, n) for s, n in zip(SEEDS, LENGTHS)]
        n_enc = sess.encode(audios)
        sess.set_word_timestamps(True, PAIRS, MAX_NEW)
        ids = _generate(sess, cfg)
        _RUNS[prec] = dict(cfg=cfg, ck=ck, sup=sup, beg=beg, sess=sess, audios=audios, prec=prec, ids=ids, scores=_scores(sess), n_enc=n_enc.tolist())
    return _RUNS[prec]


@pytest.fixture(scope="module", params=[F32, BF16], ids=["f32", "bf16"])
def run(request):
    return _run(request.param)


def test_captured_scores_are_the_oracles_cross_attention():
    """f32: soft-max of the captured rows = the float64 oracle's cross-attention probabilities of that (layer, head), teacher-forced on the session's ids,
    within the project's f32 parity figure 1e-3; every other (layer, head) is further than 1e-2 away somewhere in every utterance."""
    import torch
    from oracle.whisper_oracle import WhisperOracle
    r = _run(F32)
    cfg = r["cfg"]
    oracle = WhisperOracle(cfg, r["ck"], r["sup"], r["beg"], dtype=torch.float64)
    prompt = _prompt(cfg)[0].tolist()
    worst = 0.0
    for b in range(B):
        with torch.inference_mode():
            k, v = oracle.encode(r["audios"][b])
            probs = ref.cross_attention_probs(oracle, prompt + r["ids"][b, :-1].tolist(), k, v)[:, :, len(prompt) - 1:]     # [Ld][H][MAX_NEW][T]
        assert r["scores"][b].shape == (len(PAIRS), MAX_NEW, r["n_enc"][b]) == (len(PAIRS),) + probs.shape[2:]
        for slot, (l, h) in enumerate(PAIRS):
            for other in ALL_PAIRS:
                if other != (l, h):
                    assert np.abs(probs[l, h] - probs[other]).max() > 1e-2, (b, (l, h), other)      # the inputs can tell the heads apart
            got = ref.softmax(r["scores"][b][slot])
            err = float(np.abs(got - probs[l, h]).max())
            worst = max(worst, err)
            assert err < 1e-3, (b, l, h, err)
        for c in range(B):                                    # ... and the utterances: another utterance's rows are not a near copy either
            if c != b and r["n_enc"][c] >= r["n_enc"][b]:
                assert np.abs(ref.softmax(r["scores"][c][0][:, :r["n_enc"][b]]) - probs[PAIRS[0]]).max() > 1e-2
    print("captured scores vs the float64 oracle: largest probability error %.3g" % worst)


def test_capture_paths_agree(run):
    cfg, sess, ids = run["cfg"], run["sess"], run["ids"]
    want = run["scores"]
    sess.prefill(_prompt(cfg), want_logits=False)             # the same ids fed from the host, step by step
    for t in range(MAX_NEW - 1):
        sess.decode(ids[:, t])
    host = _scores(sess)
    sess.set_word_timestamps(False)
    off = _generate(sess, cfg)
    sess.set_word_timestamps(True, PAIRS, MAX_NEW)
    again_ids = _generate(sess, cfg)                          # toggled off and on: the step is captured again
    again = _scores(sess)
    assert np.array_equal(off, ids) and np.array_equal(again_ids, ids)
    for b in range(B):
        assert np.isfinite(want[b]).all() and np.abs(want[b]).max() > 0
        assert np.array_equal(host[b].view(np.uint32), want[b].view(np.uint32)), b
        assert np.array_equal(again[b].view(np.uint32), want[b].view(np.uint32)), b
    # another pair list: the captured step is stale, the rows are the other heads'
    sess.set_word_timestamps(True, [(0, 0)], MAX_NEW)
    _generate(sess, cfg)
    assert all(not np.array_equal(sess.align_read(0, b)[0], want[b][0]) for b in range(B))
    sess.set_word_timestamps(True, PAIRS, MAX_NEW)


def test_rows_past_max_rows_are_not_written(run):
    cfg, sess = run["cfg"], run["sess"]
    sess.set_word_timestamps(True, PAIRS, 5)
    try:
        _generate(sess, cfg, 9)
        for b in range(B):
            got = sess.align_read(0, b)
            assert got.shape == (len(PAIRS), 5, run["n_enc"][b])
            assert np.array_equal(got.view(np.uint32), run["scores"][b][:, :5].view(np.uint32))
    finally:
        sess.set_word_timestamps(True, PAIRS, MAX_NEW)


def test_align_end_to_end(run):
    cfg, sess = run["cfg"], run["sess"]
    _generate(sess, cfg)
    scores = _scores(sess)
    n_rows, n_frames = [MAX_NEW, 13, 2], [run["n_enc"][0], 30, run["n_enc"][2]]
    frames = sess.align(n_rows, n_frames, 7)
    worst = 0.0
    for b in range(B):
        N, M = n_rows[b], n_frames[b]
        assert frames[b].shape == (N,) and frames[b][0] == 0 and (np.diff(frames[b]) >= 0).all() and frames[b].max() < M, (b, frames[b])
        crop = scores[b][:, :N, :M]
        want, tol = ref.cost_matrix(crop, 7), ref.cost_budget(crop, 7)
        got = sess.align_read(1, b)
        assert got.shape == (N, M) and (np.abs(got - want) <= tol).all(), (b, float(np.abs(got - want).max()), float(tol.min()))
        # the path behind the session's frames: the same DTW kernel on the session's own matrix, through the probe (the product keeps the frames only)
        probe_frames, paths = sub("_probe").whisper_align_op("dtw", [N], [M], cost=got[None])
        path = paths[0]
        assert ref.is_monotone_path(path[:, 0], path[:, 1], N, M), b
        assert np.array_equal(probe_frames[0], frames[b]) and np.array_equal(ref.jump_frames(path[:, 0], path[:, 1]), frames[b]), b
        best = ref.path_cost(want, *ref.dtw(want))
        mine = ref.path_cost(want, path[:, 0], path[:, 1])
        slack = ref.path_slack(want, tol)
        worst = max(worst, (mine - best) / slack)
        assert mine <= best + slack, (b, mine, best, slack)
    print("align: GPU path cost above the float64 optimum, largest share of the slack = %.3g" % worst)
    with pytest.raises(sub("_lib").AsrError, match="whisper_align: the captured rows were aligned already"):
        sess.align(n_rows, n_frames, 7)
    # an utterance left out (n_rows = 0) and the whole encoder length by default
    _generate(sess, cfg)
    frames = sess.align([0, MAX_NEW, 0])
    assert frames[0].size == 0 and frames[2].size == 0 and frames[1].shape == (MAX_NEW,) and frames[1].max() < run["n_enc"][1]


def test_mode_off_costs_nothing(run):
    cfg, sess = run["cfg"], run["sess"]
    sess.profile(True)
    try:
        for on in (False, True):
            sess.set_word_timestamps(on, PAIRS, MAX_NEW)
            sess.profile_reset()
            _generate(sess, cfg, 4)
            prof = sess.profile_read()
            launches = prof.get("align_scores", {"launches": 0})["launches"]
            assert launches == (8 if on else 0), prof           # the prefill and three decode steps, one launch per layer that holds a selected head
    finally:
        sess.profile(False)
        sess.set_word_timestamps(True, PAIRS, MAX_NEW)
    _, _, _, _, fresh = _session(run["prec"])
    fresh.encode(run["audios"])
    assert np.array_equal(_generate(fresh, cfg), run["ids"])  # a session that never saw the mode: the same ids


def test_refusals(run):
    lib, cfg, sess = sub("_lib"), run["cfg"], run["sess"]
    for heads, rows in (([(2, 0)], 8), ([(0, 2)], 8), ([(-1, 0)], 8), ([(1, 0), (1, 0)], 8), (PAIRS, 0), (PAIRS, cfg.max_target_positions + 1),
                        (ALL_PAIRS + [(0, 0)], 8)):
        with pytest.raises(lib.AsrError, match="whisper_set_word_timestamps:"):
            sess.set_word_timestamps(True, heads, rows)
    sess.set_word_timestamps(True, PAIRS, MAX_NEW)
    with pytest.raises(lib.AsrError, match="whisper_align: nothing captured"):
        sess.align([2] * B, [10] * B)
    with pytest.raises(lib.AsrError, match="capture starts at a prefill"):
        sess.decode(np.zeros(B, np.int32))
    _generate(sess, cfg, 6)
    for n_rows, n_frames, width in (([7, 2, 2], None, 7), ([1, 2, 2], None, 7), ([2, 2, 2], [run["n_enc"][0] + 1, 5, 5], 7), ([2, 2, 2], [0, 5, 5], 7),
                                    ([2, 2, 2], None, 4), ([2, 2, 2], None, 11)):
        with pytest.raises(lib.AsrError, match="whisper_align:"):
            sess.align(n_rows, n_frames, width)
    sess.prefill(_prompt(cfg), want_logits=False)
    with pytest.raises(lib.AsrError, match="whisper_beam_search: word-timestamp capture is on"):
        sess.beam_search(2, 4, cfg.eot_id)
    assert np.array_equal(_generate(sess, cfg), run["ids"])   # nothing of the refused calls is left on the session


def _ordered(times, lo, hi):
    return all(lo - 1e-9 <= s <= e <= hi + 1e-9 for s, e in times) and all(a[1] <= b[0] + 1e-9 for a, b in zip(times, times[1:]))


def test_transcriber(run):
    cfg, sess = run["cfg"], run["sess"]
    wh = sub("whisper")
    sess.set_word_timestamps(False)
    pcm = [(a * 32767.0).astype(np.int16) for a in run["audios"]]
    secs = [len(p) / cfg.sample_rate for p in pcm]
    kw = dict(suppress_tokens=run["sup"], remove_repeats=False, no_speech_threshold=2.0)
    plain = wh.WhisperTranscriber(cfg, sess, **kw)
    ref_out, _ = plain.transcribe(pcm, max_new=MAX_NEW)
    try:
        # plain mode, live capture: nothing is decoded twice, the tokens are the plain transcriber's
        live = wh.WhisperTranscriber(cfg, sess, word_timestamps=True, alignment_heads=PAIRS, piece_decoder=lambda ids: "".join(" t%d" % t for t in ids), **kw)
        out, _ = live.transcribe(pcm, max_new=MAX_NEW)
        for b, (r, q) in enumerate(zip(out, ref_out)):
            assert np.array_equal(r["tokens"], q["tokens"]) and len(r["tokens"]) > 0, b
            assert len(r["token_times"]) == len(r["tokens"]) and _ordered(r["token_times"], 0.0, secs[b]), (b, r["token_times"])
            assert [w["tokens"] for w in r["words"]] == [1] * len(r["tokens"]) and [(w["start"], w["end"]) for w in r["words"]] == r["token_times"]
            if len(r["tokens"]) == MAX_NEW:                     # cut off at the limit: the last token ends with the clip
                assert r["token_times"][-1][1] == pytest.approx(secs[b])
        # timestamp mode: the forced pass over the text ids; segments gain their tokens' times
        ts = wh.WhisperTranscriber(cfg, sess, word_timestamps=True, alignment_heads=PAIRS, timestamps=True, **kw)
        out, _ = ts.transcribe(pcm, max_new=MAX_NEW)
        for b, r in enumerate(out):
            assert len(r["token_times"]) == len(r["tokens"]) and _ordered(r["token_times"], 0.0, secs[b]), (b, r["token_times"])
            assert [t for s in r["segments"] for t in s["token_times"]] == r["token_times"]
            assert all(len(s["token_times"]) == len(s["tokens"]) for s in r["segments"])
        assert any(len(r["tokens"]) for r in out)
        # two windows of one second: the second window's token times are offset by the stride
        long = np.concatenate([pcm[0][:16000], pcm[2][:14000]])
        res, _ = ts.transcribe_file(long, input_audio_length=16000, max_new=MAX_NEW)
        n0 = sum(1 for t in res["windows"][0] if t < cfg.no_timestamps_id + 1)
        assert len(res["token_times"]) == len(res["tokens"]) and _ordered(res["token_times"][:n0], 0.0, 1.0) and _ordered(res["token_times"][n0:], 1.0, 2.0)
        # beam search: the forced pass aligns the first hypothesis
        beam = wh.WhisperTranscriber(cfg, sess, word_timestamps=True, alignment_heads=PAIRS, beam_size=2, **kw)
        out, _ = beam.transcribe(pcm, max_new=12)
        want, _ = wh.WhisperTranscriber(cfg, sess, beam_size=2, **kw).transcribe(pcm, max_new=12)
        for b, (r, q) in enumerate(zip(out, want)):
            assert np.array_equal(r["tokens"], q["tokens"]) and len(r["token_times"]) == len(r["tokens"]) and _ordered(r["token_times"], 0.0, secs[b]), b
        again, _ = plain.transcribe(pcm, max_new=MAX_NEW)       # nothing of the mode is left on the session
        assert all(np.array_equal(a["tokens"], q["tokens"]) for a, q in zip(again, ref_out))
    finally:
        sess.set_word_timestamps(True, PAIRS, MAX_NEW)
