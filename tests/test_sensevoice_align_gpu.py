"""GPU, session level: SenseVoiceSession.align / asr_sensevoice_align -- the emission tap against the float64 log soft-max of the logits tap, spans, status
and path score equal to the np.float32 restatement run on the tapped emissions, the greedy round trip (aligning the collapse of the frame-wise arg-max gives
back its runs and its score), transcript variants, graph keys and profile classes beside the other forms, and the argument checks."""
import ctypes as C

import numpy as np
import pytest

import ctc_align_ref as ref
import ctc_timing_ref as R
from conftest import sub
from helpers import kaldi_audio, sensevoice_setup

pytestmark = pytest.mark.gpu

BF16, F32 = 0, 1
U32 = 2.0 ** -24


def _audios(cfg):
    # ragged batch of three; the shortest is one frame (win_length samples): a single LFR row behind the prompt rows
    return [kaldi_audio(31, 32000), kaldi_audio(32, cfg.win_length), kaldi_audio(33, 9000)], [2, 0, 4]


def _plain_collapse(ids, blank):
    """(tokens, first rows, last rows) of the plain (non-circular) collapse: maximal runs of equal ids, blank runs dropped."""
    tok, first, last = [], [], []
    t = 0
    while t < len(ids):
        e = t
        while e + 1 < len(ids) and ids[e + 1] == ids[t]:
            e += 1
        if ids[t] != blank:
            tok.append(int(ids[t])); first.append(t); last.append(e)
        t = e + 1
    return np.asarray(tok, np.int32), np.asarray(first, np.int32), np.asarray(last, np.int32)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _abs_dot(cfg, ck, enc_out, prec):
    """sum_k |a_k| |w_nk| per (row, column) of the head, over the operands as the session holds them."""
    rnd = R.bf16_round if prec == BF16 else (lambda x: x)
    return np.abs(rnd(enc_out).astype(np.float64)) @ np.abs(rnd(np.asarray(ck["ctc.ctc_lo.weight"], np.float32)).astype(np.float64)).T


@pytest.mark.parametrize("prec", [F32, BF16], ids=["f32", "bf16"])
def test_align_against_taps_and_the_greedy_round_trip(prec):
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    sess = sub("engine").SenseVoiceSession.from_checkpoint(cfg, ck, precision=prec)
    audios, langs = _audios(cfg)
    assert cfg.seq_len(audios[1].size) == cfg.n_prompt + 1
    K, P = cfg.d_model, cfg.n_prompt
    sess.taps(True)
    sess.run_timed(audios, langs)
    rows = sess.utterance_rows([a.size for a in audios])
    ids_tap, flp_tap = sess.tap("frame_ids", dtype=np.int32)[:, 0].copy(), sess.tap("frame_logprob")[:, 0].copy()
    greedy = [_plain_collapse(ids_tap[r0 + P:r0 + T], cfg.blank_id) for r0, T in rows]
    targets = [g[0] for g in greedy]
    assert sum(len(t) for t in targets) > 0
    recs = sess.align(audios, langs, targets)
    logits, em, enc = sess.tap("logits"), sess.tap("align_logprob"), sess.tap("enc_out")
    ld = em.shape[1]
    assert ld == (max(len(t) for t in targets) + 1 + 3) // 4 * 4
    abs_dot = _abs_dot(cfg, ck, enc, prec)
    excluded = 0
    for b, ((r0, T), rec, (tok, first, last)) in enumerate(zip(rows, recs, greedy)):
        L = len(tok)
        v = logits[r0:r0 + T].astype(np.float64)
        _, lp_max, spread = R.frame_logprob(v)
        lsm = v - np.logaddexp.reduce(v, axis=1)[:, None]
        lse_budget = R.budget(cfg.vocab, lp_max, spread, K=K, abs_dot=abs_dot[r0:r0 + T].max(axis=1), vmax=np.abs(v).max(axis=1))
        cols = [cfg.blank_id] + [int(c) for c in tok]
        # 1. the emission tap: log soft-max of the logits tap at the blank and the targets, -inf behind them
        worst = 0.0
        for j, c in enumerate(cols):
            bound = K * U32 * abs_dot[r0:r0 + T, c] + lse_budget
            err = np.abs(em[r0:r0 + T, j].astype(np.float64) - lsm[:, c])
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (b, j, float(err.max()), float(bound.min()))
        assert np.all(np.isneginf(em[r0:r0 + T, len(cols):]))
        print(f"align_logprob tap utterance {b}: largest error / bound = {worst:.3g}")
        # 2. spans, status and path score: the f32 restatement on the tapped emissions, bit for bit
        want = ref.align32(em[r0 + P:r0 + T, :L + 1], tok)
        assert rec["aligned"] and want["status"] == 0
        assert _bits(rec["path_score"]) == _bits(want["path_score"])
        assert np.array_equal(rec["first_frame"], want["first"] + P) and np.array_equal(rec["last_frame"], want["last"] + P)
        assert np.array_equal(_bits(rec["logprob"]), _bits(want["logprob"]))
        w64 = ref.align64(em[r0 + P:r0 + T, :L + 1], tok)
        assert abs(rec["loglik"] - w64["loglik"]) <= w64["budget"] and rec["loglik"] >= rec["path_score"] - w64["budget"]
        # 3. the greedy round trip: the frame-wise arg-max path is the best path of any transcript and an alignment of its own collapse
        top2 = np.sort(logits[r0 + P:r0 + T, :cfg.vocab], axis=1)[:, -2:]
        if (top2[:, 0] == top2[:, 1]).any():
            print(f"utterance {b}: an exact f32 tie between two columns of a row; excluded from the round trip")
            excluded += 1
            continue
        assert np.array_equal(rec["first_frame"], first + P) and np.array_equal(rec["last_frame"], last + P), b
        speech = np.arange(r0 + P, r0 + T)
        greedy_score = float(flp_tap[speech].astype(np.float64).sum())
        # per row: the recomputed logit against the head's own (two f32 accumulation orders, each within K 2^-24 sum |a_k w_k| of the exact value, + 1e-6 for
        # the roundings of the two log-sum-exp forms, as test_ctc_topk_gpu bounds the same difference); and the f32 sum of the path
        bound = float((2 * K * U32 * abs_dot[speech, ids_tap[speech]] + 1e-6).sum()) + len(speech) * U32 * abs(greedy_score)
        assert abs(rec["path_score"] - greedy_score) <= bound, (b, rec["path_score"], greedy_score, bound)
    assert excluded <= 1
    # transcript variants: two tokens swapped; longer than the speech rows; empty
    b0 = max(range(3), key=lambda b: len(targets[b]))
    t0 = targets[b0].copy()
    k = next(i for i in range(len(t0) - 1) if t0[i] != t0[i + 1])
    t0[k], t0[k + 1] = t0[k + 1], t0[k]
    var = [np.zeros(0, np.int32)] * 3
    var[b0] = t0
    b1 = 1 if b0 != 1 else 0
    n_speech = rows[b1][1] - P
    var[b1] = np.arange(1, n_speech + 2, dtype=np.int32) % (cfg.vocab - 1) + 1          # one token more than speech rows
    var[b1][var[b1] == cfg.blank_id] = cfg.blank_id + 1
    out = sess.align(audios, langs, var)
    assert out[b0]["aligned"] and out[b0]["loglik"] < recs[b0]["loglik"]
    assert not out[b1]["aligned"] and out[b1]["path_score"] == -np.inf and out[b1]["loglik"] == -np.inf and len(out[b1]["first_frame"]) == 0
    b2 = 3 - b0 - b1
    assert out[b2]["aligned"] and len(out[b2]["first_frame"]) == 0 and np.isfinite(out[b2]["path_score"]) and out[b2]["loglik"] == out[b2]["path_score"]
    sess.close()


def test_align_beside_the_other_forms():
    """run / align / run_timed / align / run on the same shapes: every form replays its own graph and nobody else's; the untimed run launches what it did."""
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    sess = sub("engine").SenseVoiceSession.from_checkpoint(cfg, ck, precision=BF16)
    audios, langs = _audios(cfg)
    timed0 = sess.run_timed(audios, langs)
    targets = [r["ids"][r["first_frame"] >= cfg.n_prompt] for r in timed0]
    u, a, t = [], [], []
    for _ in range(2):
        u.append(sess.run(audios, langs)); a.append(sess.align(audios, langs, targets)); t.append(sess.run_timed(audios, langs))
        a.append(sess.align(audios, langs, targets)); u.append(sess.run(audios, langs))
    for x in u[1:]:
        assert all(np.array_equal(p, q) for p, q in zip(u[0], x))
    for x in t:
        for p, q in zip(timed0, x):
            assert all(np.array_equal(_bits(p[k]) if k == "logprob" else p[k], _bits(q[k]) if k == "logprob" else q[k]) for k in p)
    for x in a[1:]:
        for p, q in zip(a[0], x):
            assert p["aligned"] == q["aligned"] and _bits(p["path_score"]) == _bits(q["path_score"]) and _bits(p["loglik"]) == _bits(q["loglik"])
            assert np.array_equal(p["first_frame"], q["first_frame"]) and np.array_equal(p["last_frame"], q["last_frame"])
            assert np.array_equal(_bits(p["logprob"]), _bits(q["logprob"]))
    # other transcript lengths on the same audio: another key, another answer, and the first key still replays
    shorter = [x[:-1] if len(x) else x for x in targets]
    s1 = sess.align(audios, langs, shorter)
    again = sess.align(audios, langs, targets)
    assert all(len(p["first_frame"]) == len(x) for p, x in zip(s1, shorter) if p["aligned"])
    assert all(_bits(p["path_score"]) == _bits(q["path_score"]) for p, q in zip(a[0], again))
    # profile classes
    sess.profile(True)
    prof = []
    for call in (lambda: sess.run(audios, langs), lambda: sess.align(audios, langs, targets), lambda: sess.run(audios, langs)):
        sess.profile_reset()
        call()
        prof.append({k: v["launches"] for k, v in sess.profile_read().items() if v["launches"]})
    assert prof[0] == prof[2]
    assert set(prof[1]) - set(prof[0]) == {"ctc_align_em", "ctc_align"} and prof[1]["ctc_align_em"] == 1 and prof[1]["ctc_align"] == 1
    assert all(prof[1][k] == prof[0][k] for k in prof[1] if k in prof[0]) and set(prof[0]) - set(prof[1]) <= {"ctc_tail"}
    sess.close()


def test_bad_targets_are_errors():
    eng, lib = sub("engine"), sub("_lib")
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    sess = eng.SenseVoiceSession.from_checkpoint(cfg, ck, precision=F32)
    audios, langs = _audios(cfg)
    ok = [[1, 2], [], [3]]
    assert len(sess.align(audios, langs, ok)) == 3
    for bad in ([[1, cfg.blank_id], [], [3]], [[1, 2], [cfg.vocab], [3]], [[1, 2], [], [-1]]):
        with pytest.raises(lib.AsrError):
            sess.align(audios, langs, bad)
    flat, packed, offs = sess._pack(audios)
    with pytest.raises(lib.AsrError):                                # offsets that decrease
        sess.align_packed(packed, offs, np.asarray(langs, np.int32), np.asarray([1, 2, 3], np.int32), np.asarray([0, 2, 1, 3], np.int32))
    assert len(sess.align(audios, langs, ok)) == 3                   # the session is still usable
    sess.close()
    from test_oracle_paraformer import paraformer_setup
    pcfg, pck = paraformer_setup("paraformer_tiny")
    ps = eng.ParaformerSession.from_checkpoint(pcfg, pck, precision=F32)
    audio = np.ascontiguousarray(kaldi_audio(5, 16000), np.float32)
    offs = np.asarray([0, audio.size], np.int64)
    i32 = lambda *v: np.asarray(v, np.int32)
    lang, tid, toff, first, last, st = i32(0), i32(1), i32(0, 1), i32(0), i32(0), i32(0)
    lp, path, lik = (np.zeros(1, np.float32) for _ in range(3))
    ip, fp = (lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))), (lambda x: x.ctypes.data_as(C.POINTER(C.c_float)))
    with pytest.raises(lib.AsrError):
        lib.check(lib.load().asr_sensevoice_align(ps._h, audio.ctypes.data_as(C.c_void_p), 0, offs.ctypes.data_as(C.POINTER(C.c_int64)), 1, ip(lang), ip(tid), ip(toff),
                                                  ip(first), ip(last), fp(lp), fp(path), fp(lik), ip(st)))
    ps.close()


def test_real_vocabulary_width_through_a_session():
    """sensevoice_small, batch 2: the emission kernel gathers from the real 25 055-column head."""
    cfg, ck = sensevoice_setup("sensevoice_small")
    sess = sub("engine").SenseVoiceSession.from_checkpoint(cfg, ck, precision=BF16)
    audios, langs = [kaldi_audio(41, 24000), kaldi_audio(42, 7777)], [0, 3]
    timed = sess.run_timed(audios, langs)
    targets = [r["ids"][r["first_frame"] >= cfg.n_prompt] for r in timed]
    targets[1] = np.concatenate([targets[1][:-1], np.asarray([cfg.vocab - 1], np.int32)])      # the last valid column, in the partly valid slab
    recs = sess.align(audios, langs, targets)
    for rec, t, a in zip(recs, targets, audios):
        T = cfg.seq_len(a.size)
        assert rec["aligned"] and len(rec["first_frame"]) == len(t)
        assert (rec["first_frame"] >= cfg.n_prompt).all() and (rec["last_frame"] < T).all() and (rec["first_frame"] <= rec["last_frame"]).all()
        assert (rec["first_frame"][1:] > rec["last_frame"][:-1]).all()
        assert np.isfinite(rec["logprob"]).all() and (rec["logprob"] <= 0).all() and rec["path_score"] <= rec["loglik"] + 1e-3 <= 1e-3
    sess.close()
