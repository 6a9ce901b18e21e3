"""GPU, session level: ParaformerSession.run_timed / asr_paraformer_run_timed -- ids equal the untimed run's, the fire rows equal the rule's statement on the
tapped alphas exactly, the log-probabilities match the float64 statement of the tapped logits within the derived budget -- and the transcriber's timestamps."""
import numpy as np
import pytest

import ctc_timing_ref as C
import paraformer_timing_ref as R
from conftest import sub
from helpers import golden_cases, kaldi_audio, load_golden
from test_oracle_paraformer import paraformer_setup

pytestmark = pytest.mark.gpu

BF16, F32 = 0, 1


def _tiny_batch():
    """Ragged batch of three golden clips; the middle one (400 samples, one LFR row) yields zero tokens."""
    cases = [c for _, c in golden_cases(load_golden("paraformer_tiny"))]
    picked = [cases[0], cases[2], cases[3]]
    assert int(picked[1]["num_id"][0]) == 0
    return [kaldi_audio(c["audio_seed"], c["n_samples"]) for c in picked]


def _invariants(rec, T):
    n = len(rec["ids"])
    assert len(rec["fire_frame"]) == len(rec["logprob"]) == n
    assert (np.diff(rec["fire_frame"]) > 0).all() and (rec["fire_frame"] >= 0).all() and (rec["fire_frame"] <= T).all()
    assert (rec["logprob"] <= 0).all() and np.isfinite(rec["logprob"]).all()


def _check_against_taps(cfg, sess, audios, recs):
    """The taps are what the kernels read: the fire rows need no margin (in bf16 either); the scores carry the budget of the epilogue's sum of exponentials."""
    alphas, logits = sess.tap("alphas")[:, 0], sess.tap("logits")
    fire_tap, lp_tap = sess.tap("fire_frames", dtype=np.int32), sess.tap("token_logprob")
    trow = sess.token_rows([len(r["ids"]) for r in recs])
    worst = 0.0
    for b, ((r0, T), t0, rec) in enumerate(zip(sess.utterance_rows([a.size for a in audios]), trow, recs)):
        n = len(rec["ids"])
        assert np.array_equal(rec["fire_frame"], R.fire_frames(alphas[r0:r0 + T], cfg.tail_threshold)), b
        assert np.array_equal(fire_tap[b, :n], rec["fire_frame"]) and np.array_equal(lp_tap[b, :n].view(np.uint32), rec["logprob"].view(np.uint32))
        if n == 0:
            continue
        ref_ids, ref_lp, spread = C.frame_logprob(logits[t0:t0 + n])
        bud = C.budget(cfg.vocab, ref_lp, spread)
        err = np.abs(rec["logprob"].astype(np.float64) - ref_lp)
        worst = max(worst, float((err / bud).max()))
        assert np.array_equal(rec["ids"], ref_ids), b
        assert (err <= bud).all(), (b, err.max(), bud.min())
    print(f"token logprob vs the float64 log soft-max of the logits tap: max err / budget {worst:.3f}")


@pytest.mark.parametrize("prec", [F32, BF16])
def test_timed_run_equals_untimed_and_the_reference(prec):
    cfg, ck = paraformer_setup("paraformer_tiny")
    sess = sub("engine").ParaformerSession.from_checkpoint(cfg, ck, precision=prec)
    audios = _tiny_batch()
    # graph key: the second call of a kind captures, the third replays -- nobody replays the other's graph
    t1 = sess.run_timed(audios)
    u1 = sess.run(audios)
    t2 = sess.run_timed(audios)
    u2 = sess.run(audios)
    t3 = sess.run_timed(audios)
    assert sum(len(u) for u in u1) > 0 and len(u1[1]) == 0
    for a, b, c, u, v, audio in zip(t1, t2, t3, u1, u2, audios):
        assert np.array_equal(a["ids"], u) and np.array_equal(u, v)
        for k in ("ids", "fire_frame"):
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k])
        assert np.array_equal(a["logprob"].view(np.uint32), b["logprob"].view(np.uint32)) and np.array_equal(a["logprob"].view(np.uint32), c["logprob"].view(np.uint32))
        _invariants(a, cfg.seq_len(audio.size))
    # the untimed run launches what it launched before a timed run existed; the timed run adds at most the gather launch
    sess.profile(True)
    counts = []
    for timed in (False, True, False):
        sess.profile_reset()
        sess.run_timed(audios) if timed else sess.run(audios)
        counts.append({k: v["launches"] for k, v in sess.profile_read().items()})
    sess.profile(False)
    assert counts[0] == counts[2] and set(counts[1]) == set(counts[0])
    assert 0 <= sum(counts[1].values()) - sum(counts[0].values()) <= 1
    sess.taps(True)
    recs = sess.run_timed(audios)
    logits_timed = sess.tap("logits").copy()
    _check_against_taps(cfg, sess, audios, recs)
    for a, r in zip(t1, recs):
        assert np.array_equal(a["ids"], r["ids"]) and np.array_equal(a["fire_frame"], r["fire_frame"])
        assert np.array_equal(a["logprob"].view(np.uint32), r["logprob"].view(np.uint32))
    plain = sess.run(audios)                                       # the timed scan leaves every other output as the untimed one writes it
    logits_plain = sess.tap("logits")
    for t0, u in zip(sess.token_rows([len(p) for p in plain]), plain):
        n = max(len(u), 1)
        assert np.array_equal(logits_timed[t0:t0 + n].view(np.uint32), logits_plain[t0:t0 + n].view(np.uint32))
    sess.close()


def test_real_vocabulary_width_through_a_session():
    """paraformer_large, batch 2: the 8404-column head (132 slabs, the last one partly valid) on token rows counted on the device."""
    g = load_golden("paraformer_large")
    cfg, ck = paraformer_setup(str(g["cfg_name"]), int(g["ckpt_seed"]))
    sess = sub("engine").ParaformerSession.from_checkpoint(cfg, ck, precision=BF16)
    audios = [kaldi_audio(c["audio_seed"], c["n_samples"]) for _, c in golden_cases(g)][:2]
    plain = sess.run(audios)
    sess.taps(True)
    recs = sess.run_timed(audios)
    assert sum(len(r["ids"]) for r in recs) > 0
    for rec, u, a in zip(recs, plain, audios):
        assert np.array_equal(rec["ids"], u)
        _invariants(rec, cfg.seq_len(a.size))
    _check_against_taps(cfg, sess, audios, recs)
    sess.close()


def test_transcriber_timestamps_over_two_windows(tmp_path):
    cfg, ck = paraformer_setup("paraformer_tiny")
    pf, shim = sub("paraformer"), sub("ort_shim")
    vocab = [f"t{i}" for i in range(cfg.vocab)]
    vocab[0], vocab[1], vocab[2], vocab[-1] = "<blank>", "<s>", "</s>", "<unk>"
    folder = str(tmp_path / "Paraformer_MI355X")
    pf.export_paraformer(folder, cfg, ck, vocab, "zh", "zh", precision=1)
    tr = pf.ParaformerTranscriber(folder)
    tr.audio_meta = shim.NodeArg("audio", [1, 1, 16000], np.float32)        # a static 1 s window, as the reference's fixed-length exports declare
    pcm = kaldi_audio(51, 26000).astype(np.int16)                           # 1.625 s: two windows at a 0.75 s stride, the second zero-padded
    before = tr.transcribe(pcm, sliding_window=12000)
    out = tr.transcribe(pcm, sliding_window=12000, timestamps=True)
    after = tr.transcribe(pcm, sliding_window=12000)
    assert before["windows"] == out["windows"] == 2
    assert set(before) == set(after) == set(out) - {"tokens"} and before["text"] == out["text"] == after["text"]
    for x, y, z in zip(before["token_ids"], out["token_ids"], after["token_ids"]):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    toks, dur = out["tokens"], pcm.size / 16000
    assert [t["id"] for t in toks] == [int(i) for w in out["token_ids"] for i in w] and len(toks) > 0       # stop ids dropped with their records
    assert all(set(t) == {"id", "text", "start", "end", "logprob"} and t["text"] == vocab[t["id"]] and t["logprob"] <= 0 for t in toks)
    assert all(0.0 <= t["start"] <= t["end"] <= dur for t in toks)
    native, row_s, T = tr.session._native, cfg.lfr_n * cfg.hop_length / cfg.sample_rate, cfg.seq_len(16000)
    got = iter(toks)
    late = 0
    for k, off in enumerate((0.0, 0.75)):
        win = np.zeros(16000, np.float32)
        seg = pcm[k * 12000:k * 12000 + 16000].astype(np.float32)
        win[:seg.size] = seg
        rec = native.run_timed([win])[0]
        spans = R.token_times(rec["fire_frame"], T, row_s)
        for i, (s, e), lp in zip(rec["ids"], spans, rec["logprob"]):
            if int(i) in tr.stop_token_ids:
                continue
            t = next(got)
            assert t["id"] == int(i) and t["start"] == min(off + s, dur) and t["end"] == min(off + e, dur) and t["logprob"] == float(lp)
            late += int(k == 1 and t["end"] > 0.75)
    assert next(got, None) is None
    assert late > 0 or len(out["token_ids"][1]) == 0                                                         # window offsets are applied
    assert 0.75 + T * row_s > dur                                                                           # so clipping is in play for a token on the last rows


def test_tool_dump_with_and_without_timestamps(tmp_path):
    """tools/transcribe.py --family paraformer --timestamps writes the token list into the dump; without the flag the dump is what it was."""
    import importlib.util
    import json
    import os
    import types
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("transcribe_tool", os.path.join(ROOT, "tools", "transcribe.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    cfg, ck = paraformer_setup("paraformer_tiny")
    vocab = [f"t{i}" for i in range(cfg.vocab)]
    vocab[0], vocab[1], vocab[2], vocab[-1] = "<blank>", "<s>", "</s>", "<unk>"
    folder = str(tmp_path / "Paraformer_MI355X")
    sub("paraformer").export_paraformer(folder, cfg, ck, vocab, "zh", "zh", precision=1)
    wav = str(tmp_path / "clip.wav")
    sub("audio_io").write_wav_int16(wav, kaldi_audio(61, 20000).astype(np.int16), 16000)
    base = dict(family="paraformer", model=folder, wav=[wav], language="zh", tokenizer=None, precision="f32", sliding_window=0, strict_wav=True,
                repeat_penalty=1.0, beam=1)
    plain = tool.run(types.SimpleNamespace(**base))["files"][0]
    timed = tool.run(types.SimpleNamespace(**base, timestamps=True))["files"][0]
    assert "tokens" not in plain and set(timed) == set(plain) | {"tokens"} and timed["windows"] == plain["windows"] and timed["text"] == plain["text"]
    assert [t["id"] for t in timed["tokens"]] == plain["windows"][0] and len(timed["tokens"]) > 0
    assert all(set(t) == {"id", "text", "start", "end", "logprob"} and 0.0 <= t["start"] <= t["end"] <= 1.25 and t["logprob"] <= 0 for t in timed["tokens"])
    json.dumps(timed)                                          # plain Python numbers: the dump serialises
