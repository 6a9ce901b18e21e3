"""CPU: the VAD's statement (tests/vad_ref.py) against brute force, its named edges, the committed speech clips, and the host logic of segmenter.py.

Stage 2 is checked against a frame-by-frame state machine written here independently of vad_ref's run lists."""
import numpy as np
import pytest

import vad_cases as K
import vad_ref as V
from conftest import sub


# ------------------------------------------------------------------------------------------------ brute force
def _brute_mask(q, thr, p):
    """Rules (a), (b), (c) frame by frame: one pass each, no run lists."""
    F = len(q)
    m = [bool(v >= thr) for v in q]
    out, f = list(m), 0
    while f < F:                                                     # (a)
        if m[f]:
            g = f
            while g < F and m[g]:
                g += 1
            if g - f < p.min_speech:
                for i in range(f, g):
                    out[i] = False
            f = g
        else:
            f += 1
    m, out = out, list(out)
    last_speech = None
    for f in range(F):                                               # (b): a pause is bridged when speech comes back soon enough
        if m[f]:
            if last_speech is not None and 0 < f - last_speech - 1 < p.min_pause:
                for i in range(last_speech + 1, f):
                    out[i] = True
            last_speech = f
    m = out
    return [any(m[max(0, f - p.pad):min(F, f + p.pad + 1)]) for f in range(F)]          # (c)


def _brute_segments(q, thr, p):
    mask = _brute_mask(q, thr, p)
    F, segs, f = len(q), [], 0
    while f < F:
        if not mask[f]:
            f += 1
            continue
        g = f
        while g < F and mask[g]:
            g += 1
        s = f
        while g - s > p.max_frames:
            best = None
            for c in range(s + p.max_frames // 2, s + p.max_frames + 1):
                if best is None or q[c] <= q[best]:
                    best = c
            segs.append((s, best))
            s = best
        segs.append((s, g))
        f = g
    return mask, segs


def test_stage2_against_a_state_machine():
    rng = np.random.default_rng(0)
    n_split = 0
    for trial in range(400):
        F = int(rng.integers(0, 401))
        p = V.Params(p_floor=float(rng.choice([0.05, 0.1, 0.5, 1.0])), margin=int(rng.integers(0, 6)), peak_drop=int(rng.integers(0, 6)),
                     abs_level=int(rng.integers(0, 12)), min_speech=int(rng.integers(0, 6)), min_pause=int(rng.integers(0, 9)), pad=int(rng.integers(0, 5)),
                     max_frames=int(rng.integers(2, 30)))
        # levels with structure: stretches of low and high values, so runs of every length occur
        q = np.zeros(F, dtype=np.int64)
        at = 0
        while at < F:
            n = int(rng.integers(1, 25))
            q[at:at + n] = rng.integers(0, 6, size=min(n, F - at)) + (8 if rng.random() < 0.5 else 0)
            at += n
        floor, peak, thr = V.stats(q, p)
        if F:
            cum = np.cumsum(np.bincount(q, minlength=V.LEVELS))
            need = int(np.ceil(np.float64(np.float32(p.p_floor)) * F))
            assert cum[floor] >= need and (floor == 0 or cum[floor - 1] < need) and peak == q.max()
        assert thr == max(p.abs_level, min(floor + p.margin, peak - p.peak_drop))
        runs = V.padded_runs(q, thr, p)
        segs = V.split_runs(runs, q, p.max_frames)
        mask, want = _brute_segments(q.tolist(), thr, p)
        assert segs == want, (trial, F, p)
        union = np.zeros(F, dtype=bool)
        for s, e in runs:
            union[s:e] = True
        assert np.array_equal(union, mask)                                               # the union before splitting is the padded mask
        assert all(0 <= s < e <= F and e - s <= p.max_frames for s, e in segs)
        assert all(a[1] <= b[0] for a, b in zip(segs, segs[1:]))                         # ordered and disjoint
        n_split += len(segs) - len(runs)
        if F == 0:
            assert V.stage2(np.zeros(0, np.float32), 0, 7, p)[2].shape == (0, 2)
    assert n_split > 100


def _segs(q, **kw):
    p = V.Params(**{**dict(margin=0, peak_drop=2000, abs_level=5, min_speech=4, min_pause=6, pad=3, max_frames=1000), **kw})
    q = np.asarray(q)
    return V.split_runs(V.padded_runs(q, V.stats(q, p)[2], p), q, p.max_frames)


def _q(*runs):
    return np.concatenate([np.full(n, 9 if s else 1) for s, n in runs])


def test_named_edges():
    S, P = True, False
    assert _segs(_q((P, 20), (S, 3), (P, 20))) == [] and _segs(_q((P, 20), (S, 4), (P, 20))) == [(17, 27)]                   # min_speech - 1 / min_speech
    assert _segs(_q((P, 9), (S, 5), (P, 5), (S, 5), (P, 9)), pad=0) == [(9, 24)]                                              # a pause of min_pause - 1 is bridged
    assert _segs(_q((P, 9), (S, 5), (P, 6), (S, 5), (P, 9)), pad=0) == [(9, 14), (20, 25)]                                    # one of min_pause is kept
    assert _segs(_q((P, 6), (S, 5), (P, 6)), pad=0) == [(6, 11)] and _segs(_q((P, 5), (S, 5)), min_pause=50) == [(2, 10)]     # a pause at an edge is never bridged
    assert _segs(_q((P, 1), (S, 6), (P, 30), (S, 6), (P, 2))) == [(0, 10), (34, 45)]                                          # pad clipped at both ends
    assert _segs(_q((P, 10), (S, 5), (P, 6), (S, 5), (P, 10))) == [(7, 29)]                                                   # pad merges two runs (6 = 2 pad: they touch)
    assert _segs(_q((P, 10), (S, 5), (P, 7), (S, 5), (P, 10))) == [(7, 18), (19, 30)]
    # constant level: peak - peak_drop wins and every frame is speech; all zeros: abs_level wins and none is
    const = np.full(30, 400)
    p = V.Params(abs_level=100, min_speech=1, min_pause=1, pad=0, max_frames=100)
    assert V.stats(const, p) == (400, 400, 384) and V.split_runs(V.padded_runs(const, 384, p), const, 100) == [(0, 30)]
    pz = V.default_params(16000, 32768.0)
    qz, st, sz = V.stage2(np.zeros(80, np.float32), 80 * 160, 160, pz)
    assert st == (0, 0, pz.abs_level) and sz.shape == (0, 2) and np.all(qz == 0)
    # the cut takes the latest minimum of [start + max_frames / 2, start + max_frames]
    q = np.full(40, 9)
    q[[12, 15, 18]] = 7                                                  # 18 is past the window [5 + 5 .. 5 + 10]: 15 is the latest minimum inside it
    q[:5] = 1
    assert V.split_runs([(5, 40)], q, 10)[:2] == [(5, 15), (15, 25)]     # (second window [20, 25]: all equal, the latest frame)
    # input-frame offsets: the last segment ends at n, not at F H
    qq, st, seg = V.stage2(np.full(10, 1e6, np.float32), 10 * 160 - 7, 160, V.Params(min_speech=1, pad=0))
    assert seg.tolist() == [[0, 10 * 160 - 7]]


def test_level_rule_is_monotone_and_fine():
    rng = np.random.default_rng(1)
    bits = np.sort(rng.integers(0, 0x7f800000, size=200000, dtype=np.int64)).astype(np.uint32)
    e = bits.view(np.float32)
    q = V.level(e)
    assert np.all(np.diff(q) >= 0) and q.min() == 0 and q.max() == 1023
    nxt = (bits + 1).view(np.float32)                                    # adjacent float32 values: at most one level apart
    d = V.level(nxt) - q
    assert d.min() == 0 and d.max() <= 1
    edge = ((np.arange(V.Q0 + 1, V.Q0 + 1024, dtype=np.int64) << 20) - 1).astype(np.uint32)       # the last float32 of every level: its neighbour is one level up
    assert np.array_equal(V.level((edge + 1).view(np.float32)) - V.level(edge.view(np.float32)), np.ones(edge.size, np.int64))
    assert V.level(np.float32(0)) == 0 and V.level(np.float32(2.0 ** -40)) == 0 and V.level(np.float32(2.0 ** -39)) == 8
    assert np.array_equal(V.level(e), sub("engine").vad_level(e))        # the package's host copy of the rule
    assert V.hop(16000) == 160 and V.hop(44100) == 441 and V.hop(11025) == 110 and V.hop(100) == 1


def test_default_parameters_agree():
    eng = sub("engine")
    for rate, fs in ((16000, 32768.0), (44100, 1.0), (8000, 32768.0)):
        want = V.default_params(rate, fs)
        got = eng.VadParams().to_c(rate, fs, 3000)
        assert (got.margin, got.peak_drop, got.abs_level, got.min_speech, got.min_pause, got.pad, got.max_frames) == \
               (want.margin, want.peak_drop, want.abs_level, want.min_speech, want.min_pause, want.pad, 3000)
    assert V.default_params(16000, 32768.0).abs_level == 458


# ------------------------------------------------------------------------------------------------ committed audio
def test_committed_speech_clips():
    x, spans = K.natural_with_gaps()
    p = V.default_params(K.RATE, 32768.0)
    H = V.hop(K.RATE)
    e, q, st, segs = V.vad(x, K.RATE, p)
    print(f"{segs.shape[0]} segments, floor {st[0]}, peak {st[1]}, thr {st[2]}")
    slack = (p.pad + 1) * H
    owner = []
    for s, e_ in segs:
        inside = [i for i, (a, b) in enumerate(spans) if s >= a - slack and e_ <= b + slack]
        assert len(inside) == 1, (s, e_, spans)                          # within one clip's span widened by pad + 1 frames ...
        assert sum(1 for a, b in spans if s < b and e_ > a) == 1         # ... and touching no other clip
        owner.append(inside[0])
    assert set(owner) == {0, 1, 2}                                       # every clip holds at least one segment
    assert np.all(segs[:, 1] - segs[:, 0] <= p.max_frames * H) and np.all(segs[1:, 0] >= segs[:-1, 1])


def test_planted_bursts_exactly():
    """The same audio and the same equality as tests/test_vad_gpu.py: the segments are the planted spans +- pad."""
    x, _ = K.planted_audio()
    p = V.default_params(K.RATE, 32768.0)
    e, q, st, segs = V.vad(x, K.RATE, p)
    assert np.abs(q - st[2]).min() >= 16
    assert np.array_equal(segs, K.planted_expected(p.pad, x.size))


# ------------------------------------------------------------------------------------------------ host logic
def test_pack_and_plan_batches():
    seg = sub("segmenter")
    audio = np.arange(40, dtype=np.int16).reshape(20, 2)
    segs = np.array([[2, 5], [5, 6], [10, 20]])
    packed, offs = seg.pack(audio, segs, 2)
    assert offs.tolist() == [0, 3, 4, 14] and np.array_equal(packed, np.concatenate([audio[2:5], audio[5:6], audio[10:20]]).reshape(-1))
    packed, offs = seg.pack(audio, np.zeros((0, 2), np.int64), 2)
    assert packed.size == 0 and offs.tolist() == [0]
    lens = [5, 5, 5, 30, 2, 2, 2, 2, 9]
    starts = np.cumsum([0] + [n + 1 for n in lens[:-1]])
    segs = np.stack([starts, starts + lens], axis=1)
    plan = seg.plan_batches(segs, max_batch=3, max_frames_total=12)
    assert plan == [(0, 2), (2, 3), (3, 4), (4, 7), (7, 9)]              # in order, <= 3 segments, <= 12 frames; the one of 30 alone
    assert [i for a, b in plan for i in range(a, b)] == list(range(len(lens)))
    assert seg.plan_batches(np.zeros((0, 2), np.int64), 4, 100) == []
    assert seg.limit_frames(480000, 48000, 16000) == 1440000 and seg.limit_frames(480000, 44100, 16000) == 1323000


def test_run_long_shifts_every_time(monkeypatch):
    """run_long with the detector and the session replaced: batches in file order, results joined to their segments, every time moved by the segment's start."""
    seg, eng = sub("segmenter"), sub("engine")
    segs = np.array([[1600, 4800], [8000, 9600], [16000, 20000]], dtype=np.int64)
    monkeypatch.setattr(seg, "segment", lambda frames, rate, channels, params, fs, limit: (segs, {"audio_seconds": 2.0, "speech_seconds": 0.55}))
    calls = []

    def run_batch(prepared, part):
        calls.append(part.tolist())
        return [{"token_ids": np.array([int(s)]), "tokens": [{"id": 1, "start": 0.0, "end": 0.05}, {"id": 2, "start": 0.05, "end": 0.1}],
                 "token_times": [(0.0, 0.1)], "segments": [{"start": 0.0, "end": 0.1, "tokens": [3, 4], "words": [{"word": "a", "start": 0.0, "end": 0.02}]}],
                 "nbest": [{"score": -1.0, "tokens": [{"id": 1, "start": 0.01, "end": 0.02}]}]} for s, e in part]

    records, info = seg.run_long(np.zeros(32000, np.int16), None, None, 1, 16000, 480000, lambda f: f, run_batch, max_batch=2)
    assert calls == [segs[:2].tolist(), segs[2:].tolist()] and info["speech_seconds"] == 0.55
    for (s, e), r in zip(segs, records):
        t = s / 16000
        assert (r["start"], r["end"]) == (t, e / 16000) and r["token_ids"].tolist() == [s]
        assert [(k["start"], k["end"]) for k in r["tokens"]] == [(t + 0.0, t + 0.05), (t + 0.05, t + 0.1)]
        assert r["token_times"] == [(t + 0.0, t + 0.1)]
        assert (r["segments"][0]["start"], r["segments"][0]["end"], r["segments"][0]["tokens"]) == (t + 0.0, t + 0.1, [3, 4])
        assert r["segments"][0]["words"][0] == {"word": "a", "start": t + 0.0, "end": t + 0.02}
        assert r["nbest"][0]["tokens"][0]["start"] == t + 0.01 and r["nbest"][0]["score"] == -1.0
    monkeypatch.setattr(seg, "segment", lambda *a: (np.zeros((0, 2), np.int64), {"audio_seconds": 2.0, "speech_seconds": 0.0}))
    records, _ = seg.run_long(np.zeros(32000, np.int16), None, None, 1, 16000, 480000, lambda f: 1 / 0, lambda *a: 1 / 0, max_batch=2)
    assert records == []                                                 # no segment: neither the audio is prepared nor a batch run


def test_transcribe_long_with_a_fake_session(monkeypatch):
    """SenseVoiceTranscriber.transcribe_long over a fake native session: the segments go out as ragged batches in file order, at most max_batch a call, and every
    token's span comes back moved by its segment's start and clipped to the segment's length."""
    seg, sv = sub("segmenter"), sub("sensevoice")
    segs = np.array([[1600, 4800], [8000, 9600], [16000, 20000]], dtype=np.int64)
    monkeypatch.setattr(seg, "segment", lambda frames, rate, channels, params, fs, limit: (segs, {"audio_seconds": 2.0, "speech_seconds": 0.55}))

    class Cfg:
        max_audio_len = 480000

        @staticmethod
        def row_span_seconds(first, last):
            return 0.06 * int(first), 0.06 * (int(last) + 1)

    class Native:
        cfg, input_format, calls = Cfg(), (16000, 1), []

        def run_packed_timed(self, packed, offs, lang):
            self.calls.append((packed.copy(), offs.copy(), lang.copy()))
            B = lang.size
            tok = np.tile(np.array([[7, 8]], np.int32), (B, 1)) + np.arange(B, dtype=np.int32)[:, None] * 10
            first, last = np.tile(np.array([[0, 2]], np.int32), (B, 1)), np.tile(np.array([[1, 4]], np.int32), (B, 1))
            return tok, np.full(B, 2, np.int32), first, last, np.full((B, 2), -0.5, np.float32)

    tr = object.__new__(sv.SenseVoiceTranscriber)
    tr.session = type("Shim", (), {"_native": Native()})()
    tr.sample_rate, tr.audio_pcm_scale, tr.input_audio_dtype, tr.selector_index, tr.tokenizer, tr.language = 16000, 1, "F32", 3, None, "en"
    pcm = (np.arange(32000) % 1000).astype(np.int16)
    res = tr.transcribe_long(pcm, timestamps=True, max_batch=2)
    calls = tr.session._native.calls
    assert [c[1].tolist() for c in calls] == [[0, 3200, 4800], [0, 4000]] and all(np.all(c[2] == 3) for c in calls)
    assert np.array_equal(calls[0][0], np.concatenate([pcm[1600:4800], pcm[8000:9600]]).astype(np.float32)) and np.array_equal(calls[1][0], pcm[16000:20000].astype(np.float32))
    assert res["token_ids"].tolist() == [7, 8, 17, 18, 7, 8] and res["text"] is None and (res["speech_seconds"], res["audio_seconds"]) == (0.55, 2.0)
    for (s, e), r in zip(segs, res["segments"]):
        t, dur = s / 16000, (e - s) / 16000
        assert (r["start"], r["end"]) == (t, e / 16000)
        assert [(k["start"], k["end"]) for k in r["tokens"]] == [(t + min(0.0, dur), t + min(0.12, dur)), (t + min(0.12, dur), t + min(0.3, dur))]
        assert [k["id"] for k in r["tokens"]] == r["token_ids"].tolist() and all(k["logprob"] == -0.5 for k in r["tokens"])
    assert res["segments"][1]["tokens"][1]["end"] == 9600 / 16000           # the second segment is 0.1 s long: its last span is clipped to it
