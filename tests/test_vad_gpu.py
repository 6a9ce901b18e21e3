"""GPU: the energy VAD (asr_op_vad; csrc/vad.hip) against its statement, tests/vad_ref.py.

1. energies: random ragged batches of every sample type, 1 / 2 / 3 channels, at 16000, 44100 (H = 441) and 11025 (H = 110) Hz, lengths on every edge of an
   analysis frame and of a stage-1 tile, loud utterances (+- full scale) before the first offset and between the checked ones, so a neighbour's sample in an
   edge frame shows: |e - e64| <= (H + 2 C + 4) 2^-24 sum_i (sum_c |x_ic| / C)^2 per frame (H additions in any order, one rounding per square, the channel sum
   and scale), and sum F by the ceil rule;
2. stage 2 is the statement's integer half applied to the device's own e[], bit for bit: levels, floor / peak / thr, segments, seg_utt, counts;
3. planted bursts: the segments are the planted spans +- pad exactly, and the statement's on float64 energies (test_vad_ref_cpu.py asserts the same equality);
4. seg_cap below the count; 5. host memory == device memory; 6. refusals.

TILE_F is the number of analysis frames a stage-1 workgroup of vad.hip owns. Stage 2 keeps the whole mask of an utterance in LDS and works in one pass: there is
no CHUNK, so the long case is 70 000 frames."""
import ctypes as C

import numpy as np
import pytest

import vad_cases as K
import vad_ref as V
from conftest import sub

pytestmark = pytest.mark.gpu

TILE_F = 256
CHUNK = None
LONG_F = 70000
EPS = 2.0 ** -24
DTYPES = {"f32": np.float32, "int16": np.int16, "f16": np.float16}


def _pc(**kw):
    """asr_vad_params from a vad_ref.Params."""
    p = V.Params(**kw)
    c = sub("_lib").VadParamsC()
    c.p_floor = p.p_floor
    for k in ("margin", "peak_drop", "abs_level", "min_speech", "min_pause", "pad", "max_frames"):
        setattr(c, k, getattr(p, k))
    return c, V.Params(**{**p.__dict__, "p_floor": float(np.float32(p.p_floor))})


def _samples(rng, n, channels, dtype, loud):
    if dtype == np.int16:
        return (rng.choice([-32768, 32767], size=(n, channels)) if loud else rng.integers(-300, 300, size=(n, channels))).astype(np.int16)
    if loud:
        return (rng.choice([-1.0, 1.0], size=(n, channels)) * (60000.0 if dtype == np.float16 else 32768.0)).astype(dtype)
    return (rng.standard_normal((n, channels)) * 0.01).astype(dtype)


def _edge_batch(rng, rate, channels, dtype):
    """Quiet clips of every edge length, a loud 7-frame utterance between each pair, loud frames before the first offset and after the last
    -> (packed, offsets, clips, quiet flags)."""
    H = V.hop(rate)
    lens = [0, 1, H - 1, H, H + 1, (TILE_F - 1) * H + 1, TILE_F * H, TILE_F * H + 1]
    clips, quiet = [], []
    for n in lens:
        clips += [_samples(rng, n, channels, dtype, False), _samples(rng, 7, channels, dtype, True)]
        quiet += [True, False]
    lead, trail = _samples(rng, 5, channels, dtype, True), _samples(rng, 9, channels, dtype, True)
    offs = 5 + np.concatenate([[0], np.cumsum([c.shape[0] for c in clips])]).astype(np.int64)
    packed = np.concatenate([lead.reshape(-1)] + [c.reshape(-1) for c in clips] + [trail.reshape(-1)])
    return packed, offs, clips, quiet


def _check_stage2(eng, res, offs, H, p):
    """Every integer output against the statement's stage 2 on the device's own energies -> the segments per utterance."""
    seg, utt, counts, e, q, stats = res
    F = -((-np.diff(offs)) // H)
    f_off = np.concatenate([[0], np.cumsum(F)])
    assert e.size == q.size == f_off[-1]
    want_seg, want_utt, per = [], [], []
    for b in range(offs.size - 1):
        n = int(offs[b + 1] - offs[b])
        qb, st, sb = V.stage2(e[f_off[b]:f_off[b + 1]], n, H, p)
        assert np.array_equal(q[f_off[b]:f_off[b + 1]], qb), (b, "levels")
        assert tuple(stats[b]) == st, (b, tuple(stats[b]), st)
        assert counts[b] == sb.shape[0], (b, counts[b], sb.shape[0])
        want_seg.append(sb + offs[b])
        want_utt += [b] * sb.shape[0]
        per.append(sb)
    want = np.concatenate(want_seg) if want_seg else np.zeros((0, 2), np.int64)
    assert np.array_equal(seg, want), (seg[:8], want[:8])
    assert np.array_equal(utt, want_utt)
    return per


# ------------------------------------------------------------------------------------------------ 1. energies (and 2. on the same batches)
@pytest.mark.parametrize("rate", [16000, 44100, 11025])
@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_energies_against_float64(dtype, channels, rate):
    eng = sub("engine")
    H = V.hop(rate)
    assert H == {16000: 160, 44100: 441, 11025: 110}[rate]
    rng = np.random.default_rng(1000 * list(DTYPES).index(dtype) + 100 * channels + rate % 97)
    packed, offs, clips, quiet = _edge_batch(rng, rate, channels, DTYPES[dtype])
    pc, p = _pc(abs_level=0, min_speech=2, min_pause=3, pad=1, max_frames=40)
    res = eng.op_vad(packed, offs, rate=rate, channels=channels, params=pc, details=True)
    e = res[3]
    F = [V.n_frames(c.shape[0], H) for c in clips]
    assert e.size == sum(F)
    worst, at = 0.0, 0
    for c, f in zip(clips, F):
        x = c.astype(np.float64)
        e64, _ = V.energies(x.sum(axis=1) / channels, H)
        mag, _ = V.energies(np.abs(x).sum(axis=1) / channels, H)
        err = np.abs(e[at:at + f].astype(np.float64) - e64)
        bound = (H + 2 * channels + 4) * EPS * mag
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()) if f else 0.0)
        assert np.all(err <= bound), (c.shape, np.flatnonzero(err > bound)[:4])
        at += f
    print(f"{dtype} C={channels} {rate} Hz: worst |e - e64| / bound = {worst:.3f}")
    _check_stage2(eng, res, offs, H, p)


# ------------------------------------------------------------------------------------------------ 2. stage 2, bit for bit
def _batch_of(clips):
    offs = np.concatenate([[0], np.cumsum([c.size for c in clips])]).astype(np.int64)
    return np.concatenate(clips), offs


def test_stage2_edges_bit_for_bit():
    """Parameter sets and level patterns that make every named edge occur, one utterance each and all in one batch."""
    eng = sub("engine")
    rate, H = 800, 8
    rng = np.random.default_rng(5)
    lvl = lambda amp: int(V.level(np.float32(H * amp * amp)))
    S, P = True, False
    patterns = {
        "burst of min_speech - 1 dropped, of min_speech kept": [(P, 20), (S, 3), (P, 20), (S, 4), (P, 20)],
        "pauses of 7 and 8": [(P, 9), (S, 5), (P, 7), (S, 5), (P, 8), (S, 5), (P, 9)],
        "pad clipped at both ends": [(P, 1), (S, 6), (P, 30), (S, 6), (P, 2)],
        "a pause of 6 = 2 pad": [(P, 10), (S, 5), (P, 6), (S, 5), (P, 10)],
        "constant level": [(S, 15)],
        "a run that needs three cuts": [(P, 5), (S, 95), (P, 5)],
        "a run across many mask words": [(P, 70), (S, 300), (P, 3), (S, 200), (P, 64), (S, 64), (P, 64)],
        "short bursts only": [(P, 7), (S, 2), (P, 7), (S, 3), (P, 7)],
        "empty": [],
    }
    clips = [K.clip_from_amplitudes(K.pattern_amplitudes(r, rng), H) for r in patterns.values()]
    packed, offs = _batch_of(clips)
    # thr = abs_level, between the pause and the speech amplitudes. min_pause 8: the pause of 7 is bridged, the one of 8 kept (2 runs), the pause of 6 bridged;
    # min_pause 6: both kept (3 runs), and the pause of 6 is kept by (b) and closed by the two pads of (c)
    for min_pause, n_pauses in ((8, 2), (6, 3)):
        pc, p = _pc(margin=0, peak_drop=2000, abs_level=lvl(100), min_speech=4, min_pause=min_pause, pad=3, max_frames=30)
        per = dict(zip(patterns, _check_stage2(eng, eng.op_vad(packed, offs, rate=rate, params=pc, details=True), offs, H, p)))
        assert per["burst of min_speech - 1 dropped, of min_speech kept"].tolist() == [[40 * H, 50 * H]]
        assert per["pauses of 7 and 8"].shape[0] == n_pauses
        assert per["pad clipped at both ends"].tolist() == [[0, 10 * H], [34 * H, 45 * H]]
        assert per["a pause of 6 = 2 pad"].tolist() == [[7 * H, 29 * H]]
        assert per["constant level"].tolist() == [[0, 15 * H]]
        assert per["a run that needs three cuts"].shape[0] >= 4
        assert per["short bursts only"].shape[0] == 0 and per["empty"].shape[0] == 0
        for sb in per.values():
            assert np.all(sb[:, 1] - sb[:, 0] <= p.max_frames * H)
        for c, sb in zip(clips, per.values()):                               # each alone: a batch of 1
            one = eng.op_vad(c, [0, c.size], rate=rate, params=pc, details=True)
            assert np.array_equal(one[0], sb) and one[2][0] == sb.shape[0]
    # all zeros: abs_level wins over the statistics, no segment
    z = eng.op_vad(np.zeros(50 * H, np.int16), [0, 50 * H], rate=rate, params=eng.vad_default_params(rate, 32768.0), details=True)
    assert z[0].shape == (0, 2) and z[2][0] == 0 and z[5][0, 2] == eng.vad_default_params(rate, 32768.0).abs_level
    # constant level with the default statistics: peak - peak_drop wins, one segment
    pcc, ppc = _pc(abs_level=0, min_speech=1, min_pause=1, pad=0, max_frames=100)
    c = K.clip_from_amplitudes(np.full(30, 500), H)
    r = eng.op_vad(c, [0, c.size], rate=rate, params=pcc, details=True)
    assert r[0].tolist() == [[0, 30 * H]] and r[5][0, 2] == r[5][0, 1] - 16
    _check_stage2(eng, r, np.array([0, c.size]), H, ppc)


@pytest.mark.parametrize("max_frames", [3000, 37, 2])
def test_stage2_long_utterance_bit_for_bit(max_frames):
    """One utterance of 70 000 analysis frames (1094 mask words: more than one per stage-2 thread): noise with planted bursts of every length up to several mask
    words, default statistics."""
    eng = sub("engine")
    rate, H = 800, 8
    rng = np.random.default_rng(11)
    amp = np.abs(rng.standard_normal(LONG_F) * 6.0) + 1.0
    at = 100
    while at < LONG_F - 800:
        n = int(rng.choice([1, 3, 9, 10, 11, 40, 63, 64, 65, 130, 700]))
        amp[at:at + n] = rng.choice([1500, 2500, 4000], size=n)
        at += n + int(rng.choice([5, 25, 49, 50, 51, 64, 128, 400]))
    clip = K.clip_from_amplitudes(np.round(amp), H)
    pc, p = _pc(abs_level=int(V.level(np.float32(H * 30.0 ** 2))), max_frames=max_frames)
    per = _check_stage2(eng, eng.op_vad(clip, [0, clip.size], rate=rate, params=pc, details=True), np.array([0, clip.size]), H, p)
    assert per[0].shape[0] > 50 and np.all(per[0][:, 1] - per[0][:, 0] <= max_frames * H)


# ------------------------------------------------------------------------------------------------ 3. planted audio
def test_planted_bursts_exactly():
    eng = sub("engine")
    x, _ = K.planted_audio()
    p = V.default_params(K.RATE, 32768.0)
    seg, utt, counts, e, q, stats = eng.op_vad(x, [0, x.size], rate=K.RATE, details=True)
    assert np.abs(q.astype(np.int64) - stats[0, 2]).min() >= 16          # no frame's level is near thr: rounding of e cannot move the mask
    assert np.array_equal(seg, K.planted_expected(p.pad, x.size))
    assert np.array_equal(seg, V.vad(x, K.RATE, p)[3])
    assert np.array_equal(utt, [0] * 3) and counts.tolist() == [3]


# ------------------------------------------------------------------------------------------------ 4. seg_cap
def test_seg_cap_smaller_than_count():
    eng, _lib = sub("engine"), sub("_lib")
    rate, H = 800, 8
    rng = np.random.default_rng(3)
    runs = [(False, 8)] + [(True, 6), (False, 12)] * 9
    clips = [K.clip_from_amplitudes(K.pattern_amplitudes(runs, rng), H) for _ in range(3)]
    packed, offs = _batch_of(clips)
    pc, _ = _pc(margin=0, peak_drop=2000, abs_level=int(V.level(np.float32(H * 100.0 ** 2))), min_speech=2, min_pause=3, pad=1, max_frames=50)
    full, full_utt, counts = eng.op_vad(packed, offs, rate=rate, params=pc)
    assert counts.tolist() == [9, 9, 9]
    for cap in (0, 1, 9, 13, 26):
        seg = np.full((cap + 8, 2), -7777, dtype=np.int64)
        utt = np.full(cap + 8, -7777, dtype=np.int32)
        cnt = np.full(3, -1, dtype=np.int32)
        lp, ip = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
        _lib.check(_lib.load().asr_op_vad(packed.ctypes.data_as(C.c_void_p), 0, offs.ctypes.data_as(lp), 3, eng.AUDIO_I16, rate, 1, C.byref(pc),
                                          seg.ctypes.data_as(lp), cap, utt.ctypes.data_as(ip), cnt.ctypes.data_as(ip), None, None, None))
        assert cnt.tolist() == [9, 9, 9]
        assert np.array_equal(seg[:cap], full[:cap]) and np.array_equal(utt[:cap], full_utt[:cap])
        assert np.all(seg[cap:] == -7777) and np.all(utt[cap:] == -7777)
        s2, u2, c2 = eng.op_vad(packed, offs, rate=rate, params=pc, seg_cap=cap)
        assert np.array_equal(s2, full[:cap]) and c2.tolist() == [9, 9, 9]


# ------------------------------------------------------------------------------------------------ 5. host == device memory
def test_device_pointer_equals_host_memory():
    eng, _lib = sub("engine"), sub("_lib")
    rng = np.random.default_rng(9)
    rate, channels = 44100, 2
    packed, offs, _, _ = _edge_batch(rng, rate, channels, np.int16)
    pc, _ = _pc(abs_level=0, min_speech=2, min_pause=3, pad=1, max_frames=40)
    host = eng.op_vad(packed, offs, rate=rate, channels=channels, params=pc, details=True)
    lib, ptr = _lib.load(), C.c_void_p(None)
    _lib.check(lib.asr_mem_alloc(0, packed.nbytes, C.byref(ptr)))
    try:
        _lib.check(lib.asr_mem_copy(0, ptr, packed.ctypes.data_as(C.c_void_p), packed.nbytes, 0))
        dev = eng.op_vad(packed, offs, rate=rate, channels=channels, params=pc, details=True, audio_device_ptr=ptr.value)
    finally:
        _lib.check(lib.asr_mem_free(0, ptr))
    for h, d in zip(host, dev):
        assert np.array_equal(h, d)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_op_usable():
    eng, _lib = sub("engine"), sub("_lib")
    x, _ = K.planted_audio()
    good = eng.op_vad(x, [0, x.size], rate=K.RATE)

    def refused(**kw):
        args = dict(audio=x, offsets=[0, x.size], rate=K.RATE, channels=1, params=None)
        args.update(kw)
        with pytest.raises(_lib.AsrError) as ei:
            eng.op_vad(**args)
        assert ei.value.code == 1, ei.value
        again = eng.op_vad(x, [0, x.size], rate=K.RATE)
        assert all(np.array_equal(a, b) for a, b in zip(good, again))

    big = np.zeros(V.MAX_F + 1, dtype=np.int16)                          # rate 100: H = 1, one analysis frame per sample
    refused(audio=big, offsets=[0, big.size], rate=100)
    refused(rate=99)
    refused(audio=np.zeros(x.size * 9, np.int16), channels=9)
    refused(channels=0)
    refused(params=_pc(max_frames=1)[0])
    refused(params=_pc(p_floor=0.0)[0])
    refused(params=_pc(p_floor=1.5)[0])
    ok = eng.op_vad(big[:-1], [0, V.MAX_F], rate=100)                    # exactly 2^20 analysis frames is taken (silence: no segment)
    assert ok[0].shape == (0, 2) and ok[2].tolist() == [0]
