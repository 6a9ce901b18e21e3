"""The front-end and conv-stem references (tests/front_end_ref.py) checked on the CPU: they reproduce the oracles' numbers and the reference's goldens,
the inputs are what they claim to be, and every planted mistake fails the comparison the GPU test makes.

The GPU test (test_front_end_ref_gpu.py) lets a kernel differ from the exact statement by 3 x E_round per stage, clip and statistic (worst row's RMS, max
abs; equality where E_round is zero). Here the mutated exact statement takes the kernel's place: it must FAIL that comparison, under the rounding noise of
BOTH precisions, on every clip of the edge batch it applies to. The smallest failing ratio stat / E_round per mutation is printed (run with -s).
This is a condition on the inputs, computed from the references alone. Measured (the larger statistic's ratio on the clip that shows the mistake least):

    family            mutation            f32 noise        bf16 noise    applies to
    whisper 128 / 80  reflect_left        1.2e5 / 1.5e5    96 / 58       clips whose first 201 samples are not silent (not ramp_clip, not the zero clip)
    whisper 128 / 80  reflect_right       3.8e5 / 3.8e5    194 / 289     clips whose last frame reads the right pad (length % 160 < 40) and that are not silent
    whisper 128 / 80  batch maximum       inf              inf           the all-zero clip (E_round = 0: equality); ramp_clip holds the batch maximum
    whisper 128 / 80  conv2_past_end      1.2e5 / 1.2e5    28 / 18       odd frame counts (an even clip never reads the row behind it: asserted)
    whisper 128 / 80  conv1_lead_frame0   1.3e5 / 1.4e5    29 / 24       every clip
    qwen              reflect_left        4.7e4            61            as Whisper, on `feat`
    qwen              reflect_right       1.7e5            198           as Whisper, on `feat`
    qwen              slot_tail           1.5e5            551           frames % 100 != 0 (`feat`)
    qwen              pad_slot            1.5e5            551           chunks % chunks_per_window != 0 (`feat`)
    kaldi             no_left_clamp       6.3e6 / 9.4e6    (f32 only)    every clip (`enc_in`, affine mode 0 / 1)
    kaldi             no_right_clamp      2.6e7 / 1.2e7    (f32 only)    clips whose last LFR row reaches behind the last frame (`enc_in`, affine mode 0 / 1)

Two things the inputs had to learn. The right reflect pad is read by the LAST frame only, through the last 40 - length % 160 window weights (all below 0.1),
and not at all from 40 samples beyond the last whole hop on: under full-level noise an index that is off by one there stays inside bf16 rounding (ratio
1.3 .. 2.5). The noise clips therefore fade out and end in a three-sample click (front_end_ref.noise_clip). And QwenAsrOracle's own f32 log-mel (rfft, its own
window formula) is 1e-3 away from its float64 evaluation on ramp_clip's bins 79 dB under a frame's peak, so ramp_clip is anchored through WhisperOracle, which
states the same raw log-mel the way the reference and the sessions do (a matrix product with the hann_window table).
"""
import dataclasses

import numpy as np
import pytest
import torch

import front_end_ref as R
from conftest import sub
from helpers import load_golden, sensevoice_setup

PRECISIONS = ("f32", "bf16")


@pytest.fixture(scope="module", params=[128, 80])
def whisper(request):
    cfg = dataclasses.replace(sub("config").whisper_tiny_test(), n_mels=request.param)
    return cfg, sub("checkpoints").synth_whisper_checkpoint(cfg, 0), R.edge_batch("whisper")


@pytest.fixture(scope="module")
def qwen():
    cfg = sub("config").qwen_asr_tiny()
    return cfg, sub("checkpoints").synth_qwen_asr_checkpoint(cfg, 0), R.edge_batch("qwen", cfg)


def _fails(name, got, exact, rounded, worst):
    """The mutated statement `got` must fail within(); keeps the smallest of the failing ratios."""
    ok, ratio = R.within(got, exact, rounded)
    assert not ok, (name, ratio)
    worst[name] = min(worst.get(name, float("inf")), max(ratio))


# ---- anchors ------------------------------------------------------------------------------------------------------------------------------------
def test_whisper_statements_reproduce_the_oracle_and_the_goldens():
    from oracle import natural_audio as na
    from oracle.whisper_oracle import WhisperOracle
    from test_oracle_whisper import F32_TOL, whisper_setup
    g = load_golden("whisper_tiny_natural")
    cfg, ck, sup, beg = whisper_setup(str(g["cfg_name"]), int(g["ckpt_seed"]))
    orc, orc64 = WhisperOracle(cfg, ck, sup, beg), WhisperOracle(cfg, ck, sup, beg, dtype=torch.float64)
    for n, pcm in na.load_clips().items():
        _, fin = R.whisper_log_mel(cfg, na.unit_input(pcm), rounded="f32")
        assert fin.shape == g[n + "_mel"].shape and np.abs(fin - g[n + "_mel"]).max() < F32_TOL, n
    for a in R.edge_batch("whisper")[::3]:
        with torch.inference_mode():
            taps, taps64 = {}, {}
            orc.encode(a, taps)
            orc64.encode(a, taps64)
        _, fin = R.whisper_log_mel(cfg, a, rounded="f32")
        assert np.abs(fin - taps["mel"].t().numpy()).max() < F32_TOL
        assert np.abs(R.whisper_stem(cfg, ck, taps["mel"].t().numpy(), rounded="f32") - taps["stem"].numpy()).max() < F32_TOL
        _, fin64 = R.whisper_log_mel(cfg, a)
        assert np.abs(fin64 - taps64["mel"].t().numpy()).max() < 1e-9                       # the exact statement IS the oracle in float64
        assert np.abs(R.whisper_stem(cfg, ck, fin64) - taps64["stem"].numpy()).max() < 1e-9


def test_qwen_statements_reproduce_the_oracle(qwen):
    from oracle.qwen_asr_oracle import QwenAsrOracle
    from test_oracle_qwen_asr import F32_TOL
    cfg, ck, audios = qwen
    orc = QwenAsrOracle(cfg, ck, [1], [2], [3])
    # (ramp_clip is anchored through WhisperOracle, which states the same raw log-mel as a matrix product with the hann_window table, as the reference and
    # the sessions do: this oracle's f32 rfft with its own window formula is itself 1e-3 away from float64 on bins 79 dB under a frame's peak)
    for a in audios[:10:2] + [audios[11]]:
        with torch.inference_mode():
            taps = {}
            want = orc.log_mel(torch.as_tensor(a)).t().numpy()
            orc.encode(a, taps)
        _, fin = R.qwen_log_mel(cfg, a, rounded="f32")
        assert fin.shape == want.shape and np.abs(fin - want).max() < F32_TOL
        plan, slots, wins = R.qwen_slots(cfg, [a.size])
        live = np.arange(slots) < plan[0][2]
        stem = R.qwen_stem(cfg, ck, R.qwen_feat(cfg, [want]), live, rounded="f32")
        assert stem.shape == tuple(taps["stem"].shape) and np.abs(stem - taps["stem"].numpy()).max() < F32_TOL
        assert R.qwen_tokens(cfg, plan[0][1]) == sub("engine").QwenAsrSession.audio_tokens(type("S", (), {"cfg": cfg})(), a.size)


def test_kaldi_statements_reproduce_the_oracles():
    from oracle.paraformer_oracle import ParaformerOracle
    from oracle.sensevoice_oracle import SenseVoiceOracle
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    g = load_golden("sensevoice_tiny_natural")
    from oracle import natural_audio as na
    orc64 = SenseVoiceOracle(cfg, ck, dtype=torch.float64)
    for n, pcm in list(na.load_clips().items())[:3]:
        mel = R.kaldi_fbank(cfg, ck, na.kaldi_input(pcm), rounded="f32")
        assert np.abs(mel - g[n + "_mel"]).max() < 1e-4 * max(1.0, np.abs(g[n + "_mel"]).max()), n
        lang = int(g[n + "_lang"])
        x = R.lfr_cmvn(cfg, ck, mel, 0, lang, rounded="f32")
        assert np.abs(x - g[n + "_enc_in"]).max() < 1e-4 * max(1.0, np.abs(g[n + "_enc_in"]).max()), n
        with torch.inference_mode():
            assert np.array_equal(R.lfr_cmvn(cfg, ck, mel, 0, lang), orc64.lfr_cmvn(torch.as_tensor(mel), lang).numpy())
    pcfg = sub("config").paraformer_tiny()
    pck = sub("checkpoints").synth_paraformer_checkpoint(pcfg, 0)
    po = ParaformerOracle(pcfg, pck)
    a = R.edge_batch("kaldi")[9]
    with torch.inference_mode():
        mel = po.fbank(torch.as_tensor(a))
        idx = (torch.arange(0, (mel.shape[0] + 5) // 6 * 6, 6).unsqueeze(1) + torch.arange(7) - 3).clamp(0, mel.shape[0] - 1)
        want = mel[idx].reshape(-1, pcfg.feat_dim) * po.cmvn_vars + po.in_bias[:idx.shape[0]]
    assert np.abs(R.kaldi_fbank(pcfg, pck, a, rounded="f32") - mel.numpy()).max() < 1e-4
    assert np.abs(R.lfr_cmvn(pcfg, pck, mel.numpy(), 1, rounded="f32") - want.numpy()).max() < 1e-5


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------
def test_edge_batches_have_the_named_frame_counts(qwen):
    cfg = qwen[0]
    assert cfg.chunks_per_window == 4 and cfg.chunk == 100
    w = [a.size // 160 for a in R.edge_batch("whisper")]
    assert w == [2, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, R.RAMP_FRAMES, R.ZERO_FRAMES]
    assert R.edge_batch("whisper")[0].size == 400                                           # the smallest legal clip
    assert sorted({(f + 1) // 2 for f in w} & {16, 17}) == [16, 17]                           # both sides of the 16-row group edge of round_up(T + 1, 16)
    assert len({a.size % 160 for a in R.edge_batch("whisper")}) > 6 and sum(a.size % 2 for a in R.edge_batch("whisper")) >= 4
    assert [a.size // 160 for a in qwen[2]] == [2, 99, 100, 101, 199, 200, 201, 399, 400, 401, R.RAMP_FRAMES, R.ZERO_FRAMES]
    assert [(a.size - 400) // 160 + 1 for a in R.edge_batch("kaldi")] == list(R.KALDI_FRAMES) + [R.RAMP_FRAMES, R.ZERO_FRAMES]
    assert all(np.array_equal(a, np.round(a)) and np.abs(a).max() <= 32768 for a in R.edge_batch("kaldi"))
    assert all(a.size // 160 >= 300 for a in R.long_batch("whisper"))


def test_ramp_clip_spans_the_clamp_and_peaks_in_the_last_partial_block(whisper):
    cfg = whisper[0]
    a = R.ramp_clip(160 * R.RAMP_FRAMES + 77)
    raw, fin = R.whisper_log_mel(cfg, a)
    frames = raw.shape[0]
    assert frames % 64 != 0 and int(raw.max(axis=1).argmax()) >= frames // 64 * 64              # the maximum sits in the last, partial 64-frame block
    floor = raw.max() - 8.0
    assert (raw[:frames // 4 - 3] == -10.0).all()                                               # digital silence: every bin at the 1e-10 clamp
    tone = raw[frames // 4 + 4:frames * 11 // 20 - 4]
    assert (tone > floor).any(axis=1).all() and (tone < floor).any(axis=1).all()                # max - 8 clamps some bins of a frame and leaves others
    assert raw.max() - tone.max() > 5.0 and raw.max() - raw.min() > 8.0                         # the tone's peak 50 dB down, the clip spans more than 80 dB
    q, back = R.to_int16(a)
    assert q.dtype == np.int16 and np.abs(back - a).max() <= 2.0 ** -16


# ---- the planted mistakes ---------------------------------------------------------------------------------------------------------------------------
def test_whisper_mutations_fail_the_comparison(whisper):
    cfg, ck, audios = whisper
    gmax = R.batch_max(cfg, audios)
    worst = {}
    for p in PRECISIONS:
        for i, a in enumerate(audios):
            raw, fin = R.whisper_log_mel(cfg, a)
            forms = R.rounded_forms(lambda **k: R.whisper_log_mel(cfg, a, **k)[1], p)
            rnd = forms[0]
            silent = not a.any()
            if not silent:
                left = R.whisper_log_mel(cfg, a, mut="reflect_left")[1]
                if a[:201].any():
                    _fails(f"{p} reflect_left", left, fin, forms, worst)
                else:
                    assert np.array_equal(left, fin)                                                  # ramp_clip: leading digital silence
                right = R.whisper_log_mel(cfg, a, mut="reflect_right")[1]
                if R.right_pad_read(a.size):
                    _fails(f"{p} reflect_right", right, fin, forms, worst)
                else:
                    assert np.array_equal(right, fin)
            else:
                assert (fin == -1.5).all() and all((f == -1.5).all() for f in forms)
                _fails(f"{p} batch_max", R.whisper_log_mel(cfg, a, clip_max=gmax)[1], fin, forms, worst)
            assert float(raw.max()) <= gmax and (float(raw.max()) == gmax) == (i == len(audios) - 2)      # ramp_clip holds the batch maximum
            rows = rnd if p == "bf16" else fin                                                        # the session's own tapped rows
            exact = R.whisper_stem(cfg, ck, rows)
            srnd = R.rounded_forms(lambda **k: R.whisper_stem(cfg, ck, rows, **k), p) if p == "f32" else R.whisper_stem(cfg, ck, rows, rounded=p)
            _fails(f"{p} conv1_lead_frame0", R.whisper_stem(cfg, ck, rows, mut="conv1_lead_frame0"), exact, srnd, worst)
            past = R.whisper_stem(cfg, ck, rows, mut="conv2_past_end")
            if rows.shape[0] % 2:
                _fails(f"{p} conv2_past_end", past, exact, srnd, worst)
            else:
                assert np.array_equal(past, exact)                                                    # an even clip never reads the row behind it
    for k, v in sorted(worst.items()):
        print(f"whisper n_mels={cfg.n_mels:3d} {k:24s} smallest failing ratio {v:.3g}")
    assert len(worst) == 10


def test_qwen_mutations_fail_the_comparison(qwen):
    cfg, ck, audios = qwen
    worst = {}
    for p in PRECISIONS:
        for a in audios:
            raw, fin = R.qwen_log_mel(cfg, a)
            feat = R.qwen_feat(cfg, [fin])
            frnd = [R.qwen_feat(cfg, [f]) for f in R.rounded_forms(lambda **k: R.qwen_log_mel(cfg, a, **k)[1], p)]
            fr = a.size // 160
            floor = [max(-10.0, float(raw.max()) - 8.0) * 0.25 + 1.0]
            if a[:201].any():
                _fails(f"{p} reflect_left", R.qwen_feat(cfg, [R.qwen_log_mel(cfg, a, mut="reflect_left")[1]]), feat, frnd, worst)
                if R.right_pad_read(a.size):
                    _fails(f"{p} reflect_right", R.qwen_feat(cfg, [R.qwen_log_mel(cfg, a, mut="reflect_right")[1]]), feat, frnd, worst)
            if fr % cfg.chunk:
                _fails(f"{p} slot_tail", R.qwen_feat(cfg, [fin], "slot_tail", floor), feat, frnd, worst)
            if ((fr + cfg.chunk - 1) // cfg.chunk) % cfg.chunks_per_window:
                _fails(f"{p} pad_slot", R.qwen_feat(cfg, [fin], "pad_slot", floor), feat, frnd, worst)
    for k, v in sorted(worst.items()):
        print(f"qwen {k:24s} smallest failing ratio {v:.3g}")
    assert len(worst) == 8


def test_lfr_mutations_fail_the_comparison():
    cfg, ck = sensevoice_setup("sensevoice_tiny")
    pcfg = sub("config").paraformer_tiny()
    pck = sub("checkpoints").synth_paraformer_checkpoint(pcfg, 0)
    worst = {}
    for mode, (c, k) in enumerate(((cfg, ck), (pcfg, pck))):
        for a in R.edge_batch("kaldi"):
            mel = R.kaldi_fbank(c, k, a, rounded="f32")                                               # stands for the session's own `mel`
            exact, rnd = R.lfr_cmvn(c, k, mel, mode), R.lfr_cmvn(c, k, mel, mode, rounded="f32")
            n = mel.shape[0]
            _fails(f"mode {mode} no_left_clamp", R.lfr_cmvn(c, k, mel, mode, mut="no_left_clamp"), exact, rnd, worst)
            right = R.lfr_cmvn(c, k, mel, mode, mut="no_right_clamp")
            if ((n + 5) // 6 - 1) * 6 + 3 > n - 1:
                _fails(f"mode {mode} no_right_clamp", right, exact, rnd, worst)
            else:
                assert np.array_equal(right, exact)
    for k, v in sorted(worst.items()):
        print(f"kaldi {k:24s} smallest failing ratio {v:.3g}")
    assert len(worst) == 4


def test_rounding_budgets_are_neither_vacuous_nor_loose(whisper):
    """E_round of the bf16 stages is bf16 noise (1e-3 .. 1e-2 on rows of unit scale), of the f32 stages f32 noise: a kernel error of 1e-3 in the front end,
    which the encoder budgets of the end-to-end tests swallow, is 3 .. 4 orders of magnitude beyond 3 x E_round of an f32 stage."""
    cfg, ck, audios = whisper
    a = audios[5]
    _, fin = R.whisper_log_mel(cfg, a)
    e32 = R.stat(fin - R.whisper_log_mel(cfg, a, rounded="f32")[1])
    e16 = R.stat(fin - R.whisper_log_mel(cfg, a, rounded="bf16")[1])
    assert 1e-8 < e32[1] < 1e-5 and 1e-3 < e16[1] < 8e-3, (e32, e16)
    s32 = R.stat(R.whisper_stem(cfg, ck, fin) - R.whisper_stem(cfg, ck, fin, rounded="f32"))
    s16 = R.stat(R.whisper_stem(cfg, ck, fin) - R.whisper_stem(cfg, ck, fin, rounded="bf16"))
    assert 1e-8 < s32[1] < 1e-5 and 1e-3 < s16[1] < 5e-2, (s32, s16)
