"""Every family's first stretch, from samples to encoder input, per stage against the float64 statements of tests/front_end_ref.py.

Sessions on the tiny configurations, eager, taps on. Per stage, clip and statistic (worst row's RMS, max abs):

    stat(tap - exact) <= 3 x E_round,     E_round = stat(exact - rounded), from the references alone (for an f32 contraction the largest over the
                                          float32 summation orders of front_end_ref.orders); equality where E_round is zero

A stage behind the first takes the session's OWN tapped rows of the stage before as the reference's input (Whisper `stem` <- `mel_gapped`, Qwen `feat` <-
`mel`, `stem` <- `feat`, SenseVoice / Paraformer `enc_in` <- `mel`), so an error is charged to the stage that made it. Everything a layout keeps zero
(Whisper: the leading zero row and the gap rows of `mel_gapped`, the pad rows of the 16-row groups of `stem`; Qwen: frames behind a clip and padding slots
of `feat`; SenseVoice / Paraformer: pad rows of `enc_in`) must be exactly zero, and the prompt rows of SenseVoice equal to their f32 table. Every session
runs the edge batch (front_end_ref.edge_batch: the lengths at which the kernels change path, ramp_clip next to an all-zero clip), then two long clips of
other data, then the edge batch again: the buffers then hold the long batch's values wherever the short one does not write.

What is NOT compared: the rows of Qwen's `stem` tap that belong to window padding slots or to the 16-row alignment of a window. The reference states
them as zero (QwenAsrOracle.encode), the session leaves there what the convolutions make of zero features; they are masked keys that nothing reads.
`feat` pins their input to zero. The SANM sessions have no tap that shows the bf16 operand copy of `enc_in` (x0lo), so it is not compared here.

Measured stat / E_round on an MI355X, worst clip of each length class over the edge batch and its repetition behind the long batch (RMS ratio, then max-abs
ratio). Whisper classes: F 2..3 | F 31..33 | F 63..129 | ramp_clip | all-zero clip | the long clips; Qwen: F 2 | F 99..201 | F 399..401 | ramp | zero | long;
SenseVoice / Paraformer: F 1..13 | F 63..129 | ramp | zero | long. No stage, precision or length class stands out and nothing is near the margin:

    whisper f32 n_mels=128       mel_gapped 1.07 1.18   1.00 1.18   1.04 1.01   0.63 0.77   0.00 0.00   0.89 0.64
    whisper f32 n_mels=128       stem       1.13 1.07   1.05 1.14   1.14 1.50   1.08 1.13   1.20 1.90   0.99 1.04
    whisper f32 n_mels=128 int16 mel_gapped 1.16 1.43   1.28 1.77   1.76 1.37   0.66 0.60   0.00 0.00
    whisper f32 n_mels=128 int16 stem       0.97 1.36   1.04 0.99   1.10 1.23   1.13 1.23   1.20 1.90
    whisper f32 n_mels=80        mel_gapped 1.11 0.92   1.27 0.85   1.01 1.00   0.56 0.67   0.00 0.00   0.81 0.84
    whisper f32 n_mels=80        stem       1.04 1.06   1.15 1.05   1.15 1.27   0.97 0.81   0.94 1.28   1.13 0.91
    whisper f32 n_mels=80 int16  mel_gapped 1.27 1.43   1.26 1.00   1.25 1.13   0.61 0.61   0.00 0.00
    whisper f32 n_mels=80 int16  stem       1.10 1.11   1.13 1.44   1.13 1.35   0.87 0.78   0.94 1.28
    qwen f32                     mel        0.20 0.19   1.45 1.45   1.11 1.11   0.56 0.60   0.00 0.00   1.49 1.48
    qwen f32                     feat       1.00 1.00   1.00 1.00   1.00 1.00   1.00 1.00   0.00 0.00   1.00 1.00
    qwen f32                     stem       1.16 1.31   1.18 1.24   1.12 1.35   0.91 0.50   0.96 0.59   1.17 1.42
    qwen bf16                    mel        0.20 0.19   1.45 1.45   1.11 1.11   0.56 0.60   0.00 0.00   1.49 1.48
    qwen bf16                    feat       1.00 1.00   1.00 1.00   1.00 1.00   1.00 1.00   0.00 0.00   1.00 1.00
    qwen bf16                    stem       1.00 1.00   1.00 1.00   1.00 1.00   1.00 1.00   1.00 1.00   1.00 1.00
    sensevoice f32 split=1       mel        1.78 2.10   1.67 1.33   0.59 0.60   1.00 1.00   1.53 1.33
    sensevoice f32 split=1       enc_in     0.89 1.00   0.93 1.00   0.99 0.83   0.99 0.83   0.86 0.75
    paraformer f32 split=1       mel        2.03 2.06   1.48 0.81   0.62 0.56   1.00 1.00   0.88 0.68
    paraformer f32 split=1       enc_in     0.29 0.97   0.29 0.53   0.75 0.67   0.75 0.67   0.30 0.53
    sensevoice bf16 split=1      mel        1.61 1.18   1.36 0.77   0.83 1.04   1.00 1.00   0.87 0.35
    sensevoice bf16 split=1      enc_in     0.87 1.00   0.90 1.00   0.99 0.83   0.99 0.83   0.90 1.00
    paraformer bf16 split=1      mel        1.49 1.23   1.30 0.54   0.87 1.10   1.00 1.00   0.48 0.31
    paraformer bf16 split=1      enc_in     0.29 0.77   0.30 0.59   0.75 0.67   0.75 0.67   0.30 0.53
    whisper bf16, n_mels 128 and 80, float and int16 input: mel_gapped and stem 1.00 1.00 in every class (0.00 on the all-zero clip's mel_gapped): the
    session's error IS the bf16 rounding of the documented points. bf16 SenseVoice / Paraformer with ASR_FBANK_SPLIT=0 repeat the f32 rows digit for digit
    (the same exact-f32 fbank kernel runs), as does the `mel` of bf16 Qwen (Whisper and Qwen sessions never run the split kernel).

Findings of the first runs, each fixed in the product (the summary of the change names them): Whisper sessions rejected n_mels = 80; a bin at the log floor
was the device logarithm's approximation of log10(1e-10) / ln(eps) instead of the value itself (all-zero clip: inf, E_round = 0); the Qwen position table
was numpy's, 4.6e-7 from the reference's torch table (F = 2 clip, stem max ratio 3.25). And two of the references: Paraformer's fbank table is not
SenseVoice's (ratios 3 .. 10 on `mel` when held to it), and E_round of an f32 contraction must not hang on one summation order (front_end_ref.orders).
"""
import dataclasses

import numpy as np
import pytest

import front_end_ref as R
from conftest import sub

pytestmark = pytest.mark.gpu

BF16, F32 = 0, 1
NAME = {BF16: "bf16", F32: "f32"}


def _f64(tap_u16_or_f32):
    a = np.asarray(tap_u16_or_f32)
    if a.dtype == np.uint16:
        a = (a.astype(np.uint32) << 16).view(np.float32)
    return a.astype(np.float64)


def _tap(sess, name, lowp=False):
    return _f64(sess.tap(name, np.uint16 if lowp and sess.precision == BF16 else np.float32))


class Report:
    def __init__(self, title):
        self.title, self.rows = title, []

    def add(self, stage, clip, got, exact, rounded):
        ok, ratio = R.within(got, exact, rounded)
        e = R.e_round(exact, rounded)
        print(f"{self.title:34s} {stage:10s} {clip:>16s}  rms ratio {ratio[0]:8.3f}  max ratio {ratio[1]:8.3f}   (E_round {e[0]:.3g} {e[1]:.3g})")
        self.rows.append((stage, clip, ok, ratio))

    def check(self, n):
        assert len(self.rows) == n, (len(self.rows), n)
        bad = [(s, c, r) for s, c, ok, r in self.rows if not ok]
        assert not bad, (self.title, bad)


# ---- Whisper -------------------------------------------------------------------------------------------------------------------------------------
def _whisper_check(rep, sess, cfg, ck, floats, tag):
    """One encoded batch (its samples as the floats the session computed from) against the references."""
    prec = NAME[sess.precision]
    plan, n_gapped, n_stem = R.whisper_rows([a.size for a in floats])
    mel, stem = _tap(sess, "mel_gapped", lowp=True), _tap(sess, "stem")
    assert mel.shape == (n_gapped, cfg.n_mels) and stem.shape == (n_stem, cfg.d_model) and np.isfinite(mel).all() and np.isfinite(stem).all()
    live_m, live_s = np.zeros(n_gapped, bool), np.zeros(n_stem, bool)
    for i, ((g0, Fr, r0, T), a) in enumerate(zip(plan, floats)):
        live_m[g0:g0 + Fr] = True
        live_s[r0:r0 + T] = True
        name = f"{tag}{i}:F{Fr}"
        got = mel[g0:g0 + Fr]
        rep.add("mel_gapped", name, got, R.whisper_log_mel(cfg, a)[1], R.rounded_forms(lambda **k: R.whisper_log_mel(cfg, a, **k)[1], prec))
        rep.add("stem", name, stem[r0:r0 + T], R.whisper_stem(cfg, ck, got), R.rounded_forms(lambda **k: R.whisper_stem(cfg, ck, got, **k), "f32")
                if prec == "f32" else R.whisper_stem(cfg, ck, got, rounded=prec))
    assert not mel[~live_m].any(), (tag, "a leading zero row or a gap row of mel_gapped is not zero", np.flatnonzero(mel[~live_m].any(axis=1))[:8])
    assert not stem[~live_s].any(), (tag, "a pad row of stem is not zero", np.flatnonzero(stem[~live_s].any(axis=1))[:8])
    return len(floats) * 2


@pytest.mark.parametrize("n_mels", [128, 80])
@pytest.mark.parametrize("prec", [F32, BF16])
def test_whisper_log_mel_and_stem_against_the_float64_reference(prec, n_mels):
    cfg = dataclasses.replace(sub("config").whisper_tiny_test(), n_mels=n_mels)
    ck = sub("checkpoints").synth_whisper_checkpoint(cfg, 0)
    sess = sub("engine").WhisperSession.from_checkpoint(cfg, ck, precision=prec)
    sess.taps(True)
    rep = Report(f"whisper {NAME[prec]} n_mels={n_mels}")
    edge, long_ = R.edge_batch("whisper"), R.long_batch("whisper")
    n = 0
    npos = sess.encode(edge)
    assert npos.tolist() == [(a.size // 160 + 1) // 2 for a in edge]
    n += _whisper_check(rep, sess, cfg, ck, edge, "edge")
    sess.encode(long_)
    n += _whisper_check(rep, sess, cfg, ck, long_, "long")
    sess.encode(edge)                                                   # the buffers hold the long batch's rows wherever this one does not write
    n += _whisper_check(rep, sess, cfg, ck, edge, "again")
    pcm = [R.to_int16(a) for a in edge]                                 # int16 samples, x 2^-15 in the kernel; packed, so clips start at odd sample offsets
    assert sum(np.cumsum([q.size for q, _ in pcm])[:-1] % 2) >= 3
    sess.audio_dtype = np.int16
    sess.encode([q for q, _ in pcm])
    n += _whisper_check(rep, sess, cfg, ck, [f for _, f in pcm], "int16")
    rep.check(n)


def test_whisper_rejects_a_clip_shorter_than_nfft():
    cfg = sub("config").whisper_tiny_test()
    sess = sub("engine").WhisperSession.from_checkpoint(cfg, sub("checkpoints").synth_whisper_checkpoint(cfg, 0), precision=F32)
    with pytest.raises(Exception, match="n_fft"):
        sess.encode([np.zeros(399, np.float32)])


# ---- Qwen3-ASR ---------------------------------------------------------------------------------------------------------------------------------------
def _finish_qwen(raw, rounded):
    import torch
    with torch.inference_mode():
        x = R._finish(torch.as_tensor(raw).to(R._dtype(rounded)), "qwen")
        return (R.bf16(x) if rounded == "bf16" else x).to(torch.float64).numpy()


def _qwen_check(rep, sess, cfg, ck, audios, ids_len, n_prompt, tag):
    prec = NAME[sess.precision]
    plan, slots, wins = R.qwen_slots(cfg, [a.size for a in audios])
    cpw, chunk = cfg.chunks_per_window, cfg.chunk
    rpw = R.round_up(cpw * 13, 16)
    mel, feat, stem = _tap(sess, "mel"), _tap(sess, "feat", lowp=True), _tap(sess, "stem")
    assert mel.shape == (sum(p[1] for p in plan), cfg.n_mels) and feat.shape == (slots * chunk, cfg.n_mels) and stem.shape == (wins * rpw, cfg.enc_d)
    assert np.isfinite(mel).all() and np.isfinite(feat).all() and np.isfinite(stem).all()
    feat = feat.reshape(slots, chunk, cfg.n_mels)
    live = np.zeros(slots, bool)
    for s0, Fr, nc, nw, w0 in plan:
        live[s0:s0 + nc] = True
    exact_stem = R.qwen_stem(cfg, ck, feat, live)
    rnd_stem = R.rounded_forms(lambda **k: R.qwen_stem(cfg, ck, feat, live, **k), "f32") if prec == "f32" else [R.qwen_stem(cfg, ck, feat, live, rounded=prec)]
    stem = stem.reshape(wins, rpw, cfg.enc_d)[:, :cpw * 13]
    f0 = 0
    for i, ((s0, Fr, nc, nw, w0), a) in enumerate(zip(plan, audios)):
        name = f"{tag}{i}:F{Fr}"
        assert int(ids_len[i]) - n_prompt == R.qwen_tokens(cfg, Fr), (name, ids_len[i])              # token count of the partial chunk
        raw = mel[f0:f0 + Fr]
        f0 += Fr
        rep.add("mel", name, raw, R.qwen_log_mel(cfg, a)[0], R.rounded_forms(lambda **k: R.qwen_log_mel(cfg, a, **k)[0], prec))
        own = feat[s0:s0 + nw * cpw].reshape(-1, cfg.n_mels)
        assert not own[Fr:].any(), (name, "frames behind the clip or a padding slot of feat are not zero")
        rep.add("feat", name, own[:Fr], _finish_qwen(raw, None), _finish_qwen(raw, prec))
        rows = lambda t: t[w0:w0 + nw].reshape(nw * cpw, 13, cfg.enc_d)[:nc].reshape(nc * 13, cfg.enc_d)     # the rows of the chunks that exist
        rep.add("stem", name, rows(stem), rows(exact_stem), [rows(r) for r in rnd_stem])
    return 3 * len(audios)


@pytest.mark.parametrize("prec", [F32, BF16])
def test_qwen_log_mel_feat_and_stem_against_the_float64_reference(prec):
    cfg = sub("config").qwen_asr_tiny()
    ck = sub("checkpoints").synth_qwen_asr_checkpoint(cfg, 0)
    sess = sub("engine").QwenAsrSession.from_checkpoint(cfg, ck, precision=prec)
    sess.taps(True)
    rep = Report(f"qwen {NAME[prec]}")
    edge, long_ = R.edge_batch("qwen", cfg), R.long_batch("qwen")
    pre, post = [[5, 6]], [[7]]
    n = 0
    for tag, batch in (("edge", edge), ("long", long_), ("again", edge)):
        _, _, ids_len = sess.prefill(batch, pre, post)
        n += _qwen_check(rep, sess, cfg, ck, batch, ids_len, 3, tag)
    rep.check(n)


# ---- SenseVoice, Paraformer ------------------------------------------------------------------------------------------------------------------------------
def _kaldi_check(rep, sess, cfg, ck, audios, mode, langs, tag, split):
    import torch
    rows = sess.utterance_rows([a.size for a in audios])
    mel, enc_in = _tap(sess, "mel"), _tap(sess, "enc_in")
    assert enc_in.shape[1] == cfg.feat_dim and np.isfinite(mel).all() and np.isfinite(enc_in).all()
    live = np.zeros(enc_in.shape[0], bool)
    f0 = 0
    for i, ((r0, T), a) in enumerate(zip(rows, audios)):
        fr = (a.size - cfg.win_length) // cfg.hop_length + 1
        name = f"{tag}{i}:F{fr}"
        own = mel[f0:f0 + fr]
        f0 += fr
        live[r0:r0 + T] = True
        rep.add("mel", name, own, R.kaldi_fbank(cfg, ck, a), R.rounded_forms(lambda **k: R.kaldi_fbank(cfg, ck, a, **k), NAME[sess.precision], split))
        lang = langs[i] if langs else 0
        exact = R.lfr_cmvn(cfg, ck, own, mode, lang)
        assert exact.shape[0] == T, (name, exact.shape, T)
        rep.add("enc_in", name, enc_in[r0:r0 + T], exact, R.lfr_cmvn(cfg, ck, own, mode, lang, rounded="f32"))
        if mode == 0:                                                   # the prompt rows are copies of the f32 tables
            o = R._sv_oracle(cfg, R._hold(ck), torch.float32)
            want = torch.cat([o.language_embed[lang:lang + 1], o.system_embed], 0).numpy()
            assert np.array_equal(enc_in[r0:r0 + want.shape[0]].astype(np.float32), want), name
    assert f0 == mel.shape[0]
    assert not enc_in[~live].any(), (tag, "a pad row of enc_in is not zero")
    return 2 * len(audios)


@pytest.mark.parametrize("family", ["sensevoice", "paraformer"])
@pytest.mark.parametrize("prec,split", [(F32, "1"), (BF16, "1"), (BF16, "0")])
def test_kaldi_fbank_and_lfr_against_the_float64_reference(monkeypatch, family, prec, split):
    monkeypatch.setenv("ASR_FBANK_SPLIT", split)
    cfgm, ckm, eng = sub("config"), sub("checkpoints"), sub("engine")
    if family == "sensevoice":
        cfg = cfgm.sensevoice_tiny()
        ck = ckm.synth_sensevoice_checkpoint(cfg, 0)
        sess = eng.SenseVoiceSession.from_checkpoint(cfg, ck, precision=prec)
    else:
        cfg = cfgm.paraformer_tiny()
        ck = ckm.synth_paraformer_checkpoint(cfg, 0)
        sess = eng.ParaformerSession.from_checkpoint(cfg, ck, precision=prec)
    sess.taps(True)
    rep = Report(f"{family} {NAME[prec]} split={split}")
    edge, long_ = R.edge_batch("kaldi"), R.long_batch("kaldi")
    n = 0
    for tag, batch in (("edge", edge), ("long", long_), ("again", edge)):
        langs = [i % len(cfg.language_prompt_token_ids) for i in range(len(batch))] if family == "sensevoice" else None
        sess.run(batch, langs) if langs else sess.run(batch)
        n += _kaldi_check(rep, sess, cfg, ck, batch, 0 if family == "sensevoice" else 1, langs, tag, split == "1")
    rep.check(n)
