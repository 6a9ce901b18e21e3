"""GPU: precision mode ASR_PRECISION_FP8W (include/asr_mi355x.h) -- Whisper decoder projections and cross-K/V as OCP e4m3 bytes.

What pins it:
  * the row quantiser against torch's float8_e4m3fn conversion (format, round-to-nearest-even, power-of-two scales);
  * the byte-weight decode GEMM against the SAME kernel over the dequantised bf16 weights (bit for bit: power-of-two scales commute with
    every rounding) and against a float64 product;
  * a whole session in FP8 mode against the same session with ASR_FP8_FAKE=1 (identical quantisation, bf16 kernels throughout), bit for
    bit on the logits of prefill + decode steps, i.e. the byte paths of the decode GEMM and of the cross-attention add no error of their own;
  * the quantisation error itself against the f32 oracle, with the budget written down next to the bf16 mode's error on the same input.

Precision mode ASR_PRECISION_FP8MM adds the encoder's feed-forward pair on the FP8 matrix pipe (csrc/gemm_fp8.hip):
  * the byte x byte GEMM against a float64 product of the DECODED bytes (the only error left is f32 accumulation order), its e4m3 output
    bytes within half an e4m3 ulp of the exact GELU;
  * a whole FP8MM session against the f32 oracle next to FP8W on the same input (activation quantisation costs more than weight
    quantisation: the budget says how much)."""
import os

import numpy as np
import pytest
import torch

from conftest import sub
from helpers import golden_cases, load_golden
from lowbit_ref import pow2_scale as _pow2_scale
from oracle.whisper_oracle import WhisperOracle
from test_oracle_whisper import unit_audio, whisper_setup

pytestmark = pytest.mark.gpu

BF16, F32, FP8W, FP8MM = 0, 1, 2, 3


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


def test_row_quantiser_is_ocp_e4m3_with_power_of_two_scales():
    probe = sub("_probe")
    rng = np.random.default_rng(5)
    w = (rng.standard_normal((48, 512)) * np.exp(rng.uniform(-6, 3, (48, 1)))).astype(np.float32)
    w[3] = 0.0                                               # an all-zero row keeps scale 1
    w[5, :16] = [448.0, -448.0, 447.9, 0.0009765625, 1e-4, 464.0, 0.017, -0.0195, 240.0, 208.0, 0.06, 1.0, -1.0, 3.5, 0.4375, 30.0]
    q, sc, dq = probe.quantize_fp8(w)
    wb = probe._bf16_to_f32(probe._bf16_bits(w))             # the kernel sees bf16-rounded weights
    want_s = _pow2_scale(np.abs(wb).max(axis=1))
    assert np.array_equal(sc, want_s)
    assert ((np.abs(wb).max(axis=1) / sc <= 448.0) & ((np.abs(wb).max(axis=1) / sc > 224.0) | (np.abs(wb).max(axis=1) == 0))).all()
    t8 = torch.from_numpy(wb / sc[:, None]).to(torch.float8_e4m3fn)
    assert np.array_equal(q, t8.view(torch.uint8).numpy())   # same bytes as torch: OCP e4m3fn, round to nearest even
    assert np.array_equal(dq, t8.to(torch.float32).numpy() * sc[:, None])     # and the dequantisation is exact in bf16


@pytest.mark.parametrize("M,N,K,fold", [(32, 768, 256, True), (7, 256, 1024, False), (64, 1280, 1280, True), (32, 1280, 5120, False),
                                         (64, 5120, 1280, True), (48, 5120, 1280, False), (32, 5120, 1280, True), (16, 3840, 1280, True)])
def test_byte_weight_decode_gemm_equals_the_bf16_kernel_over_dequantised_weights(M, N, K, fold):
    probe = sub("_probe")
    rng = np.random.default_rng(M + N + K)
    a = rng.standard_normal((M, K)).astype(np.float32) * 1.5 + (0.3 if fold else 0.0)
    w = (rng.standard_normal((N, K)) * 0.04 * np.exp(rng.uniform(-2, 2, (N, 1)))).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    q, sc, dq = probe.quantize_fp8(w)
    byte_path = probe.decode_gemm(a, w=dq, w8=q, scale=sc, bias=bias, fold=fold)
    bf16_path = probe.decode_gemm(a, w=dq, bias=bias, fold=fold)
    assert np.array_equal(byte_path, bf16_path)              # bit for bit (incl. the split-K hand-over of the K = 5120 case and the 4 x 2 / 2 x 2 tile instances of N = 5120)
    ab = probe._bf16_to_f32(probe._bf16_bits(a)).astype(np.float64)
    if fold:
        mu, var = ab.mean(1, keepdims=True), ab.var(1, keepdims=True)
        ab = (ab - mu) / np.sqrt(var + 1e-5)
    want = ab @ dq.astype(np.float64).T + bias
    assert np.abs(byte_path - want).max() < 2e-3 * np.abs(want).max()


def _run(sess, audios, prompts, forced):
    """prefill + teacher-forced decode steps -> logits (B, 1 + steps, V)"""
    sess.encode(audios)
    _, logits = sess.prefill(prompts)
    out = [logits]
    for s in range(forced.shape[1]):
        _, logits = sess.decode(np.ascontiguousarray(forced[:, s:s + 1]), want_logits=True)
        out.append(logits)
    return np.stack(out, 1)


def test_fp8_session_equals_fake_quantised_bf16_session_and_stays_within_budget_of_the_oracle():
    name = "whisper_d256_test"
    cfg, ck, sup, beg, s8 = _session(name, FP8W)
    _, _, _, _, sfake = _session(name, FP8W, {"ASR_FP8_FAKE": "1"})
    _, _, _, _, sbf = _session(name, BF16)
    audios = [unit_audio(71, 64000), unit_audio(72, 25600), unit_audio(73, 128000)]
    prompt = [cfg.sot_id, cfg.first_language_id, cfg.transcribe_id, cfg.no_timestamps_id]
    prompts = np.array([prompt] * 3, np.int32)
    orc = WhisperOracle(cfg, ck, sup, beg)
    ref = orc.greedy(audios, [prompt] * 3, 5)
    forced = np.stack([np.asarray(ref["token_ids"][b][:4], np.int32) for b in range(3)])
    want = np.stack([np.stack(ref["logits"][b][:5]) for b in range(3)])       # (3, 5, V): the oracle is teacher-forced on its own picks
    l8, lf, lb = _run(s8, audios, prompts, forced), _run(sfake, audios, prompts, forced), _run(sbf, audios, prompts, forced)
    V = cfg.vocab
    assert np.array_equal(l8[..., :V], lf[..., :V])          # the byte kernels add no error of their own
    scale = float(np.abs(want).max())
    e_bf, e_8 = float(np.abs(lb[..., :V] - want).max()), float(np.abs(l8[..., :V] - want).max())
    print(f"whisper_d256 logits |max| {scale:.2f}: bf16 error {e_bf:.4f}, fp8w error {e_8:.4f}")
    assert e_bf < 1e-3 * scale                                # measured 2e-4
    assert e_8 < 6e-3 * scale                                 # measured 1.5e-3 (e4m3 keeps 4 significant bits: ~3 % rms per weight / cache entry, averaged over K >= 256 terms)
    assert e_8 > e_bf                                         # (sanity: the mode really quantises)
    # FP8 mode rejects what it cannot serve, loudly
    with pytest.raises(RuntimeError):
        _session("whisper_mid_test", FP8W)                    # d_model 384 is not a multiple of 256
    cfgs, cks = sub("config").sensevoice_tiny(), None
    with pytest.raises(Exception):
        sub("engine").SenseVoiceSession.from_checkpoint(cfgs, sub("checkpoints").synth_sensevoice_checkpoint(cfgs, 0), precision=FP8W)


def test_large_v3_fp8_30s_vs_golden_budget():
    """Whisper-large-v3 at full dimensions, the 30 s clip of the reference-minted golden in a batch of 4: FP8 mode's logit error next to
    bf16 mode's, teacher-forced on the golden's token ids."""
    g = load_golden("whisper_large_v3")
    c0 = [c for _, c in golden_cases(g)][0]
    cfg, ck, sup, beg, s8 = _session("whisper_large_v3", FP8W)
    audios = [unit_audio(c0["audio_seed"], c0["n_samples"])] + [unit_audio(9100 + i, 480000) for i in range(3)]
    prompts = np.tile(c0["prompt"][None], (4, 1))
    n_new = int(g["n_new"])
    forced = np.tile(c0["token_ids"][None, :n_new - 1], (4, 1)).astype(np.int32)
    l8 = _run(s8, audios, prompts, forced)
    del s8
    _, _, _, _, sbf = _session("whisper_large_v3", BF16)
    lb = _run(sbf, audios, prompts, forced)
    scale = max(float(np.abs(c0["top1"]).max()), 50.0)
    e_bf = float(np.abs(lb[0][:, ::53][:, :c0["logits"].shape[1]] - c0["logits"]).max())
    e_8 = float(np.abs(l8[0][:, ::53][:, :c0["logits"].shape[1]] - c0["logits"]).max())
    print(f"whisper_large_v3 logits scale {scale:.1f}: bf16 error {e_bf:.3f}, fp8w error {e_8:.3f}")
    assert e_bf < 2e-3 * scale                                # measured 6e-4
    assert e_8 < 1.2e-2 * scale                               # measured 4e-3


def _nearest_e4m3(x, tab):
    finite = np.where(np.isnan(tab), np.inf, tab)
    order = np.argsort(finite)
    vals = finite[order]
    keep = np.isfinite(vals)
    vals, order = vals[keep], order[keep]
    pos = np.clip(np.searchsorted(vals, x), 1, vals.size - 1)
    return np.where(np.abs(x - vals[pos - 1]) <= np.abs(x - vals[pos]), order[pos - 1], order[pos]).astype(np.uint8)


@pytest.mark.parametrize("M,N,K", [(256, 256, 256), (300, 512, 512), (1000, 1280, 1280), (777, 1024, 256), (1500, 256, 1024), (2048, 1280, 5120)])
def test_fp8_matrix_pipe_gemm_against_float64_over_the_decoded_bytes(M, N, K):
    from math import erf
    probe = sub("_probe")
    tab = probe.e4m3_table()
    rng = np.random.default_rng(M * 7 + N * 3 + K)
    a8, w8 = _nearest_e4m3(rng.standard_normal((M, K)), tab), _nearest_e4m3(rng.standard_normal((N, K)) * 32.0, tab)
    sc = 2.0 ** rng.integers(-12, -8, N).astype(np.float64)
    bias = rng.standard_normal(N)
    add = rng.standard_normal((M, N)).astype(np.float32)
    ref = (tab[a8] @ tab[w8].T) * sc[None, :] + bias[None, :]
    mag = (np.abs(tab[a8]) @ np.abs(tab[w8]).T) * sc[None, :] + 1.0
    got, _ = probe.gemm_fp8(a8, w8, sc, bias, add=add)                       # f32 out + residual (the fc2 form)
    assert (np.abs(got - (ref + add)) / mag).max() < 2e-5                     # products are exact; f32 accumulation order only (measured 1e-6)
    out8, _ = probe.gemm_fp8(a8, w8, sc, bias, act=2)                        # erf-GELU -> e4m3 bytes (the fc1 form)
    sub_rows = slice(0, min(M, 128))
    gelu = np.clip(0.5 * ref[sub_rows] * (1.0 + np.vectorize(erf)(ref[sub_rows] / np.sqrt(2.0))), -448, 448)
    rel = np.abs(tab[out8[sub_rows]] - gelu) / np.maximum(np.abs(gelu), 2.0 ** -6)
    assert rel.max() < 0.07                                                  # half an e4m3 ulp = 1/16 of the value (+ the fast erf's 1e-6)


def test_fp8mm_session_stays_within_budget_of_the_oracle_and_rejects_what_it_cannot_serve():
    name = "whisper_d256_test"
    cfg, ck, sup, beg, smm = _session(name, FP8MM)
    _, _, _, _, s8 = _session(name, FP8W)
    audios = [unit_audio(81, 64000), unit_audio(82, 25600), unit_audio(83, 128000)]
    prompt = [cfg.sot_id, cfg.first_language_id, cfg.transcribe_id, cfg.no_timestamps_id]
    prompts = np.array([prompt] * 3, np.int32)
    orc = WhisperOracle(cfg, ck, sup, beg)
    ref = orc.greedy(audios, [prompt] * 3, 5)
    forced = np.stack([np.asarray(ref["token_ids"][b][:4], np.int32) for b in range(3)])
    want = np.stack([np.stack(ref["logits"][b][:5]) for b in range(3)])
    lmm, l8 = _run(smm, audios, prompts, forced), _run(s8, audios, prompts, forced)
    V = cfg.vocab
    scale = float(np.abs(want).max())
    e_mm, e_8 = float(np.abs(lmm[..., :V] - want).max()), float(np.abs(l8[..., :V] - want).max())
    print(f"whisper_d256 logits |max| {scale:.2f}: fp8w error {e_8:.4f}, fp8mm error {e_mm:.4f}")
    assert not np.array_equal(lmm[..., :V], l8[..., :V])     # (sanity: the encoder FFN really ran on bytes)
    assert e_mm < 3e-2 * scale                                # activations at 4 significant bits in 2 of the encoder's 6 GEMMs per layer
    assert np.array_equal(_run(smm, audios, prompts, forced), lmm)            # deterministic
    with pytest.raises(RuntimeError):
        _session("whisper_mid_test", FP8MM)                   # d_model 384 is not a multiple of 256


def test_fp8mm_saturating_gelu_operand_is_counted_and_an_activation_shift_cures_it():
    """The GELU operand of fc2 is e4m3 at a STATIC scale (2^shift, default 1): on a checkpoint whose fc1 outputs leave +-448 the bytes clamp. The clamp is
    counted (asr_whisper_fp8_stats), the Python session warns, and asr_whisper_set_fp8_act_shift moves the operand back into range. Checkpoint: the test
    model with encoder layer 0's fc1 scaled by 256 and its fc2 by 1 / 256 (GELU is positively homogeneous away from zero, so the network barely changes)."""
    name = "whisper_d256_test"
    cfg, ck, sup, beg = whisper_setup(name)
    ck = dict(ck)
    p = "model.encoder.layers.0."
    ck[p + "fc1.weight"] = ck[p + "fc1.weight"] * np.float32(256.0); ck[p + "fc1.bias"] = ck[p + "fc1.bias"] * np.float32(256.0)
    ck[p + "fc2.weight"] = ck[p + "fc2.weight"] * np.float32(1.0 / 256.0)
    smm = sub("engine").WhisperSession.from_checkpoint(cfg, ck, precision=FP8MM, suppress_tokens=sup, begin_suppress_tokens=beg)
    audios = [unit_audio(81, 64000), unit_audio(82, 25600)]
    prompt = [cfg.sot_id, cfg.first_language_id, cfg.transcribe_id, cfg.no_timestamps_id]
    prompts = np.array([prompt] * 2, np.int32)
    orc = WhisperOracle(cfg, ck, sup, beg)
    ref = orc.greedy(audios, [prompt] * 2, 3)
    forced = np.stack([np.asarray(ref["token_ids"][b][:2], np.int32) for b in range(2)])
    want = np.stack([np.stack(ref["logits"][b][:3]) for b in range(2)])
    V, scale = cfg.vocab, float(np.abs(want).max())
    assert smm.fp8_stats() == (0, 0)
    with pytest.warns(RuntimeWarning, match="saturated"):
        l_sat = _run(smm, audios, prompts, forced)
    n_sat, _ = smm.fp8_stats()
    assert n_sat > 0
    smm.set_fp8_act_shift(4)                                   # |GELU| here stays below 448 * 16
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        l_ok = _run(smm, audios, prompts, forced)
    assert smm.fp8_stats() == (n_sat, 4)
    e_sat, e_ok = float(np.abs(l_sat[..., :V] - want).max()), float(np.abs(l_ok[..., :V] - want).max())
    print(f"fp8mm on a checkpoint with |GELU| > 448: {n_sat} clamped elements, logits error {e_sat:.4f} clamped vs {e_ok:.4f} with shift 4 (|logits| max {scale:.2f})")
    assert e_ok < 3e-2 * scale and e_ok < e_sat
    with pytest.raises(RuntimeError):
        smm.set_fp8_act_shift(17)


@pytest.mark.parametrize("prec,budget", [(BF16, 1e-3), (FP8W, 6e-3)])
def test_batch64_32_steps_every_disagreement_with_the_oracle_is_an_oracle_near_tie(prec, budget):
    """64 utterances x 32 decoder steps, teacher-forced along RANDOM token histories (left to itself the random-weight decoder settles on
    one token, and its output projection is tied to the embedding, so a trained-margin head cannot be planted as in the SenseVoice /
    Paraformer twins of this test). With e = the measured logit error of this run against the f32 oracle, on all 2048 (utterance, step)
    pairs: the pick equals the oracle's wherever the oracle's margin exceeds 2 e, and wherever it differs the oracle rates the pick within
    2 e of its own. No loose thresholds, no agreement quota; the budget on e itself is the one of the smaller tests above."""
    cfg, ck, sup, beg, sess = _session("whisper_d256_test", prec)
    B, S = 64, 32
    rng = np.random.default_rng(64032)
    audios = [unit_audio(8800 + b, int(rng.integers(16000, 128001))) for b in range(B)]
    prompt = [cfg.sot_id, cfg.first_language_id, cfg.transcribe_id, cfg.no_timestamps_id]
    forced = rng.integers(0, cfg.eot_id, (B, S - 1)).astype(np.int32)
    orc = WhisperOracle(cfg, ck, sup, beg)
    want = np.zeros((B, S, cfg.vocab), np.float32)
    with torch.inference_mode():
        for b in range(B):
            ck_, cv_ = (z.unsqueeze(0) for z in orc.encode(audios[b]))
            logits, sk, sv = orc.decoder(torch.tensor([prompt], dtype=torch.long), 0, None, None, ck_, cv_)
            want[b, 0] = logits[0].float().numpy()
            for s in range(S - 1):
                logits, sk, sv = orc.decoder(torch.tensor([[int(forced[b, s])]]), len(prompt) + s, sk, sv, ck_, cv_)
                want[b, s + 1] = logits[0].float().numpy()
    sess.encode(audios)
    nxt, logits = sess.prefill(np.array([prompt] * B, np.int32))
    got, picks = [logits], [nxt.copy()]
    for s in range(S - 1):
        nxt, logits = sess.decode(np.ascontiguousarray(forced[:, s:s + 1]), want_logits=True)
        got.append(logits); picks.append(nxt.copy())
    got, picks = np.stack(got, 1)[..., :cfg.vocab], np.stack(picks, 1).reshape(B, S)
    head = want.copy()
    head[:, 0] += orc.begin_bias.float().numpy()                               # the first pick is taken under the begin-suppress mask (Export_Whisper.py:665-667)
    scale = float(np.abs(want).max())
    e = float(np.abs(got - want).max())
    assert e < budget * scale, (e, scale)
    part = np.partition(head, -2, axis=2)
    margin = part[..., -1] - part[..., -2]
    top = head.argmax(2)
    clear = margin > 2 * e
    assert np.array_equal(picks[clear], top[clear])
    gap = np.take_along_axis(head, top[..., None], 2)[..., 0] - np.take_along_axis(head, picks[..., None].astype(np.int64), 2)[..., 0]
    assert (gap <= 2 * e).all(), float(gap.max())
    print(f"whisper_d256 B = {B} x {S} steps, precision {prec}: logit error {e:.4f} of scale {scale:.1f}; {int((picks != top).sum())} of {B * S} picks "
          f"differ (all inside 2 e); {int(clear.sum())} pairs clear 2 e")


def _teacher_forced_oracle(orc, cfg, audios, prompt, forced, hidden=None):
    """f32 oracle, every utterance teacher-forced along its row of `forced`: logits (B, S, V); optionally the rows the tied projection saw."""
    B, S = forced.shape[0], forced.shape[1] + 1
    want = np.zeros((B, S, cfg.vocab), np.float32)
    with torch.inference_mode():
        for b in range(B):
            ck_, cv_ = (z.unsqueeze(0) for z in orc.encode(audios[b]))
            logits, sk, sv = orc.decoder(torch.tensor([prompt], dtype=torch.long), 0, None, None, ck_, cv_)
            want[b, 0] = logits[0].float().numpy()
            if hidden is not None:
                hidden[b, 0] = orc.last_hidden[0].double().numpy()
            for s in range(S - 1):
                logits, sk, sv = orc.decoder(torch.tensor([[int(forced[b, s])]]), len(prompt) + s, sk, sv, ck_, cv_)
                want[b, s + 1] = logits[0].float().numpy()
                if hidden is not None:
                    hidden[b, s + 1] = orc.last_hidden[0].double().numpy()
    return want


def _prototype_rows(X, alpha, target):
    """Nearest-prototype rows for a projection WITHOUT bias. The final LayerNorm gives every row x nearly the same length R, so
    x . (R m_c / |m_c| - mu) = R |x| cos(x, m_c) - x . mu ranks the classes c of a row x by the cosine to their mean direction m_c (the
    mu term is the same for every class). Rows start as classes of their own; a row whose f32 margin is below `target` has its class
    merged with its best competitor's (similar decoder states share a token, as they do under a trained head) until every margin clears
    `target`. Returns (rows (K, d), class of every row of X)."""
    N, d = X.shape
    U = X / np.linalg.norm(X, axis=1, keepdims=True)
    R, mu = float(np.linalg.norm(X, axis=1).mean()), X.mean(0)
    cls = np.arange(N)
    for _ in range(200):
        _, cls = np.unique(cls, return_inverse=True)
        K = int(cls.max()) + 1
        M = np.zeros((K, d))
        np.add.at(M, cls, U)
        M /= np.linalg.norm(M, axis=1, keepdims=True)
        P = alpha * (R * M - mu)
        lo = X @ P.T
        own = lo[np.arange(N), cls].copy()
        lo[np.arange(N), cls] = -np.inf
        rival = lo.argmax(1)
        weak = np.flatnonzero(own - lo[np.arange(N), rival] < target)
        if weak.size == 0:
            return P, cls
        for i in weak:                                                        # merge the weak row's class into its rival's
            a, b = cls[i], rival[i]
            cls[cls == max(a, b)] = min(a, b)
    raise AssertionError("prototype classes did not settle")


@pytest.mark.parametrize("prec", [BF16, FP8W])
def test_batch64_32_steps_token_for_token_on_a_prototype_head(prec):
    """bf16 parity of the Whisper decoder that does not lean on near-tie exclusions.

    The output projection is tied to the token embedding, but under teacher forcing only the embedding rows of the ids that are FED matter
    to the hidden states. So: feed ids from a small set F (distinct across the utterances of a step), and plant prototype rows in vocabulary
    ids OUTSIDE F (never fed, not suppressed) -- one class per (utterance, step) pair, pairs whose decoder states are too similar for any head
    to tell apart sharing a class (_prototype_rows: all 64 first picks follow the same prompt and do) -- built on x = the f32 oracle's final
    LayerNorm rows: a head with the margins a trained model has, on the hidden states this decoder really produces. Planting does not change
    the hidden states (asserted), the logits become peaky, and the demand is the user's: the SAME pick as the f32 oracle on all 64 x 32 = 2048
    (utterance, step) pairs, every one of them clearing twice the measured error of the logit differences that decide it."""
    cfg, ck, sup, beg = whisper_setup("whisper_d256_test")
    B, S, alpha, target = 64, 32, 2.0, 1.0
    rng = np.random.default_rng(64033)
    audios = [unit_audio(8900 + b, int(rng.integers(16000, 128001))) for b in range(B)]
    prompt = [cfg.sot_id, cfg.first_language_id, cfg.transcribe_id, cfg.no_timestamps_id]
    banned = set(sup) | set(beg)
    text = [i for i in range(cfg.eot_id) if i not in banned]
    fed, pool = np.asarray(text[:400]), np.asarray(text[400:])
    assert pool.size >= B * S
    forced = np.stack([fed[rng.permutation(fed.size)[:B]] for _ in range(S - 1)], 1).astype(np.int32)
    X = np.zeros((B, S, cfg.d_model))
    _teacher_forced_oracle(WhisperOracle(cfg, ck, sup, beg), cfg, audios, prompt, forced, hidden=X)
    P, cls = _prototype_rows(X.reshape(B * S, -1), alpha, target)
    K = P.shape[0]
    ids_of_class = pool[rng.permutation(pool.size)[:K]]
    planted = ids_of_class[cls].reshape(B, S)
    E = ck["model.decoder.embed_tokens.weight"].copy()
    E[ids_of_class] = P.astype(np.float32)
    ck2 = dict(ck)
    ck2["model.decoder.embed_tokens.weight"] = E
    orc2 = WhisperOracle(cfg, ck2, sup, beg)
    X2 = np.zeros_like(X)
    want = _teacher_forced_oracle(orc2, cfg, audios, prompt, forced, hidden=X2)
    assert np.array_equal(X, X2)                                               # planting did not touch what the decoder computes
    head = want.copy()
    head[:, 0] += orc2.begin_bias.float().numpy()
    top = head.argmax(2)
    assert np.array_equal(top, planted)                                        # the head does what it was built to do (in f32)
    part = np.partition(head, -2, axis=2)
    margin = part[..., -1] - part[..., -2]
    assert K > 0.9 * B * (S - 1), K                                            # nearly every later step is a class of its own

    sess = sub("engine").WhisperSession.from_checkpoint(cfg, ck2, precision=prec, suppress_tokens=sup, begin_suppress_tokens=beg)
    sess.encode(audios)
    nxt, logits = sess.prefill(np.array([prompt] * B, np.int32))
    got, picks = [logits], [nxt.copy()]
    for s in range(S - 1):
        nxt, logits = sess.decode(np.ascontiguousarray(forced[:, s:s + 1]), want_logits=True)
        got.append(logits); picks.append(nxt.copy())
    got, picks = np.stack(got, 1)[..., :cfg.vocab], np.stack(picks, 1).reshape(B, S)
    got[:, 0] += orc2.begin_bias.float().numpy()
    # the error of what decides a pick: logit differences to the oracle's winner
    d_orc = np.take_along_axis(head, top[..., None], 2) - head
    d_gpu = np.take_along_axis(got, top[..., None], 2) - got
    window, live = 4.0, np.isfinite(d_orc)                                     # (begin-suppressed classes sit at -inf in both: no difference to measure)
    with np.errstate(invalid="ignore"):                                        # (inf - inf at the suppressed classes, masked out by `live`)
        err = np.where(live, np.abs(d_gpu - d_orc), 0.0)
    assert np.array_equal(np.isfinite(d_gpu), live)
    e, e_all = float(err[live & (d_orc <= window)].max()), float(err.max())            # classes within `window` of the winner are the only ones that can compete
    print(f"whisper_d256 prototype head ({K} classes), B = {B} x {S} steps, precision {prec}: oracle margin min {margin.min():.3f} median {np.median(margin):.3f}; "
          f"error of logit differences {e:.4f} within {window} of the winner, {e_all:.4f} over all classes; {int((picks != top).sum())} of {B * S} picks differ")
    assert margin.min() > 2 * e, (float(margin.min()), e)                      # every pair clears twice the measured error ...
    assert e_all < window                                                      # ... no class from outside the window can get in ...
    assert np.array_equal(picks, top)                                          # ... and every pick is the oracle's, token for token
    # the production path (no logits download): prefill + decode without taps picks the same ids
    sess.encode(audios)
    nxt, _ = sess.prefill(np.array([prompt] * B, np.int32), want_logits=False)
    p2 = [nxt.copy()]
    for s in range(S - 1):
        nxt, _ = sess.decode(np.ascontiguousarray(forced[:, s:s + 1]), want_logits=False)
        p2.append(nxt.copy())
    assert np.array_equal(np.stack(p2, 1).reshape(B, S), top)


def test_large_v3_fp8mm_30s_vs_golden_budget():
    """FP8MM at full dimensions (d_model 1280, d_ffn 5120, 32 + 32 layers): the 30 s clip of the reference-minted golden in a ragged batch of 4 (30 s, 8 s, 30 s,
    2.5 s -- compacted encoder rows of different counts go through the FP8 GEMM's row tiles), prefill + decode steps teacher-forced on the golden's ids; the
    logit error next to FP8W's on the same batch, with the budget written down (activations at 4 significant bits in 64 of the encoder's 192 GEMMs)."""
    g = load_golden("whisper_large_v3")
    c0 = [c for _, c in golden_cases(g)][0]
    audios = [unit_audio(c0["audio_seed"], c0["n_samples"]), unit_audio(9201, 128000), unit_audio(9202, 480000), unit_audio(9203, 40000)]
    prompts = np.tile(c0["prompt"][None], (4, 1))
    n_new = int(g["n_new"])
    forced = np.tile(c0["token_ids"][None, :n_new - 1], (4, 1)).astype(np.int32)
    cfg, ck, sup, beg, smm = _session("whisper_large_v3", FP8MM)
    lmm = _run(smm, audios, prompts, forced)
    del smm
    _, _, _, _, s8 = _session("whisper_large_v3", FP8W)
    l8 = _run(s8, audios, prompts, forced)
    scale = max(float(np.abs(c0["top1"]).max()), 50.0)
    cols = c0["logits"].shape[1]
    e_mm = float(np.abs(lmm[0][:, ::53][:, :cols] - c0["logits"]).max())
    e_8 = float(np.abs(l8[0][:, ::53][:, :cols] - c0["logits"]).max())
    d_rest = float(np.abs(lmm[1:] - l8[1:]).max())
    print(f"whisper_large_v3 logits scale {scale:.1f}: fp8w error {e_8:.3f}, fp8mm error {e_mm:.3f}; fp8mm vs fp8w on the other three utterances {d_rest:.3f}")
    assert np.isfinite(lmm).all()
    assert e_8 < 1.2e-2 * scale
    assert e_mm < 1.5e-2 * scale                              # measured 4.9e-3 (0.244 of 50)
    assert d_rest < 1.5e-2 * scale                            # measured 4.6e-3
