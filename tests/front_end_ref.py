"""Float64 statements of every family's first stretch, from samples to encoder input, one function per stage, their rounding budgets, the layouts the
sessions keep the stages in, inputs on which front-end errors show, and mutations that prove it.

The stages (tables -- window x DFT basis, mel banks, checkpoint tensors, position tables -- are the f32 tables of the oracles, upcast to float64):

  whisper_log_mel   samples -> padded signal [x[200..1] | x | x[L-2 .. L-41]] -> 400-point DFT with the periodic Hann window (as a matrix, the way the
                    reference freezes it) -> power -> Slaney mel -> clamp(1e-10) -> log10 = raw; (max(raw, clip max - 8) + 4) / 4 = finished
  qwen_log_mel      the same raw log-mel (reflect 200 on both sides with the last frame dropped reads the very same samples);
                    max(raw, clip max - 8) * 0.25 + 1 = finished; qwen_feat lays the clips out per 100-frame chunk slot
  kaldi_fbank       SenseVoiceOracle.frontend / ParaformerOracle.fbank (snip-edges frames, DC removal + pre-emphasis + Hamming folded into the basis,
                    Kaldi mel, clamp(eps), ln), each family with its own f32 basis table
  lfr_cmvn          7 frames stacked every 6 (left replicate x 3, right clamp), CMVN, positions; affine_mode 0 = SenseVoice ((x + mean) * var + pos behind the
                    language and system prompt rows), affine_mode 1 = Paraformer (x * var + (mean * var + pos), no prompt rows)
  whisper_stem      finished mel rows of ONE clip -> conv1 (k 3, pad 1) -> GELU -> conv2 (k 3, stride 2, pad 1) -> GELU -> + positions
  qwen_stem         chunk slots -> 3 x (Conv2d k 3, stride 2, pad 1 + tanh-GELU) -> conv_out -> + sinusoidal positions -> windows of chunks_per_window chunks,
                    padding slots zero (QwenAsrOracle.encode)

`rounded=` evaluates the SAME function with the rounding points the sessions document and exists ONLY to measure the rounding noise
E_round = stat(exact - rounded); a kernel is compared with the exact statement (within()):

  "f32"   the whole stage in float32, in each of the summation orders of orders() / _mm (f32 sessions; the front end of bf16 sessions too, where a bf16
          SenseVoice / Paraformer session adds the split-operand DFT of fbank_split_kernel as one more order)
  "bf16"  Whisper (csrc/whisper.hip, encode): the finished mel is stored as bf16 (`mel_gapped`), conv1_w / conv2_w are bf16, conv1's output d_h1 is bf16
          (GemmArgs::out_lo); accumulation, bias, GELU and the positions are f32 and conv2's output is f32.
          Qwen3-ASR (csrc/qwen.hip, conv-stem section): `feat`, the im2col buffer (copies of bf16 values: no further rounding), conv2d1..3 and conv_out
          weights, c1, c2 and c3 are bf16; conv_out's output with the positions is f32.
          SenseVoice / Paraformer: `mel` and `enc_in` are f32 in both precisions ("bf16" = "f32" there).

A stem takes the session's OWN tapped rows of the stage before as its input, so the front end does not enter the stem's error.
"""
import functools

import numpy as np
import torch

from conftest import sub
from oracle.qwen_asr_oracle import feat_lengths
from oracle.whisper_oracle import slaney_mel_filterbank

F = torch.nn.functional
F64, F32 = torch.float64, torch.float32
MARGIN = 3.0                      # the project's margin (sanm_block_ref.py): summation order, hardware log / exp, flips of single roundings
HOP, NFFT = 160, 400


def bf16(t):
    return t.to(F32).to(torch.bfloat16).to(t.dtype)


def stat(diff):
    """(worst row's RMS over the columns, max abs) of a [rows][cols] difference."""
    d = np.asarray(diff, dtype=np.float64)
    d = d.reshape(-1, d.shape[-1])
    return float(np.sqrt((d * d).mean(axis=1)).max()), float(np.abs(d).max())


def e_round(exact, rounded):
    """stat(exact - rounded); `rounded` may be a list of rounded evaluations (the float32 summation orders): then per statistic the largest."""
    forms = rounded if isinstance(rounded, (list, tuple)) else [rounded]
    es = [stat(np.asarray(exact, np.float64) - r) for r in forms]
    return tuple(max(e[i] for e in es) for i in range(2))


def within(got, exact, rounded, margin=MARGIN):
    """The comparison of the GPU test: per statistic stat(got - exact) <= margin x E_round, E_round = e_round(exact, rounded); where E_round is zero (digital
    silence, zero rows) the statistic must be zero. Every element takes part. -> (ok, (rms ratio, max ratio)); a ratio is inf where E_round is zero and
    the statistic is not, 0 where both are zero."""
    s, e = stat(np.asarray(got, np.float64) - exact), e_round(exact, rounded)
    ratio = tuple((si / ei) if ei > 0 else (0.0 if si == 0 else float("inf")) for si, ei in zip(s, e))
    return all(r <= margin for r in ratio), ratio


def rounded_forms(fn, prec, split=False):
    """fn(rounded=, order=) evaluated in every float32 order that applies (bf16 stems have none: one form)."""
    return [fn(rounded=prec, order=o) for o in orders(prec, split)]


def round_up(n, m):
    return (n + m - 1) // m * m


def _t(a, dtype=F64):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def _dtype(rounded):
    assert rounded in (None, "f32", "bf16"), rounded
    return F64 if rounded is None else F32


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def ramp_clip(L):
    """Leading digital silence (a quarter), a quiet 440 Hz tone of amplitude 1e-3 (to 55 %), then a 500 -> 3500 Hz chirp whose amplitude ramps from 0.05 to
    0.8 up to the last sample: the tone's peak bins lie 58 dB under the clip maximum and stay, its skirts and the silence lie more than 80 dB under it
    and are clamped to max - 8; the maximum itself sits in the last frames of the clip."""
    n = np.arange(L, dtype=np.float64)
    a, b = L // 4, (L * 11) // 20
    x = np.zeros(L)
    x[a:b] = 1e-3 * np.sin(2 * np.pi * 440.0 * n[a:b] / 16000.0)
    t = (n[b:] - b) / 16000.0
    dur = max((L - b) / 16000.0, 1e-9)
    x[b:] = np.linspace(0.05, 0.8, L - b) * np.sin(2 * np.pi * (500.0 * t + 0.5 * (3000.0 / dur) * t * t))
    return x.astype(np.float32)


def noise_clip(L, seed):
    """Unit-range noise whose level rises eightfold over the clip. Clips of 1600 samples and more end the way a stopped recording does: the last 400
    samples fade to 1e-3 of the level and the last three are a click. The last frame then consists of the click under the window's tail and of its mirror
    image in the right reflect pad, so a reflect index that is off by one sample (the click's last sample mirrored as well) changes that frame's spectrum
    by far more than bf16 rounding does; under full-level noise the 40 pad samples, at window weights below 0.1, would not show."""
    x = sub("checkpoints").synth_audio("unit", 1, int(L), seed=int(seed))[0, 0]
    x = (x * np.linspace(0.5, 4.0, int(L), dtype=np.float32)).astype(np.float32)
    if L >= 4 * NFFT:
        x[-NFFT - 3:-3] *= np.float32(1e-3)
        x[-3:] = (0.5, -0.9, 0.7)
    return x


def to_int16(x):
    """The clip as 16-bit PCM and the float samples a Whisper / Qwen session makes of it (x 2^-15, exact in f32)."""
    q = np.clip(np.round(np.asarray(x, np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    return q, (q.astype(np.float32) * np.float32(2.0 ** -15))


def to_kaldi(x):
    """The clip in the Kaldi front ends' int16 value range (f32 samples with integer values)."""
    return np.clip(np.round(np.asarray(x, np.float64) * 32768.0), -32768, 32767).astype(np.float32)


RAMP_FRAMES, ZERO_FRAMES = 150, 40                                  # 150 = 2 x 64 + 22: the maximum lies in a partial block
WHISPER_FRAMES = (31, 32, 33, 63, 64, 65, 127, 128, 129)            # T = 16 | 17 at round_up(T + 1, 16); the 64-frame workgroup of the fbank kernels
QWEN_FRAMES = (2, 99, 100, 101, 199, 200, 201)                      # + chunks_per_window * 100 - 1, + 0, + 1
KALDI_FRAMES = (1, 5, 6, 7, 12, 13, 63, 64, 65, 129)                # LFR group edges (6 frames a row, 3 to the right), the fbank workgroup


def edge_lengths(family, cfg=None):
    """Sample counts of the edge batch of a family. Whisper / Qwen lengths carry residues of 0 .. 159 samples on top of frames x 160 (the frame count is
    L // 160), so that in a packed int16 batch clips start at odd sample offsets."""
    res = (0, 1, 79, 159, 3, 158, 80, 2, 157, 81, 5)
    if family == "whisper":
        return [400, 401, 560] + [HOP * f + res[i % len(res)] for i, f in enumerate(WHISPER_FRAMES)]
    if family == "qwen":
        w = cfg.chunks_per_window * cfg.chunk
        return [max(HOP * f + res[i % len(res)], NFFT) for i, f in enumerate(QWEN_FRAMES + (w - 1, w, w + 1))]     # 2 frames: 400 samples, the shortest clip
    if family == "kaldi":
        return [400 + HOP * (f - 1) + res[i % 4] for i, f in enumerate(KALDI_FRAMES)]
    raise ValueError(family)


def edge_batch(family, cfg=None, seed=100):
    """The primary ragged batch: the edge lengths (noise), then one ramp_clip next to one all-zero clip."""
    clips = [noise_clip(L, seed + i) for i, L in enumerate(edge_lengths(family, cfg))]
    if family == "kaldi":
        return [to_kaldi(c * 0.1) for c in clips] + [to_kaldi(ramp_clip(400 + HOP * (RAMP_FRAMES - 1) + 77)), np.zeros(400 + HOP * (ZERO_FRAMES - 1), np.float32)]
    return clips + [ramp_clip(HOP * RAMP_FRAMES + 77), np.zeros(HOP * ZERO_FRAMES + 3, np.float32)]


def long_batch(family, seed=900):
    """Two long clips (>= 300 frames) of other data: what a session's buffers hold when the short batch follows."""
    clips = [noise_clip(HOP * 333 + 11, seed), noise_clip(HOP * 302, seed + 1)]
    return [to_kaldi(c * 0.1) for c in clips] if family == "kaldi" else clips


# ---- Whisper / Qwen log-mel --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _whisper_tables(n_mels, sample_rate=16000):
    """(windowed DFT basis [2 x bins][nfft], mel bank [n_mels][bins]) in f32, as WhisperOracle._build_frontend states them."""
    bins = NFFT // 2 + 1
    t = torch.arange(NFFT, dtype=F32).unsqueeze(0)
    f = torch.arange(bins, dtype=F32).unsqueeze(1)
    omega = (2.0 * torch.pi / NFFT) * f * t
    window = torch.hann_window(NFFT, periodic=True).float()
    dft = torch.cat([torch.cos(omega) * window.unsqueeze(0), -torch.sin(omega) * window.unsqueeze(0)], dim=0)
    return dft, slaney_mel_filterbank(bins, 0.0, sample_rate // 2, n_mels, sample_rate).t().contiguous()


def raw_log_mel(cfg, audio, rounded=None, mut=None, order="seq"):
    """[frames][n_mels] log10 mel of one clip before the clamp; frames = L // 160. mut: "reflect_left" / "reflect_right" shift the reflect index by one
    sample at that end ([x[199..0] | x | ...], [... | x | x[L-1 .. L-40]])."""
    dt = _dtype(rounded)
    assert cfg.nfft == NFFT and cfg.hop_length == HOP
    x = _t(np.asarray(audio, np.float32).reshape(-1), dt)
    L, half, right = x.numel(), NFFT // 2, NFFT // 2 - HOP
    assert L >= NFFT, "the reflect index is defined from nfft samples up"
    sl, sr = (0 if mut == "reflect_left" else 1), (0 if mut == "reflect_right" else 1)
    xp = torch.cat([x[sl:sl + half].flip(0), x, x[L - right - sr:L - sr].flip(0)])
    frames = xp.unfold(0, NFFT, HOP)
    assert frames.shape[0] == L // HOP
    dft, fb = _whisper_tables(cfg.n_mels, cfg.sample_rate)
    bins = NFFT // 2 + 1
    sq = _mm(frames.contiguous(), dft.to(dt), _order(rounded, order, dft=True)) ** 2
    return _mm(sq[:, :bins] + sq[:, bins:], fb.to(dt), _order(rounded, order)).clamp(min=1e-10).log10()


def right_pad_read(L):
    """Samples of the right reflect pad that the last frame reads: the frames end at 160 (L // 160) + 240 of the padded signal, the pad starts at 200 + L,
    so a clip with 40 or more samples beyond its last whole hop never reads it."""
    return max(0, NFFT // 2 - HOP - int(L) % HOP)


def _finish(raw, scale_add, clip_max=None):
    m = raw.max() if clip_max is None else torch.as_tensor(clip_max, dtype=raw.dtype)
    x = torch.maximum(raw, m - 8.0)
    return (x + 4.0) * 0.25 if scale_add == "whisper" else x * 0.25 + 1.0


def _log_mel(kind, cfg, audio, rounded, mut, clip_max, order):
    with torch.inference_mode():
        raw = raw_log_mel(cfg, audio, rounded, mut if mut in ("reflect_left", "reflect_right") else None, order)
        fin = _finish(raw, kind, clip_max)
        if rounded == "bf16":
            fin = bf16(fin)
        return raw.to(F64).numpy(), fin.to(F64).numpy()


def whisper_log_mel(cfg, audio, rounded=None, mut=None, clip_max=None, order="seq"):
    """-> (raw [F][n_mels], finished [F][n_mels]) float64. clip_max replaces the clip's own maximum (the "batch maximum" mutation passes the batch's)."""
    return _log_mel("whisper", cfg, audio, rounded, mut, clip_max, order)


def qwen_log_mel(cfg, audio, rounded=None, mut=None, clip_max=None, order="seq"):
    return _log_mel("qwen", cfg, audio, rounded, mut, clip_max, order)


def batch_max(cfg, audios):
    """The largest raw log-mel of a batch (the wrong clamp reference)."""
    with torch.inference_mode():
        return max(float(raw_log_mel(cfg, a).max()) for a in audios)


# ---- Whisper layouts -----------------------------------------------------------------------------------------------------------------------------
def whisper_rows(lengths):
    """Per clip (first row of its frames in `mel_gapped`, frames F, first row in `stem`, T) and the row counts of the two taps. The gapped buffer is in
    frame-rate rows: clip b owns rows [2 g_b, 2 g_b + 2 round_up(T_b + 1, 16)), g_b = sum of round_up(T + 1, 16) over the clips before; its row 2 g_b is
    conv1's leading zero row, frames follow, the rest (>= 1 row: conv2's zero padding) is zero. `stem` rows are compact: clip b at sum round_up(T, 16)."""
    out, g, r = [], 0, 0
    for L in lengths:
        Fr = int(L) // HOP
        T = (Fr + 1) // 2
        out.append((2 * g + 1, Fr, r, T))
        g += round_up(T + 1, 16)
        r += round_up(T, 16)
    return out, 2 * round_up(g, 128), r


ORDERS = ("seq", "lib", "split")


def orders(prec, split=False):
    """The float32 evaluations whose noise makes up E_round of an f32 contraction (statistic-wise the largest counts, see e_round()): f32 rounding noise
    depends on the summation order, by 2 to 5 x on single clips, and no order is THE float32 evaluation. split: the session runs fbank_split_kernel --
    bf16 SenseVoice / Paraformer sessions unless ASR_FBANK_SPLIT=0. Whisper and Qwen3-ASR sessions never build the split table (FrontEnd::dft_split is set
    in csrc/sensevoice.hip only): their bf16 sessions run the exact-f32 fbank_kernel, and the split kernel's Whisper mode is not reachable."""
    return ("seq", "lib") + (("split",) if prec == "bf16" and split else ())


def _mm(a, w, order):
    """a [M][K] x w [N][K]^T. order None: the operands' own precision, library product (the float64 statements). The float32 evaluations:
      "lib"    the library's blocked f32 product
      "seq"    ONE running f32 sum per output, k ascending, every product and every partial sum rounded to f32: what a matrix-pipe kernel does along K
               (measured on an MI355X with E_round from "lib" alone: 3.4 on the Whisper stem of long clips, whose blocked sums are 2 to 3 x more accurate
               than any sequential one; with "seq" alone: 4.7 on the log-mel of clips that end in a click, where an ascending sum meets the large terms last)
      "split"  fbank_split_kernel (csrc/kernels.hip): x = xh + xl and b = bh + bm + bl in bf16 terms, x b ~ xl bm + xl bh + xh bl + xh bm + xh bh summed
               smallest first into the f32 accumulator, the term xl bl dropped"""
    if order in (None, "lib"):
        return a @ w.t()
    assert a.dtype == F32 and w.dtype == F32 and order in ("seq", "split"), order
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=F32)
    if order == "seq":
        for k in range(a.shape[1]):
            acc += a[:, k:k + 1] * w[:, k].unsqueeze(0)
        return acc
    ah = bf16(a)
    al = bf16(a - ah)
    wh = bf16(w)
    wm = bf16(w - wh)
    wl = bf16(w - wh - wm)
    for k in range(a.shape[1]):
        for x, y in ((al, wm), (al, wh), (ah, wl), (ah, wm), (ah, wh)):
            acc += x[:, k:k + 1] * y[:, k].unsqueeze(0)
    return acc


def _order(rounded, order, dft=False):
    """The _mm order of a stage: none for the float64 statements, `order` for float32 ("split" only where the stage is a DFT)."""
    if rounded is None:
        return None
    assert order in ORDERS, order
    return order if dft or order != "split" else "seq"


def _conv1d(x, w, b, stride, order):
    """x [C][n] (already padded) -> [n_out][N]: k 3 as a product over [C x 3] patches."""
    patches = x.unfold(1, 3, stride).permute(1, 0, 2).reshape(-1, x.shape[0] * 3)
    return _mm(patches, w.reshape(w.shape[0], -1), order) + b


def whisper_stem(cfg, ck, mel_rows, rounded=None, mut=None, gelu="erf", order="seq"):
    """mel_rows [F][n_mels] (one clip's finished mel) -> [T][d]. mut: "conv2_past_end" = conv2 reads, behind the clip's last frame, what conv1 makes of
    that row (frame F - 1 on its left, zeros else) instead of zero -- the row zero_gap_rows_kernel clears; it is read for odd F only;
    "conv1_lead_frame0" = conv1's leading zero row replaced by frame 0."""
    dt = F64 if rounded in (None, "bf16") else F32
    r = (lambda t: bf16(t)) if rounded == "bf16" else (lambda t: t)
    g = lambda t: F.gelu(t, approximate="tanh") if gelu == "tanh" else F.gelu(t)
    od = _order(rounded, order) if rounded == "f32" else None
    with torch.inference_mode():
        w1, b1 = r(_t(ck["model.encoder.conv1.weight"], dt)), _t(ck["model.encoder.conv1.bias"], dt)
        w2, b2 = r(_t(ck["model.encoder.conv2.weight"], dt)), _t(ck["model.encoder.conv2.bias"], dt)
        x = _t(mel_rows, dt).t()                                                      # [n_mels][F]
        Fr = x.shape[1]
        zero = torch.zeros_like(x[:, :1])
        xp = torch.cat([x[:, :1] if mut == "conv1_lead_frame0" else zero, x, zero, zero], dim=1)
        h1 = r(g(_conv1d(xp, w1, b1, 1, od))).t()                                # [d][F + 1]: column F is the row behind the clip
        if mut != "conv2_past_end":
            h1[:, Fr] = 0.0
        h1 = torch.cat([torch.zeros_like(h1[:, :1]), h1], dim=1)                      # conv2's left zero
        y = g(_conv1d(h1, w2, b2, 2, od))
        T = (Fr + 1) // 2
        assert y.shape[0] == T, (y.shape, T)
        return (y + _t(ck["model.encoder.embed_positions.weight"][:T], dt)).to(F64).numpy()


# ---- Qwen3-ASR layouts and stem -----------------------------------------------------------------------------------------------------------------------
def qwen_slots(cfg, lengths):
    """Per clip (first chunk slot, frames F, chunks, windows, first window) and the slot / window totals: a clip owns whole windows of chunks_per_window slots."""
    out, s, w = [], 0, 0
    for L in lengths:
        Fr = int(L) // HOP
        nc = (Fr + cfg.chunk - 1) // cfg.chunk
        nw = (nc + cfg.chunks_per_window - 1) // cfg.chunks_per_window
        out.append((s, Fr, nc, nw, w))
        s += nw * cfg.chunks_per_window
        w += nw
    return out, s, w


def qwen_feat(cfg, fins, mut=None, floor=None):
    """Finished log-mels [F][n_mels] of a batch -> [slots][chunk][n_mels]: frames past the clip and whole padding slots are zero. mut: "slot_tail" = the
    frames behind the clip inside its last chunk carry `floor` (what the finish makes of a silent frame), "pad_slot" = the padding slots do."""
    plan, slots, _ = qwen_slots(cfg, [f.shape[0] * HOP for f in fins])
    out = np.zeros((slots, cfg.chunk, cfg.n_mels))
    for (s0, Fr, nc, nw, _), f, fl in zip(plan, fins, floor if floor is not None else [0.0] * len(fins)):
        flat = out[s0:s0 + nw * cfg.chunks_per_window].reshape(-1, cfg.n_mels)
        flat[:Fr] = f
        if mut == "slot_tail":
            flat[Fr:nc * cfg.chunk] = fl
        if mut == "pad_slot":
            flat[nc * cfg.chunk:] = fl
    return out


@functools.lru_cache(maxsize=None)
def _qwen_positions(cfg):
    half = cfg.enc_d // 2
    inc = np.log(10000) / (half - 1)
    inv = torch.exp(-inc * torch.arange(half).float())
    st = torch.arange(cfg.max_source_positions)[:, None] * inv[None, :]
    return torch.cat([torch.sin(st), torch.cos(st)], 1)                              # f32, as QwenAsrOracle builds it


def qwen_stem(cfg, ck, feat_slots, live=None, rounded=None, order="seq"):
    """feat_slots [S][chunk][n_mels], S a multiple of chunks_per_window -> [S / cpw][cpw x 13][enc_d]; `live` [S] marks the slots that hold a chunk, the
    others (window padding) are zero rows, as in QwenAsrOracle.encode."""
    dt = F64 if rounded in (None, "bf16") else F32
    r = (lambda t: bf16(t)) if rounded == "bf16" else (lambda t: t)
    a, cpw = "thinker.audio_tower.", cfg.chunks_per_window
    od = _order(rounded, order) if rounded == "f32" else None
    with torch.inference_mode():
        x = _t(feat_slots, dt).permute(0, 2, 1).unsqueeze(1)                          # [S][1][mels][chunk]
        for i in (1, 2, 3):
            w, b = r(_t(ck[f"{a}conv2d{i}.weight"], dt)), _t(ck[f"{a}conv2d{i}.bias"], dt)
            S, _, h, wd = x.shape
            ho, wo = (h - 1) // 2 + 1, (wd - 1) // 2 + 1
            patches = F.unfold(x, 3, padding=1, stride=2).transpose(1, 2).reshape(S * ho * wo, -1)         # [S x ho x wo][C x 9]
            y = _mm(patches, w.reshape(w.shape[0], -1), od) + b
            x = r(F.gelu(y, approximate="tanh")).reshape(S, ho, wo, -1).permute(0, 3, 1, 2)
        S, nt = x.shape[0], x.shape[3]
        assert nt == 13 and S % cpw == 0
        y = _mm(x.permute(0, 3, 1, 2).reshape(S * nt, -1), r(_t(ck[a + "conv_out.weight"], dt)), od).reshape(S, nt, -1)
        y = y + _qwen_positions(cfg)[:nt].to(dt)
        if live is not None:
            y = y * _t(np.asarray(live, np.float64), dt)[:, None, None]
        return y.reshape(S // cpw, cpw * nt, cfg.enc_d).to(F64).numpy()


def qwen_tokens(cfg, frames):
    """Audio tokens of a clip of `frames` mel frames (13 per full chunk, the three stride-2 lengths of the partial one)."""
    return feat_lengths(int(frames))


# ---- Kaldi fbank, LFR + CMVN ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sv_oracle(cfg, ck_id, dtype):
    from oracle.sensevoice_oracle import SenseVoiceOracle
    return SenseVoiceOracle(cfg, _held[ck_id], dtype=dtype)


@functools.lru_cache(maxsize=None)
def _pf_oracle(cfg, ck_id):
    from oracle.paraformer_oracle import ParaformerOracle
    return ParaformerOracle(cfg, _held[ck_id])


@functools.lru_cache(maxsize=None)
def _kaldi_front(cfg, dtype):
    """The front-end half of SenseVoiceOracle alone: its tables depend on the geometry only, so a Paraformer configuration builds it too."""
    from oracle.sensevoice_oracle import SenseVoiceOracle
    o = SenseVoiceOracle.__new__(SenseVoiceOracle)
    o.cfg, o.dtype = cfg, dtype
    o._build_frontend()
    return o


_held = {}


def _hold(ck):
    _held[id(ck)] = ck
    return id(ck)


def kaldi_fbank(cfg, ck, audio, rounded=None, order="seq"):
    """[frames][n_mels] ln-mel of one clip. The two families state the same function with different f32 tables: SenseVoice folds DC removal and
    pre-emphasis into the windowed basis row by row (SenseVoiceOracle._build_frontend), Paraformer multiplies the basis by a frame-transform matrix in f32
    (ParaformerOracle._frontend). The tables differ in their last bits, which on int16-range samples is 3 .. 10 x the f32 noise of the stage: each
    family is held to its own table."""
    dt = _dtype(rounded)
    with torch.inference_mode():
        x = torch.as_tensor(np.asarray(audio, np.float32).reshape(-1))
        frames = x.to(dt).unfold(0, cfg.win_length, cfg.hop_length).contiguous()
        if hasattr(cfg, "n_dec"):
            o = _pf_oracle(cfg, _hold(ck))
            basis, nfreq, bank, eps = o.kernel, o.nfreq, o.mel_bins, float(o.eps)
        else:
            o = _kaldi_front(cfg, F32)
            basis, nfreq, bank, eps = o.fbank_kernel, o.nfreq, o.mel_filters.t().contiguous(), o.log_eps
        sq = _mm(frames, basis.to(dt), _order(rounded, order, dft=True)) ** 2
        return _mm(sq[:, :nfreq] + sq[:, nfreq:], bank.to(dt), _order(rounded, order)).clamp(min=eps).log().to(F64).numpy()


def lfr_cmvn(cfg, ck, mel, affine_mode, lang=0, rounded=None, mut=None):
    """mel [frames][n_mels] -> the encoder's input rows. affine_mode 0: SenseVoice, [language row | system rows | LFR rows]; 1: Paraformer, LFR rows.
    mut: "no_left_clamp" / "no_right_clamp" = frames before the first / behind the last read as zero rows instead of the edge frame."""
    dt = _dtype(rounded)
    with torch.inference_mode():
        m = _t(mel, dt)
        n = m.shape[0]
        n_lfr = (n + cfg.lfr_n - 1) // cfg.lfr_n
        idx = torch.arange(0, n_lfr * cfg.lfr_n, cfg.lfr_n).unsqueeze(1) + torch.arange(cfg.lfr_m) - (cfg.lfr_m - 1) // 2
        x = m[idx.clamp(min=0, max=n - 1)]
        if mut == "no_left_clamp":
            x = x * (idx >= 0).to(dt).unsqueeze(2)
        if mut == "no_right_clamp":
            x = x * (idx <= n - 1).to(dt).unsqueeze(2)
        x = x.reshape(n_lfr, cfg.feat_dim)
        if affine_mode == 0:
            o = _sv_oracle(cfg, _hold(ck), F32)
            x = (x + o.cmvn_means.to(dt)) * o.cmvn_vars.to(dt) + o.speech_position[:n_lfr].to(dt)
            x = torch.cat([o.language_embed[lang:lang + 1].to(dt), o.system_embed.to(dt), x], dim=0)
        else:
            o = _pf_oracle(cfg, _hold(ck))
            x = x * o.cmvn_vars.to(dt) + o.in_bias[:n_lfr].to(dt)
        return x.to(F64).numpy()
