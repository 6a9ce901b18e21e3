"""Float64 statement of the Whisper encoder and decoder layers, their bf16 rounding budget, inputs on which attention errors show, and the planted mistakes.

The stack (csrc/whisper.hip: `WhSession::encode` / `enqueue_step`; oracle/whisper_oracle.py: `encode`, `decoder`) runs from the conv stem's rows to the cross-K/V
slabs and from the token ids to the logits. The end-to-end tests compare it with the oracle behind all layers, on synthetic weights whose soft-max is nearly uniform
(mean top probability 0.026 over 150 encoder keys): one masked, duplicated or stale key moves `enc_out` by less than bf16 rounding does. This module restates the
oracle line for line in float64, on the oracle's own folded f32 weights (`_fold_encoder`, `_fold_decoder`), split at the session's taps so that every stage takes
the SESSION'S OWN rows of the stage before and no stage inherits another's noise (every function takes the WhisperLayers object of the checkpoint first):

  enc_layer_exact(i, rows)        `stem` / `enc{i-1}` rows of one utterance [T][d] -> `enc{i}`
  enc_out_exact(rows)             `enc{last}` -> `enc_out` (the f32 LayerNorm the tap itself runs)
  cross_exact(rows)               `enc{last}` -> (K, V) [Ld][H][T][64]: final LayerNorm + the fused cross-K/V projection (K scaled by d_head^-1/4)
  dec_in_exact(ids, pos)          token embedding + position row
  dec_layer_exact(l, xs, kv, pad) xs: the rows of ONE sequence that entered layer l at every step so far (the session's `dec_in` / `dec{l-1}` taps), oldest
                                  first, the last entry being this step's [n][d]; the self-attention K/V history is recomputed from the earlier entries.
                                  kv: the utterance's (K, V) [H][T][64] of layer l, taken from the session's own `cross` tap. pad: left-pad slots. -> `dec{l}` [n][d]
  head_exact(rows)                the last row of every sequence -> logits (final LayerNorm, tied projection, -128 suppress penalty)
  *_rounded                       the same functions with the rounding points the bf16 session documents; they exist ONLY to measure E_round = stat(exact - rounded),
                                  a kernel is always compared with the exact functions. The switches (read off csrc/whisper.hip and arena.py):
                    "h"     parameter-free LayerNorm output that feeds a GEMM is bf16: `launch_layernorm<T>(xa .. h)` in encode(), `ln_gemm` in enqueue_step
                            (the skinny GEMM's prologue or `dec_layernorm` into `hh`), `hl` / `ln_x` of the logits head, `h` of the cross-K/V projection
                    "x"     the decode GEMM forms instead read the bf16 copies xa_lo / xb_lo / xc_lo of the residual stream and fold the LayerNorm through column
                            sums (`dg(.. xa_lo .. csum ..)`, csrc/decode_gemm.hip: "rstd (x W^T - mean c)", statistics of the bf16 rows in f32)
                    "w"     GEMM weights bf16, rounded AFTER the LayerNorm affine was folded in (arena.py: build_whisper_arena, `_absorb_ln` then `w.weight`);
                            the token embedding (== tied proj_out) is such a weight; biases, position tables and the final LayerNorms' affines stay f32
                    "qkv"   `qk`, `vt` (encoder) and `qkv` (decoder) are bf16 tensors (`g.out_lo`); the self-KV cache holds copies of those rows
                    "p"     encoder (attn_bf16_kernel) and prompt attention (csrc/prompt_attn.hip, header): exp(s - max) is the bf16 operand of P V, its f32
                            sum normalises. The decode-attention kernels keep f32 probabilities (csrc/kernels.hip: decode_attn_kernel `sc`)
                    "ctx"   the attention context is bf16 (`ctx`)
                    "cq"    the cross-attention query is bf16 (`cq`)
                    "ffn"   the FFN's hidden rows are bf16 (`ffn`)
                    "cross" the cross-K/V slab is bf16 (`d_cross`, g.out_lo with lo_group = 64)
                  The residual stream (`xa`, `xb`, `xc`), every LayerNorm statistic and the logits stay f32.
  plant           a checkpoint whose position tables and token table carry code channels that chosen heads read (below)
  mutations       of the exact functions: the planted mistakes a comparison must catch (ENC_MUTATIONS ..)

Which form of enqueue_step runs (bf16 session, R = B * n rows, `dgm` needs d % 256 == 0 and d_ffn % 256 == 0):

  rows R      projections                                                    roundings        logits head
  <= 32       decode GEMM, LayerNorm folded (q|k|v, cross-q, fc1), FFN-2 too  "x"              B <= 16: LayerNorm inside the GEMM (`ln_x`), else separate
  33 .. 64    decode GEMM; FFN-2 on the tiled split-K GEMM                    "x"              separate LayerNorm (`hl`)
  > 64        plain GEMMs behind `dec_layernorm`                              "h"              separate LayerNorm
  ASR_DECODE_GEMM=0 or d % 256 != 0: <= 32 rows and d % 256 == 0 -> LayerNorm in the skinny GEMM's prologue, else `dec_layernorm`; both round "h"
  left-padded prompts (prefill_prompts, ragged or n > 8): the same projections by R, both attentions on the prompt-attention kernel ("p")

How the inputs make errors show (plant). nf = d / 8 frequencies w_k in (0.3, pi - 0.3) give every position t the code c(t) = (cos w_k t, sin w_k t): <c(i), c(j)> has
one peak at i = j, and a shift or a reflection of t is a rotation of the code, i.e. a linear map. The code sits in channels 0 .. 2 nf - 1 of
`encoder.embed_positions` and `decoder.embed_positions`; channel 2 nf of both tables is a constant; `decoder.embed_tokens` carries c(id) of the ids below
TOKEN_CODES in channels 2 nf + 1 .. 4 nf. The q and k rows of the planted heads read these channels alone (through the folded LayerNorm):
  encoder layers    head 0 row t looks at key t, head 1 at key 256 - t (across the 256-key chunk boundary), head 2 at key t + 64
  decoder self      head 0 looks at position 0 (the oldest live slot: slot pad[b] of a left-padded prompt; a pad slot holds position 0 as well and would share
                    the weight), head 1 at its own position (the newest row), head 2 at position t + 1 (behind the causal bound), head 3 at position t - 2
  decoder cross     head 0: a row whose token id is below TOKEN_CODES looks at the encoder position of that number -- the tests feed ids 0 and T - 1, the first and
                    the last position of the row's own utterance. Head 1: every key made of a real row loses PAD_LEAD through the constant channel (it cancels
                    in the soft-max), a key made of a row without it -- a pad row -- does not, and would take the whole weight
Nothing writes into the code channels (those rows of every out-projection and FFN-2 are zero), and the residual branches are damped (RES_GAIN) so that the stream
keeps the tables' scale through all layers: behind the parameter-free LayerNorm the codes then keep their amplitude, and the planted scores stay near PEAK in every
layer. The encoder's v rows read the audio channels alone and the planted heads' v is V_GAIN times as large: the same position of ANOTHER utterance has the same key
but another v, which shows. For that the utterances of a batch are different windows of the anchor clip (batch_audios), not truncations of one window.
"""
import functools

import numpy as np
import torch

from conftest import sub
from oracle.whisper_oracle import WhisperOracle, _gelu
from sanm_block_ref import MARGIN, bf16, stat                                    # noqa: F401  (re-exported: the tests take them from here)

F = torch.nn.functional
F64 = torch.float64

ENC_ROUNDINGS = frozenset({"h", "w", "qkv", "p", "ctx", "ffn"})
CROSS_ROUNDINGS = frozenset({"h", "w", "cross"})
DEC_PLAIN = frozenset({"h", "w", "qkv", "ctx", "cq", "ffn"})                     # plain / skinny GEMMs behind a LayerNorm
DEC_DGM = frozenset({"x", "w", "qkv", "ctx", "cq", "ffn"})                       # decode GEMM with the LayerNorm folded
HEAD_ROUNDINGS = frozenset({"h", "w"})
F32_FORMS = (frozenset({"f32:seq"}), frozenset({"f32:rev"}), frozenset({"f32:chunk"}))       # the f32 session's budget: three float32 evaluations, other summation orders

# ---- the fixed inputs -----------------------------------------------------------------------------------------------------------------------------------
ENC_BATCHES = {"le128": (17, 1, 128, 15, 16, 127, 113), "le256": (129, 256, 240, 255), "gt256": (257, 300)}    # encoder positions per utterance, by max_T
ANCHOR_T, ANCHOR_SEED, ANCHOR_STRIDE = 300, 4100, 1000
DEC_BATCHES = (3, 9, 17, 33, 65)                                 # sequences: n = 4 prefill + n = 1 steps -> R = 12 .. 260 and 3 .. 65 (the table above)
PROMPT_LENS = (3, 11, 20)                                        # the left-padded prompts
N_PREFILL, N_STEPS = 4, 4
TOKEN_CODES = 300
ENC_A, DEC_A = 1.5, 0.5                                          # code amplitude in the position / token tables (the synthetic rows have an RMS of 0.2 / 0.08)
PEAK = 16.0                                                      # planted score of the chosen key (the other keys ~ 0 +- 2)
PAD_LEAD = 20.0
RES_GAIN = {"encoder": 0.3, "decoder": 0.15}                                                   # on every out-projection and FFN-2 of the planted checkpoint
V_GAIN = 4.0
REV, SHIFT = 256, 64                                             # encoder head 1: key REV - t; head 2: key t + SHIFT
PLANT_SEED = 77

ENC_MUTATIONS = ("mask_last", "mask_256", "foreign_key", "zero_hidden")
CROSSATT_MUTATIONS = ("drop_last", "pad_row")
SELF_MUTATIONS = ("causal_minus", "causal_plus", "pad_slot", "wrong_slot")
EMBED_MUTATIONS = ("pos_plus_one", "pad_pos")
HEAD_MUTATIONS = ("row_n_minus_2",)
"""The planted mistakes (each changes the EXACT functions in one place):
  encoder   mask_last      key T - 1 masked                              mask_256   key 256, the first key of the second chunk, masked (T > 256)
            foreign_key    the k and v of one key taken from the same row of the neighbouring utterance
            zero_hidden    eight FFN hidden columns of one row read as zero (one lost 16-byte store); the aligned group with the largest share of the row
  cross     drop_last      the last encoder position left out            pad_row    one row past T admitted (the tests pass the row)
  self      causal_minus   row i sees the slots < its own                causal_plus  row i sees one slot behind its own (n > 1)
            pad_slot       the last pad slot of a left-padded prompt attended (layer 0, where the slot holds id 0 at position 0; what the deeper layers
                           leave in a pad slot's rows is not defined)
            wrong_slot     the previous step wrote its K/V row one slot low: slot S - 2 holds row S - 1's K/V, slot S - 1 holds zeros
  embedding pos_plus_one   position + 1                                  pad_pos    a pad slot takes its slot number as position, not 0
  head      row_n_minus_2  the final LayerNorm reads row n - 2 of each sequence (row b * n - 1 of the buffer at n = 1)"""


def round_up(n, m):
    return (n + m - 1) // m * m


def samples_of(cfg, T):
    """Samples of a clip with T encoder positions (cfg.n_enc_pos; at least one n_fft window)."""
    n = max(cfg.nfft, cfg.hop_length * (2 * T - 1))
    assert cfg.n_enc_pos(n) == T, (T, n)
    return n


@functools.lru_cache(maxsize=None)
def anchor_audio(cfg):
    return sub("checkpoints").synth_audio("unit", 1, samples_of(cfg, ANCHOR_T) + 80 * ANCHOR_STRIDE, seed=ANCHOR_SEED)[0, 0]


def batch_audios(cfg, lengths, first=0):
    """Windows of the anchor clip. Utterance u starts (first + u) strides into it: equal starts would make row j of every utterance the same row, and a key
    taken from the neighbouring utterance would show nowhere."""
    a = anchor_audio(cfg)
    return [a[(first + u) % 80 * ANCHOR_STRIDE:][:samples_of(cfg, T)].copy() for u, T in enumerate(lengths)]


def utterance_rows(lengths):
    """(first row, T) of every utterance in the packed encoder rows (16-row aligned)."""
    out, r = [], 0
    for T in lengths:
        out.append((r, T))
        r += round_up(T, 16)
    return out


def bf16_bits_to_f64(u16):
    return torch.from_numpy((np.asarray(u16, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64))


def cross_slabs(raw, cfg, f32=False):
    """The session's `cross` tap -> float64 [2][Ld][H][Mpad][64]."""
    G = 2 * cfg.n_dec_layers * cfg.n_heads
    t = torch.from_numpy(np.asarray(raw, dtype=np.float32).astype(np.float64)) if f32 else bf16_bits_to_f64(raw)
    return t.reshape(2, cfg.n_dec_layers, cfg.n_heads, t.shape[0] // G, 64)


# ---- planting -------------------------------------------------------------------------------------------------------------------------------------------
def code_freqs(nf):
    return np.random.default_rng(PLANT_SEED).uniform(0.3, np.pi - 0.3, nf)


def codes(nf, n):
    """[n][2 nf]: (cos w_k t | sin w_k t)."""
    ph = np.arange(n)[:, None] * code_freqs(nf)[None, :]
    return np.concatenate([np.cos(ph), np.sin(ph)], axis=1)


def _rotation(nf, shift):
    """M with M c(t) = c(t + shift)."""
    ph = shift * code_freqs(nf)
    c, s = np.diag(np.cos(ph)), np.diag(np.sin(ph))
    return np.block([[c, -s], [s, c]])


def _reflection(nf, about):
    """M with M c(t) = c(about - t)."""
    flip = np.diag(np.concatenate([np.ones(nf), -np.ones(nf)]))
    return _rotation(nf, about) @ flip


def plant(cfg, ck):
    """A copy of the checkpoint with the code channels and the planted q / k rows (module header)."""
    ck = {k: np.array(v, dtype=np.float32, copy=True) for k, v in ck.items()}
    d, H, nf = cfg.d_model, cfg.n_heads, cfg.d_model // 8
    m = 2 * nf
    scale = float(cfg.d_head ** -0.25)
    pos_ch, const_ch, tok_ch = slice(0, m), m, slice(m + 1, 2 * m + 1)
    ep, dp_, emb = ck["model.encoder.embed_positions.weight"], ck["model.decoder.embed_positions.weight"], ck["model.decoder.embed_tokens.weight"]
    ep[:, pos_ch] = ENC_A * codes(nf, ep.shape[0]); ep[:, const_ch] = 2 * ENC_A
    dp_[:, pos_ch] = DEC_A * codes(nf, dp_.shape[0]); dp_[:, const_ch] = 2 * DEC_A
    emb[:, tok_ch] = 0.0; emb[:, pos_ch] = 0.0; emb[:, const_ch] = 0.0
    emb[:TOKEN_CODES, tok_ch] = DEC_A * codes(nf, TOKEN_CODES)
    eye = np.eye(m)
    special = np.r_[0:2 * m + 1]
    # nothing writes into the code channels, and the residual branches are damped so that the stream keeps the scale of the tables through all layers (the
    # synthetic out-projections grow it eightfold in two layers, which would drown the codes behind the parameter-free LayerNorm)
    for side, n_layers, outs in (("encoder", cfg.n_enc_layers, ("self_attn.out_proj", "fc2")), ("decoder", cfg.n_dec_layers, ("self_attn.out_proj", "encoder_attn.out_proj", "fc2"))):
        for i in range(n_layers):
            for o in outs:
                wn, bn = f"model.{side}.layers.{i}.{o}.weight", f"model.{side}.layers.{i}.{o}.bias"
                gain = RES_GAIN[side]
                ck[wn] *= gain; ck[bn] *= gain
                ck[wn][special] = 0.0; ck[bn][special] = 0.0

    def head_rows(wname, bname, h, M, cols, gamma, gain):
        """Rows h * 64 .. + m of a projection read M x (the normalised code in `cols`); the head's other rows and its bias are zero."""
        w = ck[wname]
        w[h * 64:(h + 1) * 64] = 0.0
        w[h * 64:h * 64 + m, cols] = gain * M / (scale * gamma[cols][None, :])
        if bname is not None:
            ck[bname][h * 64:(h + 1) * 64] = 0.0

    def const_col(wname, h, dim, gamma, value):
        ck[wname][h * 64 + dim, const_ch] = value / (scale * gamma[const_ch])

    # the normalised code has an amplitude near A / (row RMS); the gains turn nf * amplitude^2 into PEAK (amplitudes measured on the anchor clip: 2.2 encoder, 1.8 decoder; the constant channels 4.4 and 3.6)
    g_enc = (PEAK / nf) ** 0.5 / 2.2
    g_dec = (PEAK / nf) ** 0.5 / 1.8
    enc_maps = [eye, _reflection(nf, REV), _rotation(nf, SHIFT)][:min(H - 1, 3)]
    for i in range(cfg.n_enc_layers):
        p = f"model.encoder.layers.{i}."
        gamma = ck[p + "self_attn_layer_norm.weight"]
        ck[p + "self_attn.v_proj.weight"][:, special] = 0.0      # v is made of the audio alone: the same position of another utterance has another v
        for h, M in enumerate(enc_maps):
            ck[p + "self_attn.v_proj.weight"][h * 64:(h + 1) * 64] *= V_GAIN         # a planted head's context weighs as much as the FFN's output: a wrong v row shows
            ck[p + "self_attn.v_proj.bias"][h * 64:(h + 1) * 64] *= V_GAIN
            head_rows(p + "self_attn.q_proj.weight", p + "self_attn.q_proj.bias", h, M, pos_ch, gamma, g_enc)
            head_rows(p + "self_attn.k_proj.weight", None, h, eye, pos_ch, gamma, g_enc)
    c0 = codes(nf, 1)[0]
    gamma_e = ck["model.encoder.layer_norm.weight"]
    for l in range(cfg.n_dec_layers):
        p = f"model.decoder.layers.{l}."
        gamma = ck[p + "self_attn_layer_norm.weight"]
        self_maps = [None, eye, _rotation(nf, 1), _rotation(nf, -2)][:H]
        for h, M in enumerate(self_maps):
            q, k = p + "self_attn.q_proj.weight", p + "self_attn.k_proj.weight"
            if M is None:                                  # position 0: a constant query (the constant channel) against the code's match with c(0)
                ck[q][h * 64:(h + 1) * 64] = 0.0
                ck[p + "self_attn.q_proj.bias"][h * 64:(h + 1) * 64] = 0.0
                ck[q][h * 64:h * 64 + m, const_ch] = g_dec * c0 / 2.0 / (scale * gamma[const_ch])        # (the constant channel is twice the code's amplitude)
                head_rows(k, None, h, eye, pos_ch, gamma, g_dec)
            else:
                head_rows(q, p + "self_attn.q_proj.bias", h, M, pos_ch, gamma, g_dec)
                head_rows(k, None, h, eye, pos_ch, gamma, g_dec)
        gamma_c = ck[p + "encoder_attn_layer_norm.weight"]
        g_tok = 1.25 * (PEAK / nf) ** 0.5 / 1.8
        head_rows(p + "encoder_attn.q_proj.weight", p + "encoder_attn.q_proj.bias", 0, eye, tok_ch, gamma_c, g_tok)
        head_rows(p + "encoder_attn.k_proj.weight", None, 0, eye, pos_ch, gamma_e, g_enc)
        if H > 1:                                          # head 1 keeps its synthetic rows; dim 63 carries the lead of a pad key
            ck[p + "encoder_attn.q_proj.weight"][64 + 63] = 0.0
            ck[p + "encoder_attn.q_proj.bias"][64 + 63] = 0.0
            const_col(p + "encoder_attn.q_proj.weight", 1, 63, gamma_c, PAD_LEAD ** 0.5 / 3.6)
            ck[p + "encoder_attn.k_proj.weight"][64 + 63] = 0.0
            ck[p + "encoder_attn.k_proj.weight"][64 + 63, const_ch] = -PAD_LEAD ** 0.5 / 4.4 / (scale * gamma_e[const_ch])
    return ck


# ---- the stack ------------------------------------------------------------------------------------------------------------------------------------------
class WhisperLayers:
    """The layers of one (cfg, checkpoint) in float64, on the oracle's folded f32 weights."""

    def __init__(self, cfg, ck, suppress_tokens=None, begin_suppress_tokens=()):
        self.cfg = cfg
        self.orc = WhisperOracle(cfg, ck, suppress_tokens, begin_suppress_tokens, dtype=F64)
        self._w = {}

    def w(self, group, name, rnd):
        """A folded weight in float64; bf16-rounded (after the fold) when "w" is switched on and it is a matrix."""
        key = (group, name, "w" in rnd)
        if key not in self._w:
            o = self.orc
            if group == "ckv":
                t = {"w": o.w_ckv, "b": o.b_ckv}[name]
            elif group == "ck":
                t = o.ck[name]
            else:
                t = (o.enc if group[0] == "e" else o.dec)[group[1]][name]
            t = t.to(F64)
            self._w[key] = bf16(t) if ("w" in rnd and t.dim() == 2) else t
        return self._w[key]

    @staticmethod
    def _arith(rnd):
        """(r, mm, ln) of a rounding set. bf16 points: r(name, t) rounds where `name` is switched on, the rest is float64. An F32 form ("f32:seq" | "f32:rev" |
        "f32:chunk" in rnd): every product, LayerNorm and stored tensor is float32, the products summed in that order (the f32 session's budget)."""
        form = next((x[4:] for x in rnd if x.startswith("f32:")), None)
        if form is None:
            return (lambda name, t: bf16(t) if name in rnd else t), (lambda a, b: a @ b), (lambda t, d, g=None, b=None: F.layer_norm(t, (d,), g, b))
        f32 = lambda t: t.to(torch.float32)

        def mm(a, b):
            a, b = f32(a), f32(b)
            if form == "rev":
                a, b = a.flip(-1), b.flip(-2)
            if form == "chunk":
                acc = torch.zeros(a.shape[:-1] + b.shape[-1:], dtype=torch.float32)
                for k0 in range(0, a.shape[-1], 32):
                    acc = acc + a[..., k0:k0 + 32] @ b[..., k0:k0 + 32, :]
                return acc.to(F64)
            return (a @ b).to(F64)
        ln = lambda t, d, g=None, b=None: F.layer_norm(f32(t), (d,), None if g is None else f32(g), None if b is None else f32(b)).to(F64)
        return (lambda name, t: f32(t).to(F64) if name != "x" else t), mm, ln

    # ---- encoder
    def enc_layer(self, i, x, rnd=frozenset(), mut=None, probs=None, foreign=None):
        """Layer i on the rows x [T][d] of one utterance. mut: (name, ...); foreign: the neighbouring utterance's rows (foreign_key)."""
        c = self.cfg
        x = torch.as_tensor(np.asarray(x, dtype=np.float64))
        T, d, H = x.shape[0], c.d_model, c.n_heads
        W = lambda n: self.w(("e", i), n, rnd)
        r, mm, ln = self._arith(rnd)
        qkv_of = lambda rows: r("qkv", mm(r("h", ln(rows, d)), W("wqkv").t()) + W("bqkv"))
        qkv = qkv_of(x)
        if mut is not None and mut[0] == "foreign_key":
            j = mut[1]
            qkv = qkv.clone()
            qkv[j, d:] = qkv_of(torch.as_tensor(np.asarray(foreign, dtype=np.float64)))[j, d:]
        q, k, v = [z.reshape(T, H, c.d_head).transpose(0, 1) for z in qkv.split(d, dim=1)]
        s = mm(q, k.transpose(1, 2))
        if mut is not None and mut[0] == "mask_key":
            s = s.clone()
            s[:, :, mut[1]] = -float("inf")
        e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
        if probs is not None:
            probs.append(e / e.sum(dim=-1, keepdim=True))
        a = r("ctx", (mm(r("p", e), v) / e.sum(dim=-1, keepdim=True)).transpose(0, 1).reshape(T, d))
        x1 = r("res", mm(a, W("wo").t()) + W("bo") + x)
        hid = r("ffn", _gelu(mm(r("h", ln(x1, d)), W("w1").t()) + W("b1"), self.orc.gelu))
        if mut is not None and mut[0] == "zero_hidden":
            hid = hid.clone()
            share = (hid[mut[1]][None, :] * W("w2")).reshape(d, -1, 8).sum(dim=2)
            col0 = 8 * int((share * share).sum(dim=0).argmax())
            hid[mut[1], col0:col0 + 8] = 0.0
        return r("res", x1 + mm(hid, W("w2").t()) + W("b2")).numpy()

    def enc_mutation(self, name, T):
        """The mutation tuple of enc_layer for an utterance of T positions (None: it does not apply)."""
        if name == "mask_last":
            return ("mask_key", T - 1) if T > 1 else None
        if name == "mask_256":
            return ("mask_key", 256) if T > 257 else None
        if name == "foreign_key":
            return ("foreign_key", T // 2)
        if name == "zero_hidden":
            return ("zero_hidden", T // 2)
        raise KeyError(name)

    def _enc_norm(self, x, rnd):
        g, b = self.w("ck", "model.encoder.layer_norm.weight", rnd), self.w("ck", "model.encoder.layer_norm.bias", rnd)
        return self._arith(rnd)[2](torch.as_tensor(np.asarray(x, dtype=np.float64)), self.cfg.d_model, g, b)

    def enc_out(self, x):
        return self._enc_norm(x, frozenset()).numpy()

    def cross(self, x, rnd=frozenset()):
        """`enc{last}` rows [T][d] -> (K, V) [Ld][H][T][64]."""
        c = self.cfg
        r, mm, _ = self._arith(rnd)
        ckv = r("cross", mm(r("h", self._enc_norm(x, rnd)), self.w("ckv", "w", rnd).t()) + self.w("ckv", "b", rnd))
        T, Ld, d = ckv.shape[0], c.n_dec_layers, c.d_model
        k = ckv[:, :Ld * d].reshape(T, Ld, c.n_heads, c.d_head).permute(1, 2, 0, 3)
        v = ckv[:, Ld * d:].reshape(T, Ld, c.n_heads, c.d_head).permute(1, 2, 0, 3)
        return k, v

    def pad_key(self, l, rnd=frozenset()):
        """(k, v) [H][64] of layer l made of an encoder row of zeros: what a slab row past T holds on the CPU (pad_row)."""
        k, v = self.cross(np.zeros((1, self.cfg.d_model)), rnd)
        return k[l, :, 0], v[l, :, 0]

    # ---- decoder
    def dec_in(self, ids, positions, rnd=frozenset()):
        e = self.w("ck", "model.decoder.embed_tokens.weight", rnd)[torch.as_tensor(np.asarray(ids), dtype=torch.long)]
        return (e + self.w("ck", "model.decoder.embed_positions.weight", frozenset())[torch.as_tensor(np.asarray(positions), dtype=torch.long)]).numpy()

    def dec_layer(self, l, xs, kv, pad=0, rnd=frozenset(), mut=None, probs=None, pad_row=None):
        """Layer l on the newest rows xs[-1] [n][d] of one sequence; xs[:-1]: the rows that entered layer l at the earlier steps (slots 0 ..); kv: (K, V) [H][T][64];
        pad: slots 0 .. pad - 1 are left-pad slots. probs receives (self, cross) probabilities [H][n][keys]. pad_row: (k, v) [H][64] of the key pad_row admits."""
        c = self.cfg
        xs = [torch.as_tensor(np.asarray(x, dtype=np.float64)) for x in xs]
        x, x_all = xs[-1], torch.cat(xs, dim=0)
        n, S, d, H = x.shape[0], x_all.shape[0], c.d_model, c.n_heads
        S0 = S - n
        W = lambda nm: self.w(("d", l), nm, rnd)
        r, mm, ln_ = self._arith(rnd)
        ln = lambda t: r("h", ln_(r("x", t), d))
        name = mut[0] if mut is not None else None
        qkv = r("qkv", mm(ln(x_all), W("wqkv").t()) + W("bqkv"))
        heads = lambda t: t.reshape(t.shape[0], H, c.d_head).transpose(0, 1)
        q, k, v = heads(qkv[S0:, :d]), heads(qkv[:, d:2 * d]), heads(qkv[:, 2 * d:])
        if name == "wrong_slot":
            assert S0 - pad >= 2, "wrong_slot needs two live cached slots"
            k, v = k.clone(), v.clone()
            k[:, S0 - 2], v[:, S0 - 2] = k[:, S0 - 1], v[:, S0 - 1]
            k[:, S0 - 1], v[:, S0 - 1] = 0.0, 0.0
        slot, row = torch.arange(S)[None, :], S0 + torch.arange(n)[:, None]
        bound = row + {"causal_minus": -1, "causal_plus": 1}.get(name, 0)
        first = pad - 1 if name == "pad_slot" else pad
        assert first >= 0, "pad_slot needs a left-padded sequence"
        s = mm(q, k.transpose(1, 2)) + torch.where(slot > bound, -128.0, 0.0).to(F64)         # the reference's additive -128 (Export_Whisper.py:468-480)
        s = torch.where(slot < first, -float("inf"), s)                                      # a pad slot does not exist
        e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
        a = r("ctx", (mm(r("p", e), v) / e.sum(dim=-1, keepdim=True)).transpose(0, 1).reshape(n, d))
        xb = r("res", mm(a, W("wo").t()) + W("bo") + x)
        cq = heads(r("cq", mm(ln(xb), W("wcq").t()) + W("bcq")))
        ck_, cv_ = kv
        if name == "drop_last":
            ck_, cv_ = ck_[:, :-1], cv_[:, :-1]
        if name == "pad_row":
            ck_, cv_ = torch.cat([ck_, pad_row[0][:, None, :]], dim=1), torch.cat([cv_, pad_row[1][:, None, :]], dim=1)
        s2 = mm(cq, ck_.transpose(1, 2))
        e2 = torch.exp(s2 - s2.max(dim=-1, keepdim=True).values)
        if probs is not None:
            probs.append((e / e.sum(dim=-1, keepdim=True), e2 / e2.sum(dim=-1, keepdim=True)))
        a = r("ctx", (mm(r("p", e2), cv_) / e2.sum(dim=-1, keepdim=True)).transpose(0, 1).reshape(n, d))
        xc = r("res", mm(a, W("wco").t()) + W("bco") + xb)
        hid = r("ffn", _gelu(mm(ln(xc), W("w1").t()) + W("b1"), self.orc.gelu))
        return r("res", xc + mm(hid, W("w2").t()) + W("b2")).numpy()

    def head(self, rows, rnd=frozenset()):
        """The last rows [B][d] -> logits [B][vocab]."""
        g, b = self.w("ck", "model.decoder.layer_norm.weight", rnd), self.w("ck", "model.decoder.layer_norm.bias", rnd)
        r, mm, ln = self._arith(rnd)
        last = r("h", ln(torch.as_tensor(np.asarray(rows, dtype=np.float64)), self.cfg.d_model, g, b))
        return r("res", mm(last, self.w("ck", "model.decoder.embed_tokens.weight", rnd).t()) + self.orc.suppress_penalty.to(F64)).numpy()


def head_rows(rows, B, n, mut=None):
    """The rows the logits head reads out of the [B * n][d] rows behind the last layer; row_n_minus_2 reads one row early (sequences whose row exists)."""
    rows = np.asarray(rows)
    if mut == "row_n_minus_2":
        idx = np.arange(B) * n + n - 2
        return rows[np.maximum(idx, 0)], idx >= 0
    return rows[np.arange(B) * n + n - 1], np.ones(B, dtype=bool)


def positions_of(hist, n, pad=0, mut=None):
    """Positions of the slots hist .. hist + n - 1 of a sequence with `pad` left-pad slots (csrc/kernels.hip: embed_pos_kernel)."""
    at = hist + np.arange(n)
    pos = np.maximum(at - pad, 0)
    if mut == "pos_plus_one":
        pos = pos + 1
    if mut == "pad_pos":
        pos = np.where(at < pad, at, pos)
    return pos


_stacks = {}


def layers_of(cfg, ck, sup=None, beg=()):
    key = (cfg, id(ck))
    if key not in _stacks:
        _stacks[key] = (ck, WhisperLayers(cfg, ck, sup, beg))          # (holds ck, so the id stays its own)
    return _stacks[key][1]


@functools.lru_cache(maxsize=None)
def setup(cfg_name, planted=True):
    """(cfg, checkpoint, suppress, begin_suppress, WhisperLayers) of a test geometry; planted: with the code channels and the planted heads."""
    cfg = getattr(sub("config"), cfg_name)()
    ckm = sub("checkpoints")
    ck = ckm.synth_whisper_checkpoint(cfg, 0)
    if planted:
        ck = plant(cfg, ck)
    sup, beg = ckm.whisper_suppress_tokens(cfg), ckm.whisper_begin_suppress_tokens(cfg)
    return cfg, ck, sup, beg, layers_of(cfg, ck, sup, beg)


def token_ids(cfg, T, n, step):
    """The ids fed to an utterance of T encoder positions: codes of its first and last position, in turn (decoder cross-attention head 0)."""
    last = min(T, TOKEN_CODES) - 1
    return [(0, last)[(step + i) % 2] for i in range(n)]


def ratio(diff, budget):
    """stat(diff) over the budget, component by component (the larger of the two)."""
    s = stat(diff)
    return max(s[0] / budget[0], s[1] / budget[1])


# ---- traces: what a session tapped (or, on the CPU, what the exact functions chained give), and the stage functions over them ------------------------------
def dec_roundings(cfg, R, prompt=False, decode_gemm=True):
    """The rounding set of the form enqueue_step takes for R rows (the table in the module header)."""
    dgm = decode_gemm and R <= 64 and cfg.d_model % 256 == 0 and cfg.d_ffn % 256 == 0
    return (DEC_DGM if dgm else DEC_PLAIN) | (frozenset({"p"}) if prompt else frozenset())


def budget(exact, fn, roundings):
    """E_round: stat(exact - fn(rnd)), the larger over the rounding sets given, component by component (one set for bf16, F32_FORMS for the f32 session)."""
    st = [stat(exact - fn(rnd)) for rnd in roundings]
    return max(s[0] for s in st), max(s[1] for s in st)


def exceeds(diff, e_round, factor):
    """Both components of stat(diff) above factor x E_round (the condition on a planted mistake)."""
    s = stat(diff)
    return s[0] > factor * e_round[0] and s[1] > factor * e_round[1], (s[0] / e_round[0], s[1] / e_round[1])


def within(diff, e_round, factor=MARGIN):
    s = stat(diff)
    return s[0] <= factor * e_round[0] and s[1] <= factor * e_round[1], (s[0] / e_round[0], s[1] / e_round[1])


def cross_rows(k, v):
    """(K, V) [Ld][H][T][64] -> [T][2 * Ld * H * 64]: one row per encoder position."""
    kv = torch.stack([torch.as_tensor(k), torch.as_tensor(v)])
    return kv.permute(3, 0, 1, 2, 4).reshape(kv.shape[3], -1).numpy()


def decode_plan(cfg, lengths, n_prefill=N_PREFILL, n_steps=N_STEPS):
    """[(ids [B][n], pads or None)]: one prefill of n_prefill ids, then n_steps single ids, each utterance fed the codes of its first and last position."""
    plan = [(np.array([token_ids(cfg, T, n_prefill, 0) for T in lengths], np.int32), None)]
    for t in range(n_steps):
        plan.append((np.array([token_ids(cfg, T, 1, 1 + t + b) for b, T in enumerate(lengths)], np.int32), None))
    return plan


def prompt_plan(cfg, lengths, prompt_lens=PROMPT_LENS, n_steps=N_STEPS):
    """The same behind ragged prompts, left-padded to the longest (a pad slot holds id 0: csrc/whisper.hip prefill_prompts)."""
    n = max(prompt_lens)
    ids, pads = np.zeros((len(lengths), n), np.int32), np.array([n - p for p in prompt_lens], np.int32)
    for b, (T, p) in enumerate(zip(lengths, prompt_lens)):
        ids[b, n - p:] = token_ids(cfg, T, p, 1)           # (the first live id is not the pad slots' id 0)
    return [(ids, pads)] + decode_plan(cfg, lengths, 1, n_steps)[1:]


def prompts_of(plan):
    ids, pads = plan[0]
    return [ids[b, pads[b]:] for b in range(ids.shape[0])]


class Trace:
    """lengths: encoder positions per utterance; enc: {"stem", "enc{i}", "enc_out"} packed rows; cross: float64 [2][Ld][H][Mpad][64];
    steps: [{"ids" [B][n], "dec_in" [R][d], "dec" [Ld x [R][d]], "logits" [B][V]}]; pads [B] (zeros without a left-padded prompt)."""

    def __init__(self, cfg, lengths):
        self.cfg, self.lengths, self.rows = cfg, tuple(lengths), utterance_rows(lengths)
        self.enc, self.cross, self.steps, self.pads = {}, None, [], np.zeros(len(lengths), np.int64)

    def kv(self, b, l):
        r0, T = self.rows[b]
        return self.cross[0, l, :, r0:r0 + T], self.cross[1, l, :, r0:r0 + T]

    def slab_row(self, b, l, row):
        """(k, v) [H][64] of slab row `row` counted from the utterance's first row (pad_row: row = T); None past the slab."""
        r = self.rows[b][0] + row
        return (self.cross[0, l, :, r], self.cross[1, l, :, r]) if r < self.cross.shape[3] else None

    def hist(self, t):
        return sum(s["ids"].shape[1] for s in self.steps[:t])

    def layer_inputs(self, t, l, b):
        """The rows of sequence b that entered layer l at the steps 0 .. t."""
        out = []
        for s in self.steps[:t + 1]:
            n = s["ids"].shape[1]
            out.append((s["dec_in"] if l == 0 else s["dec"][l - 1])[b * n:(b + 1) * n])
        return out


def enc_stage(L, tr, i, u, rnd=frozenset(), mut=None):
    """`enc{i}` of utterance u from the trace's own rows of the stage before; mut: a name of ENC_MUTATIONS (None where it does not apply)."""
    r0, T = tr.rows[u]
    src = tr.enc["stem" if i == 0 else f"enc{i - 1}"]
    m = L.enc_mutation(mut, T) if mut else None
    if mut and m is None:
        return None
    foreign = None
    if mut == "foreign_key":
        cand = [v for v in range(len(tr.rows)) if v != u and tr.rows[v][1] > T // 2]
        if not cand:
            return None
        v0 = min(cand, key=lambda v: abs(v - u))
        foreign = src[tr.rows[v0][0]:tr.rows[v0][0] + tr.rows[v0][1]]
    return L.enc_layer(i, src[r0:r0 + T], rnd, m, foreign=foreign)


def cross_stage(L, tr, u, rnd=frozenset()):
    r0, T = tr.rows[u]
    return cross_rows(*L.cross(tr.enc[f"enc{tr.cfg.n_enc_layers - 1}"][r0:r0 + T], rnd))


def cross_got(tr, u):
    r0, T = tr.rows[u]
    return cross_rows(tr.cross[0, :, :, r0:r0 + T], tr.cross[1, :, :, r0:r0 + T])


def dec_stage(L, tr, t, l, b, rnd=frozenset(), mut=None, pad_row=None):
    """The live rows of `dec{l}` of sequence b at step t from the trace's own rows; mut: a name of SELF_MUTATIONS / CROSSATT_MUTATIONS (None: it does not apply).
    pad_row None: the trace's own slab row T."""
    pad, n, S0 = int(tr.pads[b]), tr.steps[t]["ids"].shape[1], tr.hist(t)
    if mut == "pad_slot" and (pad == 0 or l > 0) or mut == "causal_plus" and n == 1 or mut == "wrong_slot" and S0 - pad < 2:
        return None
    if mut == "pad_row":
        pad_row = pad_row if pad_row is not None else tr.slab_row(b, l, tr.rows[b][1])
        if pad_row is None or tr.rows[b][1] % 16 == 0:                 # (the row behind an aligned utterance belongs to the next one)
            return None
    if mut == "drop_last" and (tr.rows[b][1] < 2 or not (tr.steps[t]["ids"][b] == min(tr.rows[b][1], TOKEN_CODES) - 1).any()):
        return None                                                     # (only a row whose id addresses the last position looks there)
    out = L.dec_layer(l, tr.layer_inputs(t, l, b), tr.kv(b, l), pad, rnd, (mut,) if mut else None, pad_row=pad_row)
    return out[max(pad - S0, 0):]


def dec_got(tr, t, l, b):
    n, live0 = tr.steps[t]["ids"].shape[1], max(int(tr.pads[b]) - tr.hist(t), 0)
    return tr.steps[t]["dec"][l][b * n + live0:(b + 1) * n]


def head_stage(L, tr, t, rnd=frozenset(), mut=None):
    """(logits [B][V], which sequences the mutation applies to)."""
    B, n = tr.steps[t]["ids"].shape
    rows, ok = head_rows(tr.steps[t]["dec"][-1], B, n, mut)
    return L.head(rows, rnd), ok


def dec_in_stage(L, tr, t, rnd=frozenset(), mut=None):
    ids = tr.steps[t]["ids"]
    B, n = ids.shape
    pos = np.stack([positions_of(tr.hist(t), n, int(tr.pads[b]), mut) for b in range(B)])
    return L.dec_in(ids.reshape(-1), pos.reshape(-1), rnd)


def cpu_trace(L, cfg, lengths, plan, via=frozenset(), encoder_only=False, first=0):
    """The trace the exact functions give when chained from the oracle's stem rows (via: a rounding set to chain through instead)."""
    tr = Trace(cfg, lengths)
    total = sum(round_up(T, 16) for T in lengths)
    names = ["stem"] + [f"enc{i}" for i in range(cfg.n_enc_layers)] + ["enc_out"]
    for nm in names:
        tr.enc[nm] = np.zeros((total, cfg.d_model))
    with torch.inference_mode():
        for (r0, T), a in zip(tr.rows, batch_audios(cfg, lengths, first)):
            taps = {}
            L.orc.encode(a, taps)
            tr.enc["stem"][r0:r0 + T] = taps["stem"].numpy()
        Mpad = round_up(total, 128)
        pk, pv = L.cross(np.zeros((1, cfg.d_model)), via)
        tr.cross = torch.stack([pk, pv]).expand(2, cfg.n_dec_layers, cfg.n_heads, Mpad, 64).clone()       # every pad row: the projection of a row of zeros
        for u, (r0, T) in enumerate(tr.rows):
            for i in range(cfg.n_enc_layers):
                tr.enc[f"enc{i}"][r0:r0 + T] = enc_stage(L, tr, i, u, via)
            last = tr.enc[f"enc{cfg.n_enc_layers - 1}"][r0:r0 + T]
            tr.enc["enc_out"][r0:r0 + T] = L.enc_out(last)
            k, v = L.cross(last, via)
            tr.cross[0, :, :, r0:r0 + T], tr.cross[1, :, :, r0:r0 + T] = k, v
        if encoder_only:
            return tr
        for t, (ids, pads) in enumerate(plan):
            if pads is not None:
                tr.pads = np.asarray(pads, np.int64)
            B, n = ids.shape
            step = {"ids": ids, "dec": []}
            tr.steps.append(step)
            step["dec_in"] = dec_in_stage(L, tr, t, via)
            for l in range(cfg.n_dec_layers):
                out = np.zeros((B * n, cfg.d_model))
                step["dec"].append(out)
                for b in range(B):
                    live = dec_stage(L, tr, t, l, b, via)
                    out[(b + 1) * n - live.shape[0]:(b + 1) * n] = live
            step["logits"] = head_stage(L, tr, t, via)[0]
    return tr


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------------
TINY_LENGTHS = (113, 17, 40)
DEC_CYCLE = (17, 1, 128, 40, 16, 113)


def dec_lengths(B):
    """Encoder positions under a decoder batch of B sequences: the three attention geometries at B = 3, short utterances above."""
    return (300, 17, 129) if B == 3 else tuple(DEC_CYCLE[b % len(DEC_CYCLE)] for b in range(B))


D256, TINY = "whisper_d256_test", "whisper_tiny_test"
MISTAKE_CASES = {                                                # where the GPU test plants the mistakes: (geometry, encoder positions, None | "steps" | "prompts")
    "enc_le128": (D256, ENC_BATCHES["le128"], None), "enc_le256": (D256, ENC_BATCHES["le256"], None), "enc_gt256": (D256, ENC_BATCHES["gt256"], None),
    "enc_tiny": (TINY, TINY_LENGTHS, None),
    "dec_b3": (D256, dec_lengths(3), "steps"), "dec_b33": (D256, dec_lengths(33), "steps"), "dec_prompts": (D256, dec_lengths(3), "prompts"),
    "dec_tiny": (TINY, TINY_LENGTHS, "steps"),
}


def relied_on(mut, case):
    """Whether the GPU test relies on this mutation in this case (whisper_tiny_test has two heads: no head looks behind the causal bound or two positions back)."""
    if mut == "mask_256":
        return case == "enc_gt256"
    if mut in ("pad_slot", "pad_pos"):
        return case == "dec_prompts"
    if mut in ("causal_plus", "wrong_slot"):
        return case != "dec_tiny"
    return True


# ---- the functions of the module header, by name (L = layers_of(cfg, ck) or setup(...)[4]) -------------------------------------------------------------------
def enc_layer_exact(L, i, rows):
    return L.enc_layer(i, rows)


def enc_layer_rounded(L, i, rows):
    return L.enc_layer(i, rows, ENC_ROUNDINGS)


def enc_out_exact(L, rows):
    return L.enc_out(rows)


def cross_exact(L, rows):
    return L.cross(rows)


def cross_rounded(L, rows):
    return L.cross(rows, CROSS_ROUNDINGS)


def dec_in_exact(L, ids, positions):
    return L.dec_in(ids, positions)


def dec_layer_exact(L, l, xs, kv, pad=0):
    return L.dec_layer(l, xs, kv, pad)


def dec_layer_rounded(L, l, xs, kv, pad=0, roundings=DEC_DGM):
    return L.dec_layer(l, xs, kv, pad, roundings)


def head_exact(L, rows):
    return L.head(rows)


def head_rounded(L, rows):
    return L.head(rows, HEAD_ROUNDINGS)
