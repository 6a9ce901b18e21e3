"""Float64 statement of the streaming Paraformer chunk step, its bf16 rounding budget, inputs on which state errors show, and the planted mistakes.

The chunk step (oracle/paraformer_streaming_oracle.py: `encoder_step`, `decoder_step`) exists as per-launch kernels, as one cluster launch for encoder layers
1.. (csrc/stream_layers.hip) and one for every decoder block (csrc/stream_dec.hip). This module restates the oracle line for line in float64, on the oracle's
own folded f32 weights, with PER-STREAM STATE HELD BY THE REFERENCE, and split at the session's taps so that no stage inherits another stage's noise or
fire decisions:

  front_end        one stream's audio chunk -> its 13 `enc_in` rows (f32, the oracle's own front end; the CPU tests make inputs with it)
  encoder_exact    13 `enc_in` rows -> the 13 `enc_out` rows behind after_norm; state: per-layer K/V history, [-(36 + 4):-4] of history ++ chunk
  cif_fire         13 `enc_out` rows -> the fired frames (f32, the oracle's unrolled integrate-and-fire; CPU tests only: the GPU tests follow the session's fires)
  decoder_exact    13 encoder rows + n fired frames -> n logits rows; state: 10-row FSMN carry per layer, 9-row cross K/V cache, advanced only when n > 0
  *_rounded        the same functions with the rounding points the kernels document; they exist ONLY to measure E_round = stat(exact - rounded), a kernel is
                   compared with the exact functions. Switches (a path is a set of them, PATH_ROUNDINGS):
                     "op"          the bf16 operand of every GEMM (normalised rows, ctx, hidden rows, the decoder's normalised 2048-wide rows)
                     "w"           GEMM weights bf16, rounded AFTER the LayerNorm affine was folded in (arena.py: _fold64 -> ArenaWriter.weight)
                     "qkv"         q|k|v are bf16 tensors, hence bf16 histories and caches; the decoder's q and k|v likewise
                     "ctx"         the attention context is bf16
                     "hid"         the encoder FFN's hidden rows are bf16 (the decoder's stay an f32 slab, normalised over 2048, then a bf16 operand: "op")
                     "enc_lo"      the decoder's k|v projection multiplies the bf16 copy of the encoder rows
                     "ln2_folded"  per-launch encoder layers evaluate the second LayerNorm inside FFN-1 from the bf16 copy of the rows + their statistics
                                   (ASR_LN_FUSED=1; on the fused paths this is layer 0, the only per-launch layer)
                     "fused_enc"   encoder layers >= 1 run in stream_layers_kernel: the soft-max weights are the bf16 operand of P V (its header)
                     "fused_dec"   the decoder runs in stream_dec_kernel: its soft-max weights are the bf16 operand of P V as well (its header)
                   The residual stream, the FSMN, the FSMN carry, soft-max and every LayerNorm statistic stay unrounded (f32 on the GPU).
  case             (cfg, checkpoint, chunk) of the two fixed cases: sharpened attention (sharpen), three heads of layer 1 that attend by position so that the
                   oldest row of a full history and the newest history row are looked at in every chunk of every stream (plant_positions), "sparse" / "dense"
                   fire counts
  mutations        of the exact functions: the planted mistakes a comparison must catch (ENC_MUTATIONS, DEC_MUTATIONS)
  schedule         the eight chunk steps shared by the CPU and GPU tests (SCHEDULE); encoder_runs / decoder_runs drive per-stream reference states through them
"""
import functools
import hashlib

import numpy as np
import torch

from conftest import sub
from helpers import kaldi_audio, load_golden
from oracle.paraformer_streaming_oracle import ParaformerStreamingOracle
from sanm_block_ref import MARGIN, bf16, stat                                    # noqa: F401  (re-exported: the tests take them from here)

F = torch.nn.functional
F64 = torch.float64

BASE_ROUNDINGS = frozenset({"op", "w", "qkv", "ctx", "hid", "enc_lo"})
PATH_ROUNDINGS = {
    "per_launch_separate_ln": BASE_ROUNDINGS,
    "per_launch_folded_ln": BASE_ROUNDINGS | {"ln2_folded"},
    "fused_encoder": BASE_ROUNDINGS | {"ln2_folded", "fused_enc"},
    "fused_both": BASE_ROUNDINGS | {"ln2_folded", "fused_enc", "fused_dec"},
    "fused_old_placement": BASE_ROUNDINGS | {"ln2_folded", "fused_enc", "fused_dec"},
}

# ---- the schedule -----------------------------------------------------------------------------------------------------------------------------
MAX_STREAMS = 12
N_STEPS = 8
STREAM_IDS = (11, 0, 7, 3, 9, 1, 5, 2, 8)                       # clip i is stream STREAM_IDS[i]: not dense, not in slot order
AUDIO_SEED = 7300
RESET_STREAM = 7
# per step: (stream ids to reset before it, stream ids that advance, in slot order)
SCHEDULE = (
    ((), STREAM_IDS), ((), STREAM_IDS), ((), STREAM_IDS),       # 0-2: history empty, then partial
    ((), (9, 0, 5, 11, 2)),                                     # 3: a subset (slot != id); from here on one launch holds different history lengths
    ((), STREAM_IDS),                                           # 4: full histories for the streams that never paused, 27 rows for the others
    ((RESET_STREAM,), (7, 3, 11, 8, 0)),                        # 5: length 0 beside 36; another subset, the reset stream in it
    ((), STREAM_IDS), ((), STREAM_IDS),                         # 6-7: histories rolling
)
MIXED_STEPS = (4, 5, 6, 7)                                      # the steps whose launch holds more than one history length
NO_ROLL_STEP = 4                                                # the step of the "no_roll" mutation

# sharpening factors on the q and k rows (encoder layers >= 1) and on src_attn.linear_q (decoder), chosen on the CPU (test_paraformer_stream_ref_cpu.py asserts
# what they were chosen for: mean top probability per head in 0.5 .. 0.9 over the schedule, every key class the top key of some query)
ENC_SHARPEN = 4.0
DEC_SHARPEN = 14.0
CIF_BIAS = {"sparse": -2.4, "dense": 4.2}                       # fire counts per chunk: 0 and 1 / 8 and 9 (asserted by the CPU test)

ENC_MUTATIONS = ("hist_shift", "mask_oldest", "roll_paused", "no_roll", "stale_reset", "fsmn_tap_lo", "fsmn_tap_hi", "pad_keys")
DEC_MUTATIONS = ("carry_on_empty", "carry_n_minus_1", "cache_window", "cache_on_empty", "pad_keys")
"""The planted mistakes (each changes the EXACT functions in one place):
  encoder  hist_shift       the history window shifted by one row: [-(36 + 4) - 1:-4 - 1] kept
           mask_oldest      the oldest history key masked once the history is full
           roll_paused      the history of a stream that sat a step out rolled anyway (nine rows of zeros appended, the last 36 kept)
           no_roll          the history not rolled on step NO_ROLL_STEP
           stale_reset      a reset stream still reading its old history
           fsmn_tap_lo/hi   FSMN tap -5 of row 0 / tap +5 of row 12 taking the neighbouring row of the chunk instead of zero
           pad_keys         keys 13..15 of the slot admitted: three keys whose k|v are those of a row that is zero behind the LayerNorm (the bias)
  decoder  carry_on_empty   the FSMN carry advanced (by one row of zeros) on a chunk that fired nothing
           carry_n_minus_1  the carry advanced by n - 1
           cache_window     the cross K/V cache keeping [-13:-4] instead of [-9:]
           cache_on_empty   the cache advanced on a chunk that fired nothing
           pad_keys         16 instead of 13 chunk keys (as above)"""


def _depthwise(rows, w):
    """F.conv1d(rows.t()[None], w, groups=d)[0].t() without padding, tap by tap (the grouped float64 convolution is slow out of all proportion)."""
    taps = w.shape[2]
    n = rows.shape[0] - taps + 1
    out = torch.zeros(n, rows.shape[1], dtype=rows.dtype)
    for j in range(taps):
        out += rows[j:j + n] * w[:, 0, j]
    return out


class StreamRef:
    """The chunk step of one (cfg, checkpoint, chunk) in float64."""

    def __init__(self, cfg, ck, chunk):
        self.cfg, self.chunk = cfg, int(chunk)
        self.orc = o = ParaformerStreamingOracle(cfg, ck, chunk=self.chunk)
        assert (o.B, o.C, o.en_keep, o.de_keep, o.fsmn_hist) == (9, 4, 36, 9, 10)
        gemm = {"wqkv", "wo", "w1", "w2", "wq", "wkv"}
        t64 = lambda v: v.to(F64) if torch.is_tensor(v) else (tuple(t.to(F64) for t in v) if isinstance(v, tuple) else v)
        lo = lambda L: {k: (bf16(v) if k in gemm else t64(v)) for k, v in L.items()}
        self.enc = {False: [{k: t64(v) for k, v in L.items()} for L in o.enc], True: [lo(L) for L in o.enc]}
        self.dec = {False: [{k: t64(v) for k, v in L.items()} for L in o.dec], True: [lo(L) for L in o.dec]}
        self.dec3 = {False: [{k: t64(v) for k, v in L.items()} for L in o.dec3], True: [lo(L) for L in o.dec3]}
        self.dec_wf = [w.to(F64) for w in o.dec_wf_raw]
        self.w_out = {False: o.w_out.to(F64), True: bf16(o.w_out)}
        self.b_out = o.b_out.to(F64)
        self.after = (o.ck["encoder.after_norm.weight"].to(F64), o.ck["encoder.after_norm.bias"].to(F64))

    # ---- state ------------------------------------------------------------------------------------------------------------------------------
    def init_state(self):
        c = self.cfg
        H, hd, d = c.n_heads, c.d_head, c.d_model
        n_en = c.n_enc0 + c.n_enc
        z = lambda: torch.zeros(H, 0, hd, dtype=F64)
        return dict(en_k=[z() for _ in range(n_en)], en_v=[z() for _ in range(n_en)],
                    de_fsmn=[torch.zeros(d, self.orc.fsmn_hist, dtype=F64) for _ in range(c.n_dec)], de_k=[z() for _ in range(c.n_dec)], de_v=[z() for _ in range(c.n_dec)],
                    fe=self.orc.init_state())

    def reset(self, st, mut=None):
        """The state of a stream after `reset`."""
        new = self.init_state()
        if mut == "stale_reset":
            new["en_k"], new["en_v"] = st["en_k"], st["en_v"]
        return new

    def sit_out(self, st, mut=None):
        """A step in which the stream does not advance: nothing happens to its state."""
        if mut == "roll_paused":
            o = self.orc
            for li in range(len(st["en_k"])):
                for name in ("en_k", "en_v"):
                    h = st[name][li]
                    st[name][li] = torch.cat([h, torch.zeros(h.shape[0], o.B, h.shape[2], dtype=F64)], 1)[:, -o.en_keep:].clone()

    def history_len(self, st):
        return int(st["en_k"][0].shape[1])

    # ---- front end and fire (f32, the oracle's own lines) ------------------------------------------------------------------------------------
    def front_end(self, st, audio_chunk):
        """encoder_step up to the encoder's input: fbank, LFR, CMVN + positions, the carried rows in front -> [13][560] f32."""
        o, c, fe = self.orc, self.cfg, st["fe"]
        with torch.inference_mode():
            mel = o.fbank(torch.as_tensor(np.asarray(audio_chunk, dtype=np.float32).reshape(-1)))
            nf = mel.shape[0]
            idx = (torch.arange(0, o.B * c.lfr_n, c.lfr_n).unsqueeze(1) + torch.arange(c.lfr_m) - (c.lfr_m - 1) // 2).clamp(min=0, max=nf - 1)
            feats = (mel[idx].reshape(o.B, c.feat_dim) + o.means) * o.vars
            feats = feats + o.pos[fe["start"]:fe["start"] + o.B]
            fe["start"] += o.B
            x = torch.cat([fe["prev"], feats], 0)
            fe["prev"] = x[-(o.A + o.C):].clone()
            return x.numpy()

    def cif_fire(self, st, enc_out_rows):
        """encoder_step behind after_norm: the CIF weights and the unrolled integrate-and-fire with the carried state -> the fired frames [n][d] f32."""
        o, c, fe = self.orc, self.cfg, st["fe"]
        with torch.inference_mode():
            enc_out = torch.as_tensor(np.asarray(enc_out_rows, dtype=np.float32))
            conv = torch.relu(F.conv1d(enc_out.t().unsqueeze(0), o.ck["predictor.cif_conv1d.weight"], o.ck["predictor.cif_conv1d.bias"], padding=c.cif_kernel // 2))[0].t()
            alphas = torch.sigmoid(conv @ o.ck["predictor.cif_output.weight"].t() + o.ck["predictor.cif_output.bias"]).squeeze(-1)
            one = torch.tensor(1.0)
            ca, ch = fe["cif_alphas"].clone(), fe["cif_hidden"]
            cond_a = (ca < one).float()
            cond_b = one - cond_a
            saves = [cond_b]
            frames = ca * ch * cond_a + ch * cond_b
            fl = [frames]
            ca = ca - cond_b
            frames = frames * cond_a + ca * ch * cond_b
            for t in range(o.A, o.A + o.B):
                alpha, hidden = alphas[t], enc_out[t]
                thr = one - ca
                cond_a = (alpha < thr).float()
                cond_b = one - cond_a
                saves.append(cond_b)
                frames = (frames + alpha * hidden) * cond_a + (frames + thr * hidden) * cond_b
                fl.append(frames)
                ca = ca + alpha
                ca = ca - cond_b
                frames = frames * cond_a + ca * hidden * cond_b
            fl = torch.stack(fl)
            fe["cif_hidden"] = fl[-1] / ca
            fe["cif_alphas"] = ca
            fired = torch.nonzero(torch.stack(saves)).squeeze(1)
            return fl[fired].numpy()

    # ---- encoder layers + after_norm ----------------------------------------------------------------------------------------------------------
    def encoder(self, st, enc_in_rows, rnd=frozenset(), mut=None, trace=None):
        """13 `enc_in` rows -> 13 `enc_out` rows; st's K/V histories advance. trace: a list that receives (layer, history length, probabilities [H][13][keys])."""
        o, c = self.orc, self.cfg
        d, H, hd = c.d_model, c.n_heads, c.d_head
        r = lambda name, t: bf16(t) if name in rnd else t
        pad = (c.fsmn_kernel - 1) // 2
        heads = lambda z: z.reshape(z.shape[0], H, hd).transpose(0, 1)
        with torch.inference_mode():
            x = torch.as_tensor(np.asarray(enc_in_rows, dtype=np.float64))
            T = x.shape[0]
            assert T == o.B + o.C
            for li, L in enumerate(self.enc["w" in rnd]):
                fused = "fused_enc" in rnd and li >= 1
                qkv = r("qkv", r("op", F.layer_norm(x, (L["in_size"],))) @ L["wqkv"].t() + L["bqkv"])
                q, k, v = qkv.split(d, dim=1)
                qh, kh, vh = heads(q), heads(k), heads(v)
                n_hist = st["en_k"][li].shape[1]
                k_all, v_all = torch.cat([st["en_k"][li], kh], 1), torch.cat([st["en_v"][li], vh], 1)
                if mut != "no_roll":
                    lo, hi = -(o.en_keep + o.en_drop), -o.en_drop
                    if mut == "hist_shift":
                        lo, hi = lo - 1, hi - 1
                    st["en_k"][li], st["en_v"][li] = k_all[:, lo:hi].clone(), v_all[:, lo:hi].clone()
                if mut == "pad_keys":
                    kp, vp = r("qkv", L["bqkv"][d:2 * d]), r("qkv", L["bqkv"][2 * d:])
                    k_all = torch.cat([k_all, heads(kp[None].expand(3, d))], 1)
                    v_all = torch.cat([v_all, heads(vp[None].expand(3, d))], 1)
                s = qh @ k_all.transpose(1, 2)
                if mut == "mask_oldest" and n_hist == o.en_keep:
                    s = s.clone()
                    s[:, :, 0] = -float("inf")
                p = torch.softmax(s, dim=-1)
                if trace is not None:
                    trace.append((li, n_hist, p.numpy()))
                ctx = r("ctx", ((bf16(p) if fused else p) @ v_all).transpose(0, 1).reshape(T, d))
                mem = _depthwise(F.pad(v, (0, 0, pad, pad)), L["wf"])                                    # zero padded; identity folded into the centre tap
                if mut == "fsmn_tap_lo":
                    mem = mem.clone()
                    mem[0] += L["wf"][:, 0, 0] * v[1]
                if mut == "fsmn_tap_hi":
                    mem = mem.clone()
                    mem[T - 1] += L["wf"][:, 0, 2 * pad] * v[T - 2]
                att = r("op", ctx) @ L["wo"].t() + L["bo"] + mem
                x = x + att if li > 0 else att
                if "ln2_folded" in rnd and not fused:
                    h2 = F.layer_norm(bf16(x), (d,))              # rstd (x_lo W^T - mean colsum(W)) + b: bf16 rows and their statistics, no rounding behind the normalisation
                else:
                    h2 = r("op", F.layer_norm(x, (d,)))
                hid = r("hid", torch.relu(h2 @ L["w1"].t() + L["b1"]))
                x = x + r("op", hid) @ L["w2"].t() + L["b2"]
            return F.layer_norm(x, (d,), self.after[0], self.after[1]).numpy()

    # ---- decoder ----------------------------------------------------------------------------------------------------------------------------------
    def _dec_ffn(self, L, dec, r):
        c = self.cfg
        hid = torch.relu(r("op", F.layer_norm(dec, (c.d_model,))) @ L["w1"].t() + L["b1"])                 # an f32 slab on the GPU
        return r("op", F.layer_norm(hid, (c.d_dec_ffn,))) @ L["w2"].t() + L["b2"]

    def decoder(self, st, enc_out_rows, list_frame_rows, rnd=frozenset(), mut=None, trace=None):
        """13 encoder rows and the n > 0 fired frames -> n logits rows; st's FSMN carries and cross K/V caches advance."""
        o, c = self.orc, self.cfg
        d, H, hd = c.d_model, c.n_heads, c.d_head
        r = lambda name, t: bf16(t) if name in rnd else t
        heads = lambda z: z.reshape(z.shape[0], H, hd).transpose(0, 1)
        with torch.inference_mode():
            enc_out = torch.as_tensor(np.asarray(enc_out_rows, dtype=np.float64))
            dec = torch.as_tensor(np.asarray(list_frame_rows, dtype=np.float64))
            n, T = dec.shape[0], enc_out.shape[0]
            assert n > 0 and T == o.B + o.C
            enc_op = r("enc_lo", enc_out)
            for li, L in enumerate(self.dec["w" in rnd]):
                x = self._dec_ffn(L, dec, r)
                x = F.layer_norm(x, (d,), L["n2"][0], L["n2"][1])
                cat = torch.cat([st["de_fsmn"][li], x.t()], 1)
                st["de_fsmn"][li] = (cat[:, :-1] if mut == "carry_n_minus_1" else cat)[:, -o.fsmn_hist:].clone()
                y = _depthwise(cat.t(), self.dec_wf[li]) + x + dec                                       # valid convolution over [10 carried rows | tokens]
                q = heads(r("qkv", r("op", F.layer_norm(y, (d,))) @ L["wq"].t() + L["bq"]))
                kv = r("qkv", enc_op @ L["wkv"].t() + L["bkv"])
                k_all, v_all = torch.cat([st["de_k"][li], heads(kv[:, :d])], 1), torch.cat([st["de_v"][li], heads(kv[:, d:])], 1)
                self._roll_cache(st, li, k_all, v_all, mut)
                if mut == "pad_keys":
                    bkv = r("qkv", L["bkv"])
                    k_all = torch.cat([k_all, heads(bkv[None, :d].expand(3, d))], 1)
                    v_all = torch.cat([v_all, heads(bkv[None, d:].expand(3, d))], 1)
                p = torch.softmax(q @ k_all.transpose(1, 2), dim=-1)
                if trace is not None:
                    trace.append((li, k_all.shape[1] - T, p.numpy()))
                ctx = r("ctx", ((bf16(p) if "fused_dec" in rnd else p) @ v_all).transpose(0, 1).reshape(n, d))
                dec = y + r("op", ctx) @ L["wo"].t() + L["bo"]
            for L in self.dec3["w" in rnd]:
                dec = self._dec_ffn(L, dec, r)
            return (r("op", F.layer_norm(dec, (d,))) @ self.w_out["w" in rnd].t() + self.b_out).numpy()

    def _roll_cache(self, st, li, k_all, v_all, mut):
        o = self.orc
        if mut == "cache_window":
            lo, hi = -(o.de_keep + o.C), -o.C
            st["de_k"][li], st["de_v"][li] = k_all[:, lo:hi].clone(), v_all[:, lo:hi].clone()
        else:
            st["de_k"][li], st["de_v"][li] = k_all[:, -o.de_keep:].clone(), v_all[:, -o.de_keep:].clone()

    def decoder_idle(self, st, enc_out_rows, rnd=frozenset(), mut=None):
        """A chunk that fired nothing: the decoder does not run and its state stays."""
        o, c = self.orc, self.cfg
        d, H, hd = c.d_model, c.n_heads, c.d_head
        if mut == "carry_on_empty":
            for li in range(c.n_dec):
                st["de_fsmn"][li] = torch.cat([st["de_fsmn"][li][:, 1:], torch.zeros(d, 1, dtype=F64)], 1)
        if mut == "cache_on_empty":
            heads = lambda z: z.reshape(z.shape[0], H, hd).transpose(0, 1)
            with torch.inference_mode():
                enc_out = torch.as_tensor(np.asarray(enc_out_rows, dtype=np.float64))
                for li, L in enumerate(self.dec["w" in rnd]):
                    kv = enc_out @ L["wkv"].t() + L["bkv"]
                    self._roll_cache(st, li, torch.cat([st["de_k"][li], heads(kv[:, :d])], 1), torch.cat([st["de_v"][li], heads(kv[:, d:])], 1), None)


def states_differ(a, b, keys):
    """Whether two reference states hold different tensors under `keys` (a mutation that acts through the state applies wherever they do)."""
    for k in keys:
        for x, y in zip(a[k], b[k]):
            if x.shape != y.shape or not torch.equal(x, y):
                return True
    return False


ENC_STATE, DEC_STATE = ("en_k", "en_v"), ("de_fsmn", "de_k", "de_v")


# ---- the functions the issue names -----------------------------------------------------------------------------------------------------------------
_refs = {}


def default_chunk():
    return int(load_golden("paraformer_streaming_large")["chunk"])


def ref_of(cfg, ck, chunk=None):
    chunk = default_chunk() if chunk is None else int(chunk)
    key = (cfg, id(ck), chunk)
    if key not in _refs:
        _refs[key] = (ck, StreamRef(cfg, ck, chunk))            # (holds ck, so the id stays its own)
    return _refs[key][1]


def init_state(cfg, ck):
    return ref_of(cfg, ck).init_state()


def front_end(cfg, ck, state, audio_chunk):
    return ref_of(cfg, ck).front_end(state, audio_chunk)


def encoder_exact(cfg, ck, state, enc_in_rows, mut=None, trace=None):
    return ref_of(cfg, ck).encoder(state, enc_in_rows, mut=mut, trace=trace)


def encoder_rounded(cfg, ck, state, enc_in_rows, roundings):
    return ref_of(cfg, ck).encoder(state, enc_in_rows, rnd=frozenset(roundings))


def decoder_exact(cfg, ck, state, enc_out_rows, list_frame_rows, mut=None, trace=None):
    return ref_of(cfg, ck).decoder(state, enc_out_rows, list_frame_rows, mut=mut, trace=trace)


def decoder_rounded(cfg, ck, state, enc_out_rows, list_frame_rows, roundings):
    return ref_of(cfg, ck).decoder(state, enc_out_rows, list_frame_rows, rnd=frozenset(roundings))


# ---- the references driven through the schedule --------------------------------------------------------------------------------------------------------
# A record is what one run of the schedule took in, per step a dict {stream id: {"enc_in": [13][560], "enc_out": [13][d], "frames": [n][d]}} of the streams that
# advanced: the GPU tests fill it from the session's taps (so the references follow the session's own rows and fire decisions), the CPU tests from the
# references themselves (reference_record).
def reference_record(cfg, ck):
    """The schedule run by the references alone: enc_in from front_end, enc_out from encoder_exact (as f32, like the tap), frames from cif_fire."""
    ref = ref_of(cfg, ck)
    st = {s: ref.init_state() for s in STREAM_IDS}
    record = []
    for resets, sids, chunks in schedule_chunks(ref.chunk):
        for s in resets:
            st[s] = ref.reset(st[s])
        step = {}
        for s, a in zip(sids, chunks):
            enc_in = ref.front_end(st[s], a)
            enc_out = ref.encoder(st[s], enc_in).astype(np.float32)
            step[s] = dict(enc_in=enc_in, enc_out=enc_out, frames=ref.cif_fire(st[s], enc_out))
        record.append(step)
    return record


_enc_runs = {}


def _record_key(record, field):
    h = hashlib.sha1()
    for step in record:
        for s in sorted(step):
            h.update(np.int64(s).tobytes())
            h.update(np.ascontiguousarray(step[s][field]).tobytes())
    return h.hexdigest()


def _snapshot(st, keys):
    return {k: list(st[k]) for k in keys}                       # (the tensors of a state are replaced, never written in place)


def _drive(ref, record, keys, reset_mut, idle, active):
    """One set of per-stream states through SCHEDULE: resets, then idle(state, stream, rows or None) for the streams that do not advance, then
    active(step, stream, state, rows) for those that do, in slot order."""
    st = {s: ref.init_state() for s in STREAM_IDS}
    for step, ((resets, sids), rows) in enumerate(zip(SCHEDULE, record)):
        assert set(rows) == set(sids), step
        for s in resets:
            st[s] = ref.reset(st[s], reset_mut)
        for s in STREAM_IDS:
            if s not in sids:
                idle(st[s])
        for s in sids:
            active(step, s, st[s], rows[s])


def encoder_runs(cfg, ck, record, roundings, trace=None):
    """{(step, stream): dict(exact, rounded, e_round, len, before)} over the record's enc_in rows: per-stream exact and rounded states go through SCHEDULE side
    by side. Cached on the rows (the encoder's inputs do not depend on the path or on the fire counts)."""
    ref, rnd = ref_of(cfg, ck), frozenset(roundings)
    base = (id(ck["encoder.after_norm.weight"]), _record_key(record, "enc_in"))          # (the two cases share the encoder's arrays, and the cached checkpoint holds them)
    if trace is None and (base, rnd) in _enc_runs:
        return _enc_runs[(base, rnd)]

    def exact(step, s, st, rows):
        exact_out[(step, s)] = dict(len=ref.history_len(st), before=_snapshot(st, ENC_STATE), exact=ref.encoder(st, rows["enc_in"], trace=trace))

    def rounded(step, s, st, rows):
        e = out[(step, s)] = dict(exact_out[(step, s)])
        e["rounded"] = ref.encoder(st, rows["enc_in"], rnd=rnd)
        e["e_round"] = stat(e["exact"] - e["rounded"])

    if trace is None and base in _enc_runs:
        exact_out = _enc_runs[base]
    else:
        exact_out = {}
        _drive(ref, record, ENC_STATE, None, lambda st: None, exact)
    out = {}
    _drive(ref, record, ENC_STATE, None, lambda st: None, rounded)
    if trace is None:
        _enc_runs[base], _enc_runs[(base, rnd)] = exact_out, out
    return out


def encoder_mutated(cfg, ck, record, base, mut):
    """{(step, stream): (enc_out of the mutated exact reference, whether the mutation applies there)}: it applies where it acts directly or where the state it
    left behind differs from the exact one (`base`: encoder_runs of the same record)."""
    ref = ref_of(cfg, ck)
    assert mut in ENC_MUTATIONS
    out = {}

    def active(step, s, st, rows):
        e = base[(step, s)]
        direct = mut in ("fsmn_tap_lo", "fsmn_tap_hi", "pad_keys") or (mut == "mask_oldest" and e["len"] == ref.orc.en_keep)
        applies = direct or states_differ(e["before"], st, ENC_STATE)
        m = mut if (mut != "no_roll" or step == NO_ROLL_STEP) else None
        out[(step, s)] = (ref.encoder(st, rows["enc_in"], mut=m), applies)

    _drive(ref, record, ENC_STATE, mut, lambda st: ref.sit_out(st, mut), active)
    return out


def decoder_runs(cfg, ck, record, roundings, trace=None):
    """The same for the decoder, over the record's enc_out rows and fired frames; entries exist for the (step, stream) that fired. A stream that fired nothing
    advances no decoder state."""
    ref, rnd = ref_of(cfg, ck), frozenset(roundings)
    out = {}

    def exact(step, s, st, rows):
        if rows["frames"].shape[0]:
            out[(step, s)] = e = dict(n=int(rows["frames"].shape[0]), before=_snapshot(st, DEC_STATE))
            e["exact"] = ref.decoder(st, rows["enc_out"], rows["frames"], trace=trace)

    def rounded(step, s, st, rows):
        if rows["frames"].shape[0]:
            e = out[(step, s)]
            e["rounded"] = ref.decoder(st, rows["enc_out"], rows["frames"], rnd=rnd)
            e["e_round"] = stat(e["exact"] - e["rounded"])

    _drive(ref, record, DEC_STATE, None, lambda st: None, exact)
    _drive(ref, record, DEC_STATE, None, lambda st: None, rounded)
    return out


def decoder_mutated(cfg, ck, record, base, mut):
    ref = ref_of(cfg, ck)
    assert mut in DEC_MUTATIONS
    out = {}

    def active(step, s, st, rows):
        if rows["frames"].shape[0] == 0:
            ref.decoder_idle(st, rows["enc_out"], mut=mut)
            return
        applies = mut == "pad_keys" or states_differ(base[(step, s)]["before"], st, DEC_STATE)
        out[(step, s)] = (ref.decoder(st, rows["enc_out"], rows["frames"], mut=mut), applies)

    _drive(ref, record, DEC_STATE, None, lambda st: None, active)
    return out


# ---- the fixed cases --------------------------------------------------------------------------------------------------------------------------------
def sharpen(cfg, ck, enc=ENC_SHARPEN, dec=DEC_SHARPEN):
    """A copy of ck with the q and k rows (weights and biases) of encoder layers >= 1 scaled by `enc` and the decoder's src_attn.linear_q by `dec`: the synthetic
    weights give a nearly flat soft-max, in which one wrong key moves the output by less than bf16 rounding does."""
    out = dict(ck)
    d = cfg.d_model
    for i in range(cfg.n_enc):
        for leaf in ("weight", "bias"):
            k = f"encoder.encoders.{i}.self_attn.linear_q_k_v.{leaf}"
            a = ck[k].copy()
            a[:2 * d] *= np.float32(enc)
            out[k] = a
    for i in range(cfg.n_dec):
        for leaf in ("weight", "bias"):
            k = f"decoder.decoders.{i}.src_attn.linear_q.{leaf}"
            out[k] = (ck[k] * np.float32(dec)).astype(np.float32)
    return out


N_FREQ = 64                                                     # the 64 fastest sinusoids of the position table: one head's 128 dims
PLANT_OFFSETS = (36, 1, 36)                                     # heads 0 and 2 look 36 rows back (row 0: the OLDEST row of a full history), head 1 one row back (row 0: the NEWEST history row)
PLANT_SCALE = 1.5                                               # the planted score is PLANT_SCALE / (s_i s_j) sum_f cos(..): top probabilities 0.45 (heads 0, 2: partial histories hold no target) and 0.75
PLANT_ZERO_ROWS = (10.0, 0.0, 10.0)                             # heads 0 and 2 keep the all-zero rows in front of a stream's first chunk in view (plant_positions)


def plant_positions(cfg, ck, scale=PLANT_SCALE):
    """Heads 0, 1 and 2 of encoder layer 1 attend by POSITION, for every stream and step alike: query row i scores sum_f cos(w_f (p_i - delta - p_j)) on key row j
    (p: the rows' absolute positions, delta = PLANT_OFFSETS[head]). Plain scaling leaves it to chance whether any query of a (stream, step) looks at the one key a
    mistake in the history window moves; this makes row 0 of every chunk look at the oldest row of a full history (heads 0, 2) and at the newest history row (head 1).

    How the positions get there. enc_in = (mel + means) vars + positions: with cmvn_vars zeroed in 130 of the 560 columns those columns hold the position table
    alone. Layer 0 copies them into channels 0 .. 129 of its output through the v rows and the FSMN's identity tap (FSMN taps, out-projection rows, FFN-2 rows
    and their biases of those channels are zero): behind LayerNorm(560) channel 2 f is (sin w_f p - sin w_279 p) / s, channel 2 f + 1 is (cos w_f p - cos w_279 p)
    / s, channel 128 is (cos w_279 p - sin w_279 p) / s ~ 1 / s, channel 129 is zero (w_279 = 1e-4: a constant over the rows of a clip). Layer 1 reads
    sin and cos of w_f p from them by combinations whose coefficients sum to zero, so its own LayerNorm's mean cancels; the row scales s stay (a few percent)."""
    out = dict(ck)
    d, hd, feat = cfg.d_model, cfg.d_head, cfg.feat_dim
    half = feat // 2
    lo_f = half - 1
    assert 2 * N_FREQ == hd and cfg.n_heads > len(PLANT_OFFSETS)
    sin_col, cos_col = np.arange(N_FREQ), half + np.arange(N_FREQ)
    ch_sin, ch_cos, ch_one, ch_zero = 2 * np.arange(N_FREQ), 2 * np.arange(N_FREQ) + 1, 2 * N_FREQ, 2 * N_FREQ + 1
    chans = np.arange(2 * N_FREQ + 2)
    v = ck["frontend.cmvn_vars"].copy()
    v[np.concatenate([sin_col, cos_col, [lo_f, half + lo_f]])] = 0.0
    out["frontend.cmvn_vars"] = v
    # ---- layer 0: the position columns into channels 0 .. 129 of its output
    p0 = "encoder.encoders0.0."
    g, be = ck[p0 + "norm1.weight"].astype(np.float64), ck[p0 + "norm1.bias"].astype(np.float64)
    W, B = ck[p0 + "self_attn.linear_q_k_v.weight"].copy(), ck[p0 + "self_attn.linear_q_k_v.bias"].copy()
    rows = np.zeros((chans.size, feat))
    rows[ch_sin, sin_col], rows[ch_sin, lo_f] = 1.0, -1.0
    rows[ch_cos, cos_col], rows[ch_cos, half + lo_f] = 1.0, -1.0
    rows[ch_one, half + lo_f], rows[ch_one, lo_f] = 1.0, -1.0
    raw = rows / g[None, :]                                      # the converter multiplies the columns by the LayerNorm's weight and adds W beta to the bias
    W[2 * d + chans], B[2 * d + chans] = raw.astype(np.float32), (-(raw.astype(np.float32).astype(np.float64) @ be)).astype(np.float32)
    out[p0 + "self_attn.linear_q_k_v.weight"], out[p0 + "self_attn.linear_q_k_v.bias"] = W, B
    for key in ("self_attn.fsmn_block.weight", "self_attn.linear_out.weight", "self_attn.linear_out.bias", "feed_forward.w_2.weight", "feed_forward.w_2.bias"):
        a = ck[p0 + key].copy()
        a[chans] = 0.0
        out[p0 + key] = a
    # ---- layer 1: q and k of heads 0 .. 2 from those channels
    p1 = "encoder.encoders.0."
    g, be = ck[p1 + "norm1.weight"].astype(np.float64), ck[p1 + "norm1.bias"].astype(np.float64)
    W, B = out[p1 + "self_attn.linear_q_k_v.weight"].copy(), out[p1 + "self_attn.linear_q_k_v.bias"].copy()
    S, Cc = np.zeros((N_FREQ, d)), np.zeros((N_FREQ, d))         # rows that read sin w_f p and cos w_f p (times the row's scale)
    S[np.arange(N_FREQ), ch_sin], S[:, ch_zero] = 1.0, -1.0
    Cc[np.arange(N_FREQ), ch_cos], Cc[:, ch_one], Cc[:, ch_zero] = 1.0, 1.0, -2.0
    w = np.exp(-np.arange(N_FREQ) * (np.log(10000.0) / (half - 1)))
    fold = float(hd ** -0.25)                                     # the converter's scale on q and k rows
    present = np.zeros(d)                                         # ~ 1 / s on a row that carries audio, 0 on the four all-zero rows in front of a stream's first chunk
    present[ch_one], present[ch_zero] = 1.0, -1.0
    for head, (delta, boost) in enumerate(zip(PLANT_OFFSETS, PLANT_ZERO_ROWS)):
        cs, sn = np.cos(w * delta)[:, None], np.sin(w * delta)[:, None]
        k_rows, q_rows = np.zeros((hd, d)), np.zeros((hd, d))
        k_rows[0::2], k_rows[1::2] = S, Cc
        q_rows[0::2], q_rows[1::2] = cs * S - sn * Cc, cs * Cc + sn * S
        k_rows[hd - 2:], q_rows[hd - 2:] = 0.0, 0.0              # the slowest of the 64 sinusoids gives its two dims away:
        k_rows[hd - 2] = present / scale ** 0.5                  #   dim 126 of k is the row's presence, of q a constant -boost (its bias): every real key loses ~ boost / s,
        for r0, m in ((head * hd, q_rows), (d + head * hd, k_rows)):      # so the all-zero rows, which no position can point at, stay visible while they are in the window
            raw = (scale ** 0.5 / fold) * m / g[None, :]
            W[r0:r0 + hd] = raw.astype(np.float32)
            B[r0:r0 + hd] = (-(raw.astype(np.float32).astype(np.float64) @ be)).astype(np.float32)
        B[head * hd + hd - 2] = np.float32(-boost / fold)
    out[p1 + "self_attn.linear_q_k_v.weight"], out[p1 + "self_attn.linear_q_k_v.bias"] = W, B
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """(cfg, checkpoint, chunk) of "sparse" / "dense": the smallest stack that needs everything (d 512, 4 x 128 heads, 2048 FFNs for the cluster kernels; three
    fused encoder layers; two full decoder blocks and the FFN-only one), sharpened and planted attention; the two differ in predictor.cif_output.bias only."""
    cfg = sub("config").ParaformerConfig(n_enc0=1, n_enc=3, n_dec=2, n_dec3=1, vocab=500)
    ck = dict(_planted_checkpoint(cfg))
    ck["predictor.cif_output.bias"] = np.asarray([CIF_BIAS[name]], dtype=np.float32)
    return cfg, ck, default_chunk()


@functools.lru_cache(maxsize=None)
def _planted_checkpoint(cfg):
    return plant_positions(cfg, sharpen(cfg, sub("checkpoints").synth_paraformer_checkpoint(cfg, 0)))


@functools.lru_cache(maxsize=None)
def clips(chunk):
    """Nine clips of N_STEPS chunks; clip i feeds stream STREAM_IDS[i]. A stream consumes its own next chunk when it advances and starts over behind a reset."""
    return tuple(kaldi_audio(AUDIO_SEED + i, N_STEPS * chunk) for i in range(len(STREAM_IDS)))


def schedule_chunks(chunk):
    """Per step: (resets, stream ids, the audio chunks [n][chunk] in slot order)."""
    audio = dict(zip(STREAM_IDS, clips(chunk)))
    nxt = {s: 0 for s in STREAM_IDS}
    out = []
    for resets, sids in SCHEDULE:
        for s in resets:
            nxt[s] = 0
        rows = []
        for s in sids:
            rows.append(audio[s][nxt[s] * chunk:(nxt[s] + 1) * chunk])
            nxt[s] += 1
        out.append((resets, sids, np.stack(rows)))
    return out
