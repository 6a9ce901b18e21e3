"""Float64 statement of the offline Paraformer tail (CIF predictor + non-autoregressive decoder), its bf16 rounding budget, inputs on which errors show, and
the planted mistakes.

The tail (csrc/sensevoice.hip: `SvSession::enqueue_paraformer_tail`; oracle/paraformer_oracle.py: `cif`, `decode_hidden`, `decode`) runs from the encoder's
after_norm rows to the token ids. This module restates the oracle line for line in float64, on the oracle's own folded f32 weights, split at the session's
taps so that every stage takes the SESSION'S OWN rows of the stage before and no stage inherits another's noise or fire decisions:

  predictor_exact  the `enc_out` rows of one utterance -> its alphas: conv k=3 (zero at the utterance's two ends) + ReLU, Linear, sigmoid
  cif_exact        f32 alphas + `enc_out` rows -> (fire count, the acoustic rows [n][d], the fire rows [n]). The fire decisions follow the rule itself: a
                   SEQUENTIAL float64 prefix sum of the f32 alphas with the tail threshold as the last term, rounded once to f32, floored (the order of
                   cif_scan_kernel and of the oracle's float64 cumsum); a fire is floor > previous floor. The integrals are float64.
  layer_exact(i)   the max(n, 1) rows of `acoustic` / `dec{i-1}` + the utterance's `enc_out` rows as memory -> `dec{i}`; i < n_dec: FFN (LayerNorm over d_dec_ffn
                   between its Linears) -> LayerNorm -> FSMN inside the token rows + residual -> cross-attention + residual; i >= n_dec: FFN alone, NO residual
  head_exact       the last `dec{i}` -> logits (after_norm folded into the output layer)
  *_rounded        the same functions with the rounding points the code documents; they exist ONLY to measure E_round = stat(exact - rounded), a kernel is
                   compared with the exact functions. The switches (BF16_ROUNDINGS), read off enqueue_paraformer_tail:
                     "enc_lo"  the predictor conv and the cross-K/V projections multiply `enc_lo`, the bf16 form of the after_norm rows
                     "w"       GEMM weights bf16, rounded AFTER the LayerNorm affine was folded in (cif_conv_w, w1, w2, wq, wkv, wo, pf_out_w); cif_out_w, the
                               FSMN taps and norm2's affine stay f32
                     "conv"    the predictor conv's output behind the ReLU is a bf16 tensor (`ctx`), which alpha_kernel reads
                     "op"      parameter-free LayerNorm outputs that feed a GEMM are bf16 (`h` over d, `ffn` over d_dec_ffn)
                     "qkv"     q, k and v^T are bf16 tensors
                     "p"       the soft-max weights exp(s - max) are the bf16 operand of P V; their f32 sum normalises (attn_bf16_kernel)
                     "ctx"     the attention context is bf16
                   The residual stream (`dec`, `x2`), `ffn32`, norm2's output, the FSMN, the CIF scan and every LayerNorm statistic stay unrounded (f32 on the
                   GPU). The rounded twin of cif_exact is the oracle's f32 `cumsum` form of the integrals with an f32 RUNNING sum, which is what cif_scan_kernel
                   documents (`hsum`: "f32 prefix sum of alpha * hidden"). torch.cumsum itself does not round there: on the CPU it keeps the running sum of
                   f32 input in double and rounds each output once (error half an ulp, where the sequential f32 sum of 276 terms is ten times that), so the
                   oracle's own line under-states the kernel's rounding. Measured on an MI355X against that line the kernel sat at 17 x E_round (sparse) and
                   at 3.0 (dense); against the sequential f32 sum it sits at 1.0.
  case / batches   paraformer_tiny (2 + 1 decoder layers, 2 heads of 128) with planted weights (plant), the "sparse" / "dense" predictor settings (CIF), and three
                   batches by maximum encoder length (BATCH_T): <= 128, 129 .. 256, > 256
  mutations        of the exact functions: the planted mistakes a comparison must catch (MUTATIONS)

How the inputs make errors show (plant). Random weights give a near-uniform cross-attention in which one dropped key moves nothing, and a predictor whose alphas
hardly depend on the clip. Encoder layer 0 writes four indicator channels into the residual stream, and the later encoder layers leave them alone:
  channel 0 is PLANT_END on an utterance's FIRST row, channel 1 on its LAST row, zero elsewhere (a constant v channel whose FSMN taps are 1 at the centre and -1
  at offset -1 / +1: the zero padding at the utterance's ends does the rest). PLANT_END dwarfs the rest of the row, so behind after_norm the step is ~ sqrt(d)
  whether the row is noise or silence. In every full decoder layer dim 0 of head 0's key reads both channels against a constant query dim, scaled so that the
  first and the last key lead all other keys by PLANT_LEAD -+ PLANT_TILT in the score, for EVERY token (a sparse utterance has one): they share most of head
  0's weight even among 280 keys, and one of them missing shows at every length. The other dims of head 0 keep the synthetic weights (bias zero: the zero dummy
  row sees the planted dim alone); head 1 keeps them sharpened (DEC_SHARPEN): there all keys compete, so another layer's keys or another row's query show;
  channel 3 is PLANT_A on every row. Dim 0 of head 1's key reads it with a negative sign: every key made of a real row loses PAD_LEAD, a key made of a row of
  zeros (a pad key) does not, and so shows instead of drowning among sharper real keys;
  channel 2 is PLANT_A on rows of digital silence and ~ 0 elsewhere (layer 0's v row of that channel is fitted to the two kinds of normalised input rows). Row 2 of
  the predictor conv passes it through and predictor.cif_output takes FLAG_DROP off the logit there: silent rows fire nothing in either setting, so that a clip
  of noise with a silent middle (GAP) has far fewer tokens than keys in the dense setting, and the all-zero clip is a zero-token clip in both. Row 4 of the conv
  reads channel 1 at tap -1 and channel 0 at tap +1: zero inside an utterance, awake only when a tap reaches across an utterance's end or the taps are swapped.
The second half of every decoder FFN's hidden columns is FFN_HALF times as wide as the first, so that statistics over d columns are not those over d_dec_ffn.
"""
import functools

import numpy as np
import torch

from conftest import sub
from front_end_ref import ramp_clip, to_kaldi
from helpers import kaldi_audio
from oracle.paraformer_oracle import ParaformerOracle
from sanm_block_ref import MARGIN, bf16, stat                                    # noqa: F401  (re-exported: the tests take them from here)

F = torch.nn.functional
F64 = torch.float64

BF16_ROUNDINGS = frozenset({"enc_lo", "w", "conv", "op", "qkv", "p", "ctx"})
F32_ROUNDINGS = frozenset()                                      # the f32 session has no rounding model

# ---- the fixed inputs ----------------------------------------------------------------------------------------------------------------------------------
PLANT_A = 8.0                                                    # height of the silence and the constant channel in the encoder's residual stream (its rows have an RMS near 4)
PLANT_END = 200.0                                                # height of the first-row and the last-row channel: it IS the row's scale there, so that behind after_norm the step is ~ sqrt(d) whatever else the row holds
PLANT_Q, PLANT_LEAD, PLANT_TILT = 4.0, 9.0, 0.8                  # the planted query dim (raw); the score lead of the first and the last key in head 0: LEAD +- TILT, the first key ahead in even layers
FLAG_DROP = 9.0                                                  # what the silence flag takes off the predictor's logit
CANARY_GAIN = 12.0                                               # size of predictor.cif_output's weight on the conv row that only a tap across an utterance's end can wake; its sign goes against the setting's alphas
PAD_LEAD = 25.0                                                  # what every key made of a real row loses in head 1 (it cancels in the soft-max unless a pad key is let in)
HEAD0_SHARPEN = 1.0                                              # on head 0's rows of src_attn.linear_q beside the planted dim
DEC_SHARPEN = 6.0                                                # on head 1's rows of src_attn.linear_q in the full decoder layers
FFN_HALF = 3.0
# predictor.cif_output: weight scale, bias, sign of the canary weight. sparse: alphas ~ 0.003, fire counts 0 and 1; dense: alphas ~ 0.95, counts approach T
CIF = {"sparse": (0.8, -5.6, 1.0), "dense": (0.8, 2.65, -1.0)}
# encoder lengths T per batch (noise clips), then a ramp clip beside an all-zero clip (their T: RAMP_T, ZERO_T); chosen with the oracle on the CPU, what they
# were chosen for is asserted in tests/test_paraformer_tail_ref_cpu.py
BATCH_T = {
    "le128": (17, 1, 128, 2, 16, 18, 97),
    "le256": (129, 1, 17, 256, 2, 16, 18),
    "gt256": (257, 16, 1, 280, 17, 2, 18, 130),
}
RAMP_T, ZERO_T = {"le128": 26, "le256": 26, "gt256": 200}, {"le128": 7, "le256": 40, "gt256": 64}
GAP = ("gt256", 7)                                               # this noise clip is silent from 8 % to 92 % of its samples
AUDIO_SEED = 8800
LONG_T = (190, 150, 171)                                         # the dense batch of other data that runs between the two runs of a batch

MUTATIONS = ("conv_across", "taps_reversed", "no_tail", "prev_hidden", "fsmn_past_count", "fsmn_no_residual", "ffnorm_over_d", "dec3_residual", "miss_last_key",
             "pad_keys", "next_layer_kv", "q_from_enc_plan")
"""The planted mistakes (each changes the EXACT functions in one place):
  predictor  conv_across       tap -1 of an utterance's first row reads the last row of the utterance before it, tap +1 of its last row the first row of the next
             taps_reversed     the three conv taps in reverse order
  cif        no_tail           the tail threshold left out of the prefix sum (acts on the fire COUNT)
             prev_hidden       `completed` formed with the hidden row BEFORE the fire row
  layer      fsmn_past_count   the FSMN window not cut at the token count: it reads the rows that follow the utterance's tokens in the packed buffer (pad rows up
                               to the 16-row boundary, behind it the next utterance's tokens)
             fsmn_no_residual  x = fsmn(norm2(x)) without + dec
             ffnorm_over_d     ff.norm's mean and variance taken over the first d of the d_dec_ffn columns
             dec3_residual     dec + FFN(dec) in a `decoders3` layer
             miss_last_key     key T - 1 masked
             pad_keys          the keys T .. round_up(T, 32) - 1 admitted; they hold the k|v of a memory row of zeros (the biases)
             next_layer_kv     the K/V of full layer (l + 1) mod n_dec
             q_from_enc_plan   the utterance's query rows taken at its ENCODER row offset in the packed token rows instead of its token row offset"""
STAGE_MUTATIONS = {"alphas": ("conv_across", "taps_reversed"), "count": ("no_tail",), "acoustic": ("prev_hidden",),
                   "full": ("fsmn_past_count", "fsmn_no_residual", "ffnorm_over_d", "miss_last_key", "pad_keys", "next_layer_kv", "q_from_enc_plan"),
                   "dec3": ("ffnorm_over_d", "dec3_residual")}


def samples_of(T):
    """Samples of a clip whose encoder length is T (6 frames a row; 6 T - 3 frames)."""
    return 400 + 160 * (6 * T - 4)


def round_up(n, m):
    return (n + m - 1) // m * m


def ratio(s, e_round):
    """stat / E_round; where E_round is zero the comparison is an equality: 0 if it holds, inf if not."""
    return s / e_round if e_round > 0 else (0.0 if s == 0 else float("inf"))


class TailRef:
    """The tail of one (cfg, checkpoint) in float64."""

    def __init__(self, cfg, ck):
        self.cfg = cfg
        self.orc = o = ParaformerOracle(cfg, ck)
        gemm = {"w1", "w2", "wq", "wkv", "wo"}
        t64 = lambda v: v.to(F64) if torch.is_tensor(v) else (tuple(t.to(F64) for t in v) if isinstance(v, tuple) else v)
        lo = lambda L: {k: (bf16(v) if k in gemm else t64(v)) for k, v in L.items()}
        layers = list(o.dec) + list(o.dec3)
        self.layers = {False: [{k: t64(v) for k, v in L.items()} for L in layers], True: [lo(L) for L in layers]}
        self.w_out = {False: o.w_out.to(F64), True: bf16(o.w_out)}
        self.b_out = o.b_out.to(F64)
        cw = o.ck["predictor.cif_conv1d.weight"]
        self.conv_w = {False: cw.to(F64), True: bf16(cw)}                                                 # [d][d][3]
        self.conv_b = o.ck["predictor.cif_conv1d.bias"].to(F64)
        self.out_w, self.out_b = o.ck["predictor.cif_output.weight"].to(F64)[0], o.ck["predictor.cif_output.bias"].to(F64)[0]
        self.n_layers = cfg.n_dec + cfg.n_dec3

    # ---- predictor ------------------------------------------------------------------------------------------------------------------------------------
    def predictor(self, enc_rows, rnd=frozenset(), mut=None, before=None, after=None):
        """[T][d] -> [T] alphas. before / after: the last row of the utterance in front and the first row of the one behind (conv_across reads them)."""
        r = lambda name, t: bf16(t) if name in rnd else t
        with torch.inference_mode():
            x = r("enc_lo", torch.as_tensor(np.asarray(enc_rows, dtype=np.float64)))
            T, d = x.shape
            zero = torch.zeros(1, d, dtype=F64)
            lo, hi = zero, zero
            if mut == "conv_across":
                lo = zero if before is None else r("enc_lo", torch.as_tensor(np.asarray(before, dtype=np.float64)).reshape(1, d))
                hi = zero if after is None else r("enc_lo", torch.as_tensor(np.asarray(after, dtype=np.float64)).reshape(1, d))
            xp = torch.cat([lo, x, hi], 0)
            w = self.conv_w["w" in rnd]
            taps = (2, 1, 0) if mut == "taps_reversed" else (0, 1, 2)
            conv = self.conv_b + sum(xp[j:j + T] @ w[:, :, taps[j]].t() for j in range(3))
            conv = r("conv", torch.relu(conv))
            return torch.sigmoid(conv @ self.out_w + self.out_b).numpy()

    # ---- integrate and fire -----------------------------------------------------------------------------------------------------------------------------
    def cif(self, alphas, enc_rows, rounded=False, mut=None):
        """f32 alphas [T] and `enc_out` rows [T][d] -> (n, acoustic [n][d], fire rows [n]; T = fired by the tail threshold behind the last row)."""
        c = self.cfg
        al = np.asarray(alphas, dtype=np.float32).reshape(-1)
        T = al.size
        tail = np.float32(0.0 if mut == "no_tail" else c.tail_threshold)
        a32 = np.concatenate([al, [tail]]).astype(np.float32)
        psum = 0.0
        p32 = np.empty(T + 1, dtype=np.float32)
        for t in range(T + 1):                                   # the rule: sequential float64 sum, rounded once
            psum += float(a32[t])
            p32[t] = np.float32(psum)
        fl = np.floor(p32)
        prev = np.concatenate([[np.float32(0.0)], fl[:-1]])
        fire = np.nonzero(fl > prev)[0]
        n = int(fire.size)
        # the oracle's form (prefix sums of alpha x hidden, `completed` = the sum at the fire row less the remainder's share, differences) in float64, or -- the
        # rounded twin -- in f32 with an f32 RUNNING sum, every product and sum rounded (numpy's cumsum is that sequential sum; cif_scan_kernel's hsum)
        dt = np.float32 if rounded else np.float64
        hidden = np.concatenate([np.asarray(enc_rows, dtype=np.float32), np.zeros((1, c.d_model), np.float32)], 0).astype(dt)
        prefix_hidden = np.cumsum(a32.astype(dt)[:, None] * hidden, axis=0, dtype=dt)
        remains = (p32 - fl).astype(dt)[fire]
        at = hidden[fire]
        if mut == "prev_hidden":
            at = np.concatenate([np.zeros((1, c.d_model), dt), hidden], 0)[fire]                          # (row fire - 1; nothing fires on row 0: alphas < 1)
        completed = np.concatenate([np.zeros((1, c.d_model), dt), prefix_hidden[fire] - remains[:, None] * at], 0)
        acoustic = (completed[1:] - completed[:-1]).astype(np.float64)
        assert acoustic.dtype == np.float64 and completed.dtype == dt
        assert n == int(fl[-1]) or (al >= 1).any()
        return n, acoustic, fire.astype(np.int32)

    # ---- decoder layers -----------------------------------------------------------------------------------------------------------------------------------
    def _ffn(self, L, dec, r, mut):
        c = self.cfg
        hid = torch.relu(r("op", F.layer_norm(dec, (c.d_model,))) @ L["w1"].t() + L["b1"])                # ffn32: an f32 slab on the GPU
        if mut == "ffnorm_over_d":
            part = hid[:, :c.d_model]
            mean, var = part.mean(1, keepdim=True), part.var(1, unbiased=False, keepdim=True)
            nrm = (hid - mean) / torch.sqrt(var + 1e-5)
        else:
            nrm = F.layer_norm(hid, (c.d_dec_ffn,))
        return r("op", nrm) @ L["w2"].t() + L["b2"]

    def pre_attention(self, i, rows, rnd=frozenset(), mut=None, tail_rows=None):
        """Full layer i up to the rows the query projection reads: y = dec + fsmn(norm2(FFN(dec))), the FSMN zero padded inside the m token rows. tail_rows: the
        (up to 5) rows that follow the utterance's tokens in the packed buffer (fsmn_past_count reads their FFN rows)."""
        c = self.cfg
        d, pad = c.d_model, (c.fsmn_kernel - 1) // 2
        r = lambda name, t: bf16(t) if name in rnd else t
        L = self.layers["w" in rnd][i]
        with torch.inference_mode():
            dec = torch.as_tensor(np.asarray(rows, dtype=np.float64))
            m = dec.shape[0]
            sa = F.layer_norm(self._ffn(L, dec, r, mut), (d,), L["n2"][0], L["n2"][1])
            behind = torch.zeros(pad, d, dtype=F64)
            if mut == "fsmn_past_count" and tail_rows is not None and len(tail_rows):
                tr = torch.as_tensor(np.asarray(tail_rows, dtype=np.float64))[:pad]
                behind[:tr.shape[0]] = F.layer_norm(self._ffn(L, tr, r, None), (d,), L["n2"][0], L["n2"][1])
            sp = torch.cat([torch.zeros(pad, d, dtype=F64), sa, behind], 0)
            mem = torch.zeros(m, d, dtype=F64)
            for j in range(c.fsmn_kernel):                       # (identity folded into the centre tap)
                mem += sp[j:j + m] * L["wf"][:, 0, j]
            return (mem if mut == "fsmn_no_residual" else dec + mem).numpy()

    def attention(self, i, y, memory, rnd=frozenset(), mut=None, q_rows=None, trace=None):
        """Full layer i from y: dec = y + out(softmax(q k^T) v); q from LayerNorm(q_rows if given else y), k | v from the memory rows."""
        c = self.cfg
        d, H, hd = c.d_model, c.n_heads, c.d_head
        r = lambda name, t: bf16(t) if name in rnd else t
        Ls = self.layers["w" in rnd]
        L = Ls[i]
        Lkv = Ls[(i + 1) % c.n_dec] if mut == "next_layer_kv" else L
        heads = lambda z: z.reshape(z.shape[0], H, hd).transpose(0, 1)
        with torch.inference_mode():
            y = torch.as_tensor(np.asarray(y, dtype=np.float64))
            qsrc = y if q_rows is None else torch.as_tensor(np.asarray(q_rows, dtype=np.float64))
            mem = r("enc_lo", torch.as_tensor(np.asarray(memory, dtype=np.float64)))
            m, T = y.shape[0], mem.shape[0]
            q = heads(r("qkv", r("op", F.layer_norm(qsrc, (d,))) @ L["wq"].t() + L["bq"]))
            kv = r("qkv", mem @ Lkv["wkv"].t() + Lkv["bkv"])
            if mut == "pad_keys" and T % 32:
                kv = torch.cat([kv, r("qkv", Lkv["bkv"])[None].expand(round_up(T, 32) - T, 2 * d)], 0)
            k, v = heads(kv[:, :d]), heads(kv[:, d:])
            s = q @ k.transpose(1, 2)
            if mut == "miss_last_key" and T >= 2:
                s = s.clone()
                s[:, :, T - 1] = -float("inf")
            e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
            if trace is not None:
                trace.append((i, (e / e.sum(-1, keepdim=True)).numpy()))
            ctx = r("ctx", ((r("p", e) @ v) / e.sum(-1, keepdim=True)).transpose(0, 1).reshape(m, d))
            return (y + ctx @ L["wo"].t() + L["bo"]).numpy()

    def layer(self, i, rows, memory, rnd=frozenset(), mut=None, tail_rows=None, trace=None):
        """`acoustic` / `dec{i-1}` rows [m][d] (m = max(n, 1): the dummy row of a zero-token clip is a live row) -> `dec{i}`."""
        if i < self.cfg.n_dec:
            return self.attention(i, self.pre_attention(i, rows, rnd, mut, tail_rows), memory, rnd, mut, trace=trace)
        r = lambda name, t: bf16(t) if name in rnd else t
        with torch.inference_mode():
            dec = torch.as_tensor(np.asarray(rows, dtype=np.float64))
            out = self._ffn(self.layers["w" in rnd][i], dec, r, mut)
            return (dec + out if mut == "dec3_residual" else out).numpy()

    def head(self, rows, rnd=frozenset()):
        r = lambda name, t: bf16(t) if name in rnd else t
        with torch.inference_mode():
            dec = torch.as_tensor(np.asarray(rows, dtype=np.float64))
            return (r("op", F.layer_norm(dec, (self.cfg.d_model,))) @ self.w_out["w" in rnd].t() + self.b_out).numpy()


# ---- the functions the tests call --------------------------------------------------------------------------------------------------------------------------
_refs = {}


def ref_of(cfg, ck):
    key = (cfg, id(ck))
    if key not in _refs:
        _refs[key] = (ck, TailRef(cfg, ck))                      # (holds ck, so the id stays its own)
    return _refs[key][1]


def predictor_exact(cfg, ck, enc_rows, mut=None, before=None, after=None):
    return ref_of(cfg, ck).predictor(enc_rows, mut=mut, before=before, after=after)


def predictor_rounded(cfg, ck, enc_rows, roundings):
    return ref_of(cfg, ck).predictor(enc_rows, rnd=frozenset(roundings))


def cif_exact(cfg, ck, alphas, enc_rows, mut=None):
    return ref_of(cfg, ck).cif(alphas, enc_rows, mut=mut)


def cif_rounded(cfg, ck, alphas, enc_rows):
    return ref_of(cfg, ck).cif(alphas, enc_rows, rounded=True)


def layer_exact(cfg, ck, i, rows, memory, mut=None, tail_rows=None, trace=None):
    return ref_of(cfg, ck).layer(i, rows, memory, mut=mut, tail_rows=tail_rows, trace=trace)


def layer_rounded(cfg, ck, i, rows, memory, roundings):
    return ref_of(cfg, ck).layer(i, rows, memory, rnd=frozenset(roundings))


def head_exact(cfg, ck, rows):
    return ref_of(cfg, ck).head(rows)


def head_rounded(cfg, ck, rows, roundings):
    return ref_of(cfg, ck).head(rows, rnd=frozenset(roundings))


# ---- one batch, stage by stage ----------------------------------------------------------------------------------------------------------------------------
# A record is what one run of a batch took in and gave out, per utterance a dict: enc_out [T][d], alphas [T], n, acoustic [m][d], dec [n_layers] x [m][d],
# logits [m][vocab] (m = max(n, 1); all f32 like the taps) and, of the timed form, fire [n]. The GPU tests fill it from the session's taps, the CPU tests from the
# references themselves (reference_record).
def reference_record(cfg, ck, enc_outs):
    """The batch run by the exact references alone on the given `enc_out` rows, each stage's output cast to f32 like a tap."""
    ref = ref_of(cfg, ck)
    record = []
    for enc in enc_outs:
        enc = np.asarray(enc, dtype=np.float32)
        alphas = ref.predictor(enc).astype(np.float32)
        n, acoustic, fire = ref.cif(alphas, enc)
        rows = np.concatenate([acoustic, np.zeros((1, cfg.d_model))], 0)[:max(n, 1)].astype(np.float32)
        u = dict(enc_out=enc, alphas=alphas, n=n, acoustic=rows, fire=fire, dec=[])
        for i in range(ref.n_layers):
            rows = ref.layer(i, rows, enc).astype(np.float32)
            u["dec"].append(rows)
        u["logits"] = ref.head(rows).astype(np.float32)
        record.append(u)
    return record


def stages(cfg):
    return ["alphas", "acoustic"] + [f"dec{i}" for i in range(cfg.n_dec + cfg.n_dec3)] + ["logits"]


def stage_runs(cfg, ck, record, roundings, trace=None):
    """Per utterance {stage: dict(exact, rounded, e_round)} over the record's rows: every stage on the record's own rows of the stage before. Also "n" and "fire":
    the count and fire rows the rule gives on the record's alphas. `alphas` is one row of T columns, `acoustic` the n fired rows (none for a zero-token clip)."""
    ref, rnd = ref_of(cfg, ck), frozenset(roundings)
    out = []
    for u in record:
        enc = u["enc_out"]
        res = {}
        res["alphas"] = dict(exact=ref.predictor(enc)[None], rounded=ref.predictor(enc, rnd=rnd)[None])
        n, acoustic, fire = ref.cif(u["alphas"], enc)
        res["n"], res["fire"] = n, fire
        res["acoustic"] = dict(exact=acoustic, rounded=ref.cif(u["alphas"], enc, rounded=True)[1])
        rows = u["acoustic"]
        for i in range(ref.n_layers):
            res[f"dec{i}"] = dict(exact=ref.layer(i, rows, enc, trace=trace), rounded=ref.layer(i, rows, enc, rnd=rnd))
            rows = u["dec"][i]
        res["logits"] = dict(exact=ref.head(rows), rounded=ref.head(rows, rnd=rnd))
        for s in stages(cfg):
            e = res[s]
            e["e_round"] = stat(e["exact"] - e["rounded"]) if e["exact"].shape[0] else (0.0, 0.0)
        out.append(res)
    return out


def packed_rows(record, field, layer=None):
    """The packed token rows of a batch as the decoder's buffers hold them: utterance b's max(n, 1) rows at ParaformerSession.token_rows, zeros elsewhere."""
    rows = [u[field] if layer is None else u[field][layer] for u in record]
    offs, r = [], 0
    for x in rows:
        offs.append(r)
        r += round_up(x.shape[0], 16)
    buf = np.zeros((r, rows[0].shape[1]), dtype=np.float64)
    for o, x in zip(offs, rows):
        buf[o:o + x.shape[0]] = x
    return buf, offs


def mutated(cfg, ck, record, stage, mut):
    """Per utterance (output of the mutated exact reference for `stage`, whether the mutation applies there). It applies where it can act: conv_across with a
    neighbour, taps_reversed from two rows on, prev_hidden with a fire, miss_last_key from two keys on (one key has the weight 1 whatever the scores), pad_keys
    unless T is a multiple of 32, fsmn_past_count where rows follow the tokens in the packed buffer, fsmn_no_residual unless the rows are the zero dummy row,
    q_from_enc_plan where the rows at the two offsets differ and there are two keys; no_tail gives the count and applies where the count changes."""
    ref = ref_of(cfg, ck)
    assert mut in MUTATIONS
    B = len(record)
    li = int(stage[3:]) if stage.startswith("dec") else None
    src = None
    if li is not None:
        src, offs = packed_rows(record, "acoustic") if li == 0 else packed_rows(record, "dec", li - 1)
        enc_offs, r = [], 0
        for u in record:
            enc_offs.append(r)
            r += round_up(u["enc_out"].shape[0], 16)
        if mut == "q_from_enc_plan":
            ys = [ref.pre_attention(li, src[o:o + max(u["n"], 1)]) for o, u in zip(offs, record)]
            ybuf = np.zeros((max(src.shape[0], r + 16 * 32), cfg.d_model))                               # fsmn_rows_kernel writes zeros outside the token rows
            for o, y in zip(offs, ys):
                ybuf[o:o + y.shape[0]] = y
    out = []
    for b, u in enumerate(record):
        enc, T, m = u["enc_out"], u["enc_out"].shape[0], max(u["n"], 1)
        if stage == "alphas":
            before = record[b - 1]["enc_out"][-1] if b > 0 else None
            after = record[b + 1]["enc_out"][0] if b + 1 < B else None
            applies = (before is not None or after is not None) if mut == "conv_across" else T >= 2
            out.append((ref.predictor(enc, mut=mut, before=before, after=after)[None], applies))
        elif stage == "count":
            n = ref.cif(u["alphas"], enc, mut=mut)[0]
            out.append((n, n != u["n"]))
        elif stage == "acoustic":
            out.append((ref.cif(u["alphas"], enc, mut=mut)[1], u["n"] >= 1))
        elif mut == "q_from_enc_plan":
            q_rows = ybuf[enc_offs[b]:enc_offs[b] + m]
            out.append((ref.attention(li, ys[b], enc, q_rows=q_rows), T >= 2 and not np.array_equal(q_rows, ys[b])))
        else:
            rows = src[offs[b]:offs[b] + m]
            tail = src[offs[b] + m:offs[b] + m + 5]
            applies = {"miss_last_key": T >= 2, "pad_keys": T % 32 != 0, "fsmn_past_count": len(tail) > 0, "fsmn_no_residual": bool(np.any(rows != 0))}.get(mut, True)
            if li >= cfg.n_dec:
                applies = mut in STAGE_MUTATIONS["dec3"]
            elif mut == "dec3_residual":
                applies = False
            out.append((ref.layer(li, rows, enc, mut=mut, tail_rows=tail), applies))
    return out


# ---- the fixed cases ------------------------------------------------------------------------------------------------------------------------------------
def _enc_out(orc, audio):
    with torch.inference_mode():
        return orc.encode(orc.fbank(torch.as_tensor(np.asarray(audio, dtype=np.float32)))).numpy()


def plant(cfg, ck):
    """A copy of ck with the indicator channels in the encoder, the decoder head that looks at two of them and the predictor row that reads the third (the module
    docstring). out["_flag_gain"]: the weight of predictor.cif_output on the silence row, which case() sets behind its scaling."""
    out = {k: v.copy() for k, v in ck.items()}
    d, feat, hd = cfg.d_model, cfg.feat_dim, cfg.d_head
    pad = (cfg.fsmn_kernel - 1) // 2
    ch = np.array([0, 1, 2, 3])                                  # (channel 3 stays the constant: PLANT_A on every row)
    enc_layers = [f"encoder.encoders0.{i}." for i in range(cfg.n_enc0)] + [f"encoder.encoders.{i}." for i in range(cfg.n_enc)]
    for k, p in enumerate(enc_layers):
        out[p + "self_attn.linear_q_k_v.weight"][2 * d + ch] = 0.0
        out[p + "self_attn.linear_q_k_v.bias"][2 * d + ch] = (PLANT_END, PLANT_END, PLANT_A, PLANT_A) if k == 0 else 0.0
        for key in ("self_attn.linear_out.weight", "self_attn.linear_out.bias", "feed_forward.w_2.weight", "feed_forward.w_2.bias"):
            out[p + key][ch] = 0.0
        out[p + "self_attn.linear_out.weight"][:, ch] = 0.0      # (the constant v channels reach the rows through the FSMN alone, not through the attention context)
        if k == 0:
            w = out[p + "self_attn.fsmn_block.weight"]                                                    # [d][1][taps]; the fold adds the identity at the centre
            w[ch] = 0.0
            w[0, 0, pad - 1] = -1.0                              # row t: v - v[t - 1] = PLANT_END on the first row
            w[1, 0, pad + 1] = -1.0                              # row t: v - v[t + 1] = PLANT_END on the last row
    # channel 2: layer 0's v row fitted to the two kinds of normalised input rows, PLANT_A on digital silence and ~ 0 on noise
    orc = ParaformerOracle(cfg, ck)
    p0 = "encoder.encoders0.0."
    g, be = orc.ck[p0 + "norm1.weight"].double(), orc.ck[p0 + "norm1.bias"].double()

    def rows(audio):
        with torch.inference_mode():
            mel = orc.fbank(torch.as_tensor(np.asarray(audio, dtype=np.float32)))
            nf = mel.shape[0]
            T = (nf + cfg.lfr_n - 1) // cfg.lfr_n
            idx = (torch.arange(0, T * cfg.lfr_n, cfg.lfr_n).unsqueeze(1) + torch.arange(cfg.lfr_m) - (cfg.lfr_m - 1) // 2).clamp(min=0, max=nf - 1)
            x = (mel[idx].reshape(T, feat) * orc.cmvn_vars + orc.in_bias[:T]).double()
            return F.layer_norm(x, (feat,)) * g + be

    clips = np.zeros(samples_of(40), np.float32), kaldi_audio(AUDIO_SEED + 999, samples_of(40))
    z, m = rows(clips[0]).mean(0), rows(clips[1]).mean(0)
    w = (z - m) / ((z - m) ** 2).sum()
    out[p0 + "self_attn.linear_q_k_v.weight"][2 * d + 2] = (PLANT_A * w).numpy().astype(np.float32)
    out[p0 + "self_attn.linear_q_k_v.bias"][2 * d + 2] = np.float32(-PLANT_A * float(w @ m))
    # what the three channels hold behind after_norm, measured on a silent and a noise clip
    mid = ParaformerOracle(cfg, out)
    silent, noise = _enc_out(mid, clips[0]), _enc_out(mid, clips[1])
    hi, lo = float(silent[:, 2].mean()), float(noise[:, 2].mean())
    step0, step1, present = float(noise[0, 0] - noise[1:, 0].mean()), float(noise[-1, 1] - noise[:-1, 1].mean()), float(noise[1:-1, 3].mean())
    present0, present1 = float(noise[0, 3]), float(noise[-1, 3])                                       # (the two end rows are scaled down as a whole)
    assert hi - lo > 1.0 and step0 > 1.0 and step1 > 1.0 and present > 1.0, (hi, lo, step0, step1, present)
    # the predictor: conv row 2 passes channel 2 through (centre tap, a threshold half way between the two kinds, ReLU: zero on noise)
    cw, cb = out["predictor.cif_conv1d.weight"], out["predictor.cif_conv1d.bias"]
    cw[2] = 0.0
    cw[2, 2, 1] = 1.0
    cb[2] = np.float32(-(hi + lo) / 2)
    out["_flag_gain"] = np.float32(-FLAG_DROP / ((hi - lo) / 2))
    # conv row 4 reads the LAST-row channel at tap -1 and the FIRST-row channel at tap +1: inside an utterance no such neighbour exists and the row stays zero
    # behind the ReLU (bias -0.7); a tap that crosses an utterance's end, or reversed taps, wake it
    cw[4] = 0.0
    cw[4, 1, 0], cw[4, 0, 2], cb[4] = 1.0, 1.0, -0.7
    # the decoder: dim 0 of head 0 gives the first and the last key the same lead PLANT_LEAD over the others for every token; head 1 keeps its weights, sharpened,
    # and its dim 0 reads the constant channel, so that a key made of a row of zeros (a pad key) leads the real keys by PAD_LEAD instead of drowning among them
    scale = float(cfg.d_head) ** 0.5                             # (the export folds d_head^-1/4 into q and into k)
    for i in range(cfg.n_dec):
        p = f"decoder.decoders.{i}."
        wq, bq, wk, bk = (out[p + "src_attn." + k] for k in ("linear_q.weight", "linear_q.bias", "linear_k_v.weight", "linear_k_v.bias"))
        wq[:hd] *= np.float32(HEAD0_SHARPEN)                     # head 0: beside the planted dim a mild dependence on the token, which decides among two or three keys
        bq[:hd] = 0.0                                            # (the zero dummy row of a zero-token clip sees the planted dim alone)
        wq[hd:2 * hd] *= np.float32(DEC_SHARPEN)
        bq[hd:2 * hd] *= np.float32(DEC_SHARPEN)
        for row in (0, hd):
            wq[row], bq[row], wk[row], bk[row] = 0.0, PLANT_Q, 0.0, 0.0
        tilt = PLANT_TILT * (1 - 2 * (i % 2))
        wk[0, 0] = np.float32((PLANT_LEAD + tilt) * scale / (PLANT_Q * step0))
        wk[0, 1] = np.float32((PLANT_LEAD - tilt) * scale / (PLANT_Q * step1))
        lose = PAD_LEAD * scale / PLANT_Q
        wk[hd, 3] = np.float32(-lose / present)                  # head 1: every key made of a real row loses PAD_LEAD,
        wk[hd, 0] = np.float32(-lose * (1.0 - present0 / present) / step0)    # the two end rows, whose constant channel is smaller, as much as the others
        wk[hd, 1] = np.float32(-lose * (1.0 - present1 / present) / step1)
    # the FFNs: the second half of the hidden columns is three times as wide as the first, so that ff.norm's statistics over d columns are not those over d_dec_ffn
    for p in [f"decoder.decoders.{i}." for i in range(cfg.n_dec)] + [f"decoder.decoders3.{i}." for i in range(cfg.n_dec3)]:
        out[p + "feed_forward.w_1.weight"][d:] *= np.float32(FFN_HALF)
        out[p + "feed_forward.w_1.bias"][d:] = out[p + "feed_forward.w_1.bias"][d:] * np.float32(FFN_HALF) + np.float32(0.5)
    return out




@functools.lru_cache(maxsize=None)
def _planted():
    cfg = sub("config").paraformer_tiny()
    return cfg, plant(cfg, sub("checkpoints").synth_paraformer_checkpoint(cfg, 0))


@functools.lru_cache(maxsize=None)
def case(name):
    """(cfg, checkpoint) of "sparse" / "dense": paraformer_tiny with the planted weights; the two differ in predictor.cif_output only."""
    cfg, base = _planted()
    ck = {k: v for k, v in base.items() if not k.startswith("_")}
    scale, bias, canary = CIF[name]
    ck["predictor.cif_output.weight"] = (base["predictor.cif_output.weight"] * np.float32(scale)).astype(np.float32)
    ck["predictor.cif_output.weight"][0, 2] = base["_flag_gain"]
    ck["predictor.cif_output.weight"][0, 4] = canary * CANARY_GAIN
    ck["predictor.cif_output.bias"] = np.asarray([bias], dtype=np.float32)
    return cfg, ck


def _toned(noise, i):
    """The noise clip under a tone of its own (300 + 450 i Hz, three times the noise's RMS): the synthetic encoder's rows are nearly parallel from clip to clip on
    noise alone, and a row taken from the neighbouring utterance would then differ from the right one by less than bf16 rounding does."""
    t = np.arange(noise.size, dtype=np.float64) / 16000.0
    amp = 3.0 * float(np.sqrt(np.mean(noise.astype(np.float64) ** 2))) * np.sqrt(2.0)
    return np.clip(np.round(noise + amp * np.sin(2 * np.pi * (300.0 + 450.0 * i) * t)), -32768, 32767).astype(np.float32)


@functools.lru_cache(maxsize=None)
def batch(name):
    """The clips of batch `name`: noise clips of the lengths BATCH_T, a ramp clip, an all-zero clip."""
    clips = [_toned(kaldi_audio(AUDIO_SEED + 16 * sorted(BATCH_T).index(name) + i, samples_of(T)), i) for i, T in enumerate(BATCH_T[name])]
    if name == GAP[0]:
        a = clips[GAP[1]] = clips[GAP[1]].copy()
        a[int(0.08 * a.size):int(0.92 * a.size)] = 0.0
    clips.append(to_kaldi(ramp_clip(samples_of(RAMP_T[name]))))
    clips.append(np.zeros(samples_of(ZERO_T[name]), np.float32))
    return tuple(clips)


def batch_lengths(name):
    return tuple(BATCH_T[name]) + (RAMP_T[name], ZERO_T[name])


@functools.lru_cache(maxsize=None)
def long_batch():
    """Dense clips of other data: what the session's buffers hold when a batch runs the second time."""
    return tuple(kaldi_audio(AUDIO_SEED + 900 + i, samples_of(T)) for i, T in enumerate(LONG_T))


@functools.lru_cache(maxsize=None)
def oracle_enc_out(case_name, batch_name):
    """The oracle's f32 `enc_out` rows of the batch's clips (the encoder does not see the predictor: shared by the two cases)."""
    cfg, ck = case(case_name)
    orc = ref_of(cfg, ck).orc
    with torch.inference_mode():
        return tuple(orc.encode(orc.fbank(torch.as_tensor(np.asarray(a, dtype=np.float32)))).numpy() for a in batch(batch_name))
