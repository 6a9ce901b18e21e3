"""Float64 statement of the SANM encoder stack behind block 0, its bf16 rounding budget, and inputs on which attention errors show.

The SANM block (LayerNorm, q|k|v projection, soft-max attention over the window, FSMN over v, out-projection + residual, LayerNorm, FFN + residual)
exists in four implementations that `SanmSession::enqueue` picks by batch shape. The end-to-end tests compare them with each other after 69 blocks, on
synthetic weights whose soft-max is nearly uniform (mean top probability 0.02 over 137 keys): one masked key moves `enc_out` by less than bf16 rounding
does. This module states ONE stack in float64 and provides:

  exact_stack     blocks 1 .., after_norm, the tp blocks, tp_norm from the rows behind block 0 -- SenseVoiceOracle.sanm_block in float64, f32 weights
  rounded_stack   the same function with the rounding points the bf16 paths document (csrc/sensevoice.hip: enqueue, arena.py: _fold64):
                    "x"    the residual stream's operand copy is bf16 before the parameter-free LayerNorm (x_lo / xalo)
                    "w"    gamma folded into the weight in float64 BEFORE its bf16 rounding, beta into the f32 bias; wout and w2 bf16 as well
                    "qkv"  q, k and v are bf16 operands of the attention (and v of the FSMN)
                    "p"    the probabilities are the bf16 operand of P.V
                    "ctx"  ctx is the bf16 operand of the out-projection
                    "x1"   the operand copy of the attention half's output (x1_lo / xblo); the f32 residual itself stays unrounded
                    "hid"  the FFN's hidden rows are bf16
                  It exists ONLY to measure the rounding noise E_round = stat(exact - rounded); a kernel is compared with exact_stack.
  plant_attention rewrites the q and k rows of every block behind block 0 so that heads 0..2 attend along permutations (identity, reversal, +64)
                  with top probabilities near 0.9: a wrong key mask, tile hand-over or K slot then moves the output far beyond E_round
  mutations       of the exact reference (a masked key, a dropped FSMN tap, eight zeroed hidden columns): the CPU test proves with them that the
                  inputs make such errors visible, and they are the "planted mistakes" a comparison must catch
"""
import functools

import numpy as np
import torch

from conftest import sub
from oracle.sensevoice_oracle import SenseVoiceOracle

F = torch.nn.functional
F64 = torch.float64

ROUNDINGS = frozenset({"x", "w", "qkv", "p", "ctx", "x1", "hid"})
WINDOWS = (144, 143, 137, 130, 129, 128, 113, 97, 33, 5)       # the lengths at which the block kernel changes path (test_sanm_block_attn_gpu.py)
ANCHOR_T = 144
ANCHOR_SEED = 5
LANG = 0
A2 = 9.0                                                        # planted score of the chosen key (others ~ 0)
SVD_RANK = 128
MARGIN = 3.0                                                    # a kernel may differ from exact_stack by MARGIN x E_round


def bf16(t):
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def samples_of(T):
    """Samples of a clip that makes a window of T rows (4 prompt rows + T - 4 LFR rows of 6 frames)."""
    return 400 + 160 * ((T - 4) * 6 - 1)


def anchor_audio():
    return sub("checkpoints").synth_audio("kaldi", 1, samples_of(ANCHOR_T), seed=ANCHOR_SEED)[0, 0]


def window_audios(windows=WINDOWS):
    """Truncations of the anchor clip: the planted weights, built from the anchor's rows, fit every one of them."""
    a = anchor_audio()
    return [a[:samples_of(T)].copy() for T in windows]


def stat(diff):
    """(worst row's RMS over the columns, max abs) of one window's difference."""
    d = np.asarray(diff, dtype=np.float64)
    return float(np.sqrt((d * d).mean(axis=1)).max()), float(np.abs(d).max())


# ---- mutations of the exact reference -------------------------------------------------------------------------------------------------
def mask_key(j):
    return ("mask_key", int(j))


def drop_tap(row, tap):
    """FSMN tap `tap` (-5 .. +5: the value of row + tap) left out of row `row`."""
    return ("drop_tap", int(row), int(tap))


def zero_hidden(row, col0=None):
    """Hidden columns col0 .. col0 + 7 of row `row` read as zero by FFN-2 (one lost 16-byte store). col0 = None: the aligned group of eight whose
    share of the row's FFN-2 output is the largest -- about half of the hidden values are zero behind the ReLU, and a group of zeros shows on no input."""
    return ("zero_hidden", int(row), None if col0 is None else int(col0))


class SanmStack:
    """The blocks behind block 0 of one (cfg, checkpoint) in float64."""

    def __init__(self, cfg, ck):
        self.cfg = cfg
        self.orc = SenseVoiceOracle(cfg, ck, dtype=F64)
        self.n_main = cfg.n_enc0 + cfg.n_enc
        self._folded = {}

    # the LayerNorm affines folded into the following Linear, in float64: LN(x; g, b) W^T + c = LN0(x) (W g)^T + (W b + c)
    def folded(self, i):
        if i not in self._folded:
            b = self.orc.blocks[i]
            t = lambda a: a.to(F64)
            g1, be1, g2, be2 = t(b["ln1"][0]), t(b["ln1"][1]), t(b["ln2"][0]), t(b["ln2"][1])
            self._folded[i] = dict(wqkv=t(b["wqkv"]) * g1[None, :], bqkv=t(b["bqkv"]) + t(b["wqkv"]) @ be1,
                                   w1=t(b["w1"]) * g2[None, :], b1=t(b["b1"]) + t(b["w1"]) @ be2,
                                   wout=t(b["wout"]), w2=t(b["w2"]), b2=t(b["b2"]), wfsmn=t(b["wfsmn"]), bfsmn=t(b["bfsmn"]))
        return self._folded[i]

    def block(self, i, x, rnd=frozenset(), mut=None, probs=None):
        """Block i on the rows x [T][d]. rnd: the rounding points switched on; mut: one mutation; probs: a list that receives the [H][T][T] probabilities."""
        c, w = self.cfg, self.folded(i)
        T, d = x.shape[0], c.d_model
        r = lambda name, t: bf16(t) if name in rnd else t
        h = F.layer_norm(r("x", x), (d,), None, None, 1e-5)
        qkv = r("qkv", h @ r("w", w["wqkv"]).t() + w["bqkv"])
        q, k, v = qkv.split(d, dim=1)
        heads = lambda t: t.reshape(T, c.n_heads, c.d_head).transpose(0, 1)
        s = heads(q) @ heads(k).transpose(1, 2)
        if mut is not None and mut[0] == "mask_key":
            s = s.clone()
            s[:, :, mut[1]] = -float("inf")
        p = torch.softmax(s, dim=-1)
        if probs is not None:
            probs.append(p)
        ctx = r("ctx", (r("p", p) @ heads(v)).transpose(0, 1).reshape(T, d))
        pad = (c.fsmn_kernel - 1) // 2
        mem = F.conv1d(v.t().unsqueeze(0), w["wfsmn"], w["bfsmn"], padding=pad, groups=d)[0].t()
        if mut is not None and mut[0] == "drop_tap":
            row, tap = mut[1], mut[2]
            assert 0 <= row < T and 0 <= row + tap < T and abs(tap) <= pad, mut
            mem = mem.clone()
            mem[row] -= w["wfsmn"][:, 0, pad + tap] * v[row + tap]
        att = ctx @ r("w", w["wout"]).t() + mem + x
        h2 = F.layer_norm(r("x1", att), (d,), None, None, 1e-5)
        hid = r("hid", torch.relu(h2 @ r("w", w["w1"]).t() + w["b1"]))
        if mut is not None and mut[0] == "zero_hidden":
            hid = hid.clone()
            col0 = mut[2]
            if col0 is None:
                share = (hid[mut[1]][None, :] * w["w2"]).reshape(d, -1, 8).sum(dim=2)          # [d][groups]: each group's term of the output row
                col0 = 8 * int((share * share).sum(dim=0).argmax())
            hid[mut[1], col0:col0 + 8] = 0.0
        return att + hid @ r("w", w["w2"]).t() + w["b2"]

    def _norm(self, x, name):
        g, b = self.orc.ck[f"encoder.{name}.weight"].to(F64), self.orc.ck[f"encoder.{name}.bias"].to(F64)
        return F.layer_norm(x, (self.cfg.d_model,), g, b, 1e-5)

    def run(self, x_block0, rnd=frozenset(), mut=None, mut_block=1, block_fn=None, stop_before=None):
        """Blocks 1 .. n_main - 1, after_norm, the tp blocks, tp_norm. block_fn(i, x) replaces self.block; stop_before = i returns block i's input."""
        x = torch.as_tensor(np.asarray(x_block0, dtype=np.float64))
        fn = block_fn or (lambda i, x: self.block(i, x, rnd, mut if i == mut_block else None))
        with torch.inference_mode():
            for i in range(1, self.cfg.n_blocks):
                if i == self.n_main:
                    x = self._norm(x, "after_norm")
                if stop_before == i:
                    return x
                x = fn(i, x)
            if self.cfg.n_blocks == self.n_main:
                x = self._norm(x, "after_norm")
            return self._norm(x, "tp_norm").numpy()

    def exact(self, x_block0):
        """The oracle's own sanm_block in float64 (the independent statement: the LayerNorm affines are not folded)."""
        return self.run(x_block0, block_fn=lambda i, x: self.orc.sanm_block(x, self.orc.blocks[i]))

    def block0(self, audio, lang=LANG):
        """The oracle's float64 rows behind block 0 (the CPU test's inputs; the GPU test takes the session's own `block0` tap instead)."""
        with torch.inference_mode():
            a = torch.as_tensor(np.asarray(audio, dtype=np.float32).reshape(-1))
            x = self.orc.lfr_cmvn(self.orc.frontend(a), lang)
            return self.orc.sanm_block(x, self.orc.blocks[0]).numpy()


_stacks = {}


def stack_of(cfg, ck):
    key = (cfg, id(ck))
    if key not in _stacks:
        _stacks[key] = (ck, SanmStack(cfg, ck))           # (holds ck, so the id stays its own)
    return _stacks[key][1]


def exact_stack(cfg, ck, x_block0):
    """enc_out [T][d] (float64) of the rows behind block 0, f32 checkpoint weights, no rounding."""
    return stack_of(cfg, ck).exact(x_block0)


def rounded_stack(cfg, ck, x_block0, roundings=ROUNDINGS):
    return stack_of(cfg, ck).run(x_block0, rnd=frozenset(roundings))


def mutated_stack(cfg, ck, x_block0, mutation, block=1):
    """exact_stack with one mutation in block `block` (CPU test and planted-mistake checks only)."""
    return stack_of(cfg, ck).run(x_block0, mut=mutation, mut_block=block)


def e_round(cfg, ck, x_block0, exact=None):
    """The rounding noise of the documented bf16 points on these rows: stat(exact - rounded). Computed from the two references alone."""
    exact = exact_stack(cfg, ck, x_block0) if exact is None else exact
    return stat(exact - rounded_stack(cfg, ck, x_block0))


# ---- planted attention -----------------------------------------------------------------------------------------------------------------
def permutations(T):
    i = np.arange(T)
    return [i, T - 1 - i, (i + 64) % T]                      # head 0: identity, head 1: reversal, head 2: +64; head 3 keeps the synthetic weights


def plant_attention(cfg, ck, audio=None, a2=A2):
    """A copy of ck whose q and k rows of heads 0..2, in every block behind block 0, make query i score a2 on key pi(i) and ~0 elsewhere.

    Per block, in order, from the exact reference's own input x to that block for the anchor window: h = LN1(x), mu = the mean of its rows,
    h - mu = U S V^T (thin SVD, r = 128 leading components), P = S_r^-1 V_r^T so that P (h_j - mu) = U_j. With M = U^T Pi U: W_k = a P,
    W_q = a M^T P, biases -W mu, and q_i . k_j = a^2 (U M U^T)_ij ~ a^2 Pi_ij. The rows are stored divided by d_head^-0.25, the scale the oracle and
    the converter both multiply q and k rows by. The v rows stay."""
    audio = anchor_audio() if audio is None else audio
    out = {k: (v.copy() if "linear_q_k_v" in k else v) for k, v in ck.items()}
    st = SanmStack(cfg, out)
    x0 = st.block0(audio)
    T, d, hd = x0.shape[0], cfg.d_model, cfg.d_head
    assert T > SVD_RANK and hd == SVD_RANK
    s = float(hd ** (-0.25))
    a = float(a2) ** 0.5
    names = [f"encoder.encoders.{i}." for i in range(cfg.n_enc)] + [f"encoder.tp_encoders.{i}." for i in range(cfg.n_tp)]
    for bi, p in enumerate(names, start=cfg.n_enc0):
        x = st.run(x0, block_fn=lambda i, x: st.orc.sanm_block(x, st.orc.blocks[i]), stop_before=bi)
        blk = st.orc.blocks[bi]
        h = F.layer_norm(x, (d,), blk["ln1"][0].to(F64), blk["ln1"][1].to(F64), 1e-5)
        mu = h.mean(dim=0)
        U, S, Vh = torch.linalg.svd(h - mu, full_matrices=False)
        U, P = U[:, :SVD_RANK], Vh[:SVD_RANK] / S[:SVD_RANK, None]
        W, B = out[p + "self_attn.linear_q_k_v.weight"], out[p + "self_attn.linear_q_k_v.bias"]
        for head, pi in enumerate(permutations(T)):
            Pi = torch.zeros(T, T, dtype=F64)
            Pi[torch.arange(T), torch.as_tensor(pi)] = 1.0
            M = U.t() @ Pi @ U
            wk, wq = a * P, a * (M.t() @ P)
            for w_, r0 in ((wq, head * hd), (wk, d + head * hd)):
                W[r0:r0 + hd] = (w_ / s).numpy().astype(np.float32)
                B[r0:r0 + hd] = (-(w_ @ mu) / s).numpy().astype(np.float32)
        # the oracle's folded copy of this block, as SenseVoiceOracle._fold_blocks makes it
        wqkv, bqkv = torch.from_numpy(W).clone(), torch.from_numpy(B).clone()
        wqkv[:-d] *= s
        bqkv[:-d] *= s
        blk["wqkv"], blk["bqkv"] = wqkv, bqkv
        st._folded.pop(bi, None)
    return out


def top_probabilities(cfg, ck, x_block0, block=1):
    """Mean over the queries of the largest probability, per head, in block `block` of the exact reference."""
    st = stack_of(cfg, ck)
    got = []
    x = st.run(x_block0, stop_before=block)
    with torch.inference_mode():
        st.block(block, x, probs=got)
    return got[0].max(dim=-1).values.mean(dim=-1).numpy(), got[0].numpy()


# ---- the fixed cases ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    """(cfg, planted checkpoint): "one" = block 0 + one block (n_tp = 0), "deep" = block 0 + three blocks, after_norm, two tp blocks."""
    cfgm, ckm = sub("config"), sub("checkpoints")
    cfg = {"one": cfgm.SenseVoiceConfig(n_enc0=1, n_enc=1, n_tp=0), "deep": cfgm.SenseVoiceConfig(n_enc0=1, n_enc=3, n_tp=2)}[name]
    return cfg, plant_attention(cfg, ckm.synth_sensevoice_checkpoint(cfg, 0))
