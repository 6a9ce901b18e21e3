"""Float64 statement of the ragged encoder attention (attn_bf16_kernel / attn_f32_kernel, csrc/kernels.hip) and of the FSMN (fsmn_kernel), the bf16
rounding twin of the attention, and inputs on which a wrong kernel fails by a wide margin.

  exact     per utterance and head softmax(q k^T) v in float64 over the keys [0, T) (keys <= the query index when causal; query head h reads k / v head
            h // kv_group), on the operand values the kernel saw (bf16-rounded for a bf16 run). Also per (query, head): vmax = max |v|, amax = max over
            the keys of sum_c |q_c k_c| -- the two figures of the f32 budget.
  rounded   the bf16 twin with the rounding points attn_bf16_kernel documents: a probability is rounded to bf16 for the P.V product RELATIVE TO THE RUNNING
            MAXIMUM of its 32-key sub-tile (p = exp(s - m_run), later rescaled in f32 by exp(m_run - m_final), which is not rounded again), the denominator
            sums the unrounded probabilities, the context is rounded to bf16 on store. It exists ONLY to measure E_round = stat(exact - rounded); it also
            stands in for a kernel in tests/test_encoder_attn_ref_cpu.py, where `mut` plants one mistake in it.
  budget    the f32 kernel's per-element bound, decode_attn_ref.budget's form: vmax * (1e-5 + 32 * 2^-24 * amax) (attn_f32_kernel uses expf).
  build     the inputs. Background: random rows at the sessions' scale (d^-1/4 on q and k, so scores ~ N(0, 1) and a key weighs ~1 / T). On top:
              planted keys       a handful of (query, key) pairs per utterance and k/v head: k = q * PLANT / |q|^2, so the score is PLANT = 11 against a
                                 background maximum near 3 and the key's weight is above 0.9; its v is a row of +-4. Positions: 0, T - 1, 31, 32, 127, 128,
                                 255, 256, the last key of the last full 32-key sub-tile and the first of the masked one, the first key of the last query
                                 block. Causal: the query is at or behind its key, some pairs sit on the diagonal, and two queries have key qi + 1
                                 planted, which they must not see. With kv_group G the pairs of k/v head g go round its G query heads, so a head mapping
                                 h % G in place of h // G reads planted keys of the wrong head.
              poisoned neighbours five coordinates of every head are reserved (zero in the background and in every key). Every query of utterance b has 1 on coordinate
                                 b % 3; the FIRST key of utterance b has POISON = 20 on coordinate (b - 1) % 3 and its LAST key on (b + 1) % 3. Inside an
                                 utterance these products are zero; one key leaked from either neighbour scores 20 for EVERY query and takes the row over.
                                 The pad rows are the probe's: 64 in every K coordinate, 1e4 in V^T. Coordinate 4 of a query makes its
                                 coordinates sum to 3, so a pad row scores 192 for EVERY query.
              peak               every query has 1 on coordinate 3; peak = "first" gives key 1, "last" key T - 2, PEAK = 13 there: every query's largest
                                 score then sits in the first sub-tile (no rescale moves afterwards) or in the last one (the rescale runs late).
  stat      (worst row's RMS, max abs) of a difference, as sanm_block_ref.stat; MARGIN is sanm_block_ref's.
  fsmn_exact / fsmn_bound   the 11-tap depth-wise convolution with zero padding inside each utterance, and the f32 kernel's bound (see fsmn_bound).

The final maximum in place of the running one is NOT the same twin: on the batches below E_round of single utterances moves by up to 78 % between the two
(rounded(..., running=False) is the simpler one), so the running maximum is modelled, as the kernel rounds p before the later rescale.
"""
import numpy as np

from decode_attn_ref import U32, bf16_round
from sanm_block_ref import MARGIN, stat  # noqa: F401  (re-exported: the comparison's statistic and margin)

RES = 5             # reserved coordinates per head
PLANT = 11.0
POISON = 20.0
PEAK = 13.0
VPLANT = 4.0
PAD_K, PAD_V = 64.0, 1e4
TAPS = 11


def geometry(max_T, hd, qt_env=None):
    """(hd, chunk, qt, waves) of the bf16 instance attention_geometry and launch_attention_bf16_hd* pick for a batch whose longest utterance has max_T keys."""
    tiles = (max_T + 15) // 16
    qt = 1 if tiles <= 8 else 2
    if qt_env is not None:
        qt = max(1, min(2, qt_env))
    return hd, (256 if hd == 64 or max_T <= 256 else 128), qt, min(8, (tiles + qt - 1) // qt)


def f32_grid_z(lens, H):
    wgs = sum((T + 63) // 64 for T in lens) * H
    return 1 if wgs >= 1024 else 4 if wgs >= 256 else 16


def _positions(T, q_rows, Tq):
    full = (T // 32) * 32
    p = {0, T - 1, 31, 32, 127, 128, 255, 256, full - 1, full, ((Tq - 1) // q_rows) * q_rows}
    return sorted(j for j in p if 0 <= j < T)


def build(lens, H, hd, seed, bf16=True, q_lens=None, G=1, causal=False, q_rows=128, peak=None):
    """The inputs of one batch, per utterance (pack() lays them out): dict(q [Tq][H][hd], k / v [T][KV][hd], plants [(query, key, head)])."""
    assert H % G == 0 and (q_lens is None or not causal)
    KV, s = H // G, hd ** -0.25
    utts = []
    for b, T in enumerate(lens):
        rng = np.random.default_rng([seed, b, T])
        Tq = T if q_lens is None else q_lens[b]
        q = rng.standard_normal((Tq, H, hd)) * s
        k = rng.standard_normal((T, KV, hd)) * s
        v = rng.standard_normal((T, KV, hd))
        q[..., :RES], k[..., :RES] = 0.0, 0.0
        q[..., b % 3], q[..., 3] = 1.0, 1.0
        q[..., 4] = 1.0 - q[..., RES:].sum(axis=-1)                     # the coordinates of every query sum to 3: a pad row (one value everywhere) scores 3 x that value
        k[0, :, (b - 1) % 3] += POISON
        k[T - 1, :, (b + 1) % 3] += POISON
        jp = None
        if peak is not None and T >= 8:
            jp = 1 if peak == "first" else T - 2
            k[jp, :, 3] = PEAK
        plants = []
        for g in range(KV):
            used_q, pairs = set(), []
            pos = [j for j in _positions(T, q_rows, Tq) if j != jp]
            edge = [j for j in ((T - 1, 0) if g % 2 == 0 else (0, T - 1)) if j in pos]
            pos = edge + [j for j in pos if j not in edge]              # few queries (the cross form's Tq = 1): the utterance's edges first, last key first on even heads
            perm = [int(i) for i in rng.permutation(Tq)]
            j_own = ((Tq - 1) // q_rows) * q_rows if Tq > len(pos) else -1       # the first key of the last query block: its query is the utterance's last
            for n, j in enumerate(pos):
                if causal:
                    i = min(T - 1, j + (n % 3) * 5)                      # at or behind its key; n % 3 == 0: on the diagonal
                elif j == j_own:
                    i = Tq - 1
                else:
                    i = next((x for x in perm if x not in used_q and (x != Tq - 1 or j_own < 0)), None)
                if i is None or i in used_q:
                    continue
                used_q.add(i)
                pairs.append((i, j))
            if causal:                                                  # the future key: planted toward query i, one row too late for it
                taken = {j for _, j in pairs}
                for i in (T // 3, (2 * T) // 3 + 1):
                    if 0 <= i and i + 1 < T and i + 1 not in taken and i not in used_q and i + 1 != jp:
                        used_q.add(i)
                        taken.add(i + 1)
                        pairs.append((i, i + 1))
            for n, (i, j) in enumerate(pairs):
                h = g * G + n % G
                qi = q[i, h, RES:]
                k[j, g, RES:] = qi * (PLANT / float(qi @ qi))
                v[j, g] = VPLANT * rng.choice([-1.0, 1.0], size=hd)
                plants.append((i, j, h))
        f = (lambda a: bf16_round(a.astype(np.float32))) if bf16 else (lambda a: a.astype(np.float32))
        utts.append(dict(q=f(q), k=f(k), v=f(v), T=T, Tq=Tq, plants=plants))
    return dict(utts=utts, H=H, hd=hd, G=G, causal=bool(causal), cross=q_lens is not None, bf16=bool(bf16))


def pack(case, order=None):
    """Dense arrays for the probe, utterance after utterance in `order`: (q [sum Tq][H hd], k, v [sum T][KV hd], key_lens, q_lens or None)."""
    us = [case["utts"][b] for b in (range(len(case["utts"])) if order is None else order)]
    cat = lambda key: np.concatenate([u[key].reshape(u[key].shape[0], -1) for u in us], axis=0)
    return cat("q"), cat("k"), cat("v"), [u["T"] for u in us], ([u["Tq"] for u in us] if case["cross"] else None)


def split(case, ctx, order=None):
    """The probe's dense context rows -> {utterance: [Tq][H hd]}."""
    out, r = {}, 0
    for b in (range(len(case["utts"])) if order is None else order):
        n = case["utts"][b]["Tq"]
        out[b] = ctx[r:r + n]
        r += n
    return out


def _utterance(case, b, twin, mut=None, running=True):
    """Utterance b -> (ctx [Tq][H hd], vmax [Tq][H], amax [Tq][H]) in float64. twin: the bf16 rounding points; mut: one planted mistake (twin only)."""
    u, H, hd, G = case["utts"][b], case["H"], case["hd"], case["G"]
    T, Tq, KV = u["T"], u["Tq"], case["H"] // case["G"]
    kind = mut[0] if mut else None
    ctx, vmax, amax = np.zeros((Tq, H, hd)), np.zeros((Tq, H)), np.zeros((Tq, H))
    qpos = np.arange(Tq)[:, None]
    for h in range(H):
        g = (h % G) % KV if kind == "head_mod" else h // G
        q, k, v = u["q"][:, h].astype(np.float64), u["k"][:, g].astype(np.float64), u["v"][:, g].astype(np.float64)
        if kind == "admit_next":
            nxt = case["utts"][b + 1]
            k, v = np.concatenate([k, nxt["k"][:1, g]]), np.concatenate([v, nxt["v"][:1, g]])
        if kind == "admit_pad":
            n = -T % 16
            k, v = np.concatenate([k, np.full((n, hd), PAD_K)]), np.concatenate([v, np.full((n, hd), PAD_V)])
        n_keys = k.shape[0]
        kpos = np.arange(n_keys)[None, :]
        s = q @ k.T
        vis = np.ones((Tq, n_keys), bool)
        if case["causal"]:
            shift = mut[1] if kind == "causal" else 0
            vis = (kpos <= qpos + shift) | (kpos == 0)
        if kind == "mask_last":
            vis[:, T - 1] = False
        if kind == "drop_key":
            vis[:, mut[1]] = False
        s = np.where(vis, s, -np.inf)
        m_fin = s.max(axis=1, keepdims=True)
        p = np.exp(s - m_fin)
        den = p.sum(axis=1, keepdims=True)
        if not twin:
            o = (p @ v) / den
        else:
            pad = -n_keys % 32
            sp = np.concatenate([s, np.full((Tq, pad), -np.inf)], axis=1).reshape(Tq, -1, 32)
            m_run = np.repeat(np.maximum.accumulate(sp.max(axis=2), axis=1), 32, axis=1)[:, :n_keys]     # (key 0 is visible to every query: finite from the start)
            if not running:
                m_run = np.broadcast_to(m_fin, m_run.shape)
            ph = bf16_round(np.exp(s - m_run).astype(np.float32)).astype(np.float64) * np.exp(m_run - m_fin)
            if kind == "den_rounded":
                den = ph.sum(axis=1, keepdims=True)
            o = bf16_round(((ph @ v) / den).astype(np.float32)).astype(np.float64)
        ctx[:, h] = o
        vmax[:, h] = np.abs(v[:T]).max()
        amax[:, h] = np.where(vis[:, :T], np.abs(q) @ np.abs(k[:T]).T, 0.0).max(axis=1)
    return ctx.reshape(Tq, H * hd), vmax, amax


def exact(case, b):
    return _utterance(case, b, twin=False)


def rounded(case, b, mut=None, running=True):
    """running=False: every probability rounded relative to the row's FINAL maximum (the simpler twin; the module docstring says how far the two are apart)."""
    return _utterance(case, b, twin=True, mut=mut, running=running)[0]


def applies(case, b, mut, chunk=None):
    """Whether the planted mistake `mut` changes what utterance b computes at all."""
    u, kind = case["utts"][b], mut[0]
    if kind == "mask_last":
        return u["T"] >= 2
    if kind == "drop_key":
        return u["T"] > mut[1]
    if kind == "admit_next":
        return b + 1 < len(case["utts"])
    if kind == "admit_pad":
        return u["T"] % 16 != 0
    if kind == "causal":
        return case["causal"] and u["T"] >= 2
    if kind == "head_mod":
        return case["G"] > 1 and case["H"] // case["G"] > 1
    return True


def budget(vmax, amax, hd):
    """Per-element bound of the f32 kernel: [Tq][H hd]."""
    return np.repeat(vmax * (1e-5 + 32 * U32 * amax), hd, axis=1)


# ---- FSMN ----------------------------------------------------------------------------------------------------------------------------------
def fsmn_exact(v, w, b, lens):
    """v [sum T][C], w [C][11], b [C] -> (out [sum T][C] in float64, S = |b| + sum_j |w_j x_j| per element): out[t] = b + sum_j w[j] v[t + j - 5], rows
    outside the utterance read as zero."""
    v, w, b = (np.asarray(a, np.float64) for a in (v, w, b))
    out, S = np.zeros_like(v), np.zeros_like(v)
    r = 0
    for T in lens:
        x = np.zeros((T + TAPS - 1, v.shape[1]))
        x[5:5 + T] = v[r:r + T]
        out[r:r + T], S[r:r + T] = b, np.abs(b)
        for j in range(TAPS):
            out[r:r + T] += w[:, j] * x[j:j + T]
            S[r:r + T] += np.abs(w[:, j] * x[j:j + T])
        r += T
    return out, S


def fsmn_bound(S):
    """fsmn_kernel computes acc = b, then 11 chained fmaf(w_j, x_j, acc) in f32: each rounds one partial sum, |partial sum| <= S (1 + u)^11 with
    S = |b| + sum_j |w_j x_j| and u = 2^-24, so |kernel - exact| <= 11 u (1 + u)^11 S; taps outside the utterance are fmaf(w, 0, acc) = acc exactly.
    The bf16 kernel widens its operands exactly, so the same bound holds on the bf16-rounded input."""
    return TAPS * U32 * (1.0 + 1e-6) * S


# ---- the fixed batches (tests/test_encoder_attn_gpu.py runs them; tests/test_encoder_attn_ref_cpu.py checks the twin on the same inputs) -------------------
L128 = [128, 113, 97, 33, 32, 31, 17, 16, 5, 1]
L256 = [256, 255, 225, 224, 160, 145, 129, 33, 16, 1]
L513 = [513, 385, 384, 300, 288, 257, 128, 31, 1]
L400 = [400, 257, 256, 129, 33, 1]
WHISPER = [1500, 1500]
TOKENS_PER_CHUNK = 13                                                   # of the Qwen3 audio encoder's conv stem (config.QwenAsrConfig.n_window)


def qwen_windows():
    """The attention window lengths of the Qwen3 audio encoder: the full windows of the three configurations, a window whose last chunk is missing, one
    chunk, and a last chunk of 7 tokens."""
    from conftest import sub
    c = sub("config")
    full = sorted({cfg.chunks_per_window * TOKENS_PER_CHUNK for cfg in (c.qwen_asr_0p6b(), c.qwen_asr_mid(), c.qwen_asr_tiny())}, reverse=True)
    return full + [full[0], full[0] - TOKENS_PER_CHUNK, TOKENS_PER_CHUNK, 7]


# name -> (head_dim, key lengths, options); the instance a batch must run is geometry(max(lens), hd, qt_env)
SELF_BATCHES = {
    "hd128_le128": (128, L128, {}), "hd128_1wave": (128, [5, 1], {}), "hd128_3waves": (128, [40, 7], {}),
    "hd128_le256": (128, L256, {}), "hd128_gt256": (128, L513, {}), "hd128_gt256_qt1": (128, L513, {"qt_env": 1}),
    "hd64_le128": (64, L128, {}), "hd64_1wave": (64, [5, 1], {}), "hd64_3waves": (64, [40, 7], {}),
    "hd64_gt128": (64, L400, {}), "hd64_whisper": (64, WHISPER, {}), "hd64_qwen": (64, None, {"packed_qk": True}),
}
PEAKS = (None, "first", "last")
# cross form (Tq != T, Tq = 1 against T = 300) and causal + grouped-query form, the smallest batch of each hd-128 instance
CROSS_BATCHES = {
    "le128": ([40, 7], [13, 7], {}), "le256": ([160, 33], [50, 20], {}), "gt256": ([300, 288, 31], [1, 100, 31], {}), "gt256_qt1": ([300, 288, 31], [1, 100, 31], {"qt_env": 1}),
}
CAUSAL_BATCHES = {"le128": ([40, 7], {}), "le256": ([160, 33], {}), "gt256": ([300, 31], {}), "gt256_qt1": ([300, 31], {"qt_env": 1})}
H_SELF = 2


def self_lens(name):
    lens = SELF_BATCHES[name][1]
    return qwen_windows() if lens is None else lens


def self_case(name, peak=None, bf16=True):
    hd, _, opt = SELF_BATCHES[name]
    lens = self_lens(name)
    inst = geometry(max(lens), hd, opt.get("qt_env"))
    return build(lens, H_SELF, hd, seed=sum(lens) + hd, bf16=bf16, q_rows=16 * inst[2] * inst[3], peak=peak), inst


def cross_case(name):
    lens, q_lens, opt = CROSS_BATCHES[name]
    inst = geometry(max(lens), 128, opt.get("qt_env"))
    return build(lens, H_SELF, 128, seed=7 + sum(lens), q_lens=q_lens, q_rows=16 * inst[2] * inst[3]), inst


def causal_case(name, G):
    lens, opt = CAUSAL_BATCHES[name]
    inst = geometry(max(lens), 128, opt.get("qt_env"))
    return build(lens, 4, 128, seed=11 + sum(lens) + G, G=G, causal=True, q_rows=16 * inst[2] * inst[3]), inst
