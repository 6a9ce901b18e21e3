"""The ragged encoder attention (attn_bf16_kernel, attn_f32_kernel) and the FSMN (fsmn_kernel) of csrc/kernels.hip against their float64 statements
(tests/encoder_attn_ref.py), through probes that lay the operands out as a session does (asr_probe_encoder_attention, asr_probe_fsmn).

These are the attention of the Whisper encoder (hd 64, 1500 keys), of the Qwen3 audio encoder (hd 64, windows, q|k in one buffer), of every SenseVoice /
Paraformer block above 144 rows and of the Paraformer decoder's cross attention (hd 128), and of the Qwen3 prefill (hd 128, causal, grouped-query).

bf16: every utterance of every batch is held to stat(got - exact) <= 3 x E_round, both statistics (worst row's RMS, max abs; equality where E_round is zero),
E_round = stat(exact - rounded) from the two references alone; no utterance is left out. The inputs carry planted keys, poisoned neighbours and poisoned pad
rows (encoder_attn_ref.build): the planted mistakes that this comparison catches, and by how much, are in tests/test_encoder_attn_ref_cpu.py. Each batch
asserts the instance <HD, CHUNK, QT> and the waves per workgroup that ran, and runs three times: as built, with every query's largest score in the first
32-key sub-tile (the rescale never moves again), and with it in the last one (the rescale runs late). Also asserted: nothing outside the query rows of the
context buffer is written; with slack_rows = 0 (the last utterance has 1 .. 16 rows, so its 32-key sub-tile reaches past the buffers and both staging clamps
act) and with zeros in place of the poison the results are the padded run's bit for bit; the batch in reverse order gives every utterance the same bits.

Measured on an MI355X, worst utterance of each batch, stat / E_round (RMS ratio, then max-abs ratio), for the three runs:

    batch              instance <HD,CHUNK,QT> x waves   as built    peak first  peak last
    hd128_le128        <128,256,1> x 8                  1.00 1.00   1.00 1.00   1.00 1.00
    hd128_1wave        <128,256,1> x 1                  1.00 1.00   1.00 1.00   1.00 1.00
    hd128_3waves       <128,256,1> x 3                  1.00 1.00   1.00 1.00   1.00 1.00
    hd128_le256        <128,256,2> x 8                  1.00 1.00   1.00 1.00   1.01 1.00
    hd128_gt256        <128,128,2> x 8                  1.00 1.00   1.00 1.00   1.00 1.00
    hd128_gt256_qt1    <128,128,1> x 8 (ASR_ATTN_QT=1)  1.00 1.00   1.00 1.00   1.00 1.00
    hd64_le128         <64,256,1> x 8                   1.00 1.00   1.00 1.00   1.00 1.00
    hd64_1wave         <64,256,1> x 1                   1.00 1.00   1.00 1.00   1.00 1.00
    hd64_3waves        <64,256,1> x 3                   1.00 1.00   1.00 1.00   1.00 1.00
    hd64_gt128         <64,256,2> x 8                   1.00 1.00   1.00 1.00   1.00 1.00
    hd64_whisper       <64,256,2> x 8                   1.00 1.00   1.00 1.00   1.00 1.00
    hd64_qwen (q|k)    <64,256,1> x 7                   1.00 1.00   1.00 1.00   1.00 1.00
    cross  (hd 128)    le128 <128,256,1> x 3, le256 <128,256,2> x 5, gt256 <128,128,2> x 8, gt256_qt1 <128,128,1> x 8      1.00 1.00 each
    causal (hd 128)    the same four instances, G = 2 and 4                                                             1.00 1.00 each

The kernel sits on the twin: to three digits every figure is 1.000 but one (1.009), so nothing beyond the documented rounding points shows. No product bug
was found by these tests; the one defect fixed with them was read from the code (the f32 launcher took more keys than its LDS row holds, below).

ASR_ATTN_QT is read at every call (attention_geometry), so <128,128,1> is reached by setting it; all six instances are asserted to have run.

f32 (attn_f32_kernel, expf): |got - exact| <= vmax (1e-5 + 32 2^-24 amax) per element (decode_attn_ref.budget's form). Worst |got - exact| / bound:

    hd 64   z = 16: 0.04   z = 4: 0.03   z = 1: 0.03   T = 2048: 0.11          hd 128   z = 16: 0.04   z = 4: 0.03   z = 1: 0.02   cross: 0.05

The batches of gridDim.z = 4 and 1 are run again in groups of 32 utterances (z = 16 each) and give the same bits. launch_attention_f32 refuses a longest
utterance above 2048 keys (the kernel's LDS score row); the test sends 2049 through the probe, where no kernel is launched.

FSMN (bf16 and f32 input): |got - exact| <= 11 2^-24 (|b| + sum |w x|) (encoder_attn_ref.fsmn_bound), worst ratio 0.36; with a single tap of 1 at offset
-5 or +5 every output row is fl32(bias + that neighbour's row), or the bias itself where the neighbour lies outside the utterance, compared for equality;
V^T's pad columns hold 1e4; pad rows of the output are zero.

NOT covered: Tq > T in the cross form -- no session produces it (the CIF fires at most T tokens: every alpha is a sigmoid below 1 and the tail threshold is
below 1) and the sessions lay the query blocks over the key rows, so the probe refuses it; NaN / Inf in pad rows, which is outside the contract (AttnArgs,
csrc/kernels.h); the f32 kernel has no causal / grouped-query form; a denominator summed from the bf16-rounded probabilities is not a mistake a bound against
`exact` can see (tests/test_encoder_attn_ref_cpu.py says why).
"""
import functools

import numpy as np
import pytest

import encoder_attn_ref as R
from conftest import sub

pytestmark = pytest.mark.gpu

SELF = tuple(R.SELF_BATCHES)
TIGHT = tuple(n for n in SELF if R.self_lens(n)[-1] <= 16)


def _probe():
    return sub("_probe")


@pytest.fixture(autouse=True)
def _geometry_env(monkeypatch):
    for name in ("ASR_ATTN_QT", "ASR_ATTN_NW"):
        monkeypatch.delenv(name, raising=False)


@functools.lru_cache(maxsize=None)
def _self(name, peak):
    case, inst = R.self_case(name, peak)
    return case, inst, _refs(case)


def _refs(case):
    """[(exact, E_round)] per utterance."""
    out = []
    for b in range(len(case["utts"])):
        ex = R.exact(case, b)[0]
        out.append((ex, R.stat(ex - R.rounded(case, b))))
    return out


def _run(case, monkeypatch, opt=None, order=None, **kw):
    opt = opt or {}
    if "qt_env" in opt:
        monkeypatch.setenv("ASR_ATTN_QT", str(opt["qt_env"]))
    q, k, v, lens, q_lens = R.pack(case, order)
    out = _probe().encoder_attention(q, k, v, lens, case["H"], case["hd"], bf16=case["bf16"], q_lens=q_lens, kv_group=case["G"], causal=case["causal"],
                                     packed_qk=bool(opt.get("packed_qk")), **kw)
    out["utts"] = R.split(case, out["ctx"], order)
    return out


def _hold(case, refs, out, label):
    """Every utterance within MARGIN x E_round of the exact reference; prints the worst ratios."""
    assert out["stray"] == 0, f"{label}: {out['stray']} context elements outside the query rows were written"
    worst, bad = [0.0, 0.0], []
    for b, (ex, e) in enumerate(refs):
        got = out["utts"][b]
        assert np.isfinite(got).all(), f"{label}: utterance {b} is not finite"
        g = R.stat(got - ex)
        for i in range(2):
            ratio = g[i] / e[i] if e[i] > 0 else (0.0 if g[i] == 0 else np.inf)
            worst[i] = max(worst[i], ratio)
            if not (g[i] <= R.MARGIN * e[i]):
                bad.append((b, case["utts"][b]["T"], ("rms", "max")[i], g[i], e[i]))
    print(f"ENCATTN {label}: stat / E_round = {worst[0]:.3f} {worst[1]:.3f}")
    assert not bad, f"{label}: (utterance, T, statistic, got, E_round) beyond {R.MARGIN} x E_round: {bad[:8]}"


@pytest.mark.parametrize("peak", R.PEAKS)
@pytest.mark.parametrize("name", SELF)
def test_self_attention_bf16(monkeypatch, name, peak):
    case, inst, refs = _self(name, peak)
    out = _run(case, monkeypatch, R.SELF_BATCHES[name][2])
    assert out["instance"] == inst and out["grid_z"] == 0, (out["instance"], inst)
    _hold(case, refs, out, f"{name} peak={peak} {inst}")


@pytest.mark.parametrize("name", TIGHT)
def test_tight_allocation_and_other_poison_give_the_same_bits(monkeypatch, name):
    """slack_rows = 0: n_rows_alloc == ld_vt == the sum of the rounded lengths, the last utterance's sub-tile reaches past both buffers."""
    case, inst, _ = _self(name, None)
    opt = R.SELF_BATCHES[name][2]
    padded = _run(case, monkeypatch, opt)
    tight = _run(case, monkeypatch, opt, slack_rows=0)
    zeros = _run(case, monkeypatch, opt, pad_fill_k=0.0, pad_fill_v=0.0)
    assert tight["instance"] == padded["instance"] == inst
    assert tight["stray"] == 0 and zeros["stray"] == 0
    assert np.array_equal(tight["ctx"], padded["ctx"])
    assert np.array_equal(zeros["ctx"], padded["ctx"])


@pytest.mark.parametrize("name", SELF)
def test_an_utterance_does_not_depend_on_its_neighbours(monkeypatch, name):
    case, inst, _ = _self(name, None)
    opt = R.SELF_BATCHES[name][2]
    fwd = _run(case, monkeypatch, opt)
    order = list(range(len(case["utts"])))[::-1]
    rev = _run(case, monkeypatch, opt, order=order)
    assert rev["instance"] == fwd["instance"] == inst
    for b in order:
        assert np.array_equal(fwd["utts"][b], rev["utts"][b]), f"utterance {b} (T = {case['utts'][b]['T']}) changes with its neighbours"


@pytest.mark.parametrize("name", tuple(R.CROSS_BATCHES))
def test_cross_attention_bf16(monkeypatch, name):
    case, inst = R.cross_case(name)
    out = _run(case, monkeypatch, R.CROSS_BATCHES[name][2])
    assert out["instance"] == inst, (out["instance"], inst)
    _hold(case, _refs(case), out, f"cross {name} {inst}")


@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("name", tuple(R.CAUSAL_BATCHES))
def test_causal_grouped_query_attention_bf16(monkeypatch, name, G):
    case, inst = R.causal_case(name, G)
    assert any(j == i + 1 for u in case["utts"] for i, j, _ in u["plants"]) and any(j == i for u in case["utts"] for i, j, _ in u["plants"])
    out = _run(case, monkeypatch, R.CAUSAL_BATCHES[name][1])
    assert out["instance"] == inst, (out["instance"], inst)
    _hold(case, _refs(case), out, f"causal {name} G={G} {inst}")


# ---- f32 -------------------------------------------------------------------------------------------------------------------------------------
F32_BATCHES = {
    16: (2, [137, 45, 1, 64, 129]),
    4: (4, [(37 * i) % 64 + 1 for i in range(64)]),                      # 64 utterances of T <= 64, 4 heads: 256 workgroups
    1: (4, [5 + (7 * i) % 16 for i in range(256)]),                      # 256 utterances of T in 5 .. 20, 4 heads: 1024 workgroups
}


def _hold_f32(case, out, label, hd):
    assert out["stray"] == 0
    worst = 0.0
    for b in range(len(case["utts"])):
        ex, vmax, amax = R.exact(case, b)
        ratio = float((np.abs(out["utts"][b] - ex) / R.budget(vmax, amax, hd)).max())
        worst = max(worst, ratio)
    print(f"ENCATTN f32 {label}: |got - exact| / bound = {worst:.3f}")
    assert worst <= 1.0, f"{label}: {worst} x the f32 bound"


@pytest.mark.parametrize("z", [16, 4, 1])
@pytest.mark.parametrize("hd", [64, 128])
def test_self_attention_f32(monkeypatch, hd, z):
    H, lens = F32_BATCHES[z]
    assert R.f32_grid_z(lens, H) == z
    case = R.build(lens, H, hd, seed=100 + z + hd, bf16=False, q_rows=64)
    out = _run(case, monkeypatch)
    assert out["grid_z"] == z and out["instance"] == (hd, 0, 0, 4), (out["grid_z"], out["instance"])
    _hold_f32(case, out, f"hd {hd} z = {z}", hd)
    if z != 16:                                                          # the same utterances in groups that get z = 16: the split leaves a row's arithmetic alone
        for g0 in range(0, len(lens), 32):
            order = list(range(g0, min(g0 + 32, len(lens))))
            part = _run(case, monkeypatch, order=order)
            assert part["grid_z"] == 16
            for b in order:
                assert np.array_equal(part["utts"][b], out["utts"][b]), f"utterance {b}: z = {z} and z = 16 differ"


def test_cross_attention_f32(monkeypatch):
    case = R.build([300, 40], 2, 128, seed=5, bf16=False, q_lens=[1, 13], q_rows=64)
    out = _run(case, monkeypatch)
    assert out["grid_z"] == 16
    _hold_f32(case, out, "hd 128 cross", 128)


def test_f32_takes_2048_keys(monkeypatch):
    case = R.build([2048], 1, 64, seed=9, bf16=False, q_rows=64)
    out = _run(case, monkeypatch)
    assert out["grid_z"] == 16
    _hold_f32(case, out, "hd 64 T = 2048", 64)


def test_f32_refuses_more_keys_than_its_score_row_holds():
    """launch_attention_f32 throws before any launch: attn_f32_kernel keeps a row's scores in 2048 floats of LDS per wave."""
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2049, 64)).astype(np.float32)
    with pytest.raises(sub("_lib").AsrError, match=r"2049.*2048"):
        _probe().encoder_attention(x, x, x, [2049], 1, 64, bf16=False)


# ---- FSMN ------------------------------------------------------------------------------------------------------------------------------------
FSMN_LENS = ([300, 137, 65, 64, 63, 9, 8, 7, 1], [17, 18, 19, 20, 21, 22, 23, 24])           # block edges; every residue of T mod 8
FSMN_C = 128


def _fsmn_input(lens, bf16):
    rng = np.random.default_rng(sum(lens))
    v = rng.standard_normal((sum(lens), FSMN_C)).astype(np.float32)
    return R.bf16_round(v) if bf16 else v


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("lens", FSMN_LENS, ids=("edges", "residues"))
def test_fsmn_against_float64(lens, bf16):
    rng = np.random.default_rng(3)
    v = _fsmn_input(lens, bf16)
    w = rng.standard_normal((FSMN_C, R.TAPS)).astype(np.float32)
    b = rng.standard_normal(FSMN_C).astype(np.float32)
    got, stray = _probe().fsmn(v, w, b, lens, bf16=bf16)
    ex, S = R.fsmn_exact(v, w, b, lens)
    ratio = float((np.abs(got - ex) / R.fsmn_bound(S)).max())
    print(f"ENCATTN fsmn bf16={bf16} {lens[:2]}..: |got - exact| / bound = {ratio:.3f}")
    assert stray == 0
    assert ratio <= 1.0


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("offset", [-5, 5])
@pytest.mark.parametrize("lens", FSMN_LENS, ids=("edges", "residues"))
def test_fsmn_single_tap_is_one_neighbouring_row(lens, offset, bf16):
    v = _fsmn_input(lens, bf16)
    w = np.zeros((FSMN_C, R.TAPS), np.float32)
    w[:, 5 + offset] = 1.0
    b = np.linspace(-2.0, 2.0, FSMN_C).astype(np.float32)
    got, stray = _probe().fsmn(v, w, b, lens, bf16=bf16)
    want, r = np.empty_like(v), 0
    for T in lens:
        for t in range(T):
            src = t + offset
            want[r + t] = b + v[r + src] if 0 <= src < T else b           # (float32 addition: fmaf(1, x, b))
        r += T
    assert stray == 0
    assert np.array_equal(got, want)
