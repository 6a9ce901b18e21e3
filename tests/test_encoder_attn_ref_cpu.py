"""The references of tests/encoder_attn_ref.py, without a GPU: the comparison of tests/test_encoder_attn_gpu.py catches planted mistakes, and the twin passes it.

The rounded twin stands in for a kernel. Each mistake is planted in it and the mutated twin is put through the GPU module's own comparison,
stat(got - exact) <= 3 x E_round per utterance; it must FAIL on every utterance the mistake applies to. Smallest failing ratio stat / E_round over those
utterances (the larger of the RMS and the max-abs ratio), over the batches named:

    key T - 1 masked                                   every self and cross batch           511    (T >= 2)
    first key of the second chunk dropped              hd128_gt256, hd128_gt256_qt1 (key 128)  538    (T > 128)
                                                       hd64_gt128, hd64_whisper (key 256)   509    (T > 256)
    one row of the next utterance admitted             every self and cross batch           1010   (all but the last utterance)
    pad rows admitted (K = 64, V^T = 1e4)              every self batch                     1.45e6 (T % 16 != 0)
    causal mask one key too far (sees key qi + 1)      the causal batches, G = 2 and 4      509    (T >= 2)
    causal mask one key short (misses the diagonal)    the causal batches, G = 2 and 4      526    (T >= 2)
    head mapping h % G in place of h // G              the causal batches, G = 2            943    (every utterance)
    (G = 4 with 4 query heads has ONE k/v head: both mappings read it, nothing to catch)

NOT catchable by this comparison: a denominator summed from the bf16-ROUNDED probabilities. The rounding of p is relative (2^-9 at most) and the largest
probability of a row is exactly 1, so the denominator moves by a fraction of 2^-9 in either direction, which is a fraction of the context's own bf16
rounding: over all self batches the mutated twin sits at 0.90 .. 1.14 x E_round, inside the margin of 3 that exists to absorb single roundings. A bound
against `exact` cannot separate the two conventions; the test below asserts that figure so that this paragraph stays true, and does not claim a catch.

Also here: the twin itself stays within its own bound on every input of the GPU module with nothing excluded (trivially 1.00 -- the point is that E_round is
finite and that `exact` and `rounded` agree on the key sets), every planted key weighs above 0.9 in the as-built batches, the f32 budget holds for a float32
evaluation of the reference, and fsmn_exact equals torch.nn.functional.conv1d in float64.
"""
import functools

import numpy as np
import pytest
import torch

import encoder_attn_ref as R

SELF = tuple(R.SELF_BATCHES)


@functools.lru_cache(maxsize=None)
def _self(name, peak=None):
    case, inst = R.self_case(name, peak)
    return case, inst


@functools.lru_cache(maxsize=None)
def _causal(name, G):
    return R.causal_case(name, G)


def _ratio(case, b, got):
    """The comparison of the GPU module on utterance b -> (passes, the larger of the two ratios stat / E_round)."""
    ex = R.exact(case, b)[0]
    e, g = R.stat(ex - R.rounded(case, b)), R.stat(got - ex)
    ok = all(gi <= R.MARGIN * ei for gi, ei in zip(g, e))
    return ok, max((gi / ei if ei > 0 else (0.0 if gi == 0 else np.inf)) for gi, ei in zip(g, e))


def _must_fail(case, mut, label):
    """The mutated twin fails the comparison on EVERY utterance the mistake applies to; returns the smallest ratio among them."""
    smallest, n = np.inf, 0
    for b in range(len(case["utts"])):
        if not R.applies(case, b, mut):
            continue
        ok, ratio = _ratio(case, b, R.rounded(case, b, mut=mut))
        assert not ok, f"{label}: {mut} passes on utterance {b} (T = {case['utts'][b]['T']}) at {ratio:.2f} x E_round"
        smallest, n = min(smallest, ratio), n + 1
    print(f"ENCATTN-CPU {label} {mut}: smallest failing ratio {smallest:.3g} over {n} utterances")
    return n


@pytest.mark.parametrize("peak", R.PEAKS)
@pytest.mark.parametrize("name", SELF)
def test_the_twin_passes_its_own_comparison(name, peak):
    case, _ = _self(name, peak)
    for b, u in enumerate(case["utts"]):
        ro = R.rounded(case, b)
        assert np.isfinite(ro).all()
        ok, ratio = _ratio(case, b, ro)
        assert ok and ratio <= 1.0, (name, b, ratio)


@pytest.mark.parametrize("name", SELF)
def test_planted_keys_carry_their_rows(name):
    """Every planted (query, key, head): the key's soft-max weight is above 0.9 and the query's context row is within 0.5 of 0.9 x its +-4 row."""
    case, _ = _self(name)
    hd = case["hd"]
    for b, u in enumerate(case["utts"]):
        assert u["plants"], (name, b)
        ex = R.exact(case, b)[0].reshape(u["Tq"], case["H"], hd)
        for i, j, h in u["plants"]:
            s = u["q"][:, h].astype(np.float64)[i] @ u["k"][:, h // case["G"]].astype(np.float64).T
            w = np.exp(s - s.max())
            w /= w.sum()
            assert int(w.argmax()) == j and w[j] > 0.9, (name, b, i, j, h, float(w[j]))
            assert np.abs(ex[i, h] - u["v"][j, h // case["G"]]).max() < 1.0


@pytest.mark.parametrize("name", SELF)
def test_a_masked_last_key_an_admitted_neighbour_and_admitted_pad_rows_are_caught(name):
    case, _ = _self(name)
    n = sum(_must_fail(case, mut, name) for mut in (("mask_last",), ("admit_next",), ("admit_pad",)))
    assert n > 0


@pytest.mark.parametrize("name,key", [("hd128_gt256", 128), ("hd128_gt256_qt1", 128), ("hd64_gt128", 256), ("hd64_whisper", 256)])
def test_a_dropped_first_key_of_the_second_chunk_is_caught(name, key):
    case, inst = _self(name)
    assert inst[1] == key
    assert _must_fail(case, ("drop_key", key), name) > 0


@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("name", tuple(R.CAUSAL_BATCHES))
def test_a_causal_mask_off_by_one_is_caught(name, G):
    case, _ = _causal(name, G)
    for shift in (1, -1):
        assert _must_fail(case, ("causal", shift), f"causal {name} G={G}") > 0


@pytest.mark.parametrize("name", tuple(R.CAUSAL_BATCHES))
def test_a_wrong_head_mapping_is_caught(name):
    case, _ = _causal(name, 2)
    assert _must_fail(case, ("head_mod",), f"causal {name} G=2") == len(case["utts"])
    one_kv, _ = _causal(name, 4)                                  # 4 query heads on one k/v head: h % G and h // G cannot differ
    assert not any(R.applies(one_kv, b, ("head_mod",)) for b in range(len(one_kv["utts"])))


@pytest.mark.parametrize("name", tuple(R.CROSS_BATCHES))
def test_the_cross_batches_are_caught_too(name):
    case, _ = R.cross_case(name)
    assert all(u["Tq"] <= u["T"] for u in case["utts"]) and any(u["Tq"] != u["T"] for u in case["utts"])
    assert _must_fail(case, ("mask_last",), f"cross {name}") > 0
    assert _must_fail(case, ("admit_next",), f"cross {name}") > 0


def test_a_denominator_of_rounded_probabilities_cannot_be_seen():
    """It stays inside the margin (module docstring): recorded, and asserted so that the docstring stays true."""
    lo, hi = np.inf, 0.0
    for name in SELF:
        case, _ = _self(name)
        for b in range(len(case["utts"])):
            ok, ratio = _ratio(case, b, R.rounded(case, b, mut=("den_rounded",)))
            assert ok and ratio <= 1.5, (name, b, ratio)
            if case["utts"][b]["T"] > 1:
                lo, hi = min(lo, ratio), max(hi, ratio)
    print(f"ENCATTN-CPU den_rounded: {lo:.2f} .. {hi:.2f} x E_round")


def test_f32_budget_holds_for_a_float32_evaluation():
    """The reference evaluated in float32 (numpy's own summation order) stays inside the f32 budget: the bound is not tighter than f32 arithmetic allows."""
    case = R.build([137, 45, 1, 64, 129], 2, 128, seed=1, bf16=False, q_rows=64)
    for b, u in enumerate(case["utts"]):
        ex, vmax, amax = R.exact(case, b)
        got = np.zeros((u["Tq"], 2, 128), np.float32)
        for h in range(2):
            s = u["q"][:, h] @ u["k"][:, h].T
            p = np.exp(s - s.max(axis=1, keepdims=True))
            got[:, h] = (p @ u["v"][:, h]) / p.sum(axis=1, keepdims=True)
        assert (np.abs(got.reshape(u["Tq"], -1) - ex) <= R.budget(vmax, amax, 128)).all()


@pytest.mark.parametrize("lens", ([300, 137, 65, 64, 63, 9, 8, 7, 1], [17, 18, 19, 20, 21, 22, 23, 24]))
def test_fsmn_reference_is_conv1d(lens):
    rng = np.random.default_rng(2)
    C = 16
    v, w, b = rng.standard_normal((sum(lens), C)), rng.standard_normal((C, R.TAPS)), rng.standard_normal(C)
    out, S = R.fsmn_exact(v, w, b, lens)
    r = 0
    for T in lens:
        x = torch.from_numpy(v[r:r + T]).t().unsqueeze(0)
        ref = torch.nn.functional.conv1d(x, torch.from_numpy(w).unsqueeze(1), torch.from_numpy(b), padding=5, groups=C)[0].t().numpy()
        assert np.abs(out[r:r + T] - ref).max() < 1e-13
        assert (S[r:r + T] >= np.abs(ref) - 1e-13).all()
        r += T
    # one dropped tap is far outside the f32 bound
    w2 = w.copy()
    w2[:, 3] = 0.0
    assert (np.abs(R.fsmn_exact(v, w2, b, lens)[0] - out) > R.fsmn_bound(S)).mean() > 0.9
