"""The SANM block references (tests/sanm_block_ref.py) checked on the CPU: the inputs make attention, FSMN and FFN errors visible, the planting does what
it says, and the rounded reference is the exact one with rounding points added.

The GPU test (test_sanm_block_ref_gpu.py) lets a kernel differ from exact_stack by 3 x E_round per window and statistic. That bound only means something
if the mistakes it is meant to catch move the output further than that: here every mutation of the exact reference must move it by at least twice the
bound, on every window of the one-block case. This is a condition on the inputs (planted weights, windows), computed from the references alone."""
import numpy as np
import pytest
import torch

import sanm_block_ref as R


@pytest.fixture(scope="module")
def one():
    """Per window of the one-block case: the oracle's float64 rows behind block 0, exact_stack of them, and the bound 3 x E_round."""
    cfg, ck = R.case("one")
    st = R.stack_of(cfg, ck)
    rows = []
    for T, a in zip(R.WINDOWS, R.window_audios()):
        x0 = st.block0(a)
        assert x0.shape == (T, cfg.d_model)
        exact = R.exact_stack(cfg, ck, x0)
        rows.append((T, x0, exact, tuple(R.MARGIN * e for e in R.e_round(cfg, ck, x0, exact))))
    return cfg, ck, rows


def mutations(T):
    """What the issue names, where it exists in a window of T rows."""
    m = [R.mask_key(j) for j in sorted({0, 15, 16, 31, 32, 127, 128, T - 1}) if 0 <= j < T]
    taps = [(T - 1, -5), (0, 5)] + [(row, tap) for row in (127, 128) for tap in (-5, 5)]
    m += [R.drop_tap(row, tap) for row, tap in taps if 0 <= row < T and 0 <= row + tap < T]
    return m + [R.zero_hidden(T - 1)]


def test_every_mutation_moves_the_output_beyond_twice_the_bound(one):
    cfg, ck, rows = one
    for T, x0, exact, bound in rows:
        assert 0.005 < bound[0] < 0.02 and 0.02 < bound[1] < 0.1, (T, bound)           # 3 x (bf16 noise of one block): neither vacuous nor unattainable
        muts = mutations(T)
        assert len(muts) >= (3 if T == 5 else 8)
        for m in muts:
            got = R.stat(R.mutated_stack(cfg, ck, x0, m) - exact)
            print(T, m, "rms %.4f max %.4f" % got, "bound %.4f %.4f" % bound)
            assert got[0] >= 2 * bound[0] and got[1] >= 2 * bound[1], (T, m, got, bound)


def test_planted_heads_are_sharp_but_not_one_hot(one):
    cfg, ck, rows = one
    T, x0, _, _ = rows[0]
    assert T == R.ANCHOR_T
    top, p = R.top_probabilities(cfg, ck, x0)
    assert all(0.5 <= t <= 0.98 for t in top[:3]), top                 # the other keys still count
    assert top[3] < 0.05, top                                          # head 3 keeps the synthetic near-uniform weights
    for head, pi in enumerate(R.permutations(T)):
        assert np.array_equal(p[head].argmax(axis=1), pi), head


def test_planted_weights_keep_their_pattern_through_bf16(one):
    """A bf16 session sees the planted rows rounded: the arg-max pattern of every planted head must survive that (weights up to 0.83 in magnitude)."""
    cfg, ck, rows = one
    T, x0, _, _ = rows[0]
    st = R.stack_of(cfg, ck)
    got = []
    with torch.inference_mode():
        st.block(1, torch.as_tensor(x0), rnd=frozenset({"w"}), probs=got)
    p = got[0].numpy()
    for head, pi in enumerate(R.permutations(T)):
        assert np.array_equal(p[head].argmax(axis=1), pi), head
    w = ck["encoder.encoders.0.self_attn.linear_q_k_v.weight"]
    assert 0.3 < np.abs(w[:2 * cfg.d_model]).max() < 1.5
    raw = R.sub("checkpoints").synth_sensevoice_checkpoint(cfg, 0)["encoder.encoders.0.self_attn.linear_q_k_v.weight"]
    assert np.array_equal(w[2 * cfg.d_model:], raw[2 * cfg.d_model:])                   # the v rows are left alone
    h3 = slice(3 * cfg.d_head, 4 * cfg.d_head)
    assert np.array_equal(w[:cfg.d_model][h3], raw[:cfg.d_model][h3])                   # ... and so is head 3


@pytest.mark.parametrize("name", ["one", "deep"])
def test_rounded_reference_without_roundings_is_the_exact_one(name):
    """exact_stack is the oracle's own sanm_block; rounded_stack folds the LayerNorm affines as the converter does. Same function to 1e-10."""
    cfg, ck = R.case(name)
    st = R.stack_of(cfg, ck)
    for T, a in zip(R.WINDOWS, R.window_audios()):
        if name == "deep" and T not in (144, 129, 5):
            continue
        x0 = st.block0(a)
        exact = R.exact_stack(cfg, ck, x0)
        assert np.abs(R.rounded_stack(cfg, ck, x0, roundings=()) - exact).max() < 1e-10
        e = R.e_round(cfg, ck, x0, exact)
        assert e[0] > 1e-3                                                               # ... and the roundings do something


def test_windows_are_truncations_with_the_named_lengths():
    cfg, _ = R.case("one")
    a = R.anchor_audio()
    for T, w in zip(R.WINDOWS, R.window_audios()):
        assert cfg.seq_len(w.size) == T and np.array_equal(w, a[:w.size])
    assert sum((T + 15) // 16 for T in R.WINDOWS) == 72                                  # more than the tile kernel's 64: its path runs two batches of five
