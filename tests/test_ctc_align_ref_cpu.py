"""The reference statements of the CTC forced alignment (tests/ctc_align_ref.py) against brute force, against each other where f32 is exact, on the hand cases of
every tie rule -- and a check that the GPU file's inputs would notice a broken rule."""
import numpy as np
import pytest

import ctc_align_ref as ref

F32 = np.float32
PATTERNS = {0: [[]], 1: [[3]], 2: [[3, 4], [3, 3]], 3: [[3, 4, 5], [3, 3, 4], [3, 4, 4], [3, 3, 3], [3, 4, 3]]}


def _check_against_brute(em, targets):
    best, arg, tot = ref.brute(em, targets)
    for fn in (ref.align64, ref.align32):
        got = fn(em, targets)
        if best == -np.inf:
            assert got["status"] == 1 and got["path_score"] == -np.inf and got["loglik"] == -np.inf
            continue
        assert got["status"] == 0
        assert float(got["path_score"]) == best                       # (the emissions are on a grid: every sum is exact in f32 and float64)
        assert tuple(int(s) for s in got["states"]) in arg
        if fn is ref.align64:
            assert abs(got["loglik"] - tot) <= 1e-12 * max(1.0, abs(tot))
        for j in range(len(targets)):                                 # the spans are the rows of the odd states
            rows = [t for t, s in enumerate(got["states"]) if s == 2 * j + 1]
            assert rows and got["first"][j] == rows[0] and got["last"][j] == rows[-1] and rows == list(range(rows[0], rows[-1] + 1))


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("L", [0, 1, 2, 3])
def test_both_statements_match_brute_force(T, L):
    for targets in PATTERNS[L]:
        for seed in range(3):
            _check_against_brute(ref.em_grid(100 * T + 10 * L + seed, T, L), targets)
            _check_against_brute(ref.em_coarse(100 * T + 10 * L + seed, T, L), targets)      # many maximisers: the chosen one must be among them
        em = ref.em_grid(7, T, L)
        if L:
            em[:, 1] = -np.inf                                        # a dead slot: infeasible
            _check_against_brute(em, targets)
        em = ref.em_grid(8, T, L)
        em[T // 2, 0] = -np.inf                                       # a blank that one row forbids
        _check_against_brute(em, targets)


@pytest.mark.parametrize("T,L,kind", [(700, 40, "grid"), (700, 300, "grid"), (64, 20, "grid"), (130, 40, "coarse"), (700, 511, "grid")])
def test_f32_and_float64_agree_exactly_on_the_grid(T, L, kind):
    """|em| <= 16 on a 2^-8 grid, T <= 700: every partial sum is exact in f32, so path, spans and score are identical and planted ties are ties in both."""
    em = ref.em_grid(T + L, T, L) if kind == "grid" else ref.em_coarse(T + L, T, L)
    assert np.abs(em).max() <= 16 and np.all(em * 256 == np.round(em * 256))
    targets = ref.targets_random(L, L)
    a, b = ref.align64(em, targets), ref.align32(em, targets)
    assert a["status"] == b["status"] == 0
    assert float(b["path_score"]) == a["path_score"]
    assert np.array_equal(a["states"], b["states"]) and np.array_equal(a["first"], b["first"]) and np.array_equal(a["last"], b["last"])
    assert a["loglik"] >= a["path_score"] and a["budget"] > 0


@pytest.mark.parametrize("name", sorted(ref.hand_cases()))
def test_hand_cases_of_the_tie_rules(name):
    em, targets, want = ref.hand_cases()[name]
    for fn in (ref.align64, ref.align32):
        got = fn(em, targets)
        assert got["status"] == 0 and list(got["states"]) == want, (name, got["states"])
    best, arg, _ = ref.brute(em, targets)
    assert tuple(want) in arg and float(ref.align32(em, targets)["path_score"]) == best
    if name in ("stay_vs_step", "step1_vs_step2", "final_odd_vs_even"):
        assert len(arg) > 1                                           # the case really is a tie
    flips = {"stay_vs_step": "tie_larger_move", "step1_vs_step2": "tie_larger_move", "final_odd_vs_even": "tie_final_blank", "forbidden_skip": "no_repeat_rule"}
    if name in flips:
        assert list(ref.mutant(flips[name], em, targets)["states"]) != want


def test_never_nan_with_inf_emissions():
    for name, em, targets in ref.gpu_groups()["inf"]:
        for fn in (ref.align64, ref.align32):
            got = fn(em, targets)
            assert not np.isnan(got["path_score"]) and not np.isnan(got["loglik"])
            assert (got["status"] == 1) == name.endswith("infeasible"), name


def _answer(r):
    return (r["status"], float(r["path_score"]), None if r["states"] is None else tuple(int(s) for s in r["states"]))


@pytest.mark.parametrize("group", sorted(ref.gpu_groups()))
def test_the_gpu_inputs_notice_a_broken_rule(group):
    """Dropping the repeated-target rule, flipping either tie rule or starting from v[1] = -inf changes the reference's answer on a named case of every group;
    so does dropping the row0 offset (the rows in front of row0 hold NaN)."""
    seqs = ref.gpu_groups()[group]
    names = [n for n, _, _ in seqs]
    assert len(set(names)) == len(names)
    want = {n: _answer(ref.align32(em, t)) for n, em, t in seqs}
    for m in ref.MUTANTS:
        changed = [n for n, em, t in seqs if _answer(ref.mutant(m, em, t)) != want[n]]
        assert changed, (group, m)
    em, lens, targets = ref.pack_group(seqs, 4)
    r = 0
    for (n, e, t), T in zip(seqs, lens):
        blk = em[r:r + T]
        r += T
        assert np.isnan(blk[:4]).all() and np.array_equal(blk[4:, :len(t) + 1], e, equal_nan=False)
        assert np.isnan(blk[4:, len(t) + 1:]).all()
        v, _, _, _ = ref._sweep(blk[:, :len(t) + 1], t, F32, forward=False)      # the sweep from row 0 instead of row0: NaN, not the answer
        assert np.isnan(v).all() or want[n][0] == 1


def test_infeasible_when_rows_are_fewer_than_targets_plus_repeats():
    for T in range(1, 8):
        for targets in ([1, 2, 3], [1, 1, 2], [1, 1, 1], [1, 2, 1]):
            need = len(targets) + sum(a == b for a, b in zip(targets, targets[1:]))
            got = ref.align32(ref.em_random(T, T, len(targets)), targets)
            assert (got["status"] == 0) == (T >= need)


def test_budget_counts_three_steps_per_row():
    assert ref.budget(np.zeros(10)) == pytest.approx(10 * 3 * 5 * 2.0 ** -24)
    assert ref.budget(np.full(700, 100.0)) == pytest.approx(700 * 3 * 105 * 2.0 ** -24)
