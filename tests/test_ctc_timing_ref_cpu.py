"""CPU: the reference of the timed CTC head (tests/ctc_timing_ref.py) against independent statements -- torch's float64 log-soft-max, the oracle's
collapse on the golden frame ids, hand-written spans -- and SenseVoiceConfig.row_span_seconds."""
import numpy as np
import pytest
import torch

import ctc_timing_ref as R
from conftest import sub
from helpers import golden_cases, load_golden
from oracle.sensevoice_oracle import SenseVoiceOracle


def test_frame_logprob_matches_torch_log_softmax():
    rng = np.random.default_rng(0)
    v = rng.normal(0.0, 3.0, (40, 1003))
    v[3] += 90.0
    v[4] -= 90.0
    v[5] = 1.25
    v[6, 77] = v[6, 900] = v[6].max() + 1.0           # a tie: the first wins
    ids, lp, spread = R.frame_logprob(v)
    ls = torch.log_softmax(torch.from_numpy(v), dim=1)
    want_ids = np.array([int(np.flatnonzero(r == r.max())[0]) for r in v])
    assert np.array_equal(ids, want_ids) and ids[6] == 77 and ids[5] == 0
    assert np.abs(lp - ls[torch.arange(40), torch.from_numpy(want_ids)].numpy()).max() < 1e-12
    assert abs(lp[5] + np.log(1003)) < 1e-12 and (lp <= 0).all() and (spread >= 0).all() and spread[5] == 0
    ids2, lp2, _ = R.frame_logprob(v, n_valid=500)
    assert np.abs(lp2 - torch.log_softmax(torch.from_numpy(v[:, :500]), dim=1).max(dim=1).values.numpy()).max() < 1e-12


def test_budget_is_tight_enough_to_see_a_dropped_slab():
    """A 25 088-wide near-uniform row: one dropped slab of 392 moves the result by 2.5e-3; the derived bound must stay well below (the issue's bar: 1e-3)."""
    rng = np.random.default_rng(1)
    a, w = R.bf16_round(rng.standard_normal((4, 512))), R.bf16_round(rng.standard_normal((25088, 512)) * (2.0 / np.sqrt(512)))
    bias = R.bf16_round(rng.normal(0, 0.5, 25088))
    ids, lp, spread, abs_dot, vmax = R.head_reference(a, w, bias, 25055)
    b = R.budget(25055, lp, spread, 512, abs_dot, vmax)
    assert b.max() < 1e-3, b
    assert R.budget(25055, lp, spread).max() < 1e-5          # against the stored logits: no accumulation term


@pytest.mark.parametrize("fixture", ["sensevoice_tiny", "sensevoice_small", "sensevoice_tiny_live"])
def test_collapse_ids_equal_the_oracle_on_golden_frame_ids(fixture):
    n = 0
    for _, c in golden_cases(load_golden(fixture)):
        if "frame_ids" not in c:
            continue
        ids = np.asarray(c["frame_ids"]).reshape(-1)
        tok, first, last, score = R.collapse_timed(ids, np.zeros(ids.size, np.float32), 0)
        want = SenseVoiceOracle.ctc_collapse(torch.tensor(ids, dtype=torch.int64), 0).numpy()
        assert np.array_equal(tok, want)
        assert (first <= last).all() and (np.diff(last) > 0).all() and (first[1:] > last[:-1]).all()
        for t, f, l in zip(tok, first, last):
            assert (ids[f:l + 1] == t).all() and (f == 0 or ids[f - 1] != t)
        n += 1
    assert n > 0


@pytest.mark.parametrize("name", sorted(R.COLLAPSE_CASES))
def test_collapse_hand_written_spans(name):
    ids, want = R.COLLAPSE_CASES[name]
    lp = R.case_logprob(len(ids), len(ids))
    tok, first, last, score = R.collapse_timed(ids, lp, 0)
    assert [(int(t), int(f), int(l)) for t, f, l in zip(tok, first, last)] == want
    assert np.array_equal(tok, SenseVoiceOracle.ctc_collapse(torch.tensor(ids, dtype=torch.int64), 0).numpy())
    for f, l, s in zip(first, last, score):
        assert abs(float(s) - float(np.mean(lp[f:l + 1].astype(np.float64)))) <= 1e-5 * (1 + abs(float(s)))
        if f == l:
            assert s == lp[f]


def test_mean_f32_is_the_sequential_sum():
    x = np.array([1e8, 1.0, -1e8, 1.0], np.float32)              # the order shows: (((1e8 + 1) - 1e8) + 1) / 4 in f32
    assert R.mean_f32(x) == np.float32(0.25)
    assert R.mean_f32(np.array([-0.3], np.float32)) == np.float32(-0.3)


def test_head_operands_carry_their_planted_rows():
    n_valid = 640 - 33
    a, w, bias, kinds = R.head_operands(3, 130, 640, n_valid)
    assert np.array_equal(R.bf16_round(a), a) and np.array_equal(R.bf16_round(w), w)
    assert kinds[129] == "plant_last" and set(kinds) == set(R.ROW_KINDS)
    ids, lp, spread, abs_dot, vmax = R.head_reference(a, w, bias, n_valid)
    v = a.astype(np.float64) @ w.astype(np.float64).T + bias.astype(np.float64)
    for m, kind in enumerate(kinds):
        if kind.startswith("plant_"):
            other = {"plant_slab0": R.COL_SLAB0, "plant_right": R.COL_RIGHT, "plant_last": n_valid - 1}[kind]
            pair = {R.COL_TOP, other}
            assert ids[m] in pair
            loser = (pair - {int(ids[m])}).pop()
            assert loser // 64 != ids[m] // 64
            # without the other peak's slab the result would move by more than 0.05 (about log 2 when the two are level)
            keep = np.ones(n_valid, bool); keep[loser // 64 * 64:(loser // 64 + 1) * 64] = False
            _, lp_drop, _ = R.frame_logprob(v[m:m + 1, :n_valid][:, keep])
            assert lp_drop[0] - lp[m] > 0.05
        elif kind == "equal":
            assert ids[m] == 0 and abs(lp[m] + np.log(n_valid)) < 1e-12
        elif kind == "dominant":
            assert ids[m] == R.COL_TOP and -1e-6 < lp[m] <= 0
        elif kind == "plus90":
            assert v[m, :n_valid].min() > 70
        elif kind == "minus90":
            assert v[m, :n_valid].max() < -70


def test_row_span_seconds():
    cfg = sub("config").sensevoice_tiny()
    npr, row = cfg.n_prompt, cfg.lfr_n * cfg.hop_length / cfg.sample_rate
    assert npr == 4 and row == 0.06
    assert cfg.row_span_seconds(0, 0) == (0.0, 0.0)                       # a prompt tag
    assert cfg.row_span_seconds(1, npr - 1) == (0.0, 0.0)                 # a run inside the prompt rows
    assert cfg.row_span_seconds(npr - 1, npr) == (0.0, row)               # starts in the prompt, ends in the first speech row
    assert cfg.row_span_seconds(npr, npr) == (0.0, row)                   # the first speech row
    assert cfg.row_span_seconds(npr + 2, npr + 4) == (2 * row, 5 * row)
    T = cfg.seq_len(32000)
    s, e = cfg.row_span_seconds(T - 1, T - 1)                             # the last row ends at or after the last whole frame
    assert s == (T - 1 - npr) * row and e == (T - npr) * row and e >= (cfg.n_frames(32000) * cfg.hop_length) / cfg.sample_rate


def test_timed_entries_are_exported_and_declared():
    """The product library exports the two new entries, the probe library the head hook, and the public header declares them; the ABI version stays."""
    import os
    lib, probe = sub("_lib").load(), sub("_probe").load()
    assert lib.asr_abi_version() == 1
    for name in ("asr_sensevoice_run_timed", "asr_op_ctc_collapse_timed"):
        assert hasattr(lib, name) and name in sub("_lib").SIGNATURES
    assert hasattr(probe, "asr_probe_ctc_head")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "asr_mi355x.h")).read()
    assert "int asr_sensevoice_run_timed(" in header and "int asr_op_ctc_collapse_timed(" in header
    assert "int asr_probe_ctc_head(" in open(os.path.join(root, "include", "asr_mi355x_probe.h")).read()
