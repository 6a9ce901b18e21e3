"""CPU: pins tests/token_scores_ref.py -- the float64 statement of the token scores that tests/test_token_scores_gpu.py and
tests/test_token_scores_session_gpu.py compare with -- against torch.log_softmax, checks its -inf rules, shows that the kernels' online reduction restated
in numpy f32 stays inside the derived budgets on every input the GPU tests use (the "reference alone stays within it" check, without a GPU), and checks
that the header declares and the libraries export the new entries."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import token_heads_ref as thr
import token_scores_ref as R
from conftest import ROOT, sub

ENTRIES = ["asr_whisper_set_token_scores", "asr_whisper_token_scores", "asr_qwen_set_token_scores", "asr_qwen_token_scores"]


def test_reference_is_torch_log_softmax_in_float64():
    for n in (1, 5, 129, 4097):
        x = thr.grid_logits([n, 71], 4, n)
        extra = thr.grid_logits([n, 72], 1, n)[0]
        for e in (None, extra):
            v = R.seen(x, e)
            lsm, M, lse = R.log_softmax(v)
            want = torch.log_softmax(torch.from_numpy(v).double(), dim=1).numpy()
            assert np.abs(lsm - want).max() < 1e-12
            assert np.array_equal(M, v.max(axis=1).astype(np.float64)) and np.abs(lse - torch.logsumexp(torch.from_numpy(v).double(), 1).numpy()).max() < 1e-12
            ids, s, _, _ = R.argmax_scores(x, e)
            assert ids.tolist() == v.argmax(axis=1).tolist() and np.abs(s - want[np.arange(4), ids]).max() < 1e-12
            at = np.array([0, n - 1, n // 2, n // 3])
            assert np.abs(R.scores_at(x, at, e)[0] - want[np.arange(4), at]).max() < 1e-12


def test_the_minus_infinity_rules():
    x = np.array([[0.5, -np.inf, 0.5, -np.inf], [-np.inf] * 4, [-np.inf, -np.inf, -np.inf, 2.0]], np.float32)
    ids, s, M, lse = R.argmax_scores(x)
    assert ids.tolist() == [0, 0, 3]                              # first maximum; an empty row picks 0
    assert s[0] == pytest.approx(-np.log(2.0)) and s[1] == -np.inf and s[2] == 0.0 and not np.isnan(s).any()
    at, _, _ = R.scores_at(x, [1, 2, 0])                          # picks at -inf columns
    assert at.tolist() == [-np.inf, -np.inf, -np.inf]
    assert R.scores_at(x, [-1, 7, 4])[0].tolist() == [-np.inf] * 3      # ids outside the row
    extra = np.array([-np.inf, 0.0, 0.0, 0.0], np.float32)       # a -inf extra removes the column from the row
    ids, s, _, _ = R.argmax_scores(x, extra)
    assert ids.tolist() == [2, 0, 3] and s.tolist() == [0.0, -np.inf, 0.0]
    lsm, _, _ = R.log_softmax(x)
    assert np.array_equal(np.isneginf(lsm), np.isneginf(np.broadcast_to(x, lsm.shape)) | np.array([[False], [True], [False]]))


def test_budgets_grow_with_the_width_and_over_budget_refuses_nan():
    b = [R.s_budget(n) for n in thr.WIDTHS]
    assert all(x <= y for x, y in zip(b, b[1:])) and 1e-4 < b[0] < 2e-4 and b[-1] < 1.2e-3        # far below the log 2 of a lost partial
    assert R.at_id_budget(129, 3.0, 5.0, -7.0) > R.fused_budget(129, 3.0, 5.0) > R.s_budget(129)
    with pytest.raises(AssertionError):
        R.over_budget(np.array([np.nan]), np.array([0.0]), 1.0)
    with pytest.raises(AssertionError):
        R.over_budget(np.array([-1.0]), np.array([-np.inf]), 1.0)
    assert R.over_budget(np.array([-np.inf, -1.0]), np.array([-np.inf, -1.5]), 1.0) == 0.5


def _restatement_within_budget(n):
    worst = 0.0
    for name, (x, extra) in R.score_cases(n).items():
        ids, want, M, lse = R.argmax_scores(x, extra)
        worst = max(worst, R.over_budget(R.online_scores(x, None, extra), want, R.fused_budget(n, M, lse)))
        for kind in R.ID_KINDS:
            at = R.ids_for(x, extra, kind)
            want, M, lse = R.scores_at(x, at, extra)
            worst = max(worst, R.over_budget(R.online_scores(x, at, extra), want, R.at_id_budget(n, M, lse, np.where(np.isfinite(want), want, 0.0))))
    return worst


@pytest.mark.parametrize("n", thr.WIDTHS)
def test_online_f32_restatement_stays_inside_the_budget(n):
    worst = _restatement_within_budget(n)
    print(f"token scores, f32 restatement, n={n}: largest error {worst:.4f} of the budget")
    assert worst <= 1.0


def test_score_cases_are_what_they_say():
    for n in (5, 4097, 12289):
        cases = R.score_cases(n)
        x, _ = cases["half each on two columns"]
        _, s, _, _ = R.argmax_scores(x)
        assert np.abs(s + np.log(2.0)).max() < 1e-6, s            # the pair holds all of the probability: a lost partial gives 0 instead
        x, _ = cases["equal, dominant, last column only, all -inf"]
        ids, s, _, _ = R.argmax_scores(x)
        assert s[0] == pytest.approx(-np.log(n)) and -1e-6 < s[1] <= 0.0 and s[2] == 0.0 and s[3] == -np.inf
        assert ids.tolist() == [0, n // 2, n - 1, 0]
        x, extra = cases["-inf columns, -inf extra"]
        assert np.isneginf(x).any() and np.isneginf(extra).any()
        for chunk in R.planted_rows(n):
            assert 3 <= len(chunk) <= 5


def test_head_steps_with_scores_keep_the_picks_and_fill_the_history():
    c = thr.HEAD_STEPS
    x, _, _ = thr.head_steps_inputs()
    for name, kw in thr.head_steps_cases().items():
        picks, save, n, decided, scores, budgets = R.head_steps(x, c["steps"], c["ld_save"], **kw)
        want = thr.head_steps(x, c["steps"], c["ld_save"], **kw)
        assert np.array_equal(picks, want[0]) and n == c["steps"], name          # scoring a pick never changes it; every pick joins the history
        assert np.array_equal(save[:, :n], picks.T) and np.isfinite(scores).all() and (scores <= 0).all() and (budgets > 0).all(), name
        assert decided.all(), name                                # the GPU test compares every step
    import whisper_timestamps_ref as wtr
    xt, _, _ = wtr.head_steps_inputs()
    for name, kw in wtr.head_steps_cases().items():
        picks, save, n, decided, scores, budgets = R.head_steps(xt, c["steps"], c["ld_save"], **kw)
        want = wtr.head_steps(xt, c["steps"], c["ld_save"], **kw)
        assert np.array_equal(picks, want[0]) and n == c["steps"] and decided.all(), name
        assert np.array_equal(save[:, :n], picks.T) and np.isfinite(scores).all() and (scores <= 0).all(), name


def test_header_declares_and_libraries_export_the_entries():
    header = open(os.path.join(ROOT, "include", "asr_mi355x.h")).read()
    assert re.search(r"#define ASR_ABI_VERSION 1\b", header)
    for name in ENTRIES:
        assert re.search(r"\bint %s\(asr_session\* s, " % name, header), name
    probe_header = open(os.path.join(ROOT, "include", "asr_mi355x_probe.h")).read()
    assert re.search(r"int32_t scores;.*\n\s*float\* logprob;", probe_header) and probe_header.index("n_saved_rows;") < probe_header.index("int32_t scores;")
    lib = ctypes.CDLL(sub("_lib").LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    lib.asr_abi_version.restype = ctypes.c_int
    assert lib.asr_abi_version() == 1
    assert all(name in sub("_lib").SIGNATURES for name in ENTRIES)
    probe = sub("_probe")
    assert hasattr(probe.load(), "asr_probe_token_head")
    assert {"argmax_logprob_rows": 8, "logprob_at_rows": 9}.items() <= probe._HEAD_OPS.items()
    names = [f[0] for f in probe.TokenHeadDesc._fields_]
    assert names[-5:] == ["n_saved_rows", "scores", "logprob", "timed", "head_ms"]                     # the descriptor grew at its end only
