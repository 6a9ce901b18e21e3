"""The two token-score kernels of csrc/kernels.hip -- launch_argmax_logprob_rows (the greedy pick and its score, fused) and launch_logprob_at_rows (the
score of an id picked elsewhere) -- and the TokenHead of csrc/decode_head.h in scores mode, through the probe library (product launchers unchanged, real
leading dimension, pad columns at +1e30) against tests/token_scores_ref.py.

Ids are compared exactly (logits on the 2^-10 grid decide every ordering), scores against the float64 log-soft-max of the same f32 row within the budget
token_scores_ref derives from the kernels' operation counts; -inf must come out as -inf and nothing may be NaN. Every output slot is pre-filled with NaN:
what a kernel does not address must come back as it went in. Each case prints its largest error as a share of the budget."""
import numpy as np
import pytest

import token_heads_ref as thr
import token_scores_ref as R
import whisper_timestamps_ref as wtr
from conftest import sub

pytestmark = pytest.mark.gpu


def _head(op, *a, **k):
    return sub("_probe").token_head(op, *a, **k)


def _table(rows):
    return np.full((rows, R.LD_SAVE), R.NAN_FILL, np.float32)


def _only_column_written(out, rows, n):
    """The history came back NaN outside the addressed column, the logits untouched, the pad at PAD_LOGIT."""
    lp = out["logprob"]
    others = np.delete(lp, R.COLUMN, axis=1)
    return lp.shape == (rows, R.LD_SAVE) and bool(np.isnan(others).all()) and bool((out["logits"][:, n:] == sub("_probe").PAD_LOGIT).all())


def _fused(x, extra, n, label):
    rows = len(x)
    ids, want, M, lse = R.argmax_scores(x, extra)
    out = _head("argmax_logprob_rows", x, vec=extra, logprob=_table(rows), n_saved=R.COLUMN)
    assert out["ids"].tolist() == ids.tolist(), label
    assert out["ids"].tolist() == _head("argmax_rows", x, vec=extra)["ids"].tolist(), label
    assert _only_column_written(out, rows, n) and np.array_equal(out["logits"][:, :n], x, equal_nan=True), label
    worst = R.over_budget(out["logprob"][:, R.COLUMN], want, R.fused_budget(n, M, lse))
    print(f"argmax_logprob_rows n={n} {label}: largest error {worst:.4f} of the budget ({R.s_budget(n):.3e})")
    assert worst <= 1.0, label
    return out["logprob"][:, R.COLUMN]


def _at_ids(x, extra, n, label):
    rows = len(x)
    for kind in R.ID_KINDS:
        at = R.ids_for(x, extra, kind)
        want, M, lse = R.scores_at(x, at, extra)
        out = _head("logprob_at_rows", x, vec=extra, logprob=_table(rows), n_saved=R.COLUMN, next_ids=at)
        assert _only_column_written(out, rows, n) and np.array_equal(out["logits"][:, :n], x, equal_nan=True), (label, kind)
        worst = R.over_budget(out["logprob"][:, R.COLUMN], want, R.at_id_budget(n, M, lse, np.where(np.isfinite(want), want, 0.0)))
        print(f"logprob_at_rows n={n} {label}, ids at the {kind}: largest error {worst:.4f} of the budget")
        assert worst <= 1.0, (label, kind)


def _check_width(n):
    extra = thr.grid_logits([n, 2], 1, n)[0]
    for i, x in enumerate(R.planted_rows(n)):                     # ids: planted maxima and exact ties, with and without extra
        for e in (None, extra):
            want, _ = thr.argmax_rows(x, e)
            out = _head("argmax_logprob_rows", x, vec=e, logprob=_table(len(x)), n_saved=R.COLUMN)
            assert out["ids"].tolist() == want.tolist() == _head("argmax_rows", x, vec=e)["ids"].tolist(), (n, i, e is not None)
    for label, (x, e) in R.score_cases(n).items():
        got = _fused(x, e, n, label)
        _at_ids(x, e, n, label)
        if label.startswith("equal"):
            assert got[3] == -np.inf and -1e-6 < got[1] <= 0.0 and got[2] == 0.0, got


@pytest.mark.parametrize("n", R.KERNEL_WIDTHS)
def test_score_kernels_at_every_loop_boundary(n):
    _check_width(n)


@pytest.mark.parametrize("n", R.WIDE_WIDTHS)
def test_score_kernels_at_the_deployment_widths(n):
    _check_width(n)


def test_a_full_history_drops_the_score_and_ids_outside_the_row_score_minus_infinity():
    n = 4097
    x = thr.grid_logits([n, 5], 3, n)
    for counter in (R.LD_SAVE, R.LD_SAVE + 7):                    # at or past the table: nothing is written, the pick still is
        out = _head("argmax_logprob_rows", x, logprob=_table(3), n_saved=counter)
        assert np.isnan(out["logprob"]).all() and out["ids"].tolist() == thr.argmax_rows(x)[0].tolist()
        out = _head("logprob_at_rows", x, logprob=_table(3), n_saved=counter, next_ids=[0, 1, 2])
        assert np.isnan(out["logprob"]).all()
    out = _head("logprob_at_rows", x, logprob=_table(3), n_saved=R.LD_SAVE - 1, next_ids=[-1, n, n + 100])       # never read: the kernel checks first
    assert out["logprob"][:, -1].tolist() == [-np.inf] * 3 and np.isnan(out["logprob"][:, :-1]).all()


# ------------------------------------------------------------------------------------------------ the head over several steps
def _steps_cases():
    cases = {}
    x, _, _ = thr.head_steps_inputs()
    for name, kw in thr.head_steps_cases().items():
        cases[name] = (x, kw)
    xt, _, _ = wtr.head_steps_inputs()
    for name, kw in wtr.head_steps_cases().items():
        cases["timestamps: " + name] = (xt, kw)
    return cases


@pytest.mark.parametrize("name", list(_steps_cases()))
def test_head_steps_with_scores(name):
    """Greedy, penalty-greedy, the sampler with caller noise and the timestamp rules: the picks are those of the same run with scores off, the score history
    is the reference applied to each step's edited logits, the counter is the step count."""
    c = thr.HEAD_STEPS
    x, kw = _steps_cases()[name]
    probe = sub("_probe")
    off = probe.head_steps(x, c["steps"], c["ld_save"], **kw)
    on = probe.head_steps(x, c["steps"], c["ld_save"], scores=True, **kw)
    assert np.array_equal(on["picks"], off["picks"]), name
    assert on["n_saved"] == c["steps"]
    picks, save, n, decided, scores, budgets = R.head_steps(x, c["steps"], c["ld_save"], **kw)
    assert decided.all(), (name, decided)                        # every step of every case is decided (test_token_scores_ref_cpu.py): nothing is left out
    assert np.array_equal(on["picks"], picks), name
    assert np.array_equal(on["save_ids"][:, :c["steps"]], picks.T), name      # every pick joins the history, beside its score
    got = on["logprob"][:, :c["steps"]].T
    worst = R.over_budget(got, scores, budgets)
    print(f"head steps with scores, {name}: largest error {worst:.4f} of the budget")
    assert worst <= 1.0, name
    assert np.isnan(on["logprob"][:, c["steps"]:]).all()           # columns no step addressed


def test_head_steps_past_the_table_drop_the_overflow():
    c = thr.HEAD_STEPS
    x, bias, _ = thr.head_steps_inputs()
    ld_save, steps = 4, 7
    probe = sub("_probe")
    on = probe.head_steps(x, steps, ld_save, c["range_"], 1.0, 0, bias=bias, scores=True)
    off = probe.head_steps(x, c["steps"], c["ld_save"], c["range_"], 1.0, 0, bias=bias)
    assert np.array_equal(on["picks"], off["picks"][:steps]) and on["n_saved"] == steps
    picks, _, _, _, scores, budgets = R.head_steps(x, steps, 16, c["range_"], 1.0, 0, bias=bias)
    assert on["logprob"].shape == (c["rows"], ld_save) and np.array_equal(on["save_ids"], picks[:ld_save].T)
    assert R.over_budget(on["logprob"].T, scores[:ld_save], budgets[:ld_save]) <= 1.0       # the first ld_save steps' scores, none of the later ones
