"""CPU: the statement of the timed Paraformer outputs (paraformer_timing_ref.py) against the golden fixtures and hand cases, the product's host rules
(paraformer.token_times, engine.stream_absolute_rows) against that statement, and tools/transcribe.py's argument check."""
import importlib.util
import os
import types

import numpy as np
import pytest

import paraformer_timing_ref as R
from conftest import ROOT, sub
from helpers import golden_cases, load_golden

TAIL = 0.45


def _golden_alphas():
    for fx in ("paraformer_tiny", "paraformer_large"):
        for i, c in golden_cases(load_golden(fx)):
            yield f"{fx}[{i}]", c["alphas"], int(c["num_id"][0])
    g = load_golden("paraformer_tiny_natural")
    for name in sorted(k[:-len("_alphas")] for k in g if k.endswith("_alphas")):
        yield f"natural[{name}]", g[name + "_alphas"], int(g[name + "_num_id"][0])


def test_reference_reproduces_the_golden_token_counts():
    """Twelve cases; the fire rows are strictly increasing and lie in [0, T]. (Five of the twelve end on the tail row T.)"""
    assert sub("config").paraformer_tiny().tail_threshold == TAIL
    n = tails = 0
    for name, alphas, num_id in _golden_alphas():
        f = R.fire_frames(alphas, TAIL)
        assert len(f) == num_id, name
        assert (np.diff(f) > 0).all() and (len(f) == 0 or (f[0] >= 0 and f[-1] <= len(alphas))), name
        n += 1
        tails += int(len(f) > 0 and f[-1] == len(alphas))
    assert n == 12 and tails > 0
    assert any(num_id == 0 for _, _, num_id in _golden_alphas())            # the zero-token clip the GPU test batches in


@pytest.mark.parametrize("name", sorted(R.FIRE_CASES))
def test_hand_cases(name):
    alphas, tail, want = R.FIRE_CASES[name]
    assert R.fire_frames(np.asarray(alphas, np.float32), tail).tolist() == want


def test_the_floor_is_taken_of_the_f32_rounding():
    alphas, tail, _ = R.FIRE_CASES["f32_rounding"]
    s = float(np.asarray(alphas, np.float32).astype(np.float64).sum())
    assert s < 2.0 and np.float32(s) == np.float32(2.0)                     # a float64 floor would give one token


def test_ragged_long_utterance():
    f = R.fire_frames(R.ragged_alphas(), TAIL)
    assert len(f) == 343 and f[-1] == 700


def test_stream_fire_steps_hand_cases():
    steps, ca = R.stream_fire_steps([0.5, 0.25, 0.25, 0.5, 0.5], 0.0)        # exact binary fractions: fires when the weight reaches 1
    assert steps.tolist() == [2, 4] and ca == 0.0
    steps, ca = R.stream_fire_steps([0.25, 0.25], 0.75)
    assert steps.tolist() == [0] and ca == 0.25
    steps, ca = R.stream_fire_steps([0.5], 1.0)                              # a carried weight of 1: the entry fire, step -1
    assert steps.tolist() == [-1] and ca == 0.5
    steps, ca = R.stream_fire_steps(np.zeros(9, np.float32), 0.5)
    assert steps.size == 0 and ca == 0.5
    # the carried weight chains chunks: two steps equal one step over the concatenation
    a = np.random.default_rng(3).uniform(0.05, 0.9, 18).astype(np.float32)
    s1, c1 = R.stream_fire_steps(a[:9], 0.0)
    s2, c2 = R.stream_fire_steps(a[9:], c1)
    s12, c12 = R.stream_fire_steps(a, 0.0)
    assert np.concatenate([s1, s2 + 9]).tolist() == s12.tolist() and c2 == c12


def test_token_times_rule():
    tt = R.token_times
    # capping: a token that fired after long silence is 4 rows long, not 21
    assert np.allclose(tt([20], 100, 0.06), [[17 * 0.06, 21 * 0.06]])
    # the first token starts at 0 when it fires early; the next starts where it ended
    assert np.allclose(tt([1, 3], 100, 0.06), [[0.0, 0.12], [0.12, 0.24]])
    # a tail fire (fire == n_rows) is clipped to n_rows; behind a token that ended there it is empty
    assert np.allclose(tt([8, 10], 10, 1.0), [[5, 9], [9, 10]])
    assert np.allclose(tt([9, 10], 10, 1.0), [[6, 10], [10, 10]])
    # the cap is a keyword
    assert np.allclose(tt([20], 100, 1.0, max_token_rows=2), [[19, 21]])
    assert tt([], 5, 0.06).shape == (0, 2)
    # monotone, non-overlapping spans on the long seeded case and on every golden case
    for fire, T in [(R.fire_frames(R.ragged_alphas(), TAIL), 700)] + [(R.fire_frames(a, TAIL), len(a)) for _, a, _ in _golden_alphas()]:
        s = tt(fire, T, 0.06)
        assert (s[:, 0] <= s[:, 1]).all() and (s[1:, 0] >= s[:-1, 1]).all() and (s >= 0).all() and (s <= T * 0.06 + 1e-12).all()
        assert (s[:, 1] - s[:, 0] <= 4 * 0.06 + 1e-12).all()
        assert np.array_equal(sub("paraformer").token_times(fire, T, 0.06), s)        # the product's rule is this rule


def test_absolute_rows_of_a_timed_step():
    """Step t of a stream's c-th chunk is absolute row c B + t - C (9 and 4 at the reference's chunk); -1 is the previous chunk's last integrated row."""
    rows = sub("engine").stream_absolute_rows
    B, C = 9, 4
    assert rows([0, 3, 4, 8], 0, B, C).tolist() == [0, 0, 0, 4]               # the zero rows carried into the first chunk clip to 0
    assert rows([0, 4, 8], 1, B, C).tolist() == [5, 9, 13]
    assert rows([-1], 2, B, C).tolist() == rows([8], 1, B, C).tolist() == [13]
    for c in range(4):                                                       # consecutive chunks tile the row axis without gap or overlap
        assert rows([B - 1], c, B, C)[0] + 1 == rows([0], c + 1, B, C)[0]
        assert np.array_equal(rows(np.arange(-1, B), c, B, C), R.absolute_rows(np.arange(-1, B), c, B, C))
    # the C carried rows of chunk c are the last C new rows of chunk c - 1: new row j of chunk c sits in slot row C + j
    assert rows([C + 0], 3, B, C)[0] == 3 * B and rows([0], 3, B, C)[0] == 2 * B + (B - C)


def _tool():
    spec = importlib.util.spec_from_file_location("transcribe_tool", os.path.join(ROOT, "tools", "transcribe.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_transcribe_tool_argument_check(tmp_path):
    tool = _tool()
    base = dict(model=str(tmp_path), wav=[], language="auto", tokenizer=None, precision="f32", sliding_window=0, strict_wav=True, repeat_penalty=1.0, beam=1)
    with pytest.raises(SystemExit, match="qwen_asr"):                       # the family the refusal still excludes is named
        tool.run(types.SimpleNamespace(**base, family="qwen_asr", timestamps=True))
    with pytest.raises(SystemExit) as e:                                    # paraformer is no longer refused for the flag: the folder is what is wrong here
        tool.run(types.SimpleNamespace(**base, family="paraformer", timestamps=True))
    assert "Paraformer.asrmodel" in str(e.value) and "--timestamps" not in str(e.value)
    with pytest.raises(SystemExit, match="SenseVoiceSmall.asrmodel"):
        tool.run(types.SimpleNamespace(**base, family="sensevoice"))
