"""CPU: the float64 statement of Whisper's token timestamps (tests/whisper_align_ref.py) against three independent witnesses -- a brute-force minimum
over all monotone paths, hand-worked ties, and the Hugging Face restatement of OpenAI's code (transformers' _dynamic_time_warping / _median_filter) --
and the host functions of whisper.py (token_times, split_words, word_times) on hand-written cases."""
import itertools
import tempfile

import numpy as np
import pytest

import whisper_align_ref as ref
from conftest import sub

wh = sub("whisper")


def _grid(rng, shape, lim=4.0):
    """Multiples of 2^-10 with |v| <= lim: every partial sum of a DTW over them is exact in f32 (and in float64)."""
    return rng.integers(-int(lim * 1024), int(lim * 1024) + 1, size=shape).astype(np.float64) / 1024.0


def test_dtw_is_the_brute_force_minimum_over_all_monotone_paths():
    rng = np.random.default_rng(7)
    for N, M in itertools.product(range(1, 5), range(1, 6)):
        for _ in range(4):
            cost = rng.standard_normal((N, M))
            rows, frames = ref.dtw(cost)
            assert ref.is_monotone_path(rows, frames, N, M), (N, M)
            assert abs(ref.path_cost(cost, rows, frames) - ref.brute_force_optimum(cost)) < 1e-12, (N, M)
            assert ref.jump_frames(rows, frames).tolist() == [int(frames[rows == r].min()) for r in range(N)]


def test_ties_follow_openais_rule():
    # all three predecessors equal: neither strict test holds -> horizontal. The path hugs the first column, then the last row.
    for N, M in ((2, 2), (3, 4), (4, 2)):
        rows, frames = ref.dtw(np.zeros((N, M)))
        assert rows.tolist() == list(range(N)) + [N - 1] * (M - 1) and frames.tolist() == [0] * N + list(range(1, M)), (N, M)
        assert ref.jump_frames(rows, frames).tolist() == [0] * N
    # c0 < c1, c0 == c2: "c0 < c2" fails, "c1 < c0" fails -> horizontal (cost 0 either way)
    rows, frames = ref.dtw(np.array([[0.0, 1.0], [0.0, 0.0]]))
    assert list(zip(rows, frames)) == [(0, 0), (1, 0), (1, 1)]
    # c0 == c1 < c2: neither strict test holds, so the rule takes the horizontal step although it costs more -- OpenAI's rule as written, not a minimum
    rows, frames = ref.dtw(np.array([[0.0, 0.0], [1.0, 0.0]]))
    assert list(zip(rows, frames)) == [(0, 0), (1, 0), (1, 1)]
    # c1 strictly least -> vertical; c0 strictly least -> diagonal
    rows, frames = ref.dtw(np.array([[0.0, -1.0], [1.0, 1.0]]) / 1024)
    assert list(zip(rows, frames)) == [(0, 0), (0, 1), (1, 1)]
    rows, frames = ref.dtw(np.array([[0.0, 1.0], [1.0, 0.0]]) / 1024)
    assert list(zip(rows, frames)) == [(0, 0), (1, 1)]
    # costs from {0, 1} / 1024 * k: ties on every diagonal; the path is still a monotone path and the float32 and float64 runs agree
    rng = np.random.default_rng(3)
    for k in (1, 3):
        cost = rng.integers(0, 2, size=(9, 14)) * (k / 1024.0)
        a, b = ref.dtw(cost), ref.dtw(cost, np.float32)
        assert ref.is_monotone_path(a[0], a[1], 9, 14) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_dtw_equals_the_transformers_restatement():
    from transformers.models.whisper.generation_whisper import _dynamic_time_warping
    rng = np.random.default_rng(11)
    for N, M in ((1, 1), (2, 1), (5, 2), (1, 20), (5, 7), (17, 33), (40, 12)):
        for cost in (_grid(rng, (N, M)), rng.integers(0, 2, size=(N, M)) / 1024.0):
            rows, frames = ref.dtw(cost)
            hf_rows, hf_frames = _dynamic_time_warping(cost.astype(np.float32))
            assert np.array_equal(rows, hf_rows) and np.array_equal(frames, hf_frames), (N, M)


def test_median_filter_equals_the_transformers_restatement():
    import torch
    from transformers.models.whisper.generation_whisper import _median_filter
    rng = np.random.default_rng(5)
    for M in (1, 3, 4, 7, 8, 65):
        for width in (1, 3, 7, 9):
            x = _grid(rng, (2, 3, M))
            want = _median_filter(torch.from_numpy(x), width).numpy()
            assert np.array_equal(ref.median_filter(x, width), want), (M, width)
    assert ref.median_filter(np.arange(3.0)[None, None], 7).tolist() == [[[0.0, 1.0, 2.0]]]          # M <= width // 2: untouched
    assert ref.median_filter(np.array([[[3.0, 0.0, 1.0, 2.0]]]), 7).tolist() != [[[3.0, 0.0, 1.0, 2.0]]]      # M = 4 is filtered


def test_cost_matrix_equals_openais_steps_in_torch():
    """Steps 2-4 as openai-whisper's find_alignment writes them (std_mean over the token axis, median filter, mean over heads), in torch float64."""
    import torch
    from transformers.models.whisper.generation_whisper import _median_filter
    rng = np.random.default_rng(2)
    scores = rng.standard_normal((3, 6, 40)) * 3
    w = torch.from_numpy(scores).softmax(dim=-1)
    std, mean = torch.std_mean(w, dim=-2, keepdim=True, unbiased=False)
    want = -_median_filter((w - mean) / std, 7).mean(dim=0).numpy()
    assert np.abs(ref.cost_matrix(scores, 7) - want).max() < 1e-12
    # a column whose rows are all equal standardises to 0 (the stated deviation: OpenAI divides by zero there)
    same = np.repeat(rng.standard_normal((2, 1, 9)), 2, axis=1)
    assert (ref.cost_matrix(same, 3) == 0).all()
    assert (ref.cost_budget(same, 3) == 0).all()


def test_token_times():
    assert wh.token_times([0, 3, 5]) == [(0.0, 0.06), (0.06, 0.1)] == ref.token_times([0, 3, 5])
    assert wh.token_times([2, 2, 10], 30.0) == [(30.04, 30.04), (30.04, 30.2)] == ref.token_times([2, 2, 10], 30.0)
    # cut off before eot: every row is a token, the last one ends with the window
    assert wh.token_times([0, 3], 1.0, 2.0) == [(1.0, 1.06), (1.06, 2.0)] == ref.token_times([0, 3], 1.0, 2.0)
    assert wh.token_times([]) == [] and wh.token_times([4]) == [] and wh.token_times([], 0.0, 1.0) == []        # an empty utterance; eot's row alone


def test_split_words_on_a_tiny_tokenizer():
    from transformers import AutoTokenizer
    from tiny_tokenizers import whisper_tokenizer_dir
    cfg = sub("config").whisper_tiny_test()
    with tempfile.TemporaryDirectory() as d:
        tok = AutoTokenizer.from_pretrained(whisper_tokenizer_dir(d, cfg))
    B = lambda ch: ord(ch)                                    # the byte tokens are the ids below 256
    cases = [
        # ids, words
        ([300, 301, B("x"), 302], [" tok300", " tok301x", " tok302"]),                          # a piece without a leading space continues the word
        ([300, B(","), 301, B(".")], [" tok300,", " tok301."]),                                 # trailing merge: appended marks join the word before them
        ([B(" "), B('"'), 300, B("!"), B("?")], [' "', " tok300!?"]),                           # leading merge: the lone ' ' joins the '"' after it
        ([300, B(" "), B("("), 301, B(")")], [" tok300", " (", " tok301)"]),
        ([0xE4, 0xBD, 0xA0, 300], ["你", " tok300"]),                                       # three byte tokens of one character count with its last one
        ([], []),
    ]
    for ids, words in cases:
        pieces = wh.decode_pieces(ids, tok.decode)
        counts = wh.split_words(pieces)
        assert sum(counts) == len(ids), (ids, counts)
        times = [(0.02 * i, 0.02 * (i + 1)) for i in range(len(ids))]
        got = wh.word_times(pieces, times)
        assert [w["word"] for w in got] == words, (ids, got)
        assert [w["tokens"] for w in got] == counts
        at = 0
        for w in got:
            assert (w["start"], w["end"]) == (times[at][0], times[at + w["tokens"] - 1][1])
            at += w["tokens"]
    assert wh.split_words([None, None]) == [2]                # ids that never complete a character stay together
    # pieces as a released vocabulary has them (' "' is one token there): the opening quote joins the word after it, the marks the words before them
    pieces = [' "', " Hello", ",", " wor", "ld", "!", '"']
    assert wh.split_words(pieces) == [3, 4]
    assert [w["word"] for w in wh.word_times(pieces, [(0.0, 0.0)] * 7)] == [' " Hello,', ' world!"']


def test_alignment_heads_of_a_checkpoint_folder():
    import json
    import os
    ckm = sub("checkpoints")
    with tempfile.TemporaryDirectory() as d:
        assert ckm.whisper_alignment_heads(d) is None
        with open(os.path.join(d, "generation_config.json"), "w") as f:
            json.dump({"alignment_heads": [[1, 0], [0, 1]], "max_length": 448}, f)
        assert ckm.whisper_alignment_heads(d) == [(1, 0), (0, 1)]
        assert ckm.whisper_alignment_heads(os.path.join(d, "model.safetensors")) == [(1, 0), (0, 1)]
        with open(os.path.join(d, "generation_config.json"), "w") as f:
            json.dump({"max_length": 448}, f)
        assert ckm.whisper_alignment_heads(d) is None
