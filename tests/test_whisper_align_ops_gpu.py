"""The five kernels of Whisper's token timestamps (csrc/whisper_align.hip), one launch at a time through asr_probe_whisper_align, against the float64
statement and the budgets of tests/whisper_align_ref.py. The DTW is compared for equality -- frames and the whole path -- on exactly representable costs
(multiples of 2^-10, |v| <= 4: every running sum is exact in f32), where both sides compute the same numbers and every tie is a real one."""
import numpy as np
import pytest

import whisper_align_ref as ref
from conftest import sub
from decode_attn_ref import bf16_round

pytestmark = pytest.mark.gpu

H = 2


def _probe():
    return sub("_probe")


# ------------------------------------------------------------------------------------------------- capture
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("lens", [(1, 15, 16), (17, 64, 65), (200, 1, 65)], ids=lambda v: "x".join(map(str, v)))
def test_scores(bf16, lens):
    rng = np.random.default_rng(sum(lens) + int(bf16))
    B, P, R = 3, 2, 3
    ld = (max(lens) + 15) // 16 * 16
    row_off, at = [], 16                                     # non-zero offsets, gaps between the sequences
    for t in lens:
        row_off.append(at)
        at = (at + t + 15) // 16 * 16 + 16
    k = rng.standard_normal((H, at, 64)).astype(np.float32)
    ks = bf16_round(k) if bf16 else k                        # the values the kernel sees
    # (n, position, p0): the row written is position + n - 1 - p0. A prefill of four positions (its last row is scored), decode steps, and rows outside [0, 3)
    cases = ((4, 0, 3, 0), (1, 5, 4, 1), (4, 0, 1, 2), (1, 3, 3, 0), (4, 3, 3, None), (1, 7, 4, None), (1, 2, 6, None))
    for sel in ([(1, 0)], [(0, 1), (1, 0)]):                 # (head, slot): head 1 only; both heads, slots crossed
        for n, position, p0, row in cases:
            q = rng.standard_normal((B * n, H * 64)).astype(np.float32)
            qs = bf16_round(q) if bf16 else q
            before = np.full((B, P, R, ld), np.nan, np.float32)
            got = _probe().whisper_align_scores(q, k, row_off, lens, sel, before, position, p0, n=n, bf16=bf16)
            written = np.zeros(got.shape, bool)
            if row is not None:
                for b in range(B):
                    for head, slot in sel:
                        qv = qs[b * n + n - 1, head * 64:(head + 1) * 64].astype(np.float64)
                        kv = ks[head, row_off[b]:row_off[b] + lens[b]].astype(np.float64)
                        want, tol = kv @ qv, ref.scores_budget(qv, kv)
                        err = np.abs(got[b, slot, row, :lens[b]] - want)
                        assert (err <= tol).all(), (sel, n, position, p0, b, head, float((err / tol).max()))
                        written[b, slot, row, :lens[b]] = True
            assert np.isnan(got[~written]).all(), (sel, n, position, p0)         # rows >= max_rows, columns >= n_lfr, slots nobody selected: untouched


# ------------------------------------------------------------------------------------------------- soft-max, statistics, filter
BATCHES = [[(2, 1), (3, 3), (33, 4)], [(2, 7), (3, 64), (33, 65)], [(33, 257), (0, 5), (2, 3)], [(3, 4), (2, 257), (3, 1)]]


@pytest.mark.parametrize("width", [1, 3, 7])
@pytest.mark.parametrize("batch", BATCHES, ids=lambda v: "_".join("%dx%d" % s for s in v))
def test_softmax_statistics_filter(width, batch):
    rng = np.random.default_rng(width * 100 + sum(m for _, m in batch))
    B, P, R, ld = len(batch), 2, 34, 272
    n_rows, n_frames = [n for n, _ in batch], [m for _, m in batch]
    scores = np.full((B, P, R, ld), np.nan, np.float32)
    for b, (N, M) in enumerate(batch):
        scores[b, :, :N, :M] = rng.standard_normal((P, N, M)) * 3
    w = _probe().whisper_align_op("softmax", n_rows, n_frames, scores=scores)
    for b, (N, M) in enumerate(batch):
        want, rel = ref.softmax(scores[b, :, :N, :M]), ref.softmax_budget(scores[b, :, :N, :M])
        assert (np.abs(w[b, :, :N, :M] - want) <= rel * want + 2.0 ** -126).all(), (b, N, M)
        rest = np.ones((P, R, ld), bool)
        rest[:, :N, :M] = False
        assert np.isnan(w[b][rest]).all(), b                                  # crop first, then soft-max: nothing outside is read or written
    stats = _probe().whisper_align_op("colstats", n_rows, n_frames, scores=w)
    cost = _probe().whisper_align_op("cost", n_rows, n_frames, scores=w, stats=stats, width=width)
    worst = 0.0
    for b, (N, M) in enumerate(batch):
        if N:                                                 # (an utterance without rows has no matrix: nothing is computed for it, on either side)
            want, tol = ref.cost_matrix(scores[b, :, :N, :M], width), ref.cost_budget(scores[b, :, :N, :M], width)
            err = np.abs(cost[b, :N, :M] - want)
            assert (err <= tol).all(), (b, N, M, float(err.max()), float(tol.min()))
            worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
        rest = np.ones((R, ld), bool)
        rest[:N, :M] = False
        assert np.isnan(cost[b][rest]).all(), b
    if width == 7 and (2, 3) in batch:                        # 3 frames <= 7 // 2: the filter is skipped, the matrix is the plain standardised mean
        b = batch.index((2, 3))
        z = ref.standardise(ref.softmax(scores[b, :, :2, :3]))[0]
        assert np.abs(cost[b, :2, :3] + z.mean(axis=0)).max() < 1e-4
    if width == 7 and (3, 4) in batch:                        # 4 frames: filtered (a reflect-padded window of 7 over 4 columns)
        b = batch.index((3, 4))
        z = ref.standardise(ref.softmax(scores[b, :, :3, :4]))[0]
        assert np.abs(cost[b, :3, :4] + z.mean(axis=0)).max() > 1e-3
    print("cost matrix, width %d: largest error / budget = %.3g" % (width, worst))


def test_equal_rows_give_a_zero_matrix():
    rng = np.random.default_rng(9)
    B, P, R, ld = 2, 2, 4, 48
    scores = np.full((B, P, R, ld), np.nan, np.float32)
    scores[0, :, :2, :40] = np.repeat((rng.standard_normal((P, 1, 40)) * 3).astype(np.float32), 2, axis=1)       # two identical rows: variance 0
    scores[1, :, :3, :33] = np.repeat((rng.standard_normal((P, 1, 33)) * 3).astype(np.float32), 3, axis=1)       # three: the rounded mean need not equal them
    n_rows, n_frames = [2, 3], [40, 33]
    w = _probe().whisper_align_op("softmax", n_rows, n_frames, scores=scores)
    stats = _probe().whisper_align_op("colstats", n_rows, n_frames, scores=w)
    cost = _probe().whisper_align_op("cost", n_rows, n_frames, scores=w, stats=stats, width=7)
    assert (cost[0, :2, :40] == 0).all() and (cost[1, :3, :33] == 0).all()
    assert (stats[0, :, 1, :40] == 0).all()                                   # 1 / std is stored as 0 for such a column


# ------------------------------------------------------------------------------------------------- DTW
def _costs(rng, N, M, kind):
    if kind == "grid":
        return rng.integers(-4096, 4097, size=(N, M)).astype(np.float32) / np.float32(1024)
    return (rng.integers(0, 2, size=(N, M)) * kind).astype(np.float32) / np.float32(1024)       # {0, 1} / 1024 * k: ties on every diagonal


def _check_dtw(shapes, kind, seed):
    rng = np.random.default_rng(seed)
    B, R, ld = len(shapes), max(max(n for n, _ in shapes), 1), max(m for _, m in shapes)
    cost = np.full((B, R, ld), np.nan, np.float32)
    for b, (N, M) in enumerate(shapes):
        cost[b, :N, :M] = _costs(rng, N, M, kind)
    frames, paths = _probe().whisper_align_op("dtw", [n for n, _ in shapes], [m for _, m in shapes], cost=cost)
    for b, (N, M) in enumerate(shapes):
        if N == 0:
            assert len(paths[b]) == 0 and (frames[b] == -1).all()
            continue
        rows, cols = ref.dtw(cost[b, :N, :M])
        assert np.array_equal(paths[b][:, 0], rows) and np.array_equal(paths[b][:, 1], cols), (N, M, kind)
        assert np.array_equal(frames[b, :N], ref.jump_frames(rows, cols)), (N, M, kind)
        assert (frames[b, N:] == -1).all()
        assert (np.diff(frames[b, :N]) >= 0).all() and frames[b, 0] == 0


# (1, 1), (2, 1), (5, 2): tokens outnumber frames, the path must run vertically. 255 / 256 / 257 straddle the kernel's thread stride of 256 cells per diagonal.
SHAPES = [(1, 1), (2, 1), (5, 2), (1, 20), (5, 7), (64, 64), (65, 257), (300, 40), (63, 1500), (448, 1500), (255, 300), (256, 300), (257, 300), (300, 256),
          (300, 257)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_dtw_path_equals_the_reference(shape):
    _check_dtw([shape], "grid", shape[0] * 7 + shape[1])
    if shape[0] * shape[1] <= 100000:
        _check_dtw([shape], 1, shape[0] + shape[1])


def test_dtw_ties_at_the_largest_shape():
    _check_dtw([(448, 1500)], 3, 5)


def test_dtw_ragged_batch():
    for kind in ("grid", 1, 3):
        _check_dtw([(5, 7), (0, 5), (65, 257), (300, 40)], kind, 21)
