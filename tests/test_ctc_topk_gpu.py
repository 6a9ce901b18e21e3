"""GPU, op level: the candidate kernel of the CTC prefix beam search (asr_probe_ctc_topk: the timed head's per-slab partials -> launch_ctc_topk) against a
float64 a w^T + b, f32 and bf16 operands (bf16: float64 on the bf16-rounded operands).

Operands (K = 64, rows cycle through three planted kinds, the rest random):
  pair   the best two tokens of the row share a 64-column slab
  last   the row's topk-th best token is the last valid column (its weight row is a multiple of the activation row, scaled to fall between the neighbours)
  equal  two identical weight rows with equal bias in different slabs are the row's best two: exactly equal logits in any arithmetic, lower id first
Columns at and past n_valid carry a bias of +50: a candidate from there would win every row.
Ids are compared where the float64 gaps between neighbours of the best topk + 1 clear twice the measured logit error (gaps of exactly 0 are the planted
identical columns, ordered by id); the seed is chosen so that every row qualifies by float64 alone (gaps > 1e-4, asserted: five times the f32 accumulation bound K 2^-24 sum |a_k w_k| of a logit of 5), within the 2 % allowance."""
import functools

import numpy as np
import pytest

from conftest import sub

pytestmark = pytest.mark.gpu

BF16, F32 = 0, 1
K = 64
SIZES = {"small": (37, 256, 200), "vocab": (5, 25088, 25055)}          # M, N, n_valid (small: the last slab has 8 valid columns)


def _bf16_round(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def _case(size, topk, prec):
    M, N, n_valid = SIZES[size]
    rng = np.random.default_rng(7 + topk)
    a = rng.normal(0.0, 1.0, (M, K)).astype(np.float32)
    w = rng.normal(0.0, 0.35, (N, K)).astype(np.float32)
    bias = rng.normal(0.0, 0.5, N).astype(np.float32)
    bias[n_valid:] = 50.0
    kinds = ["pair", "last", "equal"]
    kind = [kinds[m] if m < 3 else "random" for m in range(M)]
    rnd = (lambda x: _bf16_round(x)) if prec == BF16 else (lambda x: x)
    unit = lambda m: a[m] / float(a[m].astype(np.float64) @ a[m].astype(np.float64))          # w = s * unit(m): logit of row m = s (+ bias)
    # pair: columns 70 and 75 (slab 1) far above everything else of row 0
    w[70], w[75], bias[70], bias[75] = 30.0 * unit(0), 28.0 * unit(0), 0.0, 0.0
    # equal: columns 10 (slab 0) and 140 (slab 2) identical, the best two of row 2
    w[10] = 26.0 * unit(2); w[140] = w[10]; bias[10] = bias[140] = 0.25
    # last: the last valid column lands between the (topk - 1)-th and topk-th best of row 1
    last = n_valid - 1
    w[last], bias[last] = 0.0, 0.0
    ar, wr = rnd(a).astype(np.float64), rnd(w).astype(np.float64)
    row = np.sort((ar[1] @ wr[:n_valid].T + bias[:n_valid].astype(np.float64))[np.arange(n_valid) != last])[::-1]
    target = row[0] + 1.0 if topk == 1 else 0.5 * (row[topk - 2] + row[topk - 1])
    w[last] = np.float32(target) * unit(1)
    ar, wr = rnd(a).astype(np.float64), rnd(w).astype(np.float64)
    logits = ar @ wr[:n_valid].T + bias[:n_valid].astype(np.float64)
    lse = np.logaddexp.reduce(logits, axis=1)
    order = np.argsort(-logits, axis=1, kind="stable")[:, :topk + 1]                        # equal values: lower id first
    top = np.take_along_axis(logits, order, axis=1)
    abs_dot = np.abs(ar) @ np.abs(wr[:n_valid]).T
    for z in (a, w, bias, logits, lse, order, top, abs_dot):
        z.setflags(write=False)
    return a, w, bias, kind, logits, lse, order, top, abs_dot


@pytest.mark.parametrize("topk", [1, 8, 16])
@pytest.mark.parametrize("size", sorted(SIZES))
@pytest.mark.parametrize("prec", [F32, BF16], ids=["f32", "bf16"])
def test_candidates_equal_the_float64_top_k(prec, size, topk):
    probe = sub("_probe")
    M, N, n_valid = SIZES[size]
    a, w, bias, kind, logits, lse, order, top, abs_dot = _case(size, topk, prec)
    ids, lp, kern = probe.ctc_topk(a, w, bias, topk, n_valid=n_valid, variant=-1, precision=prec)
    assert ids.shape == lp.shape == (M, topk)
    assert (ids >= 0).all() and (ids < n_valid).all(), "a padded column among the candidates"
    assert all(len(set(r)) == topk for r in ids.tolist())
    ref_lp = logits - lse[:, None]
    err = np.abs(lp.astype(np.float64) - np.take_along_axis(ref_lp, ids.astype(np.int64), axis=1))
    e = float(err.max())                                              # the measured logit error (the row's log-sum-exp error included)
    print(f"ctc_topk {kern} {size} topk {topk}: max log-probability error {e:.2e}")
    assert e <= 1e-3
    assert (np.diff(lp, axis=1) <= 0).all()                           # higher value first
    gaps = top[:, :-1] - top[:, 1:]
    by_f64 = ((gaps == 0) | (gaps > 1e-4)).all(axis=1)
    assert by_f64.all(), "seed: a float64 near-tie among the best topk + 1"
    safe = ((gaps == 0) | (gaps > 2 * e)).all(axis=1)
    assert (~safe).mean() <= 0.02
    assert np.array_equal(ids[safe], order[safe, :topk])
    # the planted rows are what they were built to be
    assert kind[:3] == ["pair", "last", "equal"]
    assert order[0, 0] == 70 and (topk == 1 or order[0, 1] == 75)
    assert order[1, topk - 1] == n_valid - 1 and ids[1, topk - 1] == n_valid - 1
    assert order[2, 0] == 10 and ids[2, 0] == 10
    if topk > 1:
        assert ids[2, 1] == 140 and lp[2, 0] == lp[2, 1] and ids[0, 0] // 64 == ids[0, 1] // 64


@pytest.mark.parametrize("size", sorted(SIZES))
def test_top_1_is_the_heads_argmax_and_frame_logprob(size):
    """topk = 1 against asr_probe_ctc_head on the same operands: the same id; the log-probability differs only by the recomputed logit against the GEMM's
    (two f32 accumulation orders of K terms: each within K 2^-24 sum |a_k w_k| of the exact value)."""
    probe = sub("_probe")
    M, N, n_valid = SIZES[size]
    a, w, bias, kind, logits, lse, order, top, abs_dot = _case(size, 1, BF16)
    ids, lp, kern = probe.ctc_topk(a, w, bias, 1, n_valid=n_valid, variant=-1, precision=BF16)
    hid, hlp, stray, hkern = probe.ctc_head(a, w, bias, n_valid=n_valid, variant=-1)
    assert kern == hkern and np.array_equal(ids[:, 0], hid)
    bound = 2 * K * 2.0 ** -24 * abs_dot[np.arange(M), hid] + 1e-6
    d = np.abs(lp[:, 0].astype(np.float64) - hlp.astype(np.float64))
    print(f"topk 1 vs ctc_head {size}: max difference {d.max():.2e}, bound {bound.min():.2e}..{bound.max():.2e}")
    assert (d <= bound).all()
