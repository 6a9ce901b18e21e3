"""GPU, op level: the emission kernel of the CTC forced alignment (asr_probe_ctc_target_logprob: the timed head's per-slab partials ->
launch_ctc_target_logprob) against float64 a w^T + b - logsumexp, f32 and bf16 operands (bf16: float64 on the bf16-rounded operands).

Operands as test_ctc_topk_gpu builds them (K = 64, once 512; columns at and past n_valid carry a bias of +50: they would swallow the log-sum-exp). The rows
are split into three transcripts and one row that belongs to none. Per transcript, taken from the logits of its first row: column n_valid - 1, a column of
the last partly valid slab, the row's arg-max twice (a repeated id), a mid-rank column, then two random ones; the second transcript is shorter (slots behind
it are -inf), the third is empty. Slot 0 is the blank.

Bound per (row, slot): the recomputed logit's K 2^-24 sum |a_k w_k| plus ctc_timing_ref.budget for the row's log-sum-exp (its K part covers the head's own
logits). A target that asr_probe_ctc_topk also returns for the row must have that candidate's bits."""
import functools

import numpy as np
import pytest

import ctc_timing_ref as tref
from conftest import sub

pytestmark = pytest.mark.gpu

BF16, F32 = 0, 1
SIZES = {"small": (37, 256, 200), "vocab": (5, 25088, 25055)}          # M, N, n_valid (small: the last slab has 8 valid columns)
BLANK = 0


@functools.lru_cache(maxsize=None)
def _case(size, prec, K):
    M, N, n_valid = SIZES[size]
    rng = np.random.default_rng(11 + K)
    a = rng.normal(0.0, 1.0, (M, K)).astype(np.float32)
    w = rng.normal(0.0, 0.35 * (64.0 / K) ** 0.5, (N, K)).astype(np.float32)
    bias = rng.normal(0.0, 0.5, N).astype(np.float32)
    bias[n_valid:] = 50.0
    rnd = tref.bf16_round if prec == BF16 else (lambda x: x)
    ar, wr = rnd(a).astype(np.float64), rnd(w).astype(np.float64)
    logits = ar @ wr[:n_valid].T + bias[:n_valid].astype(np.float64)
    lse = np.logaddexp.reduce(logits, axis=1)
    abs_dot = np.abs(ar) @ np.abs(wr[:n_valid]).T
    _, lp_max, spread = tref.frame_logprob(logits)
    cuts = [0, (M - 1) * 2 // 5, (M - 1) * 4 // 5, M - 1]             # three transcripts; the last row belongs to none
    row_utt = np.full(M, -1, np.int32)
    targets = []
    for u in range(3):
        row_utt[cuts[u]:cuts[u + 1]] = u
        v = logits[cuts[u]]
        top, mid = int(np.argmax(v)), int(np.argsort(v)[n_valid // 2])
        t = [n_valid - 1, (n_valid - 1) // 64 * 64 + 1, top, top, mid] + [int(c) for c in rng.integers(1, n_valid, 2)]
        targets.append(np.asarray([t, t[:5], []][u], np.int32))
    for z in (a, w, bias, logits, lse, abs_dot, lp_max, spread, row_utt):
        z.setflags(write=False)
    return a, w, bias, logits, lse, abs_dot, lp_max, spread, row_utt, targets


@pytest.mark.parametrize("prec,size,K", [(F32, "small", 64), (BF16, "small", 64), (F32, "vocab", 64), (BF16, "vocab", 64), (BF16, "small", 512)],
                         ids=["f32-small", "bf16-small", "f32-vocab", "bf16-vocab", "bf16-small-K512"])
def test_emissions_equal_the_float64_log_softmax(prec, size, K):
    probe = sub("_probe")
    M, N, n_valid = SIZES[size]
    a, w, bias, logits, lse, abs_dot, lp_max, spread, row_utt, targets = _case(size, prec, K)
    em, stray, kern = probe.ctc_target_logprob(a, w, bias, row_utt, targets, blank_id=BLANK, n_valid=n_valid, precision=prec)
    ld = em.shape[1]
    assert ld == 8 and stray == 0                                    # rows at and past M are untouched
    lse_budget = tref.budget(n_valid, lp_max, spread, K=K, abs_dot=abs_dot.max(axis=1), vmax=np.abs(logits).max(axis=1))
    worst = 0.0
    for m in range(M):
        u = row_utt[m]
        if u < 0:
            assert np.all(em[m].view(np.uint32) == 0xFFFFFFFF)       # a row without a transcript keeps what the buffer held
            continue
        cols = [BLANK] + [int(c) for c in targets[u]]
        assert np.all(np.isneginf(em[m, len(cols):]))                # slots past L_b
        for j, c in enumerate(cols):
            want = logits[m, c] - lse[m]
            bound = K * 2.0 ** -24 * abs_dot[m, c] + lse_budget[m]
            err = abs(float(em[m, j]) - want)
            worst = max(worst, err / bound)
            assert err <= bound, (m, j, c, err, bound)
    print(f"ctc_target_logprob {kern} {size} K {K}: largest error / bound = {worst:.3g}")
    # a target that is also a candidate of its row has the candidate's bits
    ids, lp, _ = probe.ctc_topk(a, w, bias, 8, n_valid=n_valid, variant=-1, precision=prec)
    shared = 0
    for m in range(M):
        u = row_utt[m]
        if u < 0:
            continue
        for j, c in enumerate([BLANK] + [int(c) for c in targets[u]]):
            for k in np.nonzero(ids[m] == c)[0]:
                assert em[m, j].view(np.uint32) == lp[m, k].view(np.uint32), (m, j, c, em[m, j], lp[m, k])
                shared += 1
    assert shared >= 4                                               # at least the arg-max (twice) of the first row of both non-empty transcripts
