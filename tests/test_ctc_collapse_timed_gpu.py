"""GPU, op level: the CTC collapse with spans (asr_op_ctc_collapse_timed -> ctc_collapse_timed_kernel) against the plain-Python statement of
tests/ctc_timing_ref.py. Integers are exact; ids and counts equal asr_op_ctc_collapse on the same input. The token score is an f32 sum in ascending frame
order divided by the f32 count: the library is built without fast-math flags, hipcc's f32 division is then correctly rounded, and the numpy restatement is
asserted bit for bit."""
import numpy as np
import pytest

import ctc_timing_ref as R
from conftest import sub

pytestmark = pytest.mark.gpu

FILL = (-7, np.float32(-777.0))


def _run(seqs, max_tokens=None):
    eng = sub("engine")
    lens = [len(s) for s in seqs]
    flat = np.concatenate(seqs).astype(np.int32)
    lps = [R.case_logprob(100 + i, n) for i, n in enumerate(lens)]
    got = eng.op_ctc_collapse_timed(flat, np.concatenate(lps), lens, blank_id=0, max_tokens=max_tokens, fill=FILL)
    plain = eng.op_ctc_collapse(flat, lens, blank_id=0)
    return got, plain, lps


def _check(seqs, got, plain, lps, max_tokens=None):
    tok, first, last, tlp, num = got
    cap = tok.shape[1]
    for b, (ids, lp) in enumerate(zip(seqs, lps)):
        wt, wf, wl, ws = R.collapse_timed(ids, lp, 0)
        assert num[b] == len(wt) == len(plain[b]), (b, num[b], len(wt))
        n = min(len(wt), cap)
        assert np.array_equal(tok[b, :n], wt[:n]) and np.array_equal(tok[b, :n], plain[b][:n])
        assert np.array_equal(first[b, :n], wf[:n]) and np.array_equal(last[b, :n], wl[:n])
        assert np.array_equal(tlp[b, :n].view(np.uint32), ws[:n].view(np.uint32)), (tlp[b, :n], ws[:n])
        one = wf[:n] == wl[:n]
        assert np.array_equal(tlp[b, :n][one], lp[wl[:n][one]])                      # one-frame runs: the frame's own value
        # slots the kernel does not write keep what they held
        assert (tok[b, n:] == FILL[0]).all() and (first[b, n:] == FILL[0]).all() and (last[b, n:] == FILL[0]).all() and (tlp[b, n:] == FILL[1]).all()


@pytest.mark.parametrize("name", sorted(R.COLLAPSE_CASES))
def test_hand_written_cases(name):
    ids, want = R.COLLAPSE_CASES[name]
    got, plain, lps = _run([ids])
    tok, first, last, tlp, num = got
    assert [(int(t), int(f), int(l)) for t, f, l in zip(tok[0, :num[0]], first[0, :num[0]], last[0, :num[0]])] == want
    _check([ids], got, plain, lps)


def test_ragged_batch_one_beside_seven_hundred():
    rng = np.random.default_rng(5)
    long = np.repeat(rng.integers(0, 4, 700), rng.integers(1, 5, 700))[:700].astype(np.int32)      # short runs (1..4 frames each, so 700 runs always suffice) of ids 0..3 over three chunks
    assert long.size == 700
    seqs = [R.runs((5, 1)), long, R.COLLAPSE_CASES["run_257"][0], R.runs((0, 1)), R.COLLAPSE_CASES["straddle_511_512_from_200"][0]]
    got, plain, lps = _run(seqs)
    assert got[4][1] > 100
    _check(seqs, got, plain, lps)


def test_max_tokens_below_the_token_count():
    rng = np.random.default_rng(6)
    ids = np.repeat(rng.integers(0, 5, 200), 2).astype(np.int32)
    seqs = [ids, R.runs((0, 2), (3, 2), (0, 2))]
    got, plain, lps = _run(seqs, max_tokens=7)
    assert got[4][0] > 7 and got[4][1] == 1                    # num_id holds the full count
    tok, first, last, tlp, num = got
    wt, wf, wl, ws = R.collapse_timed(ids, lps[0], 0)
    assert np.array_equal(tok[0], wt[:7]) and np.array_equal(first[0], wf[:7]) and np.array_equal(last[0], wl[:7])
    assert np.array_equal(tlp[0].view(np.uint32), ws[:7].view(np.uint32))
    assert tok[1, 0] == 3 and (tok[1, 1:] == FILL[0]).all() and (tlp[1, 1:] == FILL[1]).all()
