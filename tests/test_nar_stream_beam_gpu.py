"""GPU, op level: the streaming beam search with carried state and fixed-lag commits (asr_op_nar_stream_beam -> nar_stream_beam_kernel, both
instantiations) against its float64 statement (tests/nar_stream_beam_ref.py): no model, orders 2 and 4, plain and with hotwords.

The cases are nar_stream_beam_ref.shape_cases' and schedule_case's: seeds whose decision gap is >= 1e-3 at every cut the search makes, with a model or
hotwords one of them with a best hypothesis the plain search does not return (test_nar_stream_beam_ref_cpu.py holds both as conditions). Token lists,
counts and `total` must be equal, committed and pending log-probabilities are the candidates' own bits; score and am within TOL = 1.02e-4: a float32
restatement of the reference differs from float64 by at most 1.7e-5 over these cases (test_nar_stream_beam_ref_cpu.py prints and pins it), 6 x that is
1.02e-4, and the bound is never more than a quarter of the gap. Measured on an MI355X: at most 1.61e-5 over all cases here (the kernel's sums are the float32
restatement's: every per-case figure equals the one the CPU test prints).

A stream of at most pend_cap rows followed by a finish is engine.op_nar_beam on the concatenated rows bit for bit, whatever the chunking: the order of
operations is the offline kernel's."""
import numpy as np
import pytest

import ctc_beam_ref as R
import ctc_lm_ref as L
import nar_beam_ref as N
import nar_stream_beam_ref as S
from conftest import sub

pytestmark = pytest.mark.gpu

GAP = L.GAP
F32_RESTATEMENT = 1.7e-5
TOL = min(6 * F32_RESTATEMENT, GAP / 4)
assert TOL <= min(6 * F32_RESTATEMENT, GAP / 4) and TOL == pytest.approx(1.02e-4)

POISON_I, POISON_F = -1, np.float32(np.nan)


def _steps(ids, lp, cuts, sid=0):
    return [[(sid, ids[a:b], lp[a:b], False)] for a, b in zip(cuts[:-1], cuts[1:])] + [[(sid, ids[:0], lp[:0], True)]]


def _run(eng, steps, n_streams, beam, nbest, cap, image=None, phrases=None, boost=0.0, alpha=L.ALPHA, beta=L.BETA, oov=L.OOV, state=None):
    trie = eng.hotword_trie(phrases) if phrases else None
    return eng.op_nar_stream_beam(steps, n_streams, beam, nbest, cap, trie=trie, boost=boost, lm=image, alpha=alpha, beta=beta, oov_logprob=oov, state=state,
                                  fill=(POISON_I, POISON_F))


def _compare(out, slot, ref, nbest):
    """one slot of one step against the reference's result of that step; returns the largest score error"""
    f32 = lambda xs: [float(np.float32(x)) for x in xs]
    nc = int(out["commit_num"][slot])
    assert int(out["total"][slot]) == ref["total"]
    assert out["commit_ids"][slot, :nc].tolist() == [c for c, _ in ref["commit"]], (out["commit_ids"][slot, :nc].tolist(), ref["commit"])
    assert out["commit_logprob"][slot, :nc].tolist() == f32(p for _, p in ref["commit"])                   # the candidates' own values, bit for bit
    assert np.all(out["commit_ids"][slot, nc:] == POISON_I) and np.all(np.isnan(out["commit_logprob"][slot, nc:]))     # nothing written past the count
    worst = 0.0
    for m in range(nbest):
        num = int(out["pend_num"][slot, m])
        if m < len(ref["pending"]):
            t = ref["pending"][m]
            assert num == len(t["tokens"]) and out["pend_ids"][slot, m, :num].tolist() == t["tokens"], (m, out["pend_ids"][slot, m, :num].tolist(), t["tokens"])
            assert out["pend_logprob"][slot, m, :num].tolist() == f32(t["logprob"])
            err = max(abs(float(out["pend_score"][slot, m]) - t["score"]), abs(float(out["pend_am"][slot, m]) - t["am_score"]))
            assert err <= TOL, (m, float(out["pend_score"][slot, m]), t["score"], float(out["pend_am"][slot, m]), t["am_score"])
            worst = max(worst, err)
        else:
            assert num == 0 and out["pend_score"][slot, m] == -np.inf and out["pend_am"][slot, m] == -np.inf
        assert np.all(out["pend_ids"][slot, m, num:] == POISON_I)
    return worst


@pytest.mark.parametrize("hot", [False, True], ids=["plain", "hotwords"])
@pytest.mark.parametrize("order", S.MODELS, ids=lambda o: f"order{o}" if o else "no_model")
@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: s[0])
def test_search_equals_the_float64_statement(shape, order, hot):
    eng = sub("engine")
    name, n, topk, beam, nbest, vocab, cap, cuts = shape
    cases = S.shape_cases(shape, order, hot)
    assert len(cases) == 2
    worst = 0.0
    for seed, ids, lp, res, gap, differs in cases:
        _, boost, image, phrases = S.case_setting(shape, order, hot, ids, seed)
        print(f"shape {name} model {order} hot {hot} seed {seed}: gap {gap:.2e}, best differs from the plain search: {differs}")
        assert gap >= GAP and TOL <= gap / 4
        outs = _run(eng, _steps(ids, lp, cuts), 1, beam, nbest, cap, image, phrases, boost)
        assert len(outs) == len(res)
        for out, ref in zip(outs, res):
            worst = max(worst, _compare(out, 0, ref, nbest))
        if differs:                                        # ... and the op without model and hotwords really returns something else
            plain = _run(eng, _steps(ids, lp, cuts), 1, beam, nbest, cap)
            got = [int(c) for o in plain for c in o["commit_ids"][0, :o["commit_num"][0]]]
            assert len(got) == n and got != res[-1]["hypotheses"][0]["tokens"]
    print(f"largest score error {worst:.2e}")


def test_several_streams_subsets_out_of_order_reuse_and_untouched_state():
    eng = sub("engine")
    c = S.SCHEDULE
    steps, results, gap, (phrases, trie, image) = S.schedule_case()
    assert gap >= GAP and TOL <= gap / 4
    words = eng.nar_stream_beam_state_words(c["beam"], c["pend_cap"])

    def poisoned():                                        # every word -1 (a NaN as f32); a stream is cleared by its first word alone
        st = np.full((c["n_streams"], words), -1, dtype=np.int32)
        st[:4, 0] = 0
        return st

    state = poisoned()
    outs = _run(eng, steps, c["n_streams"], c["beam"], c["nbest"], c["pend_cap"], image, phrases, L.BOOST, state=state)
    worst = 0.0
    for out, refs in zip(outs, results):
        for slot, ref in enumerate(refs):
            worst = max(worst, _compare(out, slot, ref, c["nbest"]))
    print(f"largest score error {worst:.2e}")
    assert np.all(state[4] == -1)                          # the stream no step names: not a byte moved
    assert np.all(state[:4, 0] == 0)                       # everything else was finished: cleared
    # a stream absent from a step keeps its bytes: stream 2 after step 0 alone, and after steps 0 and 1 (which name streams 0 and 3)
    s0, s01 = poisoned(), poisoned()
    _run(eng, steps[:1], c["n_streams"], c["beam"], c["nbest"], c["pend_cap"], image, phrases, L.BOOST, state=s0)
    _run(eng, steps[:2], c["n_streams"], c["beam"], c["nbest"], c["pend_cap"], image, phrases, L.BOOST, state=s01)
    assert s0[2, 0] == 3 and s0[2].tobytes() == s01[2].tobytes() and np.all(s0[3, 1:] == -1) and s01[3, 0] == 1
    # ... and the state is really what carries the search: the remaining steps from the saved state give the one run's outputs, byte for byte
    rest = _run(eng, steps[2:], c["n_streams"], c["beam"], c["nbest"], c["pend_cap"], image, phrases, L.BOOST, state=s01)
    for a, b in zip(rest, outs[2:]):
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
    # two identical runs: the same bytes
    again = _run(eng, steps, c["n_streams"], c["beam"], c["nbest"], c["pend_cap"], image, phrases, L.BOOST, state=poisoned())
    for a, b in zip(again, outs):
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("shape", [N.SHAPES[1], N.SHAPES[3], N.SHAPES[4], N.SHAPES[6]], ids=lambda s: "N%d_k%d_b%d_v%d" % s)
def test_within_pend_cap_a_finish_is_the_offline_search_bit_for_bit(shape):
    eng = sub("engine")
    n, topk, beam, vocab = shape
    ids, lp = N.random_case(3, n, topk, vocab)
    phrases = R.random_phrases(3, 3, vocab)
    for image, hot in ((None, None), (None, phrases), (L.shape_model(vocab, 2)[1], None), (L.shape_model(vocab, 4)[1], phrases)):
        trie = eng.hotword_trie(hot) if hot else None
        tok, num, score, am, tlp = eng.op_nar_beam(ids, lp, [n], beam, beam, trie=trie, boost=L.BOOST, lm=image, alpha=L.ALPHA, beta=L.BETA, oov_logprob=L.OOV)
        for cap, cuts in ((n, (0, n)), (64, (0, n // 3, n // 3, n - 1, n)), (n, tuple(range(n + 1)))):
            outs = _run(eng, _steps(ids, lp, cuts), 1, beam, beam, cap, image, hot, L.BOOST)
            assert all(o["commit_num"][0] == 0 for o in outs[:-1])
            fin = outs[-1]
            assert fin["total"][0] == n and fin["commit_num"][0] == n
            assert fin["pend_num"][0].tobytes() == num[0].tobytes() and fin["pend_ids"][0, :, :n].tobytes() == tok[0].tobytes()
            assert fin["pend_score"][0].tobytes() == score[0].tobytes() and fin["pend_am"][0].tobytes() == am[0].tobytes()
            assert fin["pend_logprob"][0, :, :n].tobytes() == tlp[0].tobytes()
            assert fin["commit_ids"][0, :n].tobytes() == tok[0, 0].tobytes() and fin["commit_logprob"][0, :n].tobytes() == tlp[0, 0].tobytes()


def test_two_chunkings_of_a_saturating_stream_give_the_same_bytes():
    eng = sub("engine")
    for shape in (S.SHAPES[1], S.SHAPES[3], S.SHAPES[4]):
        name, n, topk, beam, nbest, vocab, cap, cuts = shape
        seed, ids, lp, res, gap, differs = S.shape_cases(shape, 4, True)[0]
        _, boost, image, phrases = S.case_setting(shape, 4, True, ids, seed)
        runs = []
        for c in (cuts, (0, n), tuple(range(n + 1)), (0, 0, 1, n - 1, n - 1, n)):
            outs = _run(eng, _steps(ids, lp, c), 1, beam, nbest, cap, image, phrases, boost)
            commits = b"".join(o[k][0, :o["commit_num"][0]].tobytes() for k in ("commit_ids", "commit_logprob") for o in outs)
            fin = outs[-1]
            assert sum(int(o["commit_num"][0]) for o in outs[:-1]) == n - cap > 0
            runs.append((commits,) + tuple(fin[k].tobytes() for k in ("pend_ids", "pend_logprob", "pend_num", "pend_score", "pend_am", "total")))
        assert all(r == runs[0] for r in runs[1:])


def test_malformed_arguments_raise():
    eng, lib = sub("engine"), sub("_lib")
    vocab = 12
    image = L.shape_model(vocab, 4)[1]
    ids, lp = N.random_case(0, 9, 3, vocab)
    _run(eng, _steps(ids, lp, (0, 4, 9)), 1, 2, 2, 4, image)                 # the arguments themselves are fine
    for beam, nbest, cap in ((17, 1, 4), (2, 3, 4), (2, 2, 0), (2, 2, 65)):
        with pytest.raises(lib.AsrError):
            _run(eng, _steps(ids, lp, (0, 4, 9)), 1, beam, nbest, cap)
    with pytest.raises(lib.AsrError, match="once per step"):
        _run(eng, [[(0, ids, lp, False), (0, ids, lp, False)]], 2, 2, 2, 4)
    with pytest.raises(lib.AsrError, match="once per step"):
        _run(eng, [[(2, ids, lp, False)]], 2, 2, 2, 4)
    dup = ids.copy()
    dup[4, 1] = dup[4, 0]
    with pytest.raises(lib.AsrError, match="twice"):
        _run(eng, _steps(dup, lp, (0, 9)), 1, 2, 2, 4)
    wide = ids.copy()
    wide[4, 0] = vocab + 1                                 # a candidate the model's tables do not cover
    with pytest.raises(lib.AsrError, match="vocabulary"):
        _run(eng, _steps(wide, lp, (0, 9)), 1, 2, 2, 4, image)
    with pytest.raises(lib.AsrError, match="words"):
        _run(eng, _steps(ids, lp, (0, 9)), 1, 2, 2, 4, state=np.zeros((1, 7), np.int32))
    bad = np.zeros((1, eng.nar_stream_beam_state_words(2, 4)), np.int32)
    bad[0, :3] = (9, 2, 1)                                 # seven uncommitted positions in a ring of four
    with pytest.raises(lib.AsrError):
        _run(eng, _steps(ids, lp, (0, 9)), 1, 2, 2, 4, state=bad)
    with pytest.raises(ValueError):
        eng.nar_stream_beam_state_words(2, 65)
