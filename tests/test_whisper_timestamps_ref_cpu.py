"""The float64 reference of Whisper's timestamp rules against itself (tests/whisper_timestamps_ref.py): the literal OpenAI procedure and the reduced
form the kernel computes agree on every case of the GPU tests, every case is decided by the margin its generator asserts, a greedy walk under the
rules yields only grammatical streams, and whisper.split_segments turns such streams into the segments written down by hand."""
import numpy as np
import pytest

import whisper_timestamps_ref as ref
from conftest import sub


@pytest.fixture(scope="module", params=ref.GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
def cases(request):
    return request.param, ref.kernel_cases(request.param)


def test_both_statements_agree_and_every_case_is_decided(cases):
    geom, cs = cases
    seen = set()
    for name, c in cs.items():
        got, margins, budgets = ref.apply(c["logits"], c["hists"], c["params"])
        assert np.all(margins >= ref.MARGIN_FACTOR * budgets), name
        assert 3 <= len(c["hists"]) <= 5, name
        if c["openai"]:
            lit, _, _ = ref.apply(c["logits"], c["hists"], c["params"], openai=True)
            assert np.array_equal(got, lit), name
        assert not np.isnan(got).any(), name
        finite = np.isfinite(margins)
        text_masked = np.isneginf(got[:, :c["params"][0]]).all(axis=1)
        seen |= {(bool(f), bool(t)) for f, t in zip(finite, text_masked)}
        # planted margins are tight: within the asserted margin plus two steps of the logits' grid
        assert np.all(margins[finite] <= ref.MARGIN_FACTOR * budgets[finite] + 3 * ref.GRID), name
    assert seen == {(True, True), (True, False), (False, True), (False, False)}, seen       # compared and masked / kept, not compared and masked / kept


def test_the_rule_step_by_step():
    """Hand-checked rows at (n_valid, eot, ts_begin) = (12, 5, 8): text 0-4, eot 5, specials 6-7 (7 = <|notimestamps|>), timestamps 8-11."""
    p = (8, 7, 5, -1)
    flat = np.zeros(12, np.float32)
    inf = -np.inf

    def masked(row, hist, params=p):
        a, _ = ref.rules_reduced(row, hist, *params)
        assert np.array_equal(a, ref.rules_openai(row, hist, *params))
        return np.isneginf(a).tolist()

    m = lambda s: [ch == "x" for ch in s]
    # equal logits: four timestamps outweigh any single text id (log 4 > 0), so L > T wherever a timestamp is left
    assert masked(flat, []) == m("xxxxxxxx....")                             # first id: a timestamp
    assert masked(flat, [], (8, 7, 5, 1)) == m("xxxxxxxx..xx")                # max_initial 1
    assert masked(flat, [9]) == m(".......xxxxx")                            # after the opening timestamp: text (and specials), no timestamp
    assert masked(flat, [9, 2]) == m("xxxxxxxxxx..")                          # strictly later timestamps; two of them outweigh the text
    text = flat.copy(); text[3] = 1.0                                         # log 2 < 1: the text wins
    assert masked(text, [9, 2]) == m(".......xxx..")
    assert masked(text, [9, 2, 10]) == m("xxxxxxxxxx..")                      # closing at 10: no text; 10 itself stays; L = log 2 > T = 0 (eot)
    eot = flat.copy(); eot[5] = 1.0
    assert masked(eot, [9, 2, 10]) == m("xxxxx..xxx..")                       # ... unless eot outweighs them
    assert masked(flat, [9, 2, 10, 10]) == m(".......xxxxx")                  # after a pair: text
    assert masked(flat, [9, 2, 10, 10, 4]) == m(".......xxxx.")                # one timestamp left: L = T, and only L > T masks the text
    assert masked(flat, [9, 2, 11]) == m("xxxxx..xxxx.")                      # the last timestamp id can still open a segment where one closed
    assert masked(text, [11, 2]) == m(".......xxxxx")                         # nothing later than the last id
    gone = np.full(12, inf, np.float32); gone[5] = 0.5
    a, mg = ref.rules_reduced(gone, [9, 2], *p)
    assert mg == np.inf and a[5] == np.float32(0.5) and np.isneginf(np.delete(a, 5)).all()


@pytest.mark.parametrize("geom", ref.GEOMETRIES[:2], ids=lambda g: "x".join(map(str, g)))
def test_a_greedy_walk_is_grammatical(geom):
    n_valid, eot, ts_begin = geom
    lengths, kinds = [], set()
    for seed in range(12):
        for scale in (-2.0, 0.0, 2.0):
            ids = ref.greedy_walk(geom, seed, 40, max_initial=3 if seed % 2 else -1, scale=scale)
            assert ref.grammatical(ids, ts_begin, ts_begin - 1, eot), ids
            assert ids and ids[0] >= ts_begin and (seed % 2 == 0 or ids[0] <= ts_begin + 3)
            assert ts_begin - 1 not in ids
            lengths.append(len(ids))
            kinds |= {"text" if t < eot else "ts" for t in ids}
            kinds |= {"pair" for a, b in zip(ids, ids[1:]) if a >= ts_begin and b >= ts_begin}
    assert max(lengths) >= 10 and kinds == {"text", "ts", "pair"}


def test_the_grammar_check_refuses_what_the_rules_exclude():
    g = lambda ids: ref.grammatical(ids, 100, 99, 90)
    assert g([]) and g([100]) and g([100, 5]) and g([100, 5, 110]) and g([100, 5, 110, 110, 6, 120]) and g([100, 5, 110, 115, 6])
    assert not g([5])                           # text first
    assert not g([100, 101])                    # two timestamps open the stream
    assert not g([100, 5, 110, 6])              # text after a closing timestamp
    assert not g([100, 5, 110, 110, 111])       # three timestamps in a row
    assert not g([105, 5, 104])                 # a timestamp goes back
    assert not g([100, 99]) and not g([100, 95])   # <|notimestamps|>, another special


@pytest.mark.parametrize("name", list(ref.SPLIT_CASES))
def test_split_segments(name):
    ids, offset, length, want = ref.SPLIT_CASES[name]
    got = sub("whisper").split_segments(ids, ref.TS0, offset, length)
    assert [s["tokens"] for s in got] == [s["tokens"] for s in want]
    assert np.allclose([(s["start"], s["end"]) for s in got], [(s["start"], s["end"]) for s in want], rtol=0, atol=1e-9) if want else got == []
    assert sub("whisper").split_segments(np.asarray(ids, np.int32), ref.TS0, offset, length) == got        # arrays as well as lists


def test_head_steps_inputs_are_decided_and_take_every_branch():
    c = ref.HEAD_STEPS
    x, _, _ = ref.head_steps_inputs()
    n_valid, eot, ts_begin = ref.HEAD_GEOM
    for name, kw in ref.head_steps_cases().items():
        picks, save, n, decided, margins, budgets = ref.head_steps(x, c["steps"], c["ld_save"], **kw)
        assert n == c["steps"] and np.array_equal(save[:, :n], picks.T), name
        assert np.all(margins >= ref.MARGIN_FACTOR * budgets), (name, margins, budgets)
        assert decided.all(), name
        for r in range(c["rows"]):
            stream = picks[:, r].tolist()
            stream = stream[:stream.index(eot)] if eot in stream else stream
            assert all(t < eot or t >= ts_begin for t in stream) and ref.grammatical(stream, ts_begin, ts_begin - 1, eot), (name, stream)
        kinds = {"text" if t < eot else "ts" for t in picks.ravel()}
        assert kinds == {"text", "ts"}, (name, picks)
