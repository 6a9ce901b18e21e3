"""n-gram LM fusion of the autoregressive decoders at kernel level (csrc/decoder_lm.hip, TokenHead / BeamRanker of csrc/decode_head.h) through the probe
library, against the float64 statement tests/decoder_lm_ref.py. Logits are on the 2^-10 grid, the model's log-probabilities and back-offs on the 2^-6 grid
(order 3, <s> and </s>, part of the vocabulary without a unigram), alpha = 0.5 and beta on the grid: x + term is exact in f32 and in float64, ties are real,
so picks, states, histories and node tables are compared exactly; scores within the kernels' budgets."""
import numpy as np
import pytest

import decoder_lm_ref as dl
import hotword_heads_ref as hw
import token_heads_ref as thr
import token_scores_ref as tsr
from conftest import sub

pytestmark = pytest.mark.gpu
LD_SAVE = 32
F32 = np.float32
TERM_MAX = dl.ALPHA * 6.0 + abs(dl.BETA)                   # |term| of the test models: |log P| <= 4 + two back-offs below 1 each


def probe():
    return sub("_probe")


def as_arg(lm):
    return dict(image=lm["image"], alpha=lm["alpha"], beta=lm["beta"], oov=lm["oov"], topk=lm["topk"], end_ids=lm["end_ids"])


def _check_head(got, ref, steps, rows, scores=False, upto=None):
    upto = np.full(rows, steps) if upto is None else upto
    for r in range(rows):
        u = int(upto[r])
        assert np.array_equal(got["picks"][:u, r], ref["picks"][:u, r]), r
        assert np.array_equal(got["states"][:u, r], ref["states"][:u, r]), r
        assert np.array_equal(got["save_ids"][r, :u], ref["save"][r, :u]), r
    assert got["n_saved"] == steps
    if scores:
        sc = got["logprob"][:, :steps].T                       # [steps][rows]
        for r in range(rows):
            u = int(upto[r])
            worst = tsr.over_budget(sc[:u, r], ref["scores"][:u, r], ref["budgets"][:u, r])
            print(f"row {r}: score error / budget {worst:.3f}")
            assert worst <= 1.0, r


@pytest.mark.parametrize("n", hw.WIDTHS)
@pytest.mark.parametrize("rows", hw.ROWS)
def test_greedy_head_follows_the_statement(rows, n):
    x, ph, bias = hw.head_inputs(rows, n)
    lm = dl.head_model(rows, n)
    x, pair, oov = dl.plant_ties(x, lm, bias, ph)
    ref = dl.head_steps_lm(x, ph, hw.BOOST, LD_SAVE, lm, bias=bias)
    got = probe().hotword_head_steps(x, ph, hw.BOOST, LD_SAVE, bias=bias, lm=as_arg(lm))
    _check_head(got, ref, hw.STEPS, rows)
    for r in range(rows):
        assert np.array_equal(got["nodes"][:, r], ref["nodes"][:, r]), r
    if pair is not None:                                                   # the planted ties are real: the lower id wins although the other has the larger logit
        assert (ref["picks"][0] == pair[0]).all() and x[0, 0, pair[1]] > x[0, 0, pair[0]]
    if oov is not None:
        assert (ref["picks"][3] == oov[0]).all()
    assert n < 129 or (pair is not None and oov is not None)
    plain = hw.head_steps_hot(x, ph, hw.BOOST, LD_SAVE, bias=bias)
    assert (ref["picks"][1:] != plain["picks"][1:]).any()                  # the model flips picks against the plain head


def test_greedy_head_at_the_large_vocabulary():
    rows, n, steps = 3, hw.WIDE, 6
    x, ph, bias = hw.head_inputs(rows, n, steps)
    lm = dl.head_model(rows, n, steps)
    ref = dl.head_steps_lm(x, ph, hw.BOOST, LD_SAVE, lm, bias=bias)
    got = probe().hotword_head_steps(x, ph, hw.BOOST, LD_SAVE, bias=bias, scores=True, lm=as_arg(lm))
    _check_head(got, ref, steps, rows, scores=True)


@pytest.mark.parametrize("shape", hw.HEAD_SHAPES)
@pytest.mark.parametrize("setting", [k for k in hw.HEAD_SETTINGS if k != "arg-max"])
def test_head_settings(setting, shape):
    rows, n = shape
    x, ph, bias = hw.head_inputs(rows, n)
    lm = dl.head_model(rows, n)
    kw = dict(hw.HEAD_SETTINGS[setting])
    scores = setting in ("scores", "sampler")
    if "sampler" in kw:                                        # the sampling head ignores the model: picks and score bits of the run without one
        kw["sampler"], kw["noise"] = hw.sampler_setting(n), hw.sampler_noise(rows, n)
        got = probe().hotword_head_steps(x, ph, hw.BOOST, LD_SAVE, bias=bias, scores=True, lm=as_arg(lm), **kw)
        off = probe().hotword_head_steps(x, ph, hw.BOOST, LD_SAVE, bias=bias, scores=True, **kw)
        assert np.array_equal(got["picks"], off["picks"]) and np.array_equal(got["save_ids"], off["save_ids"])
        assert np.array_equal(got["logprob"].view(np.uint32), off["logprob"].view(np.uint32))
        assert (got["states"] == lm["view"]["start_node"]).all()
        return
    ref = dl.head_steps_lm(x, ph, hw.BOOST, LD_SAVE, lm, bias=bias, **kw)
    got = probe().hotword_head_steps(x, ph, hw.BOOST, LD_SAVE, bias=bias, scores=scores, lm=as_arg(lm), **kw)
    _check_head(got, ref, hw.STEPS, rows, scores=scores)


@pytest.mark.parametrize("hot", [True, False])
@pytest.mark.parametrize("geom", hw.TS_GEOMS)
def test_timestamp_rules_before_the_fused_pick(geom, hot):
    import whisper_timestamps_ref as wtr
    x, ph = hw.ts_inputs(geom)
    ph = ph if hot else []
    steps, rows, _ = x.shape
    lm = dl.ts_model(geom)
    params = wtr.params(geom, 20)
    ref = dl.head_steps_lm(x, ph, hw.BOOST, LD_SAVE, lm, timestamps=params)
    upto, skipped = hw.decided_prefix(ref["decided"])
    assert skipped <= thr.SKIP_CAP, skipped
    got = probe().hotword_head_steps(x, ph, hw.BOOST, LD_SAVE, timestamps=params, scores=True, want_logits=True, lm=as_arg(lm))
    _check_head(got, ref, steps, rows, scores=True, upto=upto)
    for r in range(rows):                                       # logits_out shows the biased, masked row bit for bit: the model changes no logit
        u = int(upto[r])
        assert np.array_equal(got["logits"][:u, r, :geom[0]], ref["rows_seen"][:u, r]), r


def test_zero_weights_equal_the_plain_head():
    rows, n = 3, 4097
    x, ph, bias = hw.head_inputs(rows, n)
    lm = dict(as_arg(dl.head_model(rows, n)), alpha=0.0, beta=0.0, oov=0.0)
    got = probe().hotword_head_steps(x, ph, hw.BOOST, LD_SAVE, bias=bias, scores=True, lm=lm)
    plain = hw.head_steps_hot(x, ph, hw.BOOST, LD_SAVE, bias=bias)
    assert np.array_equal(got["picks"], plain["picks"])
    off = probe().hotword_head_steps(x, ph, hw.BOOST, LD_SAVE, bias=bias, scores=True)
    assert np.array_equal(got["save_ids"], off["save_ids"])
    assert np.abs(got["logprob"][:, :hw.STEPS] - off["logprob"][:, :hw.STEPS]).max() < 1e-4


def test_pick_kernel_scores_an_end_id_as_eos_and_keeps_the_state():
    n, rows = 4097, 70
    lm0 = dl.head_model(65, n)
    v = lm0["view"]
    rng = np.random.default_rng(83)
    known = np.nonzero(v["uni"][:n] >= 0)[0]
    unknown = np.nonzero(v["uni"][:n] < 0)[0]
    ends = tuple(int(c) for c in rng.choice(known, 3, replace=False)) + (int(unknown[0]),)
    lm = dl.model(lm0["image"], dl.ALPHA, dl.BETA, oov=-2.0, topk=9, end_ids=ends)
    pool = np.setdiff1d(np.arange(n), ends)                    # (the ids of a row are distinct, as launch_lm_topk leaves them)
    ci = np.stack([rng.choice(pool, 9, replace=False) for _ in range(rows)]).astype(np.int32)
    ci[:, 0] = [ends[r % 4] for r in range(rows)]
    cv = -np.sort(-(np.round(rng.normal(0.0, 1.0, (rows, 9)) / thr.GRID) * thr.GRID), axis=1).astype(F32)
    cv[:, 0] = cv[:, 1] + F32(3.0)                              # the end id leads by enough to win most rows whatever its term
    cv[5, 4:] = -np.inf                                        # fewer candidates (their ids are placeholders)
    cv[6, :] = -np.inf                                         # none: id 0, the state stays, the score is -inf
    lse = (np.round(rng.normal(8.0, 0.5, rows) / thr.GRID) * thr.GRID).astype(F32)
    state = rng.integers(0, v["n_nodes"], rows).astype(np.int32)
    for n_saved in (0, 2):
        got = probe().lm_pick(as_arg(lm), cv, ci, lse, state, n_saved=n_saved, ld_save=4)
        won = 0
        for r in range(rows):
            s0 = v["start_node"] if n_saved == 0 else int(state[r])
            keyed = []
            for x, c in zip(cv[r], ci[r]):
                if x > -np.inf:
                    t, nxt = dl.lm_term(lm, s0, int(c))
                    keyed.append((float(x) + t, int(c), nxt, float(x)))
            keyed.sort(key=lambda q: (-q[0], q[1]))
            if not keyed:
                assert got["next"][r] == 0 and got["state"][r] == s0 and got["logprob"][r, n_saved] == -np.inf
                continue
            assert got["next"][r] == keyed[0][1] and got["state"][r] == keyed[0][2], r
            assert got["logprob"][r, n_saved] == F32(F32(keyed[0][3]) - lse[r]), r
            if keyed[0][1] in ends:
                won += 1
                assert got["state"][r] == s0
                want = dl.ALPHA * float(dl.clr.lm_step(v, s0, v["eos"], -2.0)[0])
                assert keyed[0][0] == keyed[0][3] + want                 # no beta, whether or not the id has a unigram
        assert won >= rows // 2
        assert np.isnan(np.delete(got["logprob"], n_saved, axis=1)).all()


@pytest.mark.parametrize("hot", [True, False])
@pytest.mark.parametrize("n", [129, 4097])
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("beam", [1, 3, 8])
def test_ranking_pass(beam, first, n, hot):
    c = hw.rank_inputs(beam, n, first)
    lm, state = dl.rank_model(beam, n, first, hot)
    ref = dl.rank_reference_lm(c, beam, first, lm, state, hot)
    undecided = ref["cross"] <= 0                               # on these grids a gap is a tie or at least 2^-10: a tie across different delta + term is not bit-defined
    assert undecided.mean() <= thr.SKIP_CAP, ref["cross"]
    got = probe().hotword_rank(c["x"], c["phrases"] if hot else [], hw.BOOST, beam, c["n_slots"], c["cum"], c["fin"], c["len"], c["next"], c["done"], c["src"], c["tok"],
                               c["node"], stop=c["stop"], first=first, bias=c["bias"], lm=as_arg(lm), state_in=state)
    R = len(c["x"])
    depth = ref["trie"]["depth"] if hot else None
    for r in range(R):
        if undecided[r]:
            continue
        assert np.array_equal(got["topi"][r], ref["topi"][r]), r
        nd = 0 if first or not hot else int(c["node"][r])
        fin = np.isfinite(ref["topv"][r])
        assert np.array_equal(np.isfinite(got["topv"][r]), fin), r
        x = c["x"][r] if c["bias"] is None else (c["x"][r] + c["bias"]).astype(F32)
        size = np.abs(ref["topv"][r][fin]) + TERM_MAX           # bounds |x - lse| and |x - lse + delta| from the fused value
        bud = hw.rerank_budget(n, x, ref["lse"][r], size, hw.BOOST if hot else 0.0, int(depth[nd]) if hot else 0) + thr.U32 * size
        err = np.abs(got["topv"][r][fin] - ref["topv"][r][fin])
        print(f"row {r}: topv error / budget {float((err / bud).max()) if fin.any() else 0.0:.3f}")
        assert (err <= bud).all(), r
    assert not undecided.any()                                  # (SKIP_CAP of at most 24 rows is none: the seeds were chosen so)
    sel = ref["sel"]
    for k in ("fin", "len", "next", "done"):
        assert np.array_equal(got[k], sel[k]), k
    assert np.array_equal(got["state_out"], sel["state"])
    if hot:
        assert np.array_equal(got["node_out"], sel["node"])
    else:
        assert (got["node_out"] == -1).all()                    # no trie: the node tables are not touched
    assert np.abs(got["cum"] - sel["cum"]).max() < 1e-4
    N = c["done"].size * beam
    for row in range(N):
        base = row // beam * beam
        if c["n_slots"] > 0:
            assert got["src_out"][row, c["n_slots"] - 1] == base + sel["parent"][row], row
        if sel["tok"][row] >= 0:
            assert got["tok_out"][row, sel["len"][row] - 1] == sel["tok"][row], row
    if beam == 8 and not hot:                                   # the model reorders: the plain ranking of the same rows differs
        _, plain, _, _ = thr.beam_topk(c["x"], beam, c["bias"])
        assert (plain != ref["topi"]).any()


def test_topk_below_the_beam_is_refused():
    c = hw.rank_inputs(3, 129, False)
    lm, state = dl.rank_model(3, 129, False, True)
    with pytest.raises(sub("_lib").AsrError, match="topk 2 is below the beam width 3"):
        probe().hotword_rank(c["x"], c["phrases"], hw.BOOST, 3, c["n_slots"], c["cum"], c["fin"], c["len"], c["next"], c["done"], c["src"], c["tok"], c["node"],
                             stop=c["stop"], lm=dict(as_arg(lm), topk=2), state_in=state)
