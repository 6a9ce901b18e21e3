"""Hotword boosting of the autoregressive decoders at kernel level (csrc/hotword.hip, TokenHead / BeamRanker of csrc/decode_head.h) through the probe
library, against the float64 statement tests/hotword_heads_ref.py. Inputs are grid logits (multiples of 2^-10) and a boost on the grid: every biased
value is exact, ties are real, so picks, histories and node tables are compared exactly; scores within the kernels' budgets."""
import numpy as np
import pytest

import hotword_heads_ref as hw
import token_heads_ref as thr
import token_scores_ref as tsr
from conftest import sub
from ctc_beam_ref import build_trie

pytestmark = pytest.mark.gpu
LD_SAVE = 32


def probe():
    return sub("_probe")


def _check_head(got, ref, steps, rows, scores=False, upto=None):
    upto = np.full(rows, steps) if upto is None else upto
    for r in range(rows):
        u = int(upto[r])
        assert np.array_equal(got["picks"][:u, r], ref["picks"][:u, r]), r
        assert np.array_equal(got["nodes"][:u, r], ref["nodes"][:u, r]), r
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
def test_argmax_head_follows_the_statement(rows, n):
    x, ph, bias = hw.head_inputs(rows, n)
    ref = hw.head_steps_hot(x, ph, hw.BOOST, LD_SAVE, bias=bias)
    got = probe().hotword_head_steps(x, ph, hw.BOOST, LD_SAVE, bias=bias)
    _check_head(got, ref, hw.STEPS, rows)
    plain = hw.head_steps_hot(x, [], hw.BOOST, LD_SAVE, bias=bias)
    assert (ref["picks"] != plain["picks"]).any()              # the boosts flip picks


def test_argmax_head_at_the_large_vocabulary():
    rows, n, steps = 3, hw.WIDE, 6
    x, ph, bias = hw.head_inputs(rows, n, steps)
    ref = hw.head_steps_hot(x, ph, hw.BOOST, LD_SAVE, bias=bias)
    got = probe().hotword_head_steps(x, ph, hw.BOOST, LD_SAVE, bias=bias, scores=True)
    _check_head(got, ref, steps, rows, scores=True)


@pytest.mark.parametrize("shape", hw.HEAD_SHAPES)
@pytest.mark.parametrize("setting", [k for k in hw.HEAD_SETTINGS if k != "arg-max"])
def test_head_settings(setting, shape):
    rows, n = shape
    x, ph, bias = hw.head_inputs(rows, n)
    kw = dict(hw.HEAD_SETTINGS[setting])
    upto = None
    if "sampler" in kw:
        kw["sampler"], kw["noise"] = hw.sampler_setting(n), hw.sampler_noise(rows, n)
    ref = hw.head_steps_hot(x, ph, hw.BOOST, LD_SAVE, bias=bias, **kw)
    if "sampler" in kw:
        upto, skipped = hw.decided_prefix(ref["decided"])
        assert skipped <= thr.SKIP_CAP, skipped
    got = probe().hotword_head_steps(x, ph, hw.BOOST, LD_SAVE, bias=bias, scores=setting in ("scores", "sampler"), **kw)
    _check_head(got, ref, hw.STEPS, rows, scores=setting in ("scores", "sampler"), upto=upto)


@pytest.mark.parametrize("geom", hw.TS_GEOMS)
def test_timestamp_rules_after_the_bias(geom):
    import whisper_timestamps_ref as wtr
    x, ph = hw.ts_inputs(geom)
    steps, rows, _ = x.shape
    params = wtr.params(geom, 20)
    ref = hw.head_steps_hot(x, ph, hw.BOOST, LD_SAVE, timestamps=params)
    upto, skipped = hw.decided_prefix(ref["decided"])
    assert skipped <= thr.SKIP_CAP, skipped
    got = probe().hotword_head_steps(x, ph, hw.BOOST, LD_SAVE, timestamps=params, scores=True, want_logits=True)
    _check_head(got, ref, steps, rows, scores=True, upto=upto)
    for r in range(rows):                                       # logits_out shows the biased, masked row bit for bit
        u = int(upto[r])
        assert np.array_equal(got["logits"][:u, r, :geom[0]], ref["rows_seen"][:u, r]), r


@pytest.mark.parametrize("phrases,boost", [([], hw.BOOST), ("planted", 0.0)])
def test_off_and_zero_boost_equal_the_plain_head(phrases, boost):
    rows, n = 3, 4097
    x, ph, bias = hw.head_inputs(rows, n)
    ph = ph if phrases == "planted" else []
    got = probe().hotword_head_steps(x, ph, boost, LD_SAVE, bias=bias, scores=True)
    plain = hw.head_steps_hot(x, [], 0.0, LD_SAVE, bias=bias)
    assert np.array_equal(got["picks"], plain["picks"])
    for t in range(hw.STEPS):                                   # ... and op 6's plain head on each step's rows gives the same picks and score bits
        one = probe().head_steps(x[t], 1, LD_SAVE, 4, 1.0, 0, bias=bias if t == 0 else None, scores=True)
        assert np.array_equal(one["picks"][0], got["picks"][t]), t
        assert np.array_equal(one["logprob"][:, 0].view(np.uint32), got["logprob"][:, t].view(np.uint32)), t
    if not ph:
        assert (got["nodes"] == -1).all()                       # the mode off: no node table exists


def test_bias_kernel_writes_shared_columns_once_and_saves_the_root():
    n, rows = 4097, 5
    x = thr.grid_logits([n, 3], rows, n)
    a, b, c = 7, 300, 4096
    ph = [[a, b], [b, 5], [a, c], [c]] + hw.wide_children(n)
    trie = build_trie(ph)
    n_root = int(trie["child_off"][1])
    nodes = np.array([0, 1, 2, n_root + 1, n_root + 2], np.int32)          # the root, the hub (80 children), another root child, two depth-2 nodes
    assert nodes.max() < len(trie["depth"]) and trie["child_off"][2] - trie["child_off"][1] > 64 and n_root > 64
    x[2, b] = -np.inf
    for n_saved in (0, 3):
        got = probe().hotword_op("bias", ph, hw.BOOST, nodes, logits=x, n_saved=n_saved, n_root=n_root)
        want = np.stack([hw.bias_sparse(x[r], trie, 0 if n_saved == 0 else int(nodes[r]), hw.BOOST) for r in range(rows)])
        assert np.array_equal(got["logits"][:, :n].view(np.uint32), want.view(np.uint32)), n_saved
        assert (got["logits"][:, n:] == probe().PAD_LOGIT).all()
        roots = trie["child_tok"][:n_root]
        if n_saved == 0:
            assert np.array_equal(got["root_save"], x[:, roots])
        else:
            assert np.isnan(got["root_save"]).all()


def test_advance_kernel_is_trie_step():
    n = 4097
    ph = [[7, 300], [300, 5], [7, 4096], [4096], [9, 9, 9]] + hw.wide_children(n)
    trie = build_trie(ph)
    n_nodes = len(trie["depth"])
    rng = np.random.default_rng(5)
    toks = np.concatenate([trie["child_tok"], rng.integers(0, n, 200).astype(np.int32), [-1, n + 5]])
    nodes = rng.integers(0, n_nodes, toks.size).astype(np.int32)
    from ctc_beam_ref import trie_step
    for n_saved in (0, 2):
        got = probe().hotword_op("advance", ph, hw.BOOST, nodes, next_ids=toks, n_saved=n_saved)
        want = [trie_step(trie, 0 if n_saved == 0 else int(q), 0.0, int(c), 1.0)[0] for q, c in zip(nodes, toks)]
        assert got["node"].tolist() == want, n_saved


@pytest.mark.parametrize("n", [129, 4097])
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("beam", [1, 3, 8])
def test_ranking_pass(beam, first, n):
    c = hw.rank_inputs(beam, n, first)
    ref = hw.rank_reference(c, beam, first)
    assert ref["dense_ok"] and ref["cross"] > 0
    got = probe().hotword_rank(c["x"], c["phrases"], hw.BOOST, beam, c["n_slots"], c["cum"], c["fin"], c["len"], c["next"], c["done"], c["src"], c["tok"], c["node"],
                               stop=c["stop"], first=first, bias=c["bias"])
    assert np.array_equal(got["topi"], ref["topi"])
    depth = ref["trie"]["depth"]
    for r in range(len(c["x"])):
        nd = 0 if first else int(c["node"][r])
        fin = np.isfinite(ref["topv"][r])
        assert np.array_equal(np.isfinite(got["topv"][r]), fin), r
        x = c["x"][r] if c["bias"] is None else (c["x"][r] + c["bias"]).astype(np.float32)
        bud = hw.rerank_budget(n, x, ref["lse"][r], ref["topv"][r][fin], hw.BOOST, int(depth[nd]))
        err = np.abs(got["topv"][r][fin] - ref["topv"][r][fin])
        print(f"row {r}: topv error / budget {float((err / bud).max()) if fin.any() else 0.0:.3f}")
        assert (err <= bud).all(), r
    sel = ref["sel"]
    for k in ("fin", "len", "next", "done"):
        assert np.array_equal(got[k], sel[k]), k
    assert np.array_equal(got["node_out"], sel["node"])
    assert np.abs(got["cum"] - sel["cum"]).max() < 1e-4
    N = c["done"].size * beam
    for row in range(N):
        base = row // beam * beam
        if c["n_slots"] > 0:
            assert got["src_out"][row, c["n_slots"] - 1] == base + sel["parent"][row], row
        if sel["tok"][row] >= 0:
            assert got["tok_out"][row, sel["len"][row] - 1] == sel["tok"][row], row
