"""The streaming-Paraformer references (tests/paraformer_stream_ref.py) checked on the CPU: they are the oracle's chunk step, the two cases exercise what they
were built for, and every planted mistake moves the output beyond the bound of the GPU test.

The GPU test (test_paraformer_stream_ref_gpu.py) lets a kernel differ from encoder_exact / decoder_exact by MARGIN x E_round per (stream, step) and statistic.
That bound only means something if the mistakes it is meant to catch move the output further: here every mutation is put on the REFERENCE side of that very
comparison, with the rounded twin of the noisiest path (fused_both: every rounding point) standing in for a kernel that is nothing but rounding noise away from
the exact reference, and the comparison must fail -- both statistics beyond MARGIN x E_round -- on every (stream, step) the mutation applies to (where it acts
directly, or where the state it left behind differs from the exact one). This is a condition on the inputs (sharpened and planted weights, the schedule),
computed from the references alone.

Smallest ratio stat(rounded - mutated) / E_round over the (stream, step) a mutation applies to (the smaller of the two statistics; the bound is MARGIN = 3):

    encoder  hist_shift 4.2   mask_oldest 4.9   roll_paused 29.9   no_roll 10.3   stale_reset 17.3   fsmn_tap_lo 10.6   fsmn_tap_hi 9.8   pad_keys 17.6
    decoder  carry_on_empty 25.2 (sparse)   carry_n_minus_1 22.2 (sparse) 12.8 (dense)   cache_window 9.8 (sparse) 14.8 (dense)   cache_on_empty 4.3 (sparse)
             pad_keys 18.6 (sparse) 30.3 (dense)          (the dense case has no chunk without a fire, so the two `_on_empty` mistakes apply in the sparse one only)
"""
import numpy as np
import pytest

import paraformer_stream_ref as R
from oracle.paraformer_streaming_oracle import ParaformerStreamingOracle
from test_oracle_paraformer_streaming import F32_TOL

NOISIEST = R.PATH_ROUNDINGS["fused_both"]


@pytest.fixture(scope="module")
def runs():
    """Per case: (cfg, ck, the schedule's record made by the references alone, encoder_runs, decoder_runs) with the rounding points of the noisiest path."""
    out = {}
    for name in ("sparse", "dense"):
        cfg, ck, _ = R.case(name)
        rec = R.reference_record(cfg, ck)
        out[name] = (cfg, ck, rec, R.encoder_runs(cfg, ck, rec, NOISIEST), R.decoder_runs(cfg, ck, rec, NOISIEST))
    return out


@pytest.mark.parametrize("name", ["sparse", "dense"])
def test_references_are_the_oracle_chunk_by_chunk(name):
    """front_end -> encoder_exact -> cif_fire -> decoder_exact, chunk by chunk with the references' own state, against ParaformerStreamingOracle.run (which is
    pinned to the reference goldens): enc_out and logits of every chunk within F32_TOL, equal fire counts."""
    cfg, ck, chunk = R.case(name)
    orc = ParaformerStreamingOracle(cfg, ck, chunk=chunk)
    for clip in R.clips(chunk)[:4]:
        want = orc.run(clip)
        assert len(want) == R.N_STEPS
        st = R.init_state(cfg, ck)
        ref = R.ref_of(cfg, ck)
        for k, w in enumerate(want):
            enc = R.encoder_exact(cfg, ck, st, R.front_end(cfg, ck, st, clip[k * chunk:(k + 1) * chunk]))
            assert np.abs(enc - w["enc_out"]).max() < F32_TOL, (name, k)
            frames = ref.cif_fire(st, w["enc_out"])              # (the oracle's own f32 rows: a fire decision is a comparison, not a number to compare)
            assert frames.shape[0] == w["n"], (name, k)
            if w["n"]:
                assert np.abs(frames - w["list_frame"]).max() < F32_TOL
                logits = R.decoder_exact(cfg, ck, st, w["enc_out"], w["list_frame"])
                assert np.abs(logits - w["logits"]).max() < F32_TOL, (name, k)


def test_the_schedule_is_what_the_issue_describes():
    chunk = R.default_chunk()
    steps = R.schedule_chunks(chunk)
    assert len(steps) == R.N_STEPS == 8 and len(R.STREAM_IDS) == 9 and max(R.STREAM_IDS) < R.MAX_STREAMS == 12
    assert list(R.STREAM_IDS) != sorted(R.STREAM_IDS) and sorted(R.STREAM_IDS) != list(range(9))       # not in slot order, not dense
    sizes = [len(sids) for _, sids, _ in steps]
    assert sizes == [9, 9, 9, 5, 9, 5, 9, 9]
    assert set(steps[3][1]) != set(steps[5][1]) and R.RESET_STREAM in steps[5][1] and steps[5][0] == (R.RESET_STREAM,)
    assert all(a.shape == (len(sids), chunk) for _, sids, a in steps)


def test_history_lengths_and_fire_counts_cover_the_edges(runs):
    cfg, ck, rec, enc, _ = runs["sparse"]
    lens = [{s: enc[(k, s)]["len"] for s in sids} for k, (_, sids) in enumerate(R.SCHEDULE)]
    assert [set(l.values()) for l in lens[:4]] == [{0}, {9}, {18}, {27}]                               # empty, then partial
    assert set(lens[4].values()) == {27, 36}                                                             # mixed within one launch from here on
    assert lens[5][R.RESET_STREAM] == 0 and 36 in lens[5].values()                                       # a reset stream beside full histories
    assert set(lens[6].values()) == {9, 36} and set(lens[7].values()) == {18, 36}                        # rolling
    assert all(len(set(lens[k].values())) > 1 for k in R.MIXED_STEPS)
    counts = {name: {int(r["frames"].shape[0]) for step in runs[name][2] for r in step.values()} for name in runs}
    both = counts["sparse"] | counts["dense"]
    assert 0 in both and 1 in both and any(2 <= n <= 8 for n in both) and any(n >= 9 for n in both), counts
    assert 0 in counts["sparse"] and max(counts["dense"]) >= 9, counts


def test_attention_is_sharp_and_every_key_class_is_somebodys_top_key(runs):
    """Mean top probability per head between 0.5 and 0.9 (encoder layers >= 1, decoder) in the exact reference over the schedule; the oldest row of a full
    history, the newest history row, a carried row and a new row are each the top key of some query -- the planted heads of layer 1 make row 0 of EVERY chunk
    look at the oldest row of a full history (heads 0, 2; the all-zero rows in front of a stream's first chunk share it while they are the oldest) and at the
    newest history row (head 1)."""
    for name in ("sparse", "dense"):
        cfg, ck, rec, _, _ = runs[name]
        for fn in (R.encoder_runs, R.decoder_runs):
            trace = []
            fn(cfg, ck, rec, NOISIEST, trace=trace)
            tops, classes = {}, set()
            for li, n_hist, p in trace:
                if fn is R.encoder_runs and li == 0:
                    continue                                                                             # layer 0 keeps the synthetic near-uniform weights
                tops.setdefault(li, []).append(p.max(axis=-1).mean(axis=-1))
                top = p.argmax(axis=-1)
                if n_hist > 0:
                    classes |= {"newest"} if (top == n_hist - 1).any() else set()
                    classes |= {"oldest"} if (top == 0).any() and n_hist in (9, 36) else set()           # (9: the decoder's cache, 36: the encoder's full history)
                classes |= {"carried"} if ((top >= n_hist) & (top < n_hist + 4)).any() else set()
                classes |= {"new"} if (top >= n_hist + 4).any() else set()
                if fn is R.encoder_runs and li == 1 and n_hist > 0:
                    assert top[1, 0] == n_hist - 1, (name, n_hist)
                    if n_hist == 36:
                        assert p[0, 0, 0] > 0.15 and p[2, 0, 0] > 0.15, (name, p[0, 0, 0], p[2, 0, 0])
            per_head = np.mean([np.mean(v, axis=0) for v in tops.values()], axis=0)
            print(name, fn.__name__, "mean top probability per head", per_head.round(3), "per layer", {li: np.mean(v, axis=0).round(2) for li, v in tops.items()})
            assert ((per_head >= 0.5) & (per_head <= 0.9)).all(), (name, fn.__name__, per_head)
            assert classes == {"oldest", "newest", "carried", "new"}, (name, fn.__name__, classes)


def test_the_rounding_points_do_something_and_nothing_else(runs):
    cfg, ck, rec, enc, dec = runs["sparse"]
    ref = R.ref_of(cfg, ck)
    st_a, st_b = ref.init_state(), ref.init_state()
    x = rec[0][R.STREAM_IDS[0]]["enc_in"]
    assert np.array_equal(R.encoder_rounded(cfg, ck, st_a, x, ()), R.encoder_exact(cfg, ck, st_b, x))
    for runs_ in (enc, dec):
        e = np.array([v["e_round"] for v in runs_.values()])
        print("E_round rms %.4f .. %.4f  max %.4f .. %.4f" % (e[:, 0].min(), e[:, 0].max(), e[:, 1].min(), e[:, 1].max()))
        assert e[:, 0].min() > 1e-3 and e[:, 1].max() < 0.3                                            # bf16 noise of 4 + 3 layers: neither vacuous nor unattainable


def _smallest_ratio(base, mutated):
    """Over the (stream, step) the mutation applies to: min of stat(rounded - mutated) / E_round (both statistics); elsewhere the mutation must change nothing."""
    ratios = []
    for key, (m, applies) in mutated.items():
        e = base[key]
        if not applies:
            assert np.array_equal(m, e["exact"]), key
            continue
        s = R.stat(e["rounded"] - m)
        ratios.append((min(s[0] / e["e_round"][0], s[1] / e["e_round"][1]), key))
    return min(ratios) if ratios else None, len(ratios)


@pytest.mark.parametrize("mut", R.ENC_MUTATIONS)
def test_every_planted_encoder_mistake_fails_the_comparison(runs, mut):
    cfg, ck, rec, enc, _ = runs["sparse"]                          # (the encoder does not see the CIF bias: one case)
    worst, n = _smallest_ratio(enc, R.encoder_mutated(cfg, ck, rec, enc, mut))
    print(mut, "applies to", n, "(stream, step); smallest ratio", worst)
    assert n >= {"stale_reset": 3, "mask_oldest": 20, "roll_paused": 8, "no_roll": 15}.get(mut, 50), (mut, n)
    assert worst[0] > R.MARGIN, (mut, worst)


@pytest.mark.parametrize("mut", R.DEC_MUTATIONS)
def test_every_planted_decoder_mistake_fails_the_comparison(runs, mut):
    seen = 0
    for name in ("sparse", "dense"):
        cfg, ck, rec, _, dec = runs[name]
        worst, n = _smallest_ratio(dec, R.decoder_mutated(cfg, ck, rec, dec, mut))
        print(name, mut, "applies to", n, "(stream, step); smallest ratio", worst)
        seen += n
        if n:
            assert worst[0] > R.MARGIN, (name, mut, worst)
    assert seen >= 10, (mut, seen)
