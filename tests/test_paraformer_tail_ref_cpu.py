"""The offline-Paraformer-tail references (tests/paraformer_tail_ref.py) checked on the CPU: they are the oracle's `cif` / `decode`, the cases exercise what they
were built for, and every planted mistake moves the output beyond the bound of the GPU test.

The GPU test (test_paraformer_tail_ref_gpu.py) lets a kernel differ from the exact functions by MARGIN x E_round per utterance, stage and statistic. That bound
only means something if the mistakes it is meant to catch move the output further: here every mutation is put on the REFERENCE side of that very comparison, with
the rounded twin standing in for a kernel that is nothing but rounding noise away from the exact reference, and the comparison must fail -- both statistics beyond
MARGIN x E_round -- on every utterance and stage the mutation applies to (R.mutated says where that is). `no_tail` acts on the fire count, which the GPU test
demands exactly: it must change the count of some utterance of either case. This is a condition on the inputs (planted weights, lengths), computed from the
references alone.

Smallest ratio stat(rounded - mutated) / E_round over the utterances, stages and batches a mutation applies to (the smaller of the two statistics; the bound is
MARGIN = 3), sparse / dense:

    predictor  conv_across 4900 / 33      taps_reversed 4900 / 27            (the canary row of the planted conv wakes; sparse alphas of ~ 0.003 jump to 1)
    cif        prev_hidden 8.6e5 / 9.1e4  no_tail: the count of 5 / 14 utterances drops by one
    layer      fsmn_past_count 27 / 16    fsmn_no_residual 66 / 30    ffnorm_over_d 22 / 12    dec3_residual 409 / 536
               miss_last_key 14 / 12      pad_keys 29 / 20            next_layer_kv 56 / 35    q_from_enc_plan 5.8 / 17

How the inputs got there (each step after a mutation had NOT failed): rows of the synthetic encoder are nearly parallel from clip to clip on noise alone, so a
query row taken from the neighbouring utterance changed nothing -- every noise clip now lies under a tone of its own; a pad key made of a row of zeros drowned
among sharpened real keys -- head 1 takes PAD_LEAD off every key made of a real row; ff.norm over d instead of d_dec_ffn columns vanished behind the following
LayerNorm -- the two halves of the hidden columns differ in width; a conv tap across an utterance's end moved one alpha by less than the rounding of a half
silent clip's transition rows -- conv row 4 is the canary; with the first and the last key planted in one head each, both heads saturated and nothing else
showed -- head 0 holds both, head 1 none; the indicator's height depended on whether the end row was noise or silence -- PLANT_END sets the row's scale itself.
"""
import numpy as np
import pytest
import torch

import paraformer_tail_ref as R
from helpers import golden_cases, kaldi_audio, load_golden
from oracle.paraformer_oracle import ParaformerOracle
from test_oracle_paraformer import F32_TOL, paraformer_setup

CASES, BATCHES = ("sparse", "dense"), tuple(R.BATCH_T)


@pytest.fixture(scope="module")
def runs():
    """Per (case, batch): (cfg, ck, the record made by the references alone on the oracle's enc_out rows, stage_runs with the bf16 rounding points)."""
    out = {}
    for name in CASES:
        cfg, ck = R.case(name)
        for b in BATCHES:
            rec = R.reference_record(cfg, ck, R.oracle_enc_out(name, b))
            out[(name, b)] = (cfg, ck, rec, R.stage_runs(cfg, ck, rec, R.BF16_ROUNDINGS))
    return out


def test_references_are_the_oracle_on_the_golden_cases():
    """predictor_exact -> cif_exact -> layer_exact -> head_exact, each on the ORACLE's f32 rows of the stage before, against ParaformerOracle.stages (pinned to the
    reference goldens) within F32_TOL; equal fire counts (the rule on the oracle's own alphas is the oracle's rule)."""
    g = load_golden("paraformer_tiny")
    cfg, ck = paraformer_setup(str(g["cfg_name"]), int(g["ckpt_seed"]))
    orc = ParaformerOracle(cfg, ck)
    for i, c in golden_cases(g):
        st = orc.stages(kaldi_audio(c["audio_seed"], c["n_samples"]))
        enc, n = st["enc_out"], int(st["num_id"][0])
        assert np.abs(R.predictor_exact(cfg, ck, enc) - st["alphas"]).max() < F32_TOL, i
        got_n, acoustic, fire = R.cif_exact(cfg, ck, st["alphas"], enc)
        assert got_n == n and fire.size == n, i
        assert R.cif_rounded(cfg, ck, st["alphas"], enc)[0] == n
        if n:
            assert np.abs(acoustic - st["acoustic"]).max() < F32_TOL, i
            assert np.abs(R.cif_rounded(cfg, ck, st["alphas"], enc)[1] - st["acoustic"]).max() < F32_TOL, i       # the twin is the oracle's f32 form, its running sum f32 as well
        rows = np.concatenate([st["acoustic"], np.zeros((1, cfg.d_model), np.float32)], 0)[:max(n, 1)]
        with torch.inference_mode():
            want = orc.decode(torch.as_tensor(st["acoustic"]), torch.as_tensor(enc), n).numpy()
        for li in range(cfg.n_dec + cfg.n_dec3):
            rows = R.layer_exact(cfg, ck, li, rows, enc)
        assert np.abs(R.head_exact(cfg, ck, rows) - want).max() < F32_TOL, i


def test_lengths_and_fire_counts_cover_the_edges(runs):
    for b in BATCHES:
        lens = R.batch_lengths(b)
        assert len(lens) <= 12 and {1, 2, 16, 17} <= set(lens), (b, lens)
        for name in CASES:
            assert tuple(u["enc_out"].shape[0] for u in runs[(name, b)][2]) == lens              # samples_of gives the encoder lengths it promises
    assert max(R.batch_lengths("le128")) == 128
    le256, gt256 = R.batch_lengths("le256"), R.batch_lengths("gt256")
    assert max(le256) == 256 and 129 in le256
    assert 256 < max(gt256) <= 280 and 257 in gt256                                              # 257: the last 128-key chunk holds one live key
    counts = {key: [u["n"] for u in v[2]] for key, v in runs.items()}
    print(counts)
    for b in BATCHES:
        assert set(counts[("sparse", b)]) <= {0, 1} and 0 in counts[("sparse", b)], counts[("sparse", b)]
        dense = counts[("dense", b)]
        assert {15, 16, 17} <= set(dense), dense                                                 # straddle the 16-row packing
        assert all(n <= T for n, T in zip(dense, R.batch_lengths(b)))
        assert sum(n >= 0.9 * T for n, T in zip(dense, R.batch_lengths(b))) >= 6, dense            # counts approach T
    assert any(1 in counts[("sparse", b)] for b in BATCHES)
    dense = counts[("dense", "gt256")]
    assert max(dense) > 256                                                                      # the second query block of an utterance has live token rows
    assert any(1 <= n <= T // 4 and T >= 100 for n, T in zip(dense, gt256)), dense                # far fewer tokens than keys
    # the tail threshold decides some count in either case (no_tail applies there)
    for name in CASES:
        assert any(R.mutated(*runs[(name, b)][:3], "count", "no_tail")[i][1] for b in BATCHES for i in range(len(R.batch_lengths(b)))), name


def test_cross_attention_looks_at_the_first_and_the_last_key(runs):
    """In every utterance some head gives the FIRST key a weight above 0.4 for some token, and likewise the LAST key, in the exact reference; in the long utterances
    the planted heads do not take everything (the rest of the soft-max is where a pad key or a neighbour's key would show)."""
    for (name, b), (cfg, ck, rec, _) in runs.items():
        trace = []
        R.stage_runs(cfg, ck, rec, R.BF16_ROUNDINGS, trace=trace)
        assert len(trace) == cfg.n_dec * len(rec)
        for i, u in enumerate(rec):
            ps = [p for _, p in trace[i * cfg.n_dec:(i + 1) * cfg.n_dec]]
            T = u["enc_out"].shape[0]
            assert all(p.shape == (cfg.n_heads, max(u["n"], 1), T) for p in ps)
            first, last = max(float(p[:, :, 0].max()) for p in ps), max(float(p[:, :, T - 1].max()) for p in ps)
            assert first > 0.4 and last > 0.4, (name, b, i, T, first, last)
            if T >= 97 and u["n"] >= 16:
                rest = max(float(1.0 - p[0, :, 0].min()) for p in ps), max(float(1.0 - p[1, :, T - 1].min()) for p in ps)
                assert min(rest) > 0.2, (name, b, i, rest)


def test_the_rounding_points_do_something_and_nothing_else(runs):
    cfg, ck, rec, res = runs[("dense", "le128")]
    u = rec[0]
    assert np.array_equal(R.predictor_rounded(cfg, ck, u["enc_out"], ()), R.predictor_exact(cfg, ck, u["enc_out"]))
    assert np.array_equal(R.layer_rounded(cfg, ck, 0, u["acoustic"], u["enc_out"], ()), R.layer_exact(cfg, ck, 0, u["acoustic"], u["enc_out"]))
    assert np.array_equal(R.head_rounded(cfg, ck, u["dec"][-1], ()), R.head_exact(cfg, ck, u["dec"][-1]))
    for s in R.stages(cfg):
        e = np.array([r[s]["e_round"] for (name, _), v in runs.items() for r, uu in zip(v[3], v[2]) if name == "dense" and (s != "acoustic" or uu["n"])])
        print(s, "E_round rms %.3g .. %.3g  max %.3g .. %.3g" % (e[:, 0].min(), e[:, 0].max(), e[:, 1].min(), e[:, 1].max()))
        if s == "acoustic":
            assert 0 < e[:, 1].max() < 1e-3                       # f32 prefix sums of up to 276 terms (the end rows hold a 16) against float64 ones
        elif s == "alphas":
            assert e[:, 1].min() > 1e-6 and e[:, 1].max() < 0.02
        else:
            assert e[:, 0].min() > 1e-3 and e[:, 1].max() < 0.2                                  # bf16 noise of one layer: neither vacuous nor unattainable


def _stage_names(cfg, kind):
    if kind == "full":
        return [f"dec{i}" for i in range(cfg.n_dec)]
    if kind == "dec3":
        return [f"dec{i}" for i in range(cfg.n_dec, cfg.n_dec + cfg.n_dec3)]
    return [kind]


def _smallest_ratio(cfg, ck, rec, res, stage, mut):
    """Over the utterances the mutation applies to: min of stat(rounded - mutated) / E_round (both statistics); elsewhere the mutation must change nothing."""
    ratios = []
    for i, (m, applies) in enumerate(R.mutated(cfg, ck, rec, stage, mut)):
        e = res[i][stage]
        if not applies:
            assert np.array_equal(m, e["exact"]), (stage, mut, i)
            continue
        s = R.stat(e["rounded"] - m)
        ratios.append((min(R.ratio(s[0], e["e_round"][0]), R.ratio(s[1], e["e_round"][1])), i))
    return ratios


@pytest.mark.parametrize("mut", [m for m in R.MUTATIONS if m != "no_tail"])
def test_every_planted_mistake_fails_the_comparison(runs, mut):
    kinds = [k for k, muts in R.STAGE_MUTATIONS.items() if mut in muts]
    per_case = {}
    for (name, b), (cfg, ck, rec, res) in runs.items():
        for kind in kinds:
            for stage in _stage_names(cfg, kind):
                for ratio, i in _smallest_ratio(cfg, ck, rec, res, stage, mut):
                    per_case.setdefault(name, []).append((ratio, b, stage, i))
    for name in CASES:
        print(mut, name, "applies to", len(per_case.get(name, [])), "(batch, stage, utterance); smallest ratio", min(per_case[name]) if name in per_case else None)
    for name, v in per_case.items():
        assert min(v)[0] > R.MARGIN, (mut, name, sorted(v)[:4])
    assert sum(len(v) for v in per_case.values()) >= 10, mut
    assert "dense" in per_case


def test_no_tail_changes_a_fire_count(runs):
    for name in CASES:
        changed = [(b, i, u["n"], n) for b in BATCHES for i, (u, (n, applies)) in
                   enumerate(zip(runs[(name, b)][2], R.mutated(*runs[(name, b)][:3], "count", "no_tail"))) if applies]
        print(name, "no_tail changes", len(changed), "counts:", changed[:6])
        assert changed and all(n == want - 1 for _, _, want, n in changed), name
