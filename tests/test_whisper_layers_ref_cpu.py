"""tests/whisper_layers_ref.py against the oracle, against itself, and the condition on every planted mistake (no GPU).

The condition: a mutation moves the tapped output of its stage by more than 2 x MARGIN x E_round in both components of `stat`, at every length and row count
where test_whisper_layers_ref_gpu.py relies on it. A kernel may sit at MARGIN x E_round and the mistake must still push it over; the factor 2 is not a measurement."""
import numpy as np
import pytest
import torch

import whisper_layers_ref as R
from oracle.whisper_oracle import WhisperOracle
from whisper_layers_ref import MARGIN, stat

F64 = torch.float64
CASES = R.MISTAKE_CASES


def _oracle_run(orc, cfg, lengths, prompts, steps_ids):
    """Per utterance: (enc_out, K, V, [logits per step]) from the oracle's own encode / decoder."""
    out = []
    with torch.inference_mode():
        for b, a in enumerate(R.batch_audios(cfg, lengths)):
            taps = {}
            k, v = orc.encode(a, taps)
            ids = torch.tensor([list(prompts[b])], dtype=torch.long)
            lg, sk, sv = orc.decoder(ids, 0, None, None, k.unsqueeze(0), v.unsqueeze(0))
            logits, hist = [lg[0].numpy()], ids.shape[1]
            for row in steps_ids:
                lg, sk, sv = orc.decoder(torch.tensor([[int(row[b])]]), hist, sk, sv, k.unsqueeze(0), v.unsqueeze(0))
                hist += 1
                logits.append(lg[0].numpy())
            out.append((taps["enc_out"].numpy(), k.numpy(), v.numpy(), logits))
    return out


@pytest.mark.parametrize("cfg_name", ["whisper_d256_test", "whisper_tiny_test"])
def test_exact_chain_is_the_float64_oracle_and_the_f32_oracle_sits_in_the_f32_budget(cfg_name):
    cfg, ck, sup, beg, L = R.setup(cfg_name, planted=False)
    lengths = (40, 17)
    plan = R.decode_plan(cfg, lengths)
    tr = R.cpu_trace(L, cfg, lengths, plan)
    prompts, steps_ids = plan[0][0], [p[0][:, 0] for p in plan[1:]]
    ref = _oracle_run(L.orc, cfg, lengths, prompts, steps_ids)
    for b, (r0, T) in enumerate(tr.rows):
        eo, k, v, logits = ref[b]
        assert np.abs(tr.enc["enc_out"][r0:r0 + T] - eo).max() < 1e-11
        assert np.abs(tr.cross[0, :, :, r0:r0 + T].numpy() - k).max() < 1e-11 and np.abs(tr.cross[1, :, :, r0:r0 + T].numpy() - v).max() < 1e-11
        for t, want in enumerate(logits):
            assert np.abs(tr.steps[t]["logits"][b] - want).max() < 1e-10, (b, t)
    # the f32 oracle against the exact chain: the budget is the chain evaluated in float32 in three summation orders
    forms = [R.cpu_trace(L, cfg, lengths, plan, via=f) for f in R.F32_FORMS]
    ref32 = _oracle_run(WhisperOracle(cfg, ck, sup, beg), cfg, lengths, prompts, steps_ids)
    for t in range(len(plan)):
        exact = tr.steps[t]["logits"]
        e = [stat(exact - f.steps[t]["logits"]) for f in forms]
        e_round = max(x[0] for x in e), max(x[1] for x in e)
        ok, ratios = R.within(exact - np.stack([r[3][t] for r in ref32]), e_round)
        print(f"f32 oracle {cfg_name} step {t}: ratio rms {ratios[0]:.2f} max {ratios[1]:.2f} (E_round {e_round[0]:.2e} {e_round[1]:.2e})")
        assert ok, (t, ratios)


def test_carried_history_equals_recomputing_the_sequence_and_left_padding_changes_nothing():
    cfg, ck, sup, beg, L = R.setup("whisper_d256_test")
    lengths = (40, 17, 33)
    carried = R.cpu_trace(L, cfg, lengths, R.decode_plan(cfg, lengths, 4, 4))
    ids = np.concatenate([s["ids"] for s in carried.steps], axis=1)                     # the same 8 ids as one prefill
    whole = R.cpu_trace(L, cfg, lengths, [(ids, None)])
    assert np.abs(whole.steps[0]["logits"] - carried.steps[-1]["logits"]).max() < 1e-10
    for l in range(cfg.n_dec_layers):
        for b in range(3):
            assert np.abs(whole.steps[0]["dec"][l][b * 8 + 7] - carried.steps[-1]["dec"][l][b]).max() < 1e-11
    plan = R.prompt_plan(cfg, lengths)
    padded = R.cpu_trace(L, cfg, lengths, plan)
    for b, T in enumerate(lengths):
        solo_plan = [(plan[0][0][b:b + 1, plan[0][1][b]:], None)] + [(p[0][b:b + 1], None) for p in plan[1:]]
        solo = R.cpu_trace(L, cfg, (T,), solo_plan, first=b)
        for t in range(len(plan)):
            assert np.abs(padded.steps[t]["logits"][b] - solo.steps[t]["logits"][0]).max() < 1e-10, (b, t)


@pytest.mark.parametrize("cfg_name", ["whisper_d256_test", "whisper_tiny_test"])
def test_planted_heads_are_peaked_at_every_tested_length(cfg_name):
    cfg, ck, sup, beg, L = R.setup(cfg_name)
    batches = R.ENC_BATCHES.values() if cfg_name == "whisper_d256_test" else [R.TINY_LENGTHS]
    worst = {}
    note = lambda k, p: worst.__setitem__(k, min(worst.get(k, 1.0), float(p.min()))) if p.numel() else None
    for lengths in batches:
        tr = R.cpu_trace(L, cfg, lengths, None, encoder_only=True)
        for u, (r0, T) in enumerate(tr.rows):
            t = torch.arange(T)
            for i in range(cfg.n_enc_layers):
                pr = []
                L.enc_layer(i, tr.enc["stem" if i == 0 else f"enc{i - 1}"][r0:r0 + T], probs=pr)
                p = pr[0]
                note("enc identity", p[0, t, t])
                if cfg.n_heads > 3:
                    tt = t[(R.REV - t >= 0) & (R.REV - t < T)]
                    note("enc reversal", p[1, tt, R.REV - tt])
                    tt = t[t + R.SHIFT < T]
                    note("enc shift", p[2, tt, tt + R.SHIFT])
    lengths = R.dec_lengths(3) if cfg_name == "whisper_d256_test" else R.TINY_LENGTHS
    for plan in (R.decode_plan(cfg, lengths), R.prompt_plan(cfg, lengths)):
        tr = R.cpu_trace(L, cfg, lengths, plan)
        for t, step in enumerate(tr.steps):
            n, S0 = step["ids"].shape[1], tr.hist(t)
            for l in range(cfg.n_dec_layers):
                for b in range(len(lengths)):
                    pr, pad = [], int(tr.pads[b])
                    L.dec_layer(l, tr.layer_inputs(t, l, b), tr.kv(b, l), pad, probs=pr)
                    ps, pc = pr[0]
                    rows = torch.arange(max(pad - S0, 0), n)
                    own = S0 + rows
                    note("self oldest", ps[0, rows, pad])
                    note("self newest", ps[1, rows, own])
                    if cfg.n_heads > 3:
                        ok = own - 2 >= pad
                        note("self t-2", ps[3, rows[ok], own[ok] - 2])
                    note("cross token-addressed", pc[0, rows, torch.as_tensor(step["ids"][b, rows.numpy()], dtype=torch.long)])
    for k, v in worst.items():
        print(f"{cfg_name} planted head '{k}': lowest probability of the planted key {v:.3f}")
        assert v >= 0.5, (k, v)


def _condition(what, exact, rounded_fn, mutated, case):
    e_round = R.budget(exact, rounded_fn, [None])
    ok, ratios = R.exceeds(exact - mutated, e_round, 2 * MARGIN)
    return ok, min(ratios), f"{case} {what}: moved by {ratios[0]:.1f} (rms) {ratios[1]:.1f} (max) x E_round"


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_planted_mistake_moves_its_stage_beyond_twice_the_margin(case):
    cfg_name, lengths, kind = CASES[case]
    cfg, ck, sup, beg, L = R.setup(cfg_name)
    plan = {"steps": R.decode_plan, "prompts": R.prompt_plan, None: lambda *a: None}[kind](cfg, lengths)
    tr = R.cpu_trace(L, cfg, lengths, plan, encoder_only=kind is None)
    lows, applied = {}, {}

    def judge(mut, key, exact, rounded_fn, mutated):
        if not R.relied_on(mut, case):
            return
        applied[mut] = applied.get(mut, 0) + (mutated is not None)
        if mutated is None:
            return
        ok, low, msg = _condition(f"{mut} {key}", exact, rounded_fn, mutated, case)
        if mut not in lows or low < lows[mut][0]:
            lows[mut] = (low, msg, ok)
        assert ok, msg

    if kind is None:
        for i in range(cfg.n_enc_layers):
            for u in range(len(lengths)):
                exact = R.enc_stage(L, tr, i, u)
                for mut in R.ENC_MUTATIONS:
                    judge(mut, f"enc{i} T={lengths[u]}", exact, lambda _: R.enc_stage(L, tr, i, u, R.ENC_ROUNDINGS), R.enc_stage(L, tr, i, u, mut=mut))
    else:
        for t, step in enumerate(tr.steps):
            B, n = step["ids"].shape
            rnd = R.dec_roundings(cfg, B * n, prompt=step is tr.steps[0] and kind == "prompts")
            for mut in R.EMBED_MUTATIONS:
                if not R.relied_on(mut, case) or mut == "pad_pos" and t > 0:
                    continue
                exact, bad = R.dec_in_stage(L, tr, t), R.dec_in_stage(L, tr, t, mut=mut)
                applied[mut] = applied.get(mut, 0) + 1
                assert np.abs(exact - bad).max() > 0.1 * R.DEC_A, (mut, t)           # dec_in is compared bit for bit: any move shows; the code channels move by ~ DEC_A
            for l in range(cfg.n_dec_layers):
                for b in range(B):
                    exact = R.dec_stage(L, tr, t, l, b)
                    for mut in R.SELF_MUTATIONS + R.CROSSATT_MUTATIONS:
                        pad_row = L.pad_key(l) if mut == "pad_row" else None
                        judge(mut, f"step {t} dec{l} seq {b}", exact, lambda _: R.dec_stage(L, tr, t, l, b, rnd), R.dec_stage(L, tr, t, l, b, mut=mut, pad_row=pad_row))
            exact, _ = R.head_stage(L, tr, t)
            bad, ok_rows = R.head_stage(L, tr, t, mut="row_n_minus_2")
            rounded = R.head_stage(L, tr, t, R.HEAD_ROUNDINGS)[0]
            for b in np.nonzero(ok_rows)[0]:
                judge("row_n_minus_2", f"step {t} logits seq {b}", exact[b:b + 1], lambda _: rounded[b:b + 1], bad[b:b + 1])
    for mut, (low, msg, ok) in sorted(lows.items()):
        print("LOWEST", msg)
    expected = R.ENC_MUTATIONS if kind is None else R.SELF_MUTATIONS + R.CROSSATT_MUTATIONS + R.HEAD_MUTATIONS + R.EMBED_MUTATIONS
    for mut in expected:
        if R.relied_on(mut, case):
            assert applied.get(mut, 0) > 0, f"{mut} never applied in {case}"
