"""CPU: pins tests/token_heads_ref.py, the float64 / bit-defined-f32 statement the GPU tests of the token-selection heads compare with --
against torch's own argmax / softmax, against the reference graphs' formulas restated here from their description in csrc/kernels.h
(TOPK_TOPP_SAMPLING, APPLY_PENALTY, NO_SPEECH_DETECTION), on planted ties, on the generator's known values, and on the margins of every
seeded input tests/test_token_heads_gpu.py uses."""
import numpy as np
import pytest
import torch

import token_heads_ref as R


def _smooth(seed, rows, n):
    """Tie-free inputs: continuous draws; a row in which two f32 values collide is drawn again."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 3.0, (rows, n)).astype(np.float32)
    for r in range(rows):
        while len(np.unique(x[r])) < n:
            x[r] = rng.normal(0.0, 3.0, n).astype(np.float32)
    return x


@pytest.mark.parametrize("n", [1, 5, 129, 4097])
def test_argmax_agrees_with_torch(n):
    x, extra = _smooth(n, 4, n), _smooth(n + 1, 1, n)[0]
    ids, margin = R.argmax_rows(x)
    assert ids.tolist() == torch.argmax(torch.from_numpy(x), dim=1).tolist()
    ids_e, _ = R.argmax_rows(x, extra)
    assert ids_e.tolist() == torch.argmax(torch.from_numpy(x) + torch.from_numpy(extra), dim=1).tolist()
    if n > 1:
        top2 = np.sort(x.astype(np.float64), axis=1)[:, -2:]
        assert np.array_equal(margin, top2[:, 1] - top2[:, 0]) and (margin > 0).all()


@pytest.mark.parametrize("n,K", [(5, 3), (129, 8), (4097, 8), (4097, 1)])
def test_beam_topk_agrees_with_torch_log_softmax(n, K):
    x = _smooth(10 + n, 3, n)
    topv, topi, lse, margin = R.beam_topk(x, K)
    lp = torch.log_softmax(torch.from_numpy(x).double(), dim=1)
    o = torch.argsort(lp, dim=1, descending=True)[:, :K]
    assert topi.tolist() == o.tolist()
    assert np.abs(topv - torch.gather(lp, 1, o).numpy()).max() < 1e-12
    assert np.abs(lse - torch.logsumexp(torch.from_numpy(x).double(), dim=1).numpy()).max() < 1e-12 and (margin > 0).all()


def test_beam_topk_bias_drops_minus_inf_columns_from_list_and_normaliser():
    x = _smooth(3, 2, 129)
    bias = np.zeros(129, np.float32)
    drop = [int(i) for i in R.order(x[0])[:3]] + [0, 128]
    bias[drop] = -np.inf
    topv, topi, _, _ = R.beam_topk(x, 8, bias)
    keep = np.setdiff1d(np.arange(129), drop)
    want_v, want_i, _, _ = R.beam_topk(x[:, keep], 8)
    assert np.array_equal(topi, keep[want_i]) and np.abs(topv - want_v).max() < 1e-12
    few_v, few_i, _, _ = R.beam_topk(np.array([[-np.inf, 1.0, -np.inf, 0.5]], np.float32), 3)
    assert few_i.tolist() == [[1, 3, 0]] and few_v[0, 2] == -np.inf and np.isfinite(few_v[0, :2]).all()
    assert R.beam_topk(np.full((1, 5), -np.inf, np.float32), 3)[1].tolist() == [[0, 0, 0]]
    assert R.argmax_rows(np.full((1, 5), -np.inf, np.float32))[0].tolist() == [0]


def test_tie_order_on_planted_ties():
    x = R.grid_logits(5, 2, 300)
    x[0, [7, 200, 40]] = 20.0
    x[1, [299, 0]] = 21.0
    ids, margin = R.argmax_rows(x)
    assert ids.tolist() == [7, 0] and margin.tolist() == [0.0, 0.0]
    _, topi, _, m = R.beam_topk(x, 3)
    assert topi[0].tolist() == [7, 40, 200] and topi[1, :2].tolist() == [0, 299] and m.tolist() == [0.0, 0.0]
    # the sampler: equal scores astride the top_k boundary -- the lower id is in, the higher one out
    save = np.zeros((2, 4), np.int32)
    noise = np.array([[1e-7, 1e-7, 0.999], [1e-7, 0.999, 0.5]], np.float32)         # strongly favours the last rank (row 0), the second (row 1)
    nxt, margin, _ = R.sample_topk_topp(x, save, 0, 1.0, 3, 1.0, 1.0, noise=noise)
    assert nxt.tolist() == [200, 299] and margin[0, 2] > 0
    nxt2, margin2, _ = R.sample_topk_topp(x, save, 0, 1.0, 2, 1.0, 1.0, noise=noise[:, 1:])
    assert nxt2.tolist() == [40, 0] and margin2[0, 2] == 0.0                        # row 0: rank 2 is id 40, id 200 ties with it and stays out


def _torch_sample(logits, previous_ids, noise, temperature, top_k, top_p, rp):
    """TOPK_TOPP_SAMPLING as kernels.h describes it, in torch f32: repetition penalty on every saved id (negative logits multiplied, the others
    divided; gathered before scattered), x 1 / temperature, top-k, soft-max, keep where cumsum - p <= top_p, Gumbel-max with clamped uniforms."""
    x = torch.from_numpy(logits.copy())
    if len(previous_ids):
        idx = torch.as_tensor(np.asarray(previous_ids), dtype=torch.long)
        pv = x[idx].clone()
        x[idx] = torch.where(pv < 0, pv * rp, pv / rp)
    s = x * (1.0 / temperature)
    order = torch.argsort(s, descending=True, stable=True)[:top_k]
    vals = s[order]
    p = torch.softmax(vals, dim=-1)
    keep = (torch.cumsum(p, dim=-1) - p) <= top_p
    u = torch.clamp(torch.from_numpy(noise), 1.0e-7, 1.0 - 1.0e-7)
    score = torch.where(keep, vals - torch.log(-torch.log(u)), torch.tensor(float("-inf")))
    return int(order[int(torch.argmax(score))]), x.numpy()


@pytest.mark.parametrize("n,hist,k,t,p,rp", [(129, 0, 10, 0.7, 0.95, 1.0), (129, 40, 10, 1.3, 0.3, 1.3), (4097, 300, 64, 0.5, 0.95, 1.3), (4097, 5, 2, 0.7, 1.0, 1.3),
                                             (129, 7, 1, 0.5, 0.3, 1.3)])
def test_sampler_agrees_with_the_restated_torch_formula(n, hist, k, t, p, rp):
    rows = 16
    x = _smooth(100 + n + hist, rows, n)
    save = R.history(1, rows, n, hist, 512)
    noise = np.random.default_rng(n + k).uniform(0, 1, (rows, k)).astype(np.float32)
    nxt, margin, after = R.sample_topk_topp(x, save, hist, t, k, p, rp, noise=noise)
    ok = R.sampler_decided(margin, k)
    assert ok.mean() >= 0.8
    for r in range(rows):
        want, want_after = _torch_sample(x[r], save[r, :hist], noise[r], t, k, p, rp)
        np.testing.assert_allclose(after[r], want_after, rtol=2.0 ** -22, atol=0)      # x * float32(1 / rp) against x / rp: an ulp
        if ok[r]:
            assert nxt[r] == want, (r, margin[r])
    if k == 1:
        assert nxt.tolist() == R.argmax_rows(after)[0].tolist()


def test_sampler_scales_a_repeated_id_once_and_by_sign():
    x = np.array([[2.0, -2.0, 1.0, 0.5]], np.float32)
    save = np.array([[0, 1, 0, 0, 1, 3]], np.int32)
    _, _, after = R.sample_topk_topp(x, save, 5, 1.0, 1, 1.0, 1.3, noise=np.full((1, 1), 0.5, np.float32))
    inv = np.float32(1.0) / np.float32(1.3)
    assert after[0].tolist() == [np.float32(2.0) * inv, np.float32(-2.0) * np.float32(1.3), 1.0, 0.5]      # id 3 sits past n_saved = 5


@pytest.mark.parametrize("partial", [0, 1])
@pytest.mark.parametrize("n_saved", [0, 1, 3, 4, 5, 9])
def test_apply_penalty_agrees_with_the_restated_torch_formula(partial, n_saved):
    """APPLY_PENALTY: gather the logits of save_id[:, -range:], multiply, scatter back. The host applies it once `range` ids are saved (Whisper); with
    partial = 1 the slice is taken of whatever exists (Qwen3)."""
    rng_, value, rows, n = 4, 0.8, 3, 129
    x = _smooth(n_saved, rows, n)
    save = R.history(2, rows, n, 9, 9)
    got = R.apply_penalty(x, save, n_saved, rng_, value, partial)
    t = torch.from_numpy(x.copy())
    if n_saved >= rng_ or (partial and n_saved > 0):
        ids = torch.from_numpy(save[:, :n_saved]).long()[:, -rng_:]
        t.scatter_(1, ids, torch.gather(t, 1, ids) * value)
    assert np.array_equal(got, t.numpy())
    assert (got != x).any() == (n_saved >= rng_ or (partial == 1 and n_saved > 0))


def test_append_ids():
    save = np.arange(12, dtype=np.int32).reshape(3, 4)
    assert R.append_ids(save, [70, 71, 72], 2)[:, 2].tolist() == [70, 71, 72]
    assert np.array_equal(R.append_ids(save, [70, 71, 72], 4), save)
    assert (R.append_ids(save, [70, 71, 72], 2) != save).sum() == 3


@pytest.mark.parametrize("target", [1e-6, 0.5, 1.0])
def test_no_speech_agrees_with_torch_softmax(target):
    n, nid = 4097, 4094
    x, pen, _ = R.no_speech_inputs(n, nid, target)
    p, d = R.no_speech_prob(x, pen, nid)
    want = torch.softmax(torch.from_numpy(x).double() - torch.from_numpy(pen).double(), dim=1)[:, nid].numpy()
    np.testing.assert_allclose(p, want, rtol=1e-12)
    want32 = torch.softmax(torch.from_numpy(x) - torch.from_numpy(pen), dim=1)[:, nid].numpy()
    assert (np.abs(want32 - p) <= R.no_speech_budget(n, p, d)).all()


def test_generator_known_values():
    # (seed 0, counter 1, 2, 3) is the published splitmix64 stream of seed 0: 0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F
    for j, z in enumerate([0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]):
        assert R.uniform_from_counter(0, 0, 0, j) == np.float32((z >> 40) / 2.0 ** 24)
    # the counter: step * 0x100000001B3 + row * 256 + j + 1, so (step 0, row 1, j 0) is the stream's 257th value and the seed shifts the state
    def mix(z):
        z = np.uint64(z)
        with np.errstate(over="ignore"):
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return int(z ^ (z >> np.uint64(31)))
    g = 0x9E3779B97F4A7C15
    for seed, step, row, j in [(0, 0, 1, 0), (42, 3, 2, 9), (0xDEADBEEFCAFEF00D, 19, 4, 63), (7, 2 ** 31 + 5, 0, 1)]:
        ctr = step * 0x100000001B3 + row * 256 + j + 1
        want = mix((seed + g * ctr) % 2 ** 64) >> 40
        got = R.uniform_from_counter(seed, step, row, j)
        assert got == np.float32(want / 2.0 ** 24) and 0.0 <= got < 1.0
    assert R.uniform_from_counter(0, 0, 0, 0) == np.float32(0xE220A8 / 2.0 ** 24)
    u = np.array([R.uniform_from_counter(5, 0, r, 0) for r in range(4096)], np.float64)
    assert abs(u.mean() - 0.5) < 5 * (1 / 12 / 4096) ** 0.5


def test_grid_inputs_are_exact_and_keep_their_order_under_f32_scaling():
    x = R.grid_logits(1, 3, 4097)
    assert np.array_equal(x.astype(np.float64) / R.GRID, np.round(x.astype(np.float64) / R.GRID))
    for s in (np.float32(1.0) / np.float32(0.5), np.float32(1.0) / np.float32(0.7), np.float32(1.0) / np.float32(1.3), np.float32(1.3)):
        for row in x:
            u = np.unique(row)
            assert (np.diff((u * s).astype(np.float32)) > 0).all()


def test_margins_of_the_seeded_sampler_inputs_respect_the_skip_cap():
    """Every seeded input of the GPU file: the share of rows whose margin is inside the budget stays under the cap, and the histories do what the
    issue asks of them (ids repeat, and land on positive and negative logits)."""
    for case in R.sampler_noise_cases():
        n, h, k, t, p, rp = case
        x, save, noise = R.sampler_noise_inputs(case)
        _, margin, after = R.sample_topk_topp(x, save, h, t, k, p, rp, noise=noise)
        assert np.abs(after).max() / t <= 64.0                                       # the budget's bound on the scores
        assert 1.0 - R.sampler_decided(margin, k).mean() <= R.SKIP_CAP, (case, margin)
        if h > 7:
            picked = np.take_along_axis(x, save[:, :h], 1)
            assert (picked < 0).any() and (picked > 0).any() and all(len(np.unique(s[:h])) < h for s in save)
    c = R.SEEDED
    for case in R.sampler_seeded_cases():
        x, save = R.sampler_seeded_inputs(case)
        _, margin, _ = R.sample_topk_topp(x, save, case[1], c["temperature"], c["top_k"], c["top_p"], c["rp"], seed=case[0])
        assert 1.0 - R.sampler_decided(margin, c["top_k"]).mean() <= R.SKIP_CAP, (case, margin)
    e = R.EXTRA
    for k in (1, 10):
        x, save, extra, noise = R.sampler_extra_inputs(k)
        _, margin, _ = R.sample_topk_topp(x, save, e["n_saved"], e["temperature"], k, e["top_p"], e["rp"], extra=extra, noise=noise)
        assert 1.0 - R.sampler_decided(margin, k).mean() <= R.SKIP_CAP, (k, margin)
    u = R.UNIFORM
    x, save = R.sampler_uniform_inputs()
    _, margin, _ = R.sample_topk_topp(x[:u["checked"]], save[:u["checked"]], u["n_saved"], 1.0, 4, 1.0, 1.0, seed=u["seed"])
    assert 1.0 - R.sampler_decided(margin, 4).mean() <= R.SKIP_CAP, margin
    assert {c[1] for c in R.sampler_noise_cases()} == set(R.HISTORIES) and {c[2] for c in R.sampler_noise_cases()} == {1, 2, 10, 64}
    assert {c[3] for c in R.sampler_noise_cases()} == {0.5, 0.7, 1.3} and {c[4] for c in R.sampler_noise_cases()} == {0.3, 0.95, 1.0}
    assert {(c[1] > 0, c[5]) for c in R.sampler_noise_cases()} >= {(True, 1.0), (True, 1.3)}


def test_budgets_hold_for_a_plain_f32_evaluation():
    """A straightforward f32 numpy evaluation of the same formulas sits inside the derived budgets (it has no fast exponential and another summation order)."""
    for n in (129, 4097, 51866):
        x = R.grid_logits([n, 77], 3, n)
        topv, topi, lse, _ = R.beam_topk(x, 8)
        m = x.max(axis=1, keepdims=True)
        lse32 = (m[:, 0] + np.log(np.exp(x - m).sum(axis=1, dtype=np.float32))).astype(np.float32)
        v32 = np.take_along_axis(x, topi, 1) - lse32[:, None]
        assert (np.abs(v32 - topv) <= R.beam_topv_budget(n, m.astype(np.float64), lse[:, None], topv)).all()


def test_head_steps_inputs_show_what_the_head_does():
    """The inputs of test_head_steps (tests/test_token_heads_gpu.py): the same rows at every step, so every change of pick is the head's doing -- a head that
    skips the bias, the penalty, the history or the hand-over of the noise gives other picks than these."""
    c = R.HEAD_STEPS
    x, bias, noise = R.head_steps_inputs()
    cases = R.head_steps_cases()
    run = lambda kw: R.head_steps(x, c["steps"], c["ld_save"], **kw)
    raw, rng = R.argmax_rows(x)[0], c["range_"]
    assert c["steps"] > rng + 1 and c["steps"] <= c["ld_save"] and len(cases) == 5
    # partial 0 (Whisper): nothing is penalised until `range` ids are saved -- the pick is kept through the first `range` steps and changes at step range + 1
    # (index `range`); the biased step 0 takes the second-best column instead of the raw arg-max
    p, save, n, _ = run(dict(cases["partial 0, step-0 bias"], bias=None))
    assert (p[:rng] == raw).all() and (p[rng] != raw).all()
    p, save, n, _ = run(cases["partial 0, step-0 bias"])
    assert (p[0] != raw).all() and (p[1:rng] == raw).all() and (p[rng] != raw).all()
    assert n == c["steps"] and np.array_equal(save[:, :n], p.T) and (save[:, n:] == 0).all()
    # partial 1 (Qwen3): whatever is saved is penalised -- the pick changes at the second step
    p1, save, n, _ = run(cases["partial 1"])
    assert (p1[0] == raw).all() and (p1[1] != p1[0]).all() and np.array_equal(save[:, :n], p1.T)
    # value 1.0 with the history tracked: the picks never move, the history fills
    p, save, n, _ = run(cases["value 1.0, history tracked"])
    assert (p == raw).all() and n == c["steps"] and (save[:, :n] == raw[:, None]).all()
    assert run(dict(cases["value 1.0, history tracked"], track_history=False))[2] == 0
    # the sampler: every pick decided; noise kept armed for a second step, or never used, gives other picks
    kw = cases["sampler, noise on step 0"]
    p, save, n, decided = run(kw)
    assert decided.all() and np.array_equal(save[:, :n], p.T) and len(np.unique(p)) > c["rows"]
    every = [R.sample_topk_topp(x, save, t, *kw["sampler"][:4], noise=noise, seed=kw["sampler"][4])[0] for t in (1, 2)]
    assert (every[0] != p[1]).any() or (every[1] != p[2]).any()
    assert (run(dict(kw, noise=None))[0][0] != p[0]).any()
    # the change of penalty shows in the steps after it and in none before
    pc = run(cases["penalty changed after step 4"])[0]
    at = cases["penalty changed after step 4"]["change"][0]
    assert at == 5 and np.array_equal(pc[:at], p1[:at]) and (pc[at:] != p1[at:]).any()
