"""The six token-selection heads of csrc/kernels.hip -- argmax_rows, beam_topk, apply_penalty, append_ids, sample_topk_topp, no_speech_prob --
through the probe library (product launchers unchanged, real leading dimension, pad columns at +1e30) against tests/token_heads_ref.py:
vocabulary widths across every loop boundary up to the deployment widths, planted maxima and exact ties at every level of the merges,
-inf columns, the penalty windows and the history counter, the sampler with caller noise and with its own generator.

Logits sit on a 2^-10 grid, so orderings (and the f32 penalty / temperature arithmetic) are decided without tolerance; only log-probabilities,
the no-speech probability and the sampler's soft-max / top-p / Gumbel comparisons carry budgets, all derived in token_heads_ref.py.

Column ownership the plants rely on: in argmax_rows_kernel and beam_topk_kernel thread t (lane t % 64 of wave t / 64, 16 waves) reads columns
4 t .. 4 t + 3 of every 4096-column stripe; argmax takes two stripes per trip of its loop (8192 columns)."""
import numpy as np
import pytest

import token_heads_ref as R
from conftest import sub

pytestmark = pytest.mark.gpu

TOP = np.float32(20.0)                 # above every N(0, 3^2) draw used here (|x| < 6.7 sigma)


def _head(op, *a, **k):
    return sub("_probe").token_head(op, *a, **k)


def _pad_ok(out, n):
    return bool((out["logits"][:, n:] == sub("_probe").PAD_LOGIT).all())


def _chunks(rows):
    """Calls of 3 to 5 rows: the list is cut in fives, a short tail is filled up with copies of its first row."""
    for i in range(0, len(rows), 5):
        part = rows[i:i + 5]
        yield i, np.stack(part + [part[0]] * (3 - len(part)) if len(part) < 3 else part), len(part)


# pairs of columns that meet at one level of the kernels' merges (see the module docstring)
PAIRS = {"one float4": (8, 10), "two lanes of a wave": (9, 101), "two waves": (8, 300), "two loads of a trip": (11, 4104), "later wave, lower id": (300, 4106),
         "two trips": (8, 8200), "two trips, other thread": (4100, 8461)}
SPOTS = [0, 4095, 4096, 8191, 8192]


def _planted_rows(n, seed):
    """(label, row, winner or None): random rows, the maximum planted at each boundary column, equal maxima in pairs."""
    base = R.grid_logits([n, seed], 3, n)
    rows = [("random", base[i].copy(), None) for i in range(3)]
    for p in sorted({s for s in SPOTS if s < n} | {n - 1}):
        x = base[p % 3].copy()
        x[p] = TOP
        rows.append((f"maximum at {p}", x, p))
    for label, (a, b) in PAIRS.items():
        if b < n:
            x = base[a % 3].copy()
            x[[a, b]] = TOP
            rows.append((f"equal maxima, {label}", x, a))
    return rows


# ------------------------------------------------------------------------------------------------ argmax_rows
@pytest.mark.parametrize("n", R.WIDTHS)
def test_argmax_rows_widths_plants_and_ties(n):
    plan = _planted_rows(n, 1)
    extra = R.grid_logits([n, 2], 1, n)[0]
    for i, x, m in _chunks([p[1] for p in plan]):
        want, _ = R.argmax_rows(x)
        out = _head("argmax_rows", x)
        assert out["ids"].tolist() == want.tolist(), [p[0] for p in plan[i:i + m]]
        for j in range(m):
            if plan[i + j][2] is not None:
                assert out["ids"][j] == plan[i + j][2], plan[i + j][0]
        assert np.array_equal(out["logits"][:, :n], x) and _pad_ok(out, n)
        want_e, _ = R.argmax_rows(x, extra)                     # `extra` moves the maximum: the kernel must add it
        assert _head("argmax_rows", x, vec=extra)["ids"].tolist() == want_e.tolist()
    # an extra that lifts one column over the planted maximum
    x = np.stack([p[1] for p in plan[:3]])
    lift = np.zeros(n, np.float32)
    lift[n // 2] = 64.0
    assert _head("argmax_rows", x, vec=lift)["ids"].tolist() == [n // 2] * 3


@pytest.mark.parametrize("n", [5, 129, 4097, 12289])
def test_argmax_rows_empty_row_gives_id_zero(n):
    """A row with no column above -inf: torch.argmax returns 0, and the id is used as an embedding row by the next step."""
    x = R.grid_logits([n, 3], 3, n)
    x[1] = -np.inf
    out = _head("argmax_rows", x)
    assert out["ids"].tolist() == R.argmax_rows(x)[0].tolist() and out["ids"][1] == 0
    x[2, :n - 1] = -np.inf                                       # one finite column, the last
    assert _head("argmax_rows", x)["ids"].tolist()[1:] == [0, n - 1]


# ------------------------------------------------------------------------------------------------ beam_topk
def _check_topk(x, K, bias=None, label=""):
    n = x.shape[1]
    topv, topi, lse, _ = R.beam_topk(x, K, bias)
    out = _head("beam_topk", x, vec=bias, K=K)
    assert out["topi"].tolist() == topi.tolist(), label
    fin = np.isfinite(topv)
    assert np.array_equal(out["topv"][~fin], topv[~fin].astype(np.float32)), label        # ranks past the last candidate: -inf
    xb = x if bias is None else (x + bias[None, :]).astype(np.float32)
    tol = R.beam_topv_budget(n, xb.max(axis=1, keepdims=True).astype(np.float64), lse[:, None], np.where(fin, topv, 0.0))
    err = np.abs(out["topv"].astype(np.float64) - np.where(fin, topv, 0.0))
    worst = float((err / tol)[fin].max()) if fin.any() else 0.0
    print(f"beam_topk n={n} K={K} {label}: worst |topv error| {float(err[fin].max()) if fin.any() else 0.0:.3e}, {worst:.3f} of the budget ({float(tol[fin].min()) if fin.any() else 0:.3e})")
    assert np.isfinite(out["topv"][fin]).all() and worst <= 1.0, label
    assert np.array_equal(out["logits"][:, :n], x) and _pad_ok(out, n)
    return out


@pytest.mark.parametrize("n,K", [(n, K) for n in R.WIDTHS for K in (1, 3, 8) if n <= R.WIDE or K == 8])
def test_beam_topk_widths_plants_and_ties(n, K):
    plan = _planted_rows(n, 4)
    for i, x, m in _chunks([p[1] for p in plan]):
        out = _check_topk(x, K, label="; ".join(p[0] for p in plan[i:i + m]))
        for j in range(m):
            label, _, win = plan[i + j]
            if win is not None:
                assert out["topi"][j, 0] == win, label
            if label.startswith("equal maxima") and K >= 2:
                a, b = PAIRS[label.split(", ", 1)[1]]
                assert out["topi"][j, :2].tolist() == [a, b] and out["topv"][j, 0] == out["topv"][j, 1], label


def test_beam_topk_per_thread_lists():
    """Thread 2 owns columns 8 .. 11 of every stripe. Nine equal top values there: its sorted list keeps eight, and they must be the eight lowest ids.
    Then the eight best values of the row all in that thread's columns (in falling, rising and mixed order), then one per wave."""
    n = 12289
    own = [8, 9, 10, 11, 4104, 4105, 4106, 4107, 8200]
    base = R.grid_logits([n, 5], 5, n)
    x = base.copy()
    x[0, own] = TOP
    x[1, own[:8]] = TOP + np.arange(8, 0, -1, dtype=np.float32)
    x[2, own[:8]] = TOP + np.arange(1, 9, dtype=np.float32)
    x[3, own[:8]] = TOP + np.array([3, 7, 1, 8, 2, 6, 4, 5], np.float32)
    spread = [w * 256 + 8 for w in range(8)]
    x[4, spread] = TOP + np.array([5, 1, 8, 3, 7, 2, 6, 4], np.float32)
    out = _check_topk(x, 8, label="per-thread lists")
    assert out["topi"][0].tolist() == own[:8]
    assert out["topi"][1].tolist() == own[:8] and out["topi"][2].tolist() == own[:8][::-1]
    assert out["topi"][4].tolist() == [spread[w] for w in (2, 4, 6, 0, 7, 3, 5, 1)]          # by the planted increments 8, 7, ... 1
    y = base[:3].copy()                                           # nine equal values, K = 3: still the lowest ids, in order
    y[:, own] = TOP
    assert _check_topk(y, 3, label="nine equal, K = 3")["topi"].tolist() == [own[:3]] * 3


@pytest.mark.parametrize("n", [129, 4097, 12289])
def test_beam_topk_bias_drops_minus_inf_columns(n):
    """Whisper's BEGIN_SUPPRESS: a column the bias takes to -inf is neither a candidate nor part of the normaliser; a finite bias is added."""
    x = R.grid_logits([n, 6], 4, n)
    bias = np.zeros(n, np.float32)
    best = [int(R.order(x[r])[0]) for r in range(4)]
    bias[best + [0, n - 1]] = -np.inf
    bias[n // 3] = 30.0
    out = _check_topk(x, 8, bias, label="bias")
    assert not np.isin(out["topi"], best + [0, n - 1]).any() and (out["topi"][:, 0] == n // 3).all()


@pytest.mark.parametrize("n", [129, 4097, 12289])
def test_beam_topk_minus_inf_logits_without_bias(n):
    """-inf logits as the first column several threads see (columns 4 t), no bias: they carry zero weight, the log-probabilities stay finite."""
    x = R.grid_logits([n, 7], 4, n)
    first = [c for c in (0, 4, 40, 256, 1024, 4092) if c < n]
    x[0, first] = -np.inf
    x[1, ::4] = -np.inf                                           # the first column of every thread
    x[2, :n - 2] = -np.inf                                        # two candidates left for K = 8
    out = _check_topk(x, 8, label="-inf logits")
    assert np.isfinite(out["topv"][:2]).all() and np.isfinite(out["topv"][3]).all()
    assert out["topi"][2].tolist() == [int(i) for i in R.order(x[2])[:2]] + [0] * 6


@pytest.mark.parametrize("n", [5, 129, 4097])
def test_beam_topk_empty_row_gives_id_zero(n):
    x = R.grid_logits([n, 8], 3, n)
    x[1] = -np.inf
    out = _head("beam_topk", x, K=3)
    assert out["topi"][1].tolist() == [0, 0, 0]
    want = R.beam_topk(x, 3)[1]
    assert out["topi"].tolist() == want.tolist()


# ------------------------------------------------------------------------------------------------ apply_penalty
LD_SAVE = 80


@pytest.mark.parametrize("range_", [1, 4, 64])
@pytest.mark.parametrize("partial", [0, 1])
def test_apply_penalty_windows(partial, range_):
    n, rows = 129, 5
    x = R.grid_logits([n, 9, range_], rows, n)
    ld = 256
    for n_saved in sorted({0, 1, range_ - 1, range_, range_ + 1, LD_SAVE}):
        for value in (0.8, 1.25):
            save = R.history(4, rows, n, LD_SAVE, LD_SAVE)
            lo = max(0, n_saved - range_)
            save[0, lo:n_saved] = 77                                # the window holds one id up to `range` times
            save[1, lo:n_saved] = ([0, n - 1] * range_)[:n_saved - lo]      # the row's first and last column, alternating
            want = R.apply_penalty(x, save, n_saved, range_, value, partial)
            out = _head("apply_penalty", x, save_ids=save, n_saved=n_saved, range_=range_, value=value, partial=partial)
            label = (partial, range_, n_saved, value)
            assert out["logits"].shape == (rows, ld) and _pad_ok(out, n), label
            assert np.array_equal(out["logits"][:, :n].view(np.uint32), want.view(np.uint32)), label      # bit-identical, inside and outside the window
            active = n_saved >= range_ or (partial == 1 and n_saved > 0)
            assert (want != x).any() == active, label
            if active:
                assert out["logits"][0, 77] == x[0, 77] * np.float32(value) and (np.delete(out["logits"][0, :n], 77) == np.delete(x[0], 77)).all(), label
            assert out["n_saved"] == n_saved and np.array_equal(out["save_ids"], save), label


# ------------------------------------------------------------------------------------------------ append_ids
@pytest.mark.parametrize("n_saved", [0, 5, 11, 12])
def test_append_ids_writes_one_column(n_saved):
    rows, ld_save = 70, 12                                          # 70 rows: two blocks of 64, the second partly idle
    rng = np.random.default_rng(n_saved)
    save = rng.integers(0, 50000, (rows, ld_save)).astype(np.int32)
    nxt = rng.integers(50000, 151936, rows).astype(np.int32)
    out = _head("append_ids", save_ids=save, n_saved=n_saved, next_ids=nxt)
    assert np.array_equal(out["save_ids"], R.append_ids(save, nxt, n_saved)) and out["n_saved"] == n_saved
    changed = np.argwhere(out["save_ids"] != save)
    assert (len(changed) == 0) if n_saved == ld_save else (changed[:, 1] == n_saved).all() and len(changed) == rows


# ------------------------------------------------------------------------------------------------ sample_topk_topp, caller noise
def _sample(x, save, n_saved, t, k, p, rp, **kw):
    return _head("sample_topk_topp", x, K=k, save_ids=save, n_saved=n_saved, temperature=t, top_p=p, repetition_penalty=rp, **kw)


def _check_sample(x, save, n_saved, t, k, p, rp, noise=None, seed=0, skip_none=False, extra=None, label=""):
    n = x.shape[1]
    want, margin, after = R.sample_topk_topp(x, save, n_saved, t, k, p, rp, extra=extra, noise=noise, seed=seed)
    out = _sample(x, save, n_saved, t, k, p, rp, noise=noise, seed=seed, vec=extra)
    ok = R.sampler_decided(margin, k)
    skipped = 1.0 - ok.mean()
    print(f"sampler {label}: skipped {skipped:.3f} of {len(x)} rows")
    assert skipped <= (0.0 if skip_none else R.SKIP_CAP), (label, margin)
    assert out["next"][ok].tolist() == want[ok].tolist(), (label, margin)
    assert np.array_equal(out["logits"][:, :n].view(np.uint32), after.view(np.uint32)) and _pad_ok(out, n), label
    assert out["n_saved"] == n_saved and np.array_equal(out["save_ids"], save), label
    return out, want


@pytest.mark.parametrize("case", R.sampler_noise_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_sampler_with_caller_noise(case):
    n, h, k, t, p, rp = case
    x, save, noise = R.sampler_noise_inputs(case)
    _check_sample(x, save, h, t, k, p, rp, noise=noise, label=str(case))


def test_sampler_extra_bias_and_top_k_one_is_the_argmax():
    c = R.EXTRA
    n = c["n_valid"]
    x, save, extra, noise = R.sampler_extra_inputs(1)
    out, want = _check_sample(x, save, c["n_saved"], c["temperature"], 1, c["top_p"], c["rp"], noise=noise, extra=extra, skip_none=True, label="top_k 1 + extra")
    assert out["next"].tolist() == R.argmax_rows(out["logits"][:, :n], extra)[0].tolist()
    x, save, extra, noise10 = R.sampler_extra_inputs(10)
    _check_sample(x, save, c["n_saved"], c["temperature"], 10, c["top_p"], c["rp"], noise=noise10, extra=extra, label="top_k 10 + extra")


@pytest.mark.parametrize("n", [129, 4097])
def test_sampler_top_p_cut_and_ties_at_the_top_k_boundary(n):
    save = np.zeros((3, 8), np.int32)
    x = R.grid_logits([n, 13], 3, n)
    a, b = 40, n - 2
    x[:, [a, b]] = TOP                                              # two equal dominant logits: p = 0.5 each, exclusive sums 0 and 0.5
    noise = np.array([[1.0e-7, 0.999]] * 3, np.float32)             # strongly favours the second rank
    out, _ = _check_sample(x, save, 0, 1.0, 2, 0.4, 1.0, noise=noise, skip_none=True, label="top-p pair, 0.4")
    assert out["next"].tolist() == [a] * 3                          # 0.5 > 0.4: the second is cut, the first, lower id wins
    out, _ = _check_sample(x, save, 0, 1.0, 2, 1.0, 1.0, noise=noise, skip_none=True, label="top-p pair, 1.0")
    assert out["next"].tolist() == [b] * 3
    # three equal dominant logits, top_p = 0.5: the exclusive sums 0, 1/3, 2/3 keep two ranks (the sums after adding p would keep one)
    z = R.grid_logits([n, 16], 3, n)
    c = n // 2
    z[:, [a, c, b]] = TOP
    out, _ = _check_sample(z, save, 0, 1.0, 3, 0.5, 1.0, noise=np.array([[1.0e-7, 0.999, 0.9999]] * 3, np.float32), skip_none=True, label="top-p triple, 0.5")
    assert out["next"].tolist() == [c] * 3                          # the third, most favoured, is cut; the second wins
    # exact ties astride the top_k boundary: ranks 2 and 3 are equal, top_k = 2 -- the lower id is in, the higher one out, whatever the noise says
    y = R.grid_logits([n, 14], 3, n)
    lo, hi = 17, n - 1
    y[:, 5] = TOP
    y[:, [lo, hi]] = TOP - np.float32(1.0)
    fav2 = np.array([[1.0e-7, 0.999]] * 3, np.float32)
    out, _ = _check_sample(y, save, 0, 1.3, 2, 1.0, 1.0, noise=fav2, skip_none=True, label="tie at the top_k boundary")
    assert out["next"].tolist() == [lo] * 3
    fav3 = np.array([[1.0e-7, 1.0e-7, 0.999]] * 3, np.float32)
    out, _ = _check_sample(y, save, 0, 1.3, 3, 1.0, 1.0, noise=fav3, skip_none=True, label="tie inside top_k")
    assert out["next"].tolist() == [hi] * 3


# ------------------------------------------------------------------------------------------------ sample_topk_topp, its own generator
@pytest.mark.parametrize("case", R.sampler_seeded_cases(), ids=lambda c: f"{c[0]:x}-{c[1]}")
def test_sampler_with_its_own_generator(case):
    seed, n_saved = case
    c = R.SEEDED
    x, save = R.sampler_seeded_inputs(case)
    out, want = _check_sample(x, save, n_saved, c["temperature"], c["top_k"], c["top_p"], c["rp"], seed=seed, label=f"seed {seed:x} n_saved {n_saved}")
    again = _sample(x, save, n_saved, c["temperature"], c["top_k"], c["top_p"], c["rp"], seed=seed)
    assert again["next"].tolist() == out["next"].tolist()
    if n_saved > R.SEEDED_LD_SAVE:
        # the history is clamped to the table, the generator step is not: a reference driven by the clamped counter picks other ids
        clamped, _, _ = R.sample_topk_topp(x, save, R.SEEDED_LD_SAVE, c["temperature"], c["top_k"], c["top_p"], c["rp"], seed=seed)
        assert clamped.tolist() != want.tolist() and out["next"].tolist() != clamped.tolist()


def test_sampler_generator_is_uniform_over_four_equal_logits():
    """4096 rows of four equal top logits, top_p = 1: each id is drawn with p = 1 / 4. Binomial(4096, 1 / 4): mean 1024, sigma 27.7; 5 sigma = 139."""
    c = R.UNIFORM
    x, save = R.sampler_uniform_inputs()
    out = _sample(x, save, c["n_saved"], 1.0, 4, 1.0, 1.0, seed=c["seed"])
    counts = [int((out["next"] == i).sum()) for i in c["ids"]]
    print("sampler distribution over four equal logits:", counts)
    assert sum(counts) == c["rows"] and all(abs(k - 1024) <= 139 for k in counts), counts
    m = c["checked"]
    want, margin, _ = R.sample_topk_topp(x[:m], save[:m], c["n_saved"], 1.0, 4, 1.0, 1.0, seed=c["seed"])
    ok = R.sampler_decided(margin, 4)
    assert 1.0 - ok.mean() <= R.SKIP_CAP, margin
    assert out["next"][:m][ok].tolist() == want[ok].tolist()


# ------------------------------------------------------------------------------------------------ the head over several steps
@pytest.mark.parametrize("name", list(R.head_steps_cases()))
def test_head_steps(name):
    """TokenHead (csrc/decode_head.h), the one head sequence of the Whisper and Qwen3-ASR sessions, over nine steps on the same three rows (257 valid columns
    in rows of 384, pads at +1e30, a history table of 16): restart, then per step apply-penalty, sampler or arg-max, append, counter + 1, consumed.
    tests/test_token_heads_ref_cpu.py shows on these inputs that a head which skips any of it gives other picks."""
    c = R.HEAD_STEPS
    x, _, _ = R.head_steps_inputs()
    kw = R.head_steps_cases()[name]
    want, save, n, decided = R.head_steps(x, c["steps"], c["ld_save"], **kw)
    out = sub("_probe").head_steps(x, c["steps"], c["ld_save"], **kw)
    print(f"head steps, {name}: picks\n{out['picks'].T}\ncounter {out['n_saved']}")
    assert out["n_saved"] == n
    if "sampler" not in kw:
        assert np.array_equal(out["picks"], want) and np.array_equal(out["save_ids"], save)
        return
    ok = np.logical_and.accumulate(decided, axis=0)                 # a row's later steps read its earlier picks
    skipped = 1.0 - ok.mean()
    print(f"head steps, {name}: skipped {skipped:.3f} of {ok.size} picks")
    assert skipped <= R.SKIP_CAP
    assert out["picks"][ok].tolist() == want[ok].tolist()
    assert np.array_equal(out["save_ids"][:, :n], out["picks"].T) and (out["save_ids"][:, n:] == 0).all()


# ------------------------------------------------------------------------------------------------ no_speech_prob
@pytest.mark.parametrize("n", R.LOOP_WIDTHS)
def test_no_speech_prob(n):
    for nid in sorted({n - 1, n // 2}):                             # n - 1: the row's last float4
        for target in (1e-6, 0.5, 1.0):
            x, pen, sup = R.no_speech_inputs(n, nid, target)
            want, d = R.no_speech_prob(x, pen, nid)
            out = _head("no_speech_prob", x, vec=pen, no_speech_id=nid)
            tol = R.no_speech_budget(n, want, d)
            err = np.abs(out["prob"].astype(np.float64) - want)
            print(f"no_speech n={n} id={nid} p~{target:g}: prob {want[0]:.6e}, worst relative error {float((err / want).max()):.3e}, "
                  f"{float((err / tol).max()):.3f} of the budget ({float((tol / want).min()):.3e} relative)")
            assert (err <= tol).all(), (n, nid, target, err / tol)
            assert np.array_equal(out["logits"][:, :n], x) and _pad_ok(out, n)
            assert (np.abs(np.log(want / target)) < 0.01).all() if target < 1 else (want > 1 - 1e-6).all()
