"""The Whisper encoder and decoder layers (`WhSession::encode`, `enqueue_step`) against the float64 reference of their stages (tests/whisper_layers_ref.py),
per utterance and per stage, on the planted checkpoint.

Sessions run eager with taps on. Every stage is compared on the session's OWN tapped rows of the stage before:

    enc{i}    enc_layer on its `stem` / `enc{i-1}` rows                                    stat(tap - exact) <= 3 x E_round
    enc_out   the f32 LayerNorm of its `enc{last}` rows                                    <= LN_F32 (below)
    cross     final LayerNorm + cross-K/V projection of its `enc{last}` rows               <= 3 x E_round (E_round holds the slab's own bf16 rounding)
    dec_in    embedding (the arena's, bf16 in a bf16 session) + position row in f32        bit for bit, pad slots (id 0, position 0) included
    dec{l}    dec_layer on the rows that entered layer l at this and at every earlier step (self-K/V recomputed from them), its own `cross` rows
    logits    head on the last row of every sequence of its last `dec{l}`

with E_round = stat(exact - rounded) from the two references alone (the rounding set of the form that runs: R.dec_roundings), both statistics. The f32 session's
E_round is the larger of three float32 evaluations in other summation orders (R.F32_FORMS). MARGIN is the project's 3.0.

LN_F32: the `enc_out` tap is one f32 LayerNorm. Its statistics are two sums over d terms; in any order their relative error stays below d x eps, and the output
takes three more roundings: |error| <= (d + 3) x eps32 x |output| <= 2^-15 x max |output| at d = 256. No measurement went into it.

Measured stat / E_round on an MI355X: DESIGN.md section 7 ("Whisper encoder and decoder layers, per stage"); the largest are 1.21 / 1.56 (bf16, step `dec{l}` at
B = 17 and 33) and 1.89 / 2.82 (f32, `enc0`). The planted mistakes: every mutation of the exact functions is applied on the reference side and the
comparison with the session's rows must FAIL at that stage (test_planted_mistakes_are_caught); that they move the stage beyond 2 x MARGIN x E_round on the CPU is in
tests/test_whisper_layers_ref_cpu.py.

NOT covered: the low-bit sessions, beam rows, the mel front end and conv stem, the token heads (each has its own reference test); pad-slot rows of a left-padded
prefill behind `dec_in` (they hold nothing defined and no live row reads them)."""
import os

import numpy as np
import pytest

import whisper_layers_ref as R
from conftest import sub
from whisper_layers_ref import D256, MARGIN, TINY, stat

pytestmark = pytest.mark.gpu

BF16, F32 = 0, 1
SWITCHES = ("ASR_DECODE_GEMM", "ASR_KV_PAGED", "ASR_KV_PAGE_SHUFFLE", "ASR_DECODE_ATTN_WAVE", "ASR_DECODE_ATTN_ONLINE")
FORMS = {"default": {}, "no_decode_gemm": {"ASR_DECODE_GEMM": "0"}, "contiguous_kv": {"ASR_KV_PAGED": "0"}, "shuffled_pages": {"ASR_KV_PAGE_SHUFFLE": "1"},
         "general_attn": {"ASR_DECODE_ATTN_WAVE": "0"}, "two_pass_attn": {"ASR_DECODE_ATTN_WAVE": "0", "ASR_DECODE_ATTN_ONLINE": "0"}}
_sessions = {}


def _session(cfg_name, prec, form="default"):
    """One session per (geometry, precision, form): the switches are read at session creation."""
    key = (cfg_name, prec, form)
    if key not in _sessions:
        cfg, ck, sup, beg, L = R.setup(cfg_name)
        old = {k: os.environ.pop(k, None) for k in SWITCHES}
        os.environ.update(FORMS[form])
        try:
            sess = sub("engine").WhisperSession.from_checkpoint(cfg, ck, precision=prec, suppress_tokens=sup, begin_suppress_tokens=beg)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
        sess.taps(True)
        sess.profile(True)
        _sessions[key] = sess
    return R.setup(cfg_name) + (_sessions[key],)


def _tap64(sess, name):
    return sess.tap(name).astype(np.float64)


def gpu_trace(sess, cfg, lengths, plan, prec=BF16):
    """Encode, prefill and step with the plan's ids fed from the host; every tap of every step."""
    tr = R.Trace(cfg, lengths)
    sess.encode(R.batch_audios(cfg, lengths))
    for nm in ["stem", "enc_out"] + [f"enc{i}" for i in range(cfg.n_enc_layers)]:
        tr.enc[nm] = _tap64(sess, nm)
    tr.cross = R.cross_slabs(sess.tap("cross", dtype=np.float32 if prec == F32 else np.uint16), cfg, f32=prec == F32)
    tr.launches = []
    for t, (ids, pads) in enumerate(plan or []):
        sess.profile_reset()
        if t == 0 and pads is not None:
            tr.pads = np.asarray(pads, np.int64)
            sess.prefill_prompts(R.prompts_of(plan))
        elif t == 0:
            sess.prefill(ids)
        else:
            sess.decode(ids[:, 0], want_logits=True)
        tr.launches.append({k: v["launches"] for k, v in sess.profile_read().items()})
        tr.steps.append({"ids": ids, "dec_in": sess.tap("dec_in"), "dec": [_tap64(sess, f"dec{l}") for l in range(cfg.n_dec_layers)], "logits": _tap64(sess, "logits")})
    return tr


def _roundings(cfg, prec, R_rows, prompt, form):
    """(decoder layer, head) rounding sets whose stat(exact - rounded) is the budget."""
    if prec == F32:
        return R.F32_FORMS, R.F32_FORMS
    return [R.dec_roundings(cfg, R_rows, prompt, decode_gemm=form != "no_decode_gemm")], [R.HEAD_ROUNDINGS]


class Worst:
    def __init__(self, what):
        self.what, self.by_stage, self.fails = what, {}, []

    def judge(self, stage, key, got, exact, e_round):
        ok, ratios = R.within(got - exact, e_round)
        w = self.by_stage.setdefault(stage, [0.0, 0.0])
        w[0], w[1] = max(w[0], ratios[0]), max(w[1], ratios[1])
        if not ok:
            self.fails.append(f"{stage} {key}: {ratios[0]:.2f} {ratios[1]:.2f} x E_round ({e_round[0]:.3g}, {e_round[1]:.3g})")
        return ok

    def report(self):
        for stage, (a, b) in self.by_stage.items():
            print(f"RATIO {self.what} {stage}: rms {a:.2f} max {b:.2f}")
        assert not self.fails, self.fails[:12]


def check_encoder(L, cfg, tr, prec, worst):
    enc_rnd = R.F32_FORMS if prec == F32 else [R.ENC_ROUNDINGS]
    cross_rnd = R.F32_FORMS if prec == F32 else [R.CROSS_ROUNDINGS]
    last = f"enc{cfg.n_enc_layers - 1}"
    for u, (r0, T) in enumerate(tr.rows):
        for i in range(cfg.n_enc_layers):
            exact = R.enc_stage(L, tr, i, u)
            worst.judge(f"enc{i}", f"T={T}", tr.enc[f"enc{i}"][r0:r0 + T], exact, R.budget(exact, lambda rnd: R.enc_stage(L, tr, i, u, rnd), enc_rnd))
        exact = L.enc_out(tr.enc[last][r0:r0 + T])
        err = float(np.abs(tr.enc["enc_out"][r0:r0 + T] - exact).max())
        bound = (cfg.d_model + 3) * 2.0 ** -24 * float(np.abs(exact).max())
        w = worst.by_stage.setdefault("enc_out (x LN_F32)", [0.0, 0.0])
        w[1] = max(w[1], err / bound)
        if err > bound:
            worst.fails.append(f"enc_out T={T}: {err:.3g} > {bound:.3g}")
        exact = R.cross_stage(L, tr, u)
        worst.judge("cross", f"T={T}", R.cross_got(tr, u), exact, R.budget(exact, lambda rnd: R.cross_stage(L, tr, u, rnd), cross_rnd))


def expected_dec_in(cfg, ck, tr, t, prec, mut=None):
    """Embedding row (as the arena stores it) + position row, one f32 addition."""
    emb = np.asarray(ck["model.decoder.embed_tokens.weight"], np.float32)
    if prec == BF16:
        emb = R.bf16(R.torch.from_numpy(emb)).numpy().astype(np.float32)
    pos = np.asarray(ck["model.decoder.embed_positions.weight"], np.float32)
    ids = tr.steps[t]["ids"]
    B, n = ids.shape
    at = np.stack([R.positions_of(tr.hist(t), n, int(tr.pads[b]), mut) for b in range(B)]).reshape(-1)
    return emb[ids.reshape(-1)] + pos[at]


def check_decoder(L, cfg, ck, tr, prec, form, worst, prompts):
    for t, step in enumerate(tr.steps):
        B, n = step["ids"].shape
        assert np.array_equal(step["dec_in"], expected_dec_in(cfg, ck, tr, t, prec)), f"dec_in differs at step {t}"
        dec_rnd, head_rnd = _roundings(cfg, prec, B * n, prompts and t == 0, form)
        tag = "prefill" if t == 0 else "step"
        for l in range(cfg.n_dec_layers):
            for b in range(B):
                exact = R.dec_stage(L, tr, t, l, b)
                worst.judge(f"{tag} dec{l}", f"step {t} seq {b}", R.dec_got(tr, t, l, b), exact, R.budget(exact, lambda rnd: R.dec_stage(L, tr, t, l, b, rnd), dec_rnd))
        exact = R.head_stage(L, tr, t)[0]
        rounded = [R.head_stage(L, tr, t, rnd)[0] for rnd in head_rnd]
        for b in range(B):
            e = [stat(exact[b:b + 1] - r[b:b + 1]) for r in rounded]
            worst.judge(f"{tag} logits", f"step {t} seq {b}", step["logits"][b:b + 1], exact[b:b + 1], (max(x[0] for x in e), max(x[1] for x in e)))


def assert_form(cfg, tr, prec, form):
    """Which form of enqueue_step ran, from the profile's launch counts: a `dec_layernorm` launch only where the table in whisper_layers_ref.py has a separate
    LayerNorm (three per layer), none under the decode GEMM or the LayerNorm prologue of the skinny GEMM."""
    Ld = cfg.n_dec_layers
    for t, step in enumerate(tr.steps):
        B, n = step["ids"].shape
        rows = B * n
        dgm = prec == BF16 and form != "no_decode_gemm" and rows <= 64 and cfg.d_model % 256 == 0 and cfg.d_ffn % 256 == 0
        fused = prec == BF16 and rows <= 32 and cfg.d_model % 256 == 0           # (every N / 16 of these geometries is <= 256)
        want = 0 if dgm or fused else 3 * Ld
        got = tr.launches[t].get("dec_layernorm", 0)
        assert got == want, (f"step {t}: {rows} rows", got, want, tr.launches[t])
        assert tr.launches[t].get("dec_gemm", 0) == 6 * Ld and tr.launches[t].get("dec_self_attn", 0) == Ld and tr.launches[t].get("dec_cross_attn", 0) == Ld, tr.launches[t]


@pytest.mark.parametrize("case", ["enc_le128", "enc_le256", "enc_gt256", "enc_tiny"])
def test_bf16_encoder_stages(case):
    cfg_name, lengths, _ = R.MISTAKE_CASES[case]
    cfg, ck, sup, beg, L, sess = _session(cfg_name, BF16)
    tr = gpu_trace(sess, cfg, lengths, None)
    worst = Worst(f"bf16 {case}")
    check_encoder(L, cfg, tr, BF16, worst)
    worst.report()


@pytest.mark.parametrize("B", R.DEC_BATCHES)
def test_bf16_decoder_stages_by_row_count(B):
    cfg, ck, sup, beg, L, sess = _session(D256, BF16)
    lengths = R.dec_lengths(B)
    tr = gpu_trace(sess, cfg, lengths, R.decode_plan(cfg, lengths))
    print("launches", tr.launches[0], tr.launches[1], sub("_probe").gemm_counts())
    assert_form(cfg, tr, BF16, "default")
    worst = Worst(f"bf16 B={B}")
    check_decoder(L, cfg, ck, tr, BF16, "default", worst, False)
    worst.report()


@pytest.mark.parametrize("cfg_name,prec", [(D256, BF16), (D256, F32), (TINY, BF16)], ids=["d256_bf16", "d256_f32", "tiny_bf16"])
def test_left_padded_prompts_then_steps(cfg_name, prec):
    cfg, ck, sup, beg, L, sess = _session(cfg_name, prec)
    lengths = R.dec_lengths(3) if cfg_name == D256 else R.TINY_LENGTHS
    tr = gpu_trace(sess, cfg, lengths, R.prompt_plan(cfg, lengths), prec)
    assert_form(cfg, tr, prec, "default")
    worst = Worst(f"prompts {cfg_name} {'f32' if prec else 'bf16'}")
    check_decoder(L, cfg, ck, tr, prec, "default", worst, True)
    worst.report()


def test_tiny_takes_the_plain_path():
    cfg, ck, sup, beg, L, sess = _session(TINY, BF16)
    tr = gpu_trace(sess, cfg, R.TINY_LENGTHS, R.decode_plan(cfg, R.TINY_LENGTHS))
    assert_form(cfg, tr, BF16, "default")
    worst = Worst("bf16 tiny")
    check_decoder(L, cfg, ck, tr, BF16, "default", worst, False)
    worst.report()


@pytest.mark.parametrize("case", ["enc_gt256", "enc_le128", "dec_b3"])
def test_f32_session(case):
    cfg_name, lengths, kind = R.MISTAKE_CASES[case]
    cfg, ck, sup, beg, L, sess = _session(cfg_name, F32)
    tr = gpu_trace(sess, cfg, lengths, R.decode_plan(cfg, lengths) if kind else None, F32)
    worst = Worst(f"f32 {case}")
    if kind:
        assert_form(cfg, tr, F32, "default")
        check_decoder(L, cfg, ck, tr, F32, "default", worst, False)
    else:
        check_encoder(L, cfg, tr, F32, worst)
    worst.report()


@pytest.mark.parametrize("form", [f for f in FORMS if f != "default"])
def test_every_decoder_form_is_held_to_the_reference(form):
    """B = 9: a 36-row prefill (decode GEMM with the tiled FFN-2) and 9-row steps (decode GEMM / LayerNorm prologue, wave or general attention)."""
    cfg, ck, sup, beg, L, sess = _session(D256, BF16, form)
    lengths = R.dec_lengths(9)
    tr = gpu_trace(sess, cfg, lengths, R.decode_plan(cfg, lengths))
    assert_form(cfg, tr, BF16, form)
    worst = Worst(f"bf16 form {form}")
    check_decoder(L, cfg, ck, tr, BF16, form, worst, False)
    worst.report()


def test_slab_rows_behind_the_utterances_do_not_reach_the_decoder():
    """The batch, a larger batch of other lengths (it leaves its own data in every row of the slab, under another Mpad), the batch again: every decoder tap of the
    third run equals the first run's bit for bit, so neither the rows T .. round_up(T, 16) nor the rows behind the last utterance reach a live row."""
    cfg, ck, sup, beg, L, sess = _session(D256, BF16)
    lengths = R.dec_lengths(3)
    plan = R.decode_plan(cfg, lengths)
    first = gpu_trace(sess, cfg, lengths, plan)
    other = R.ENC_BATCHES["le256"] + R.ENC_BATCHES["gt256"]
    gpu_trace(sess, cfg, other, R.decode_plan(cfg, other, 4, 1))
    again = gpu_trace(sess, cfg, lengths, plan)
    for u, (r0, T) in enumerate(first.rows):
        assert np.array_equal(R.cross_got(first, u), R.cross_got(again, u))
    for a, b in zip(first.steps, again.steps):
        assert np.array_equal(a["logits"], b["logits"])
        for x, y in zip(a["dec"], b["dec"]):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("case", sorted(R.MISTAKE_CASES))
def test_planted_mistakes_are_caught(case):
    """Every mutation on the reference side: the comparison of the session's rows with the mutated reference must fail (beyond MARGIN x E_round in a component)
    at the stage the mutation sits in, wherever the mutation applies."""
    cfg_name, lengths, kind = R.MISTAKE_CASES[case]
    cfg, ck, sup, beg, L, sess = _session(cfg_name, BF16)
    plan = {"steps": R.decode_plan, "prompts": R.prompt_plan, None: lambda *a: None}[kind](cfg, lengths)
    tr = gpu_trace(sess, cfg, lengths, plan)
    caught, missed = {}, []

    def judge(mut, key, got, exact, mutated, e_round):
        if mutated is None or not R.relied_on(mut, case):
            return
        ok, ratios = R.within(got - mutated, e_round)
        caught[mut] = min(caught.get(mut, np.inf), max(ratios))
        if ok:
            missed.append(f"{mut} {key}: {ratios[0]:.2f} {ratios[1]:.2f}")

    if kind is None:
        for i in range(cfg.n_enc_layers):
            for u, (r0, T) in enumerate(tr.rows):
                exact = R.enc_stage(L, tr, i, u)
                e_round = R.budget(exact, lambda rnd: R.enc_stage(L, tr, i, u, rnd), [R.ENC_ROUNDINGS])
                for mut in R.ENC_MUTATIONS:
                    judge(mut, f"enc{i} T={T}", tr.enc[f"enc{i}"][r0:r0 + T], exact, R.enc_stage(L, tr, i, u, mut=mut), e_round)
    else:
        for t, step in enumerate(tr.steps):
            B, n = step["ids"].shape
            rnd = R.dec_roundings(cfg, B * n, kind == "prompts" and t == 0)
            for mut in R.EMBED_MUTATIONS:
                if R.relied_on(mut, case) and not (mut == "pad_pos" and t > 0):
                    caught[mut] = 1.0
                    if np.array_equal(step["dec_in"], expected_dec_in(cfg, ck, tr, t, BF16, mut)):
                        missed.append(f"{mut} step {t}")
            for l in range(cfg.n_dec_layers):
                for b in range(B):
                    exact = R.dec_stage(L, tr, t, l, b)
                    e_round = R.budget(exact, lambda r_: R.dec_stage(L, tr, t, l, b, r_), [rnd])
                    for mut in R.SELF_MUTATIONS + R.CROSSATT_MUTATIONS:
                        judge(mut, f"step {t} dec{l} seq {b}", R.dec_got(tr, t, l, b), exact, R.dec_stage(L, tr, t, l, b, mut=mut), e_round)
            exact = R.head_stage(L, tr, t)[0]
            rounded = R.head_stage(L, tr, t, R.HEAD_ROUNDINGS)[0]
            bad, rows = R.head_stage(L, tr, t, mut="row_n_minus_2")
            for b in np.nonzero(rows)[0]:
                judge("row_n_minus_2", f"step {t} seq {b}", step["logits"][b:b + 1], exact[b:b + 1], bad[b:b + 1], stat(exact[b:b + 1] - rounded[b:b + 1]))
    for mut, low in sorted(caught.items()):
        print(f"CAUGHT {case} {mut}: the session's rows are at least {low:.1f} x E_round from the mutated reference")
    assert not missed, missed[:12]
    expected = R.ENC_MUTATIONS if kind is None else R.SELF_MUTATIONS + R.CROSSATT_MUTATIONS + R.HEAD_MUTATIONS + R.EMBED_MUTATIONS
    for mut in expected:
        assert not R.relied_on(mut, case) or mut in caught, f"{mut} never applied in {case}"
