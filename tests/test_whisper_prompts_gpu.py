"""asr_whisper_prefill_prompts: text prompts of ragged / long lengths (left-padded on the device, one shared slot counter) against the oracle,
which takes a prompt of any length per utterance (WhisperOracle.decoder / .greedy), and its composition with generate, beam search, token
scores and word-timestamp capture."""
import os

import numpy as np
import pytest

from conftest import sub
from helpers import golden_cases, load_golden
from oracle.whisper_oracle import WhisperOracle
from test_oracle_whisper import unit_audio, whisper_setup
from test_whisper_beam_gpu import CLIPS
from whisper_beam_ref import as_lists, beam_reference

pytestmark = pytest.mark.gpu

BF16, F32, FP8W = 0, 1, 2
LOGIT_TOL_F32 = 1e-3                             # the project's f32 logits bar
MARGIN = 2e-3


def _session(cfg_name, prec, env=None):
    cfg, ck, sup, beg = whisper_setup(cfg_name)
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        sess = sub("engine").WhisperSession.from_checkpoint(cfg, ck, precision=prec, suppress_tokens=sup, begin_suppress_tokens=beg)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return cfg, ck, sup, beg, sess


def _head(cfg):
    return [cfg.sot_id, cfg.first_language_id, cfg.transcribe_id, cfg.no_timestamps_id]


def _prompt(cfg, rng, length):
    """`length` ids ending in the decoding head; random text ids in front, <|startofprev|> first where there is room for it."""
    head = _head(cfg)
    if length <= 4:
        return np.array(head[-length:], np.int32)
    text = rng.integers(0, cfg.eot_id, length - 5).tolist()
    return np.array([cfg.sot_prev_id] + text + head, np.int32)


def _teacher_forced(sess, audios, prompts, ref, steps):
    """Prefill logits + `steps` decode steps fed from the host with the oracle's ids -> [B][steps + 1][V]."""
    sess.encode(audios)
    _, logits = sess.prefill_prompts(prompts)
    out = [logits]
    for t in range(steps):
        _, lg = sess.decode(np.array([r[t] for r in ref["token_ids"]], np.int32), want_logits=True)
        out.append(lg)
    return np.stack(out, 1)


def _assert_parity(got, ref, tol, what):
    for b, want in enumerate(ref["logits"]):
        err = float(np.abs(got[b] - want).max())
        print(f"{what} sequence {b}: max |logits - oracle| = {err:.3g}")
        assert err < tol, (what, b, err)
        s = np.sort(want, axis=1)
        safe = s[:, -1] - s[:, -2] > MARGIN
        assert np.array_equal(np.argmax(got[b], axis=1)[safe], np.argmax(want, axis=1)[safe]), (what, b)


@pytest.mark.parametrize("env", [None, {"ASR_KV_PAGED": "0"}, {"ASR_KV_PAGE_SHUFFLE": "1"}], ids=["paged", "contig", "shuffled"])
def test_f32_tiny_ragged_prompts_match_the_oracle(env):
    cfg, ck, sup, beg, sess = _session("whisper_tiny_test", F32, env)
    orc = WhisperOracle(cfg, ck, sup, beg)
    rng = np.random.default_rng(11)
    audios = [unit_audio(s, n) for s, n in CLIPS["whisper_tiny_test"][0][:4]]       # 0.8 .. 2 s
    prompts = [_prompt(cfg, rng, L) for L in (4, 9, 23, 40)]
    steps = 6
    ref = orc.greedy(audios, [p.tolist() for p in prompts], steps + 1)
    _assert_parity(_teacher_forced(sess, audios, prompts, ref, steps), ref, LOGIT_TOL_F32, "tiny")
    # reversed clip order: every sequence gets another pad
    rev = dict(token_ids=ref["token_ids"][::-1], logits=ref["logits"][::-1])
    _assert_parity(_teacher_forced(sess, audios[::-1], prompts[::-1], rev, steps), rev, LOGIT_TOL_F32, "tiny reversed")


def test_f32_mid_full_size_prompt():
    cfg, ck, sup, beg, sess = _session("whisper_mid_test", F32)
    orc = WhisperOracle(cfg, ck, sup, beg)
    rng = np.random.default_rng(12)
    audios = [unit_audio(s, n) for s, n in CLIPS["whisper_mid_test"][0][:2]]
    prompts = [_prompt(cfg, rng, L) for L in (228, 5)]
    ref = orc.greedy(audios, [p.tolist() for p in prompts], 4)
    _assert_parity(_teacher_forced(sess, audios, prompts, ref, 3), ref, LOGIT_TOL_F32, "mid")


def test_bf16_d256_no_worse_than_twice_the_parent_chain():
    """Uniform prompt of 24 ids, B = 3: prefill_prompts against the chain the parent code offers for the same prompt (prefill of the first 8 ids
    + 16 host-fed decode steps), both measured against the f32 oracle in this run; the new path may be at most 2x the chain's distance (another
    summation order and bf16 probabilities, not another precision class). Then a ragged batch under the same measured bound.
    Measured on an MI355X: see DESIGN.md section 4.6."""
    cfg, ck, sup, beg, sess = _session("whisper_d256_test", BF16)
    orc = WhisperOracle(cfg, ck, sup, beg)
    rng = np.random.default_rng(13)
    audios = [unit_audio(900 + i, n) for i, n in enumerate((20000, 36000, 11200))]
    prompts = [_prompt(cfg, rng, 24) for _ in range(3)]
    ref = orc.greedy(audios, [p.tolist() for p in prompts], 1)
    sess.encode(audios)
    ids = np.stack(prompts)
    sess.prefill(ids[:, :8], want_logits=False)
    for t in range(8, 24):
        _, chain = sess.decode(ids[:, t], want_logits=True)
    _, new = sess.prefill_prompts(prompts)
    want = np.stack([r[0] for r in ref["logits"]])
    d_chain, d_new = float(np.abs(chain - want).max()), float(np.abs(new - want).max())
    print(f"bf16 d256, 24-id prompt: max |logits - oracle| parent chain {d_chain:.4f}, prefill_prompts {d_new:.4f}")
    assert d_new <= 2 * d_chain, (d_new, d_chain)
    ragged = [p[-L:] for p, L in zip(prompts, (24, 7, 12))]
    ref_r = orc.greedy(audios, [p.tolist() for p in ragged], 1)
    _, got = sess.prefill_prompts(ragged)
    d_ragged = float(np.abs(got - np.stack([r[0] for r in ref_r["logits"]])).max())
    print(f"bf16 d256, ragged (24, 7, 12): max |logits - oracle| {d_ragged:.4f}")
    assert d_ragged <= 2 * d_chain, (d_ragged, d_chain)


def _log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def test_composition_generate_beam_scores_and_capture():
    cfg, ck, sup, beg, sess = _session("whisper_tiny_test", F32)
    orc = WhisperOracle(cfg, ck, sup, beg)
    rng = np.random.default_rng(14)
    clips, max_new = CLIPS["whisper_tiny_test"]
    audios = [unit_audio(s, n) for s, n in clips[:3]]
    prompts = [_prompt(cfg, rng, L) for L in (4, 17, 30)]
    B, n = 3, 8
    # generate == the step-by-step loop; token scores == log-soft-max of the returned logits
    sess.set_token_scores(True)
    sess.encode(audios)
    nxt, logits = sess.prefill_prompts(prompts)
    bias = np.zeros(cfg.vocab)
    bias[list(beg)] = -np.inf
    ids, want_scores = [nxt.copy()], [_log_softmax(logits + bias)[np.arange(B), nxt]]
    for _ in range(n - 1):
        nxt, lg = sess.decode(None, want_logits=True)
        ids.append(nxt.copy())
        want_scores.append(_log_softmax(lg)[np.arange(B), nxt])
    scores = sess.token_scores()
    assert scores.shape == (B, n) and np.abs(scores - np.stack(want_scores, 1)).max() < 1e-4
    sess.set_token_scores(False)
    sess.prefill_prompts(prompts, want_logits=False)
    gen = sess.generate(n, eos_id=-1)
    for b in range(B):
        assert gen[b].tolist() == np.stack(ids, 1)[b].tolist(), b
    # beam search == the restatement driven by the oracle with the ragged prompts
    width = 3
    refs, margins = [], []
    for a, p in zip(audios, prompts):
        m = []
        refs.append(beam_reference(orc, a, p.tolist(), width, max_new, margins=m))
        margins.append(min(m))
    sess.prefill_prompts(prompts, want_logits=False)
    got = sess.beam_search(width, max_new, -1)
    ok = [b for b in range(B) if margins[b] > 10 * LOGIT_TOL_F32]
    assert ok, margins
    for b in ok:
        t_ref, s_ref = as_lists(refs[b])
        t_got, s_got = as_lists(got[b])
        assert t_got == t_ref, b
        assert np.abs(s_got - s_ref).max() < LOGIT_TOL_F32 * max_new, b
    after = sess.generate(n, eos_id=-1)          # the search leaves the prefill's greedy state
    for b in range(B):
        assert after[b].tolist() == gen[b].tolist(), b
    # word-timestamp capture: the prefill's last slot is row 0, every step adds one
    sess.set_word_timestamps(True, [(1, 0), (1, 1)], max_rows=16)
    sess.prefill_prompts(prompts, want_logits=False)
    steps = 5
    for _ in range(steps):
        sess.decode(None, sync=False)
    for b in range(B):
        shape = sess.align_read_shape(0, b)
        assert shape == (2, steps + 1, cfg.n_enc_pos(audios[b].size)), shape
        assert np.isfinite(sess.align_read(0, b)).all()
    alone = []
    for b in range(B):                           # each sequence alone has no pad (row 0 = its last prompt slot): its captured rows are the batch's
        sess.encode([audios[b]])
        sess.prefill_prompts([prompts[b]], want_logits=False)
        for _ in range(steps):
            sess.decode(None, sync=False)
        alone.append(sess.align_read(0, 0))
    sess.encode(audios)
    sess.prefill_prompts(prompts, want_logits=False)
    for _ in range(steps):
        sess.decode(None, sync=False)
    for b in range(B):
        assert np.abs(sess.align_read(0, b) - alone[b]).max() < LOGIT_TOL_F32, b
    sess.set_word_timestamps(False)


def test_uniform_short_prompts_forward_to_prefill():
    cfg, ck, sup, beg, sess = _session("whisper_tiny_test", F32)
    audios = [unit_audio(31, 16000), unit_audio(32, 9600)]
    head = np.array([_head(cfg)] * 2, np.int32)
    sess.encode(audios)
    nxt0, lg0 = sess.prefill(head)
    nxt1, lg1 = sess.prefill_prompts([head[0], head[1]])
    assert np.array_equal(nxt0, nxt1) and np.array_equal(lg0.view(np.uint32), lg1.view(np.uint32))


def test_errors():
    cfg, ck, sup, beg, sess = _session("whisper_tiny_test", F32)
    lib, eng = sub("_lib"), sub("engine")
    rng = np.random.default_rng(15)
    audios = [unit_audio(31, 16000), unit_audio(32, 9600)]
    sess.encode(audios)
    head = np.array(_head(cfg), np.int32)
    with pytest.raises(lib.AsrError, match="at least one id"):
        sess.prefill_prompts([head, np.zeros(0, np.int32)])
    with pytest.raises(lib.AsrError, match="max_target_positions"):
        sess.prefill_prompts([head, _prompt(cfg, rng, cfg.max_target_positions + 1)])
    with pytest.raises(ValueError):
        sess.prefill_prompts([head])
    # offsets that do not ascend: the C entry itself
    ids = np.concatenate([head, head]).astype(np.int32)
    offs = np.array([4, 8, 4], np.int32)
    ip = lambda a: a.ctypes.data_as(eng.C.POINTER(eng.C.c_int32))
    assert lib.load().asr_whisper_prefill_prompts(sess._h, ip(ids), ip(offs), None, None) != 0
    assert "ascend" in lib.load().asr_last_error().decode()
    # the longest prompt bounds the whole batch
    sess.prefill_prompts([head, _prompt(cfg, rng, 40)], want_logits=False)
    with pytest.raises(lib.AsrError, match="max_target_positions"):
        sess.beam_search(2, cfg.max_target_positions - 40 + 1, -1)
    sess.beam_search(2, cfg.max_target_positions - 40, -1)
    out = sess.generate(cfg.max_target_positions, eos_id=-1)         # generate stops at the limit
    assert all(len(t) == cfg.max_target_positions - 40 + 1 for t in out)
    # low-bit sessions: equal lengths of at most 8 ids only
    cfg8, _, _, _, sess8 = _session("whisper_d256_test", FP8W)
    sess8.encode(audios)
    head8 = np.array(_head(cfg8), np.int32)
    sess8.prefill_prompts([head8, head8], want_logits=False)
    with pytest.raises(lib.AsrError, match="F32 or BF16"):
        sess8.prefill_prompts([head8, head8[1:]])
    with pytest.raises(lib.AsrError, match="F32 or BF16"):
        sess8.prefill_prompts([_prompt(cfg8, rng, 9)] * 2)


def test_plain_prefill_after_prompts_gives_the_golden_logits():
    """Nothing stale from the left pads: after a ragged prefill the session's plain prefill / decode path is the golden one again."""
    g = load_golden("whisper_tiny")
    cfg, ck, sup, beg, sess = _session(str(g["cfg_name"]), F32)
    cases = [c for _, c in golden_cases(g)]
    audios = [unit_audio(c["audio_seed"], c["n_samples"]) for c in cases]
    rng = np.random.default_rng(16)
    sess.encode(audios)
    sess.prefill_prompts([_prompt(cfg, rng, 4 + 5 * b) for b in range(len(cases))], want_logits=False)
    sess.decode(None, sync=False)
    nxt, logits = sess.prefill(np.stack([c["prompt"] for c in cases]))
    got = [logits]
    for _ in range(int(g["n_new"]) - 1):
        nxt, lg = sess.decode(None, want_logits=True)
        got.append(lg)
    got = np.stack(got, 1)
    for b, c in enumerate(cases):
        lg = got[b][:, ::53] if "top1" in c else got[b]
        assert np.abs(lg - c["logits"]).max() < LOGIT_TOL_F32, b


def test_transcriber_prompts_live_and_forced_alignment():
    """WhisperTranscriber.transcribe(prompts=...) == the same prefill_prompts + generate by hand; word timestamps come from the live capture behind ragged
    prompts and from the forced pass (timestamp mode), which keeps the previous text in front of its <|notimestamps|> head."""
    wmod = sub("whisper")
    cfg, ck, sup, beg, sess = _session("whisper_tiny_test", F32)
    clips = [(unit_audio(s, n) * 32767).astype(np.int16) for s, n in ((1001, 24000), (1002, 14400), (1003, 19200))]
    rng = np.random.default_rng(17)
    prev = [rng.integers(0, cfg.eot_id, L).tolist() for L in (0, 6, 20)]
    n = 8
    kw = dict(suppress_tokens=sup, detect_language=False, no_speech_detection=False, remove_repeats=False, initial_prompt=[7, 8])
    out, _ = wmod.WhisperTranscriber(cfg, sess, **kw).transcribe(clips, max_new=n, prompts=prev)
    prompts = [np.asarray(wmod.build_prompt(cfg, _head(cfg), [7, 8] + p), np.int32) for p in prev]
    assert [o["prompt_len"] for o in out] == [len(p) for p in prompts] == [7, 13, 27]
    sess.encode([wmod.prepare_audio_input(c) for c in clips])
    sess.prefill_prompts(prompts, want_logits=False)
    want = sess.generate(n, eos_id=cfg.eot_id)
    for b in range(3):
        assert out[b]["tokens"].tolist() == want[b].tolist(), b
    pairs = [(1, 0), (1, 1)]
    live, _ = wmod.WhisperTranscriber(cfg, sess, word_timestamps=True, alignment_heads=pairs, **kw).transcribe(clips, max_new=n, prompts=prev)
    for b in range(3):
        assert live[b]["tokens"].tolist() == want[b].tolist() and len(live[b]["token_times"]) == len(want[b]), b
        starts = [s for s, _ in live[b]["token_times"]]
        assert all(x <= y for x, y in zip(starts, starts[1:])) and 0.0 <= starts[0], b
    forced, _ = wmod.WhisperTranscriber(cfg, sess, word_timestamps=True, alignment_heads=pairs, timestamps=True, **kw).transcribe(clips, max_new=n, prompts=prev)
    for b in range(3):
        assert forced[b]["prompt_len"] == len(prompts[b]) - 1 and len(forced[b]["token_times"]) == len(forced[b]["tokens"]), b
