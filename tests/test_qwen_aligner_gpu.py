"""GPU: Qwen3-ForcedAligner sessions (asr_qwen_align) against the goldens minted from the reference's classes
(tests/golden/qwen_aligner_tiny.npz) and the float oracle (tests/qwen_aligner_ref.py): f32 slot logits within 1e-3 and equal buckets,
all-positions mode, bf16 under the margin rule and on a head with trained margins, batch independence, refusals, the host aligner and the
reference's host call order through the onnxruntime-API shim."""
import json

import numpy as np
import pytest

from conftest import sub
from helpers import golden_cases, load_golden
from qwen_aligner_ref import QwenAlignerOracle
from test_qwen_aligner_cpu import aligner_setup, clip_audio

pytestmark = pytest.mark.gpu

BF16, F32, TOL = 0, 1, 1e-3


def _golden():
    g = load_golden("qwen_aligner_tiny")
    cfg, ck = aligner_setup(g)
    return g, cfg, ck, json.loads(str(g["special"])), [c for _, c in golden_cases(g)]


def _prompts(cases, special):
    pre = [[special["audio_start"]]] * len(cases)
    post = [[special["audio_end"]] + c["input_ids"].tolist() for c in cases]
    return pre, post


def _session(cfg, ck, prec):
    return sub("engine").QwenAlignerSession.from_checkpoint(cfg, ck, precision=prec)


def test_f32_slot_logits_and_buckets_match_the_reference():
    g, cfg, ck, sp, cases = _golden()
    sess = _session(cfg, ck, F32)
    pre, post = _prompts(cases, sp)
    audios = [clip_audio(c) for c in cases]
    bk, lg, ids_len = sess.align(audios, pre, post, timestamp_id=sp["timestamp"], want_logits=True)
    for i, c in enumerate(cases):
        assert ids_len[i] == c["output_ids"].size, i
        assert lg[i].shape == c["slot_logits"].shape, i
        err = np.abs(lg[i] - c["slot_logits"]).max()
        assert err < TOL, (i, err)
        assert np.array_equal(bk[i], c["output_ids"][c["slot_rows"]]), i
    # all-positions mode: the merged graph's output_ids (1, L)
    allb, _, _ = sess.align(audios, pre, post, timestamp_id=-1)
    for i, c in enumerate(cases):
        assert np.array_equal(allb[i], c["output_ids"]), (i, np.flatnonzero(allb[i] != c["output_ids"]))


def _margins(logits):
    s = np.sort(logits, axis=-1)
    return s[:, -1] - s[:, -2]


def test_bf16_buckets_follow_the_margin_rule():
    g, cfg, ck, sp, cases = _golden()
    sess = _session(cfg, ck, BF16)
    pre, post = _prompts(cases, sp)
    bk, lg, _ = sess.align([clip_audio(c) for c in cases], pre, post, timestamp_id=sp["timestamp"], want_logits=True)
    err = max(np.abs(lg[i] - c["slot_logits"]).max() for i, c in enumerate(cases))
    n_safe = n_all = 0
    for i, c in enumerate(cases):
        want = c["output_ids"][c["slot_rows"]]
        assert np.array_equal(bk[i], lg[i].argmax(-1)), i                  # the fused arg-max is the arg-max of the returned logits
        safe = _margins(c["slot_logits"]) > 2 * err
        assert np.array_equal(bk[i][safe], want[safe]), i
        n_safe += int(safe.sum()); n_all += safe.size
    print(f"bf16: max slot-logit error {err:.4f}; {n_safe} / {n_all} slots clear the margin")
    assert err < 0.25


def _prototype_head(orc, cases, sp, cfg, m=4.0, lam=1e-3):
    """A head with trained margins on these clips: both slots of word w of clip i are class k (distinct per word), the rows are the least-squares
    (ridge) solution of H W^T = m * onehot over the oracle's final-norm hidden rows of every slot."""
    H, lab = [], []
    k = 0
    for c in cases:
        h = orc.hidden(clip_audio(c), c["input_ids"]).numpy()[c["slot_rows"]]
        H.append(h)
        lab += [k + j // cfg.timestamp_tokens_per_word for j in range(h.shape[0])]
        k += h.shape[0] // cfg.timestamp_tokens_per_word
    H = np.concatenate(H).astype(np.float64)
    assert k <= cfg.classify_num
    T = np.zeros((H.shape[0], cfg.classify_num))
    T[np.arange(H.shape[0]), lab] = m
    W = (H.T @ np.linalg.solve(H @ H.T + lam * np.eye(H.shape[0]), T)).T
    return W.astype(np.float32), np.asarray(lab)


def test_bf16_every_slot_matches_on_a_head_with_trained_margins():
    g, cfg, ck, sp, cases = _golden()
    cases = [c for c in cases if c["output_ids"].size < 400]                 # 4 clips, 86 slots
    ck2 = dict(ck)
    orc0 = QwenAlignerOracle(cfg, ck, sp)
    W, lab = _prototype_head(orc0, cases, sp, cfg)
    ck2["thinker.lm_head.weight"] = W
    orc = QwenAlignerOracle(cfg, ck2, sp)
    sess = _session(cfg, ck2, BF16)
    pre, post = _prompts(cases, sp)
    bk, lg, _ = sess.align([clip_audio(c) for c in cases], pre, post, timestamp_id=sp["timestamp"], want_logits=True)
    ref = [orc.align(clip_audio(c), c["input_ids"])[1][c["slot_rows"]] for c in cases]
    err = max(np.abs(lg[i] - ref[i]).max() for i in range(len(cases)))
    margins = np.concatenate([_margins(r) for r in ref])
    print(f"prototype head: {margins.size} slots, oracle margin min {margins.min():.3f}, bf16 logit error {err:.4f}")
    assert margins.min() > 2 * err, (margins.min(), err)
    want = np.concatenate([r.argmax(-1) for r in ref])
    assert np.array_equal(want, lab)
    assert np.array_equal(np.concatenate(bk), want)


def _random_batch(cfg, sp, n, seed):
    rng = np.random.default_rng(seed)
    audios, posts = [], []
    for b in range(n):
        secs = float(rng.uniform(0.5, 10.0))
        audios.append(sub("checkpoints").synth_audio("unit", 1, int(secs * 16000), seed=500 + b)[0, 0])
        words = int(rng.integers(1, int(2.5 * secs) + 2))
        ids = [[int(t) for t in rng.integers(3, 500, int(rng.integers(1, 4)))] for _ in range(words)]
        posts.append([sp["audio_end"]] + sub("qwen_aligner").alignment_ids(ids, sp["timestamp"], 2))
    return audios, posts


def test_batch_of_64_equals_one_at_a_time():
    g, cfg, ck, sp, _ = _golden()
    sess = _session(cfg, ck, F32)
    audios, posts = _random_batch(cfg, sp, 64, 9)
    pre = [[sp["audio_start"]]]
    bk, lg, _ = sess.align(audios, pre, posts, timestamp_id=sp["timestamp"], want_logits=True)
    for b in range(64):
        one, lg1, _ = sess.align([audios[b]], pre, [posts[b]], timestamp_id=sp["timestamp"], want_logits=True)
        assert np.abs(lg[b] - lg1[0]).max() < 1e-4, b
        assert np.array_equal(bk[b], one[0]), b
    # the slot offsets follow the prompts: two per word
    assert [x.size for x in bk] == [sum(1 for t in p if t == sp["timestamp"]) for p in posts]


def test_utterance_without_slots_and_bad_prompts():
    g, cfg, ck, sp, cases = _golden()
    sess = _session(cfg, ck, F32)
    pre, post = _prompts(cases[:3], sp)
    audios = [clip_audio(c) for c in cases[:3]]
    post[1] = [sp["audio_end"], 7, 8, 9]                                      # no <timestamp> id: an empty slot range
    bk, lg, ids_len = sess.align(audios, pre, post, timestamp_id=sp["timestamp"], want_logits=True)
    assert bk[1].size == 0 and lg[1].shape == (0, cfg.classify_num) and ids_len[1] > 4
    for i in (0, 2):
        assert np.array_equal(bk[i], cases[i]["output_ids"][cases[i]["slot_rows"]]), i
    none, _, _ = sess.align(audios[1:2], pre[:1], post[1:2], timestamp_id=sp["timestamp"])
    assert none[0].size == 0
    AsrError = sub("_lib").AsrError
    long_post = [sp["audio_end"]] + [5, sp["timestamp"], sp["timestamp"]] * 400                # > max_seq_len 1024 with the clip's audio
    with pytest.raises(AsrError, match="max_seq_len"):
        sess.align(audios[:1], pre[:1], [long_post], timestamp_id=sp["timestamp"])
    with pytest.raises(AsrError, match="out of range"):
        sess.align(audios[:1], pre[:1], [[cfg.vocab + 3]], timestamp_id=sp["timestamp"])
    # the session keeps working after a refusal
    again, _, _ = sess.align(audios[:1], pre[:1], post[:1], timestamp_id=sp["timestamp"])
    assert np.array_equal(again[0], cases[0]["output_ids"][cases[0]["slot_rows"]])


def test_wrong_session_kinds_are_refused():
    g, cfg, ck, sp, cases = _golden()
    AsrError, lib = sub("_lib").AsrError, sub("_lib")
    al = _session(cfg, ck, BF16)
    audio = [clip_audio(cases[0])]
    with pytest.raises(AsrError, match="forced-aligner session"):
        al.prefill(audio, [[sp["audio_start"]]], [[sp["audio_end"]]])
    with pytest.raises(AsrError, match="no decode loop"):
        al.decode(np.zeros(1, np.int32))
    with pytest.raises(AsrError, match="no decode loop"):
        al.generate(4)
    with pytest.raises(AsrError, match="no decode loop"):
        al.beam_search(2, 4)
    asr_cfg = sub("config").qwen_asr_tiny()
    asr = sub("engine").QwenAsrSession.from_checkpoint(asr_cfg, sub("checkpoints").synth_qwen_asr_checkpoint(asr_cfg, 0), precision=BF16)
    with pytest.raises(AsrError, match="not a forced-aligner session"):
        sub("engine").QwenAlignerSession.align_packed(asr, audio[0], np.array([0, audio[0].size]), [[sp["audio_start"]]], [[sp["audio_end"]]],
                                                      timestamp_id=sp["timestamp"])
    with pytest.raises(AsrError, match="FP8W"):
        sub("engine").QwenAlignerSession(cfg, sub("arena").build_qwen_aligner_arena(cfg, ck, cfg.classify_num, BF16), sub("arena").PRECISION_FP8W)
    assert lib.load() is not None


def test_forced_aligner_end_to_end_matches_the_golden_words():
    g, cfg, ck, sp, cases = _golden()
    ha = sub("qwen_aligner")
    sess = _session(cfg, ck, F32)
    meta = ha.aligner_metadata(cfg, sp)
    aligner = ha.QwenForcedAligner(cfg, sess, meta)
    transcripts = []
    for c in cases:
        ids, at = [], 0
        for n in c["word_lens"]:
            ids.append(c["word_ids"][at:at + n].tolist()); at += n
        transcripts.append(list(zip(c["words"].tolist(), ids)))
    pcm = [np.round(clip_audio(c) * 32768.0) for c in cases]
    out = aligner.align([clip_audio(c) for c in cases] + [pcm[0].astype(np.int16)], transcripts + [[]], "English")
    assert out[-1] == []
    for i, c in enumerate(cases):
        assert [r["text"] for r in out[i]] == c["words"].tolist(), i
        assert [[r["start_time"], r["end_time"]] for r in out[i]] == c["word_ts"].tolist(), i


def test_reference_host_loop_through_the_shim(tmp_path):
    """Inference_Qwen_ForcedAligner_ONNX.py:487-575 on ort_shim: metadata session, merged session, io_binding with `audio` and
    `input_ids`, outputs bound to the device, output_ids[0] gathered at the <timestamp> positions, x timestamp_segment_ms, parse_timestamp."""
    g, cfg, ck, sp, cases = _golden()
    ort, io, wq, ha = sub("ort_shim"), sub("ort_io"), sub("ort_shim_qwen"), sub("qwen_aligner")
    folder = wq.export_qwen_aligner_folder(str(tmp_path / "Qwen_ForcedAligner_MI355X"), cfg, ck, ha.aligner_metadata(cfg, sp), F32)
    meta = ort.InferenceSession(f"{folder}/{wq.METADATA_FILE}.onnx").get_modelmeta().custom_metadata_map
    merged = ort.InferenceSession(f"{folder}/{wq.ALIGNER_MERGED_FILE}.onnx")
    special = json.loads(meta["special_token_ids"])
    seg, per = int(meta["timestamp_segment_ms"]), int(meta["timestamp_tokens_per_word"])
    binding = merged.io_binding()
    out_names = [x.name for x in merged.get_outputs()]
    input_meta = io.metadata_by_name(merged.get_inputs())
    device = ort.OrtDevice(ort.OrtDevice.cuda(), ort.OrtDevice.default_memory(), 0)
    for i, c in enumerate(cases):
        text_ts_ids = c["input_ids"].tolist()
        audio_np = io.array_for(input_meta["audio"], clip_audio(c).reshape(1, 1, -1), axes={0: 1, 1: 1, 2: int(c["n_samples"])})
        ids_np = io.array_for(input_meta["input_ids"], [text_ts_ids], axes={0: 1, 1: len(text_ts_ids)})
        binding.bind_ortvalue_input("audio", ort.OrtValue.ortvalue_from_numpy(np.ascontiguousarray(audio_np), "cuda", 0))
        binding.bind_ortvalue_input("input_ids", ort.OrtValue.ortvalue_from_numpy(np.ascontiguousarray(ids_np), "cuda", 0))
        for name in out_names:
            binding._iobinding.bind_output(name, device)
        merged.run_with_iobinding(binding, run_options=ort.RunOptions())
        output_ids = binding.get_outputs()[0].numpy()[0]
        assert np.array_equal(output_ids, c["output_ids"]), i
        text_start = output_ids.shape[0] - len(text_ts_ids)
        pos = [text_start + j for j, t in enumerate(text_ts_ids) if t == special["timestamp"]]
        got = ha.parse_timestamp(c["words"].tolist(), output_ids[pos].astype(np.int64) * seg, per)
        assert [[r["start_time"], r["end_time"]] for r in got] == c["word_ts"].tolist(), i
