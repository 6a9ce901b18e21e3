"""CPU: Qwen3-ForcedAligner -- the float oracle against the reference-minted goldens (tests/golden/qwen_aligner_tiny.npz,
tools/gen_golden_qwen_aligner.py), the host restatements (word splitting, fix_timestamp, parse_timestamp) on known answers and, when the
reference tree is mounted, against its AlignerTextProcessor; the aligner arena (classify head, f16 rotary table) and the converter."""
import importlib.util
import json
import os
import struct

import numpy as np
import pytest

from conftest import ROOT, sub
from helpers import golden_cases, load_golden
from qwen_aligner_ref import QwenAlignerOracle

F32_TOL = 1e-3


def aligner_setup(g):
    cfg = getattr(sub("config"), str(g["cfg_name"]))()
    ck = sub("checkpoints").synth_qwen_aligner_checkpoint(cfg, int(g["ckpt_seed"]))
    return cfg, ck


def clip_audio(c):
    return sub("checkpoints").synth_audio("unit", 1, int(c["n_samples"]), seed=int(c["audio_seed"]))[0, 0]


def test_oracle_reproduces_the_reference_goldens():
    g = load_golden("qwen_aligner_tiny")
    cfg, ck = aligner_setup(g)
    orc = QwenAlignerOracle(cfg, ck, str(g["special"]))
    for i, c in golden_cases(g):
        ids, logits = orc.align(clip_audio(c), c["input_ids"])
        assert ids.shape == c["output_ids"].shape, i
        assert np.abs(logits[c["slot_rows"]] - c["slot_logits"]).max() < F32_TOL, i
        assert np.array_equal(ids, c["output_ids"]), (i, np.flatnonzero(ids != c["output_ids"]))


def test_goldens_cover_the_required_clips():
    g = load_golden("qwen_aligner_tiny")
    cfg = getattr(sub("config"), str(g["cfg_name"]))()
    cases = [c for _, c in golden_cases(g)]
    lens = [c["output_ids"].size for c in cases]
    assert len(set(int(c["n_samples"]) for c in cases)) == len(cases)                       # ragged lengths
    assert any(c["words"].size == 1 for c in cases)                                          # one word
    assert max(lens) > cfg.max_seq_len - 16 and max(lens) <= cfg.max_seq_len                 # near the prompt limit


# ---------------------------------------------------------------------------------------------------- host restatements
FIX_CASES = [
    ([], []),
    ([0, 80, 160], [0, 80, 160]),
    ([0, 80, 40, 160, 240], [0, 80, 80, 160, 240]),                                    # run of 1, tie -> left
    ([0, 300, 310, 100, 120, 400], [0, 300, 310, 310, 400, 400]),                        # run of 2, nearer neighbour each
    ([0, 1000, 900, 800, 300, 400, 500, 600], [0, 75, 150, 225, 300, 400, 500, 600]),    # run of 3, spread
    ([0, 900, 800, 700, 110, 200], [0, 27, 55, 82, 110, 200]),                           # spread, truncated to int
    ([900, 100, 200, 300], [100, 100, 200, 300]),                                        # leading, run of 1
    ([900, 950, 990, 100, 200, 300, 400], [100, 100, 100, 100, 200, 300, 400]),          # leading, run of 3
    ([0, 500, 510, 520, 100, 200], [0, 500, 510, 520, 520, 520]),                        # trailing, run of 2
    ([0, 100, 200, 50, 40, 30], [0, 100, 200, 200, 200, 200]),                           # trailing, run of 3
    ([160, 160, 80, 80, 240], [160, 160, 160, 240, 240]),                                # equal values, run of 2 split
]
WORD_CASES = [
    ("Hello, world! don't", "English", ["Hello", "world", "don't"]),
    ("你好世界", "Chinese", ["你", "好", "世", "界"]),
    ("abc中def 123 -- ...", "English", ["abc", "中", "def", "123"]),
    ("  ", "English", []),
    ("état-civil Ünïcode", "French", ["étatcivil", "Ünïcode"]),
]


@pytest.mark.parametrize("data,want", FIX_CASES)
def test_fix_timestamp_known_answers(data, want):
    assert sub("qwen_aligner").fix_timestamp(data) == want


@pytest.mark.parametrize("text,lang,want", WORD_CASES)
def test_word_units_known_answers(text, lang, want):
    assert sub("qwen_aligner").word_units(text, lang) == want


def test_word_units_refuses_japanese_and_korean():
    ha = sub("qwen_aligner")
    for lang in ("Japanese", "korean"):
        with pytest.raises(NotImplementedError, match="segmenter"):
            ha.word_units("テスト", lang)


def test_parse_timestamp_and_prompt_ids():
    ha = sub("qwen_aligner")
    assert ha.parse_timestamp(["a", "b"], [0, 80, 160, 240], 2) == [{"text": "a", "start_time": 0, "end_time": 80},
                                                                    {"text": "b", "start_time": 160, "end_time": 240}]
    assert ha.parse_timestamp(["a", "b"], [160, 80, 240, 320], 2)[0] == {"text": "a", "start_time": 160, "end_time": 160}
    assert ha.parse_timestamp([], [], 2) == []
    assert ha.alignment_ids([[5, 6], [7]], 99, 2) == [5, 6, 99, 99, 7, 99, 99]


def test_goldens_words_follow_from_their_buckets():
    """the host path (gather slots, x 80 ms, repair, group) on the reference's own buckets gives the reference's word timestamps"""
    ha = sub("qwen_aligner")
    g = load_golden("qwen_aligner_tiny")
    cfg = getattr(sub("config"), str(g["cfg_name"]))()
    for i, c in golden_cases(g):
        ms = c["output_ids"][c["slot_rows"]].astype(np.int64) * cfg.timestamp_segment_ms
        got = ha.parse_timestamp(list(c["words"]), ms, cfg.timestamp_tokens_per_word)
        assert [[r["start_time"], r["end_time"]] for r in got] == c["word_ts"].tolist(), i


def _reference_processor():
    oracle = pytest.importorskip("oracle.reference_harness")
    if not oracle.reference_available() or not os.path.isdir(os.path.join(oracle.REFERENCE_ROOT, "Qwen_ForcedAligner")):
        pytest.skip("reference tree not mounted")
    spec = importlib.util.spec_from_file_location("gen_golden_qwen_aligner", os.path.join(ROOT, "tools", "gen_golden_qwen_aligner.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.reference_text_processor()


def test_live_reference_text_processor_agrees():
    ref = _reference_processor()
    ha = sub("qwen_aligner")
    rng = np.random.default_rng(3)
    cases = [d for d, _ in FIX_CASES] + [list(rng.integers(0, 40, n) * 80) for n in (1, 2, 5, 17, 60)]
    for data in cases:
        assert ha.fix_timestamp(data) == ref.fix_timestamp(data), data
        words = [f"w{k}" for k in range(len(data) // 2)]
        assert ha.parse_timestamp(words, data, 2) == ref.parse_timestamp(words, data, 2), data
    for text, lang, _ in WORD_CASES:
        assert ha.word_units(text, lang) == ref.word_units(text, lang), text


# ---------------------------------------------------------------------------------------------------- arena, converter
def _records(blob):
    _, _, n, _, _ = struct.unpack("<8sIIQQ", blob[:32].tobytes())
    out = {}
    for i in range(n):
        name, dt, nd, s0, s1, s2, s3, off = struct.unpack("<80sII4qQ", blob[32 + 128 * i: 160 + 128 * i].tobytes())
        out[name.rstrip(b"\0").decode()] = (dt, (s0, s1, s2, s3)[:nd], off)
    return out


def _f32(blob, rec):
    dt, shape, off = rec
    assert dt == sub("arena").DT_F32
    return blob[off: off + 4 * int(np.prod(shape))].view(np.float32).reshape(shape)


def test_aligner_arena_head_and_f16_rope():
    arena, cfgm, ckm = sub("arena"), sub("config"), sub("checkpoints")
    cfg = cfgm.qwen_aligner_tiny()
    ck = ckm.synth_qwen_aligner_checkpoint(cfg, 1)
    asr = _records(arena.build_qwen_asr_arena(cfgm.qwen_asr_tiny(), ckm.synth_qwen_asr_checkpoint(cfgm.qwen_asr_tiny(), 1), arena.PRECISION_F32))
    blob = arena.build_qwen_aligner_arena(cfg, ck, cfg.classify_num, arena.PRECISION_F32)
    rec = _records(blob)
    assert set(rec) == set(asr)                                                   # the same tensors as a Qwen3-ASR arena
    hpad = (cfg.classify_num + 127) // 128 * 128
    head = _f32(blob, rec["dec.lm_head"])
    assert head.shape == (hpad, cfg.d_model) and asr["dec.lm_head"][1][0] == (cfg.vocab + 127) // 128 * 128
    assert np.array_equal(head[:cfg.classify_num], ck["thinker.lm_head.weight"]) and not head[cfg.classify_num:].any()
    rope = _f32(blob, rec["dec.rope"])
    assert rope.shape == (cfg.max_seq_len, cfg.d_head)
    assert np.array_equal(rope, rope.astype(np.float16).astype(np.float32))       # every entry is an f16 value
    pos = np.arange(cfg.max_seq_len, dtype=np.float32)[:, None]
    inv = 1.0 / (cfg.rope_theta ** (np.arange(0, cfg.d_head, 2, dtype=np.float32) / cfg.d_head))
    assert np.abs(rope[:, :64] - np.cos(pos * inv)).max() < 1e-3 and np.abs(rope[:, 64:] - np.sin(pos * inv)).max() < 1e-3
    # the Qwen3-ASR table stays f32 (not f16-rounded)
    asr_blob = arena.build_qwen_asr_arena(cfgm.qwen_asr_tiny(), ckm.synth_qwen_asr_checkpoint(cfgm.qwen_asr_tiny(), 1), arena.PRECISION_F32)
    r2 = _f32(asr_blob, _records(asr_blob)["dec.rope"])
    assert not np.array_equal(r2, r2.astype(np.float16).astype(np.float32))


def test_aligner_arena_refuses_low_bit_and_bad_heads():
    arena, cfgm, ckm = sub("arena"), sub("config"), sub("checkpoints")
    cfg = cfgm.qwen_aligner_tiny()
    ck = ckm.synth_qwen_aligner_checkpoint(cfg, 0)
    for p in (arena.PRECISION_FP8W, arena.PRECISION_MXFP4W):
        with pytest.raises(ValueError, match="bf16 or f32"):
            arena.build_qwen_aligner_arena(cfg, ck, cfg.classify_num, p)
    with pytest.raises(ValueError, match="lm_head"):
        arena.build_qwen_aligner_arena(cfg, ck, cfg.classify_num + 1, arena.PRECISION_BF16)


def test_synth_aligner_checkpoint_is_the_asr_synth_with_a_classify_head():
    cfgm, ckm = sub("config"), sub("checkpoints")
    cfg = cfgm.qwen_aligner_tiny()
    a, b = ckm.synth_qwen_aligner_checkpoint(cfg, 4), ckm.synth_qwen_asr_checkpoint(cfg, 4)
    assert set(a) == set(b) and a["thinker.lm_head.weight"].shape == (cfg.classify_num, cfg.d_model)
    assert all(np.array_equal(a[k], b[k]) for k in a if k != "thinker.lm_head.weight")


def test_aligner_config_from_hf_config():
    cfgm = sub("config")
    hf = {"thinker_config": {"classify_num": 5000,
                             "audio_config": {"d_model": 896, "encoder_attention_heads": 14, "encoder_ffn_dim": 3584, "encoder_layers": 18,
                                              "downsample_hidden_size": 480, "n_window": 50, "n_window_infer": 800, "max_source_positions": 1500},
                             "text_config": {"hidden_size": 1024, "num_attention_heads": 16, "num_key_value_heads": 8, "head_dim": 128,
                                             "intermediate_size": 3072, "num_hidden_layers": 28, "vocab_size": 151936, "rms_norm_eps": 1e-6,
                                             "rope_theta": 1000000}}}
    cfg = cfgm.qwen_aligner_0p6b(hf)
    assert (cfg.enc_d, cfg.n_enc_layers, cfg.d_model, cfg.n_layers, cfg.n_kv_heads, cfg.classify_num, cfg.max_seq_len) == (896, 18, 1024, 28, 8, 5000, 1024)
    small = json.loads(json.dumps(hf))
    small["thinker_config"]["text_config"]["num_hidden_layers"] = 3
    small["thinker_config"]["classify_num"] = 77
    assert (cfgm.qwen_aligner_0p6b(small).n_layers, cfgm.qwen_aligner_0p6b(small).classify_num) == (3, 77)


def test_converter_maps_an_aligner_state_dict(tmp_path):
    from safetensors.numpy import save_file
    spec = importlib.util.spec_from_file_location("convert_checkpoint", os.path.join(ROOT, "tools", "convert_checkpoint.py"))
    cc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cc)
    cfgm, ckm = sub("config"), sub("checkpoints")
    cfg = cfgm.qwen_aligner_tiny()
    ck = ckm.synth_qwen_aligner_checkpoint(cfg, 2)
    save_file({k: np.ascontiguousarray(v) for k, v in ck.items()}, str(tmp_path / "model.safetensors"))
    sd = cc.load_state_dict(str(tmp_path / "model.safetensors"))
    with pytest.raises(ValueError, match="special token ids"):
        cc.convert("qwen_aligner", dict(sd), str(tmp_path / "o1"), 0)
    special = {"audio_start": 524, "audio_end": 520, "audio_pad": 525, "timestamp": 550}
    got = cc.convert("qwen_aligner", dict(sd), str(tmp_path / "out"), 1, tokens={"special_token_ids": special})
    for f in ("enc_d", "enc_heads", "enc_ffn", "n_enc_layers", "conv_channels", "d_model", "n_heads", "n_kv_heads", "d_head", "d_ffn", "n_layers",
              "vocab", "classify_num"):
        assert getattr(got, f) == getattr(cfg, f), f
    info, blob = sub("ort_shim").load_model(str(tmp_path / "out" / "ForcedAligner_Merged.asrmodel"))
    meta = info["metadata"]
    assert info["kind"] == "qwen_aligner" and json.loads(meta["special_token_ids"]) == special
    assert (meta["timestamp_segment_ms"], meta["timestamp_tokens_per_word"], meta["classify_num"]) == ("80", "2", str(cfg.classify_num))
    assert np.array_equal(blob, sub("arena").build_qwen_aligner_arena(got, ck, cfg.classify_num, 1))
    assert os.path.isfile(tmp_path / "out" / "ASR_Metadata.asrmodel")
    no_head = {k: v for k, v in sd.items() if k != "thinker.lm_head.weight"}
    with pytest.raises(ValueError, match="timestamp classifier"):
        cc.convert("qwen_aligner", no_head, str(tmp_path / "o2"), 0, tokens=special)
