#!/usr/bin/env python
"""Mint tests/golden/qwen_aligner_tiny.npz from the REAL reference classes of Qwen_ForcedAligner/Export_Qwen_ForcedAligner.py
(FORCED_ALIGNER_ENCODER / _EMBED / _ROTARY_MASK / _DECODER_MAIN, the merged graph's four parts) on a seeded synthetic checkpoint, the
way oracle/reference_harness.build_reference_qwen_asr builds the Qwen3-ASR modules: only the class / function definitions are compiled
from the reference file where it lies (oracle.reference_harness._compile_defs), torchaudio is replaced by transformers' mel_filter_bank,
f32 audio, and the quantisation-only channel re-orderings are off (exact permutations). The reference's AlignerTextProcessor
(Inference_Qwen_ForcedAligner_ONNX.py:164-345) turns the buckets into word timestamps.

The file stores seeds (checkpoint, audio), the special ids, and per clip: the words and their ids, the merged graph's `input_ids`,
its `output_ids` (L,), the f32 logits of the <timestamp> rows and the reference's word timestamps (ms).

    python tools/gen_golden_qwen_aligner.py
"""
from __future__ import annotations

import importlib
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "automatic-speech-recognition-asr-onnx_amd"

from oracle.reference_harness import REFERENCE_ROOT, _compile_defs, reference_available  # noqa: E402

# synthetic vocabulary roles (the tiny checkpoint has 600 ids; the real ones are 151669 / 151670 / 151676 / the tokenizer's <timestamp>)
SPECIAL = {"audio_start": 524, "audio_end": 520, "audio_pad": 525, "timestamp": 550}
CKPT_SEED = 7
# (audio seed, seconds, words); words = None: as many as fit a prompt of NEAR_MAX positions
CLIPS = [(11, 3.7, 9), (12, 1.2, 1), (13, 30.0, None), (14, 8.0, 20), (15, 5.3, 13)]
NEAR_MAX = 1020


def aligner_dir():
    return os.path.join(REFERENCE_ROOT, "Qwen_ForcedAligner")


def build_reference_aligner(cfg, ck: dict, special: dict):
    """-> dict(encoder, embed, rotary, main, processor) of the reference's classes on checkpoint `ck`."""
    from typing import Dict, List, Tuple
    from transformers import AutoConfig, AutoModel, AutoTokenizer
    from transformers.activations import ACT2FN
    from transformers.audio_utils import mel_filter_bank
    from transformers.configuration_utils import PretrainedConfig
    from transformers.generation import GenerationMixin
    from transformers.modeling_layers import GradientCheckpointingLayer
    from transformers.modeling_rope_utils import ROPE_INIT_FUNCTIONS
    from transformers.modeling_utils import PreTrainedModel
    from torch.onnx import symbolic_helper
    spec = importlib.util.spec_from_file_location("aligner_stft_process", os.path.join(aligner_dir(), "STFT_Process.py"))
    stft_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(stft_mod)
    ns = dict(torch=torch, np=np, json=json, F=torch.nn.functional, nn=torch.nn, Tensor=torch.Tensor, Dict=Dict, List=List, Tuple=Tuple,
              AutoConfig=AutoConfig, AutoModel=AutoModel, AutoTokenizer=AutoTokenizer, ACT2FN=ACT2FN, PretrainedConfig=PretrainedConfig,
              GenerationMixin=GenerationMixin, GradientCheckpointingLayer=GradientCheckpointingLayer, ROPE_INIT_FUNCTIONS=ROPE_INIT_FUNCTIONS,
              PreTrainedModel=PreTrainedModel, symbolic_helper=symbolic_helper, STFT_Process=stft_mod.STFT_Process, INPUT_AUDIO_DTYPE="F32",
              REORDER_DOWNPROJ_FOR_QUANT=False, REORDER_OPROJ_FOR_QUANT=False, REORDER_KEY="absmean", MAX_INPUT_AUDIO_LENGTH=cfg.max_audio_len,
              MAX_SEQ_LEN=cfg.max_seq_len, _MODEL_SAMPLE_RATE=cfg.sample_rate, _MODEL_WINDOW_TYPE="hann", _MODEL_NUM_MELS=cfg.n_mels,
              _MODEL_NFFT_STFT=cfg.nfft, _MODEL_WINDOW_LENGTH=cfg.nfft, _MODEL_HOP_LENGTH=cfg.hop_length, _MODEL_AUDIO_PCM_SCALE=32768,
              _MODEL_TIMESTAMP_SEGMENT_MS=cfg.timestamp_segment_ms, _MODEL_TIMESTAMP_TOKENS_PER_WORD=cfg.timestamp_tokens_per_word,
              _AUDIO_SUBSAMPLING_STAGE_NAMES=("conv2d1", "conv2d2", "conv2d3"),
              _MODEL_AUDIO_START_TOKEN_ID=int(special["audio_start"]), _MODEL_AUDIO_END_TOKEN_ID=int(special["audio_end"]),
              torchaudio=types.SimpleNamespace(functional=types.SimpleNamespace(
                  melscale_fbanks=lambda n_freqs, f_min, f_max, n_mels, sample_rate, norm, mel_scale: torch.from_numpy(
                      mel_filter_bank(n_freqs, n_mels, float(f_min), float(f_max), sample_rate, norm=norm, mel_scale=mel_scale)).float())))
    mod = types.ModuleType("qwen_aligner_reference_defs")       # transformers resolves string annotations through sys.modules
    mod.__dict__.update(ns)
    sys.modules[mod.__name__] = mod
    ns = mod.__dict__
    _compile_defs(os.path.join(aligner_dir(), "Export_Qwen_ForcedAligner.py"), ns)
    audio_cfg = dict(num_mel_bins=cfg.n_mels, encoder_layers=cfg.n_enc_layers, encoder_attention_heads=cfg.enc_heads, encoder_ffn_dim=cfg.enc_ffn,
                     d_model=cfg.enc_d, max_source_positions=cfg.max_source_positions, n_window=cfg.n_window, output_dim=cfg.d_model,
                     n_window_infer=cfg.n_window_infer, downsample_hidden_size=cfg.conv_channels, activation_function="gelu")
    text_cfg = dict(vocab_size=cfg.vocab, hidden_size=cfg.d_model, intermediate_size=cfg.d_ffn, num_hidden_layers=cfg.n_layers,
                    num_attention_heads=cfg.n_heads, num_key_value_heads=cfg.n_kv_heads, head_dim=cfg.d_head, rms_norm_eps=cfg.rms_eps,
                    rope_theta=cfg.rope_theta, tie_word_embeddings=False, max_position_embeddings=4096)
    config = ns["Qwen3ASRConfig"](thinker_config=dict(audio_config=audio_cfg, text_config=text_cfg, classify_num=cfg.classify_num))
    with torch.inference_mode():
        model = ns["Qwen3ForcedAlignerForConditionalGeneration"](config).float().eval()
        assert model.thinker.lm_head.weight.shape == (cfg.classify_num, cfg.d_model)
        sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in ck.items()}
        missing, unexpected = model.load_state_dict(sd, strict=False)
        assert not unexpected, unexpected
        assert all("positional_embedding" in m or "inv_freq" in m for m in missing), missing
        ns["refresh_non_persistent_buffers"](model, config.thinker_config.text_config)
        enc = ns["FORCED_ALIGNER_ENCODER"](model.thinker.audio_tower, model.thinker.model.embed_tokens).eval()
        embed = ns["FORCED_ALIGNER_EMBED"](model).eval()
        rot = ns["FORCED_ALIGNER_ROTARY_MASK"](model.thinker.model, cfg.max_seq_len).eval()
        main = ns["FORCED_ALIGNER_DECODER_MAIN"](model, cfg.n_heads, cfg.n_kv_heads, cfg.d_head, cfg.n_layers, cfg.d_model).eval()
    inf = {}
    _compile_defs(os.path.join(aligner_dir(), "Inference_Qwen_ForcedAligner_ONNX.py"), inf)
    import unicodedata
    from typing import Dict as _D, List as _L
    inf.update(unicodedata=unicodedata, Dict=_D, List=_L)
    return dict(encoder=enc, embed=embed, rotary=rot, main=main, processor=inf["AlignerTextProcessor"]())


def reference_text_processor():
    """The reference's AlignerTextProcessor (definitions only), for the live-reference checks of the host restatement."""
    import unicodedata
    from typing import Dict, List
    ns = dict(unicodedata=unicodedata, Dict=Dict, List=List, np=np)
    _compile_defs(os.path.join(aligner_dir(), "Inference_Qwen_ForcedAligner_ONNX.py"), ns)
    return ns["AlignerTextProcessor"]()


def run_reference(ref, audio: np.ndarray, input_ids) -> tuple:
    """The merged graph: -> (output_ids (L,) int32, logits (L, classify_num) f32)."""
    captured = {}
    hook = ref["main"].lm_head.register_forward_hook(lambda m, i, o: captured.__setitem__("logits", o.detach().clone()))
    try:
        with torch.inference_mode():
            text_embed = ref["embed"](torch.as_tensor(np.asarray(input_ids, np.int64).reshape(1, -1)))
            concat, ids_len = ref["encoder"](torch.as_tensor(np.asarray(audio, np.float32).reshape(1, 1, -1)), text_embed)
            cos, sin, mask = ref["rotary"](ids_len)
            out = ref["main"](concat, cos, sin, mask)
    finally:
        hook.remove()
    return out.numpy().reshape(-1).astype(np.int32), captured["logits"].numpy().reshape(out.shape[-1], -1).astype(np.float32)


def make_words(rng, n_words, cfg, special):
    """Synthetic words: names w<k> with 1..3 ids each from the ordinary part of the vocabulary."""
    reserved = set(special.values())
    words, ids = [], []
    for k in range(n_words):
        n = int(rng.integers(1, 4))
        t = [int(x) for x in rng.integers(3, 500, n) if int(x) not in reserved] or [5]
        words.append(f"w{k}")
        ids.append(t)
    return words, ids


def main():
    assert reference_available(), "the reference tree is not mounted"
    cfgm = importlib.import_module(PKG + ".config")
    ckm = importlib.import_module(PKG + ".checkpoints")
    ha = importlib.import_module(PKG + ".qwen_aligner")
    cfg = cfgm.qwen_aligner_tiny()
    ck = ckm.synth_qwen_aligner_checkpoint(cfg, CKPT_SEED)
    ref = build_reference_aligner(cfg, ck, SPECIAL)
    out = dict(cfg_name=np.array("qwen_aligner_tiny"), ckpt_seed=np.int64(CKPT_SEED), n_cases=np.int64(len(CLIPS)),
               special=np.array(json.dumps(SPECIAL)))
    per = cfg.timestamp_tokens_per_word
    for i, (seed, secs, n_words) in enumerate(CLIPS):
        n = int(round(secs * cfg.sample_rate))
        audio = ckm.synth_audio("unit", 1, n, seed=seed)[0, 0]
        rng = np.random.default_rng(1000 + seed)
        n_audio = importlib.import_module("oracle.qwen_asr_oracle").feat_lengths(n // cfg.hop_length)
        if n_words is None:                     # fill the prompt up to NEAR_MAX positions
            words, ids = make_words(rng, 400, cfg, SPECIAL)
            room, k, used = NEAR_MAX - n_audio - 2, 0, 0
            while k < len(words) and used + len(ids[k]) + per <= room:
                used += len(ids[k]) + per
                k += 1
            words, ids = words[:k], ids[:k]
        else:
            words, ids = make_words(rng, n_words, cfg, SPECIAL)
        input_ids = ha.alignment_ids(ids, SPECIAL["timestamp"], per)
        out_ids, logits = run_reference(ref, audio, input_ids)
        L = out_ids.size
        assert L == n_audio + 2 + len(input_ids), (L, n_audio, len(input_ids))
        text_start = L - len(input_ids)
        slots = np.asarray([text_start + j for j, t in enumerate(input_ids) if t == SPECIAL["timestamp"]], np.int64)
        ts = ref["processor"].parse_timestamp(words, out_ids[slots].astype(np.int64) * cfg.timestamp_segment_ms, per)
        p = f"c{i}_"
        out.update({p + "audio_seed": np.int64(seed), p + "n_samples": np.int64(n), p + "input_ids": np.asarray(input_ids, np.int32),
                    p + "output_ids": out_ids, p + "slot_rows": slots.astype(np.int32), p + "slot_logits": logits[slots],
                    p + "words": np.asarray(words), p + "word_ids": np.asarray([t for w in ids for t in w], np.int32),
                    p + "word_lens": np.asarray([len(w) for w in ids], np.int32),
                    p + "word_ts": np.asarray([[r["start_time"], r["end_time"]] for r in ts], np.int64).reshape(-1, 2)})
        print(f"clip {i}: {secs} s, {len(words)} words, L = {L}, slots = {slots.size}, buckets {out_ids[slots][:8]} ...")
    path = os.path.join(ROOT, "tests", "golden", "qwen_aligner_tiny.npz")
    np.savez(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
