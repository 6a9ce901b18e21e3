"""Float oracle of the Qwen3-ForcedAligner pass, built from oracle.qwen_asr_oracle.QwenAsrOracle (front-end, audio encoder, embeddings,
decoder folds) with what the aligner changes (Qwen_ForcedAligner/Export_Qwen_ForcedAligner.py):
  * prompt [<|audio_start|> | audio | <|audio_end|> | input_ids] (FORCED_ALIGNER_ENCODER :833-835);
  * rotary cos / sin rounded through f16 (FORCED_ALIGNER_ROTARY_MASK :855-880), causal -128 mask;
  * every position's final RMSNorm -> classify head -> arg-max (FORCED_ALIGNER_DECODER_MAIN :1104-1109).
Pinned against the reference's classes by tests/test_qwen_aligner_cpu.py (tests/golden/qwen_aligner_tiny.npz)."""
import json

import numpy as np
import torch

from conftest import sub  # noqa: F401  (puts the repository root on sys.path)
from oracle.qwen_asr_oracle import QwenAsrOracle

F = torch.nn.functional


class QwenAlignerOracle(QwenAsrOracle):
    def __init__(self, cfg, ck: dict, special: dict):
        if isinstance(special, str):
            special = json.loads(special)
        super().__init__(cfg, ck, [int(special["audio_start"])], [int(special["audio_end"])], [])
        self.special = dict(special)

    def hidden(self, audio_1d, input_ids):
        """final-norm input rows of every position (L, d_model)"""
        c = self.cfg
        with torch.inference_mode():
            x = self.prompt(self.encode(audio_1d), (), [int(t) for t in input_ids])
            n, H, KV, hd = x.shape[0], c.n_heads, c.n_kv_heads, c.d_head
            theta = torch.arange(n, dtype=torch.float32)[:, None] * self.inv_freq[None, :]
            cos = torch.cat([torch.cos(theta)] * 2, -1).half().float()
            sin = torch.cat([torch.sin(theta)] * 2, -1).half().float()
            rot = lambda z: torch.cat([-z[..., hd // 2:], z[..., :hd // 2]], -1)
            mask = torch.where(torch.arange(n)[None, :] <= torch.arange(n)[:, None], 0.0, -128.0)
            for L in self.dec:
                qkv = self._rms(x, c.rms_eps) @ L["wqkv"].t()
                q = self._rms(qkv[:, :H * hd].reshape(n, H, hd), c.rms_eps) * L["qn"]
                k = self._rms(qkv[:, H * hd:(H + KV) * hd].reshape(n, KV, hd), c.rms_eps) * L["kn"]
                v = qkv[:, (H + KV) * hd:].reshape(n, KV, hd)
                q = q * cos[:, None, :] + rot(q) * sin[:, None, :]
                k = k * cos[:, None, :] + rot(k) * sin[:, None, :]
                G = H // KV
                qg = q.reshape(n, KV, G, hd).permute(1, 2, 0, 3)
                att = torch.softmax(qg @ k.permute(1, 2, 0)[:, None] + mask, dim=-1) @ v.transpose(0, 1)[:, None]
                x = x + att.permute(2, 0, 1, 3).reshape(n, H * hd) @ L["wo"].t()
                gu = self._rms(x, c.rms_eps) @ L["gate_up"].t()
                x = x + (F.silu(gu[:, :c.d_ffn]) * gu[:, c.d_ffn:]) @ L["down"].t()
            return self._rms(x, c.rms_eps) * self.ck["thinker.model.norm.weight"]

    def align(self, audio_1d, input_ids):
        """-> (output_ids (L,) int32, logits (L, classify_num) f32)"""
        with torch.inference_mode():
            logits = self.hidden(audio_1d, input_ids) @ self.ck["thinker.lm_head.weight"].t()
        return logits.argmax(-1).numpy().astype(np.int32), logits.numpy().astype(np.float32)
