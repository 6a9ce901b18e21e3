"""Restatement of the Whisper beam search for the tests: oracle/qwen_asr_oracle.py:beam_search_core (the build's one statement of the rule)
driven by WhisperOracle.decoder. The state of a hypothesis is (history length, self-K per layer, self-V per layer); the first ranking reads the
prefill's logits plus BEGIN_SUPPRESS, as the arg-max head after a prefill does; the stop set is {eos_id}."""
import numpy as np
import torch

from oracle.qwen_asr_oracle import beam_search_core


def beam_reference(orc, audio, prompt, beam: int, max_new: int, eos_id=None, margins=None):
    """One utterance -> best-first list of (token ids, score), as asr_whisper_beam_search defines it."""
    with torch.inference_mode():
        ck, cv = (t.unsqueeze(0) for t in orc.encode(audio))
        ids = torch.tensor([list(prompt)], dtype=torch.long)
        logits, sk, sv = orc.decoder(ids, 0, None, None, ck, cv)
        first = (logits[0] + orc._c(orc.begin_bias)).float().numpy()

        def step(state, tok):
            hist, k, v = state
            lg, nk, nv = orc.decoder(torch.tensor([[int(tok)]], dtype=torch.long), hist, k, v, ck, cv)
            return lg[0].float().numpy(), (hist + 1, nk, nv)

        return beam_search_core(first, (len(prompt), sk, sv), step, beam, max_new, stop_ids=() if eos_id is None else (int(eos_id),), margins=margins)


def as_lists(hyps):
    """[(tokens, score)] -> ([token lists], scores array), for comparisons."""
    return [np.asarray(t).astype(int).tolist() for t, _ in hyps], np.asarray([s for _, s in hyps], np.float64)
