"""The Whisper beam-search restatement (tests/whisper_beam_ref.py) on its own: beam_search_core driven by WhisperOracle.decoder."""
import numpy as np

from oracle.whisper_oracle import WhisperOracle
from test_oracle_whisper import unit_audio, whisper_setup
from whisper_beam_ref import as_lists, beam_reference


def _setup():
    cfg, ck, sup, beg = whisper_setup("whisper_tiny_test")
    return cfg, WhisperOracle(cfg, ck, sup, beg), [cfg.sot_id, cfg.first_language_id, cfg.transcribe_id, cfg.no_timestamps_id]


def test_width_one_is_the_oracle_greedy():
    cfg, orc, prompt = _setup()
    for seed, n in ((41, 16000), (42, 9600)):
        audio = unit_audio(seed, n)
        (toks, score), = beam_reference(orc, audio, prompt, 1, 6)
        ref = orc.greedy([audio], [prompt], 6)
        assert toks.tolist() == ref["token_ids"][0].tolist()
        assert np.isfinite(score) and score <= 0.0


def test_lists_are_sorted_distinct_and_end_at_the_stop_id():
    cfg, orc, prompt = _setup()
    audio = unit_audio(43, 12800)
    margins = []
    hyps = beam_reference(orc, audio, prompt, 4, 6, margins=margins)
    toks, scores = as_lists(hyps)
    assert len(hyps) == 4 and len(margins) >= 1
    assert (np.diff(scores) <= 0).all()
    assert len({tuple(t) for t in toks}) == 4
    assert all(len(t) == 6 for t in toks)
    # a stop id taken from the second hypothesis: that hypothesis ends there (the id is not emitted) and keeps its score
    eos = toks[1][1]
    hyps2 = beam_reference(orc, audio, prompt, 4, 6, eos_id=eos)
    toks2, scores2 = as_lists(hyps2)
    assert (np.diff(scores2) <= 0).all() and len({tuple(t) for t in toks2}) == len(toks2)
    assert all(eos not in t for t in toks2)
    assert any(len(t) < 6 for t in toks2)
