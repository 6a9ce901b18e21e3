"""CPU: the host side of Whisper's token scores -- avg_logprob, compression_ratio, word probabilities -- and WhisperTranscriber's temperature fallback
over a scripted session: which attempts run, with which sampler settings and seeds, how many prefills they cost, whose results are kept, and that the
head is left as attempt 0 configured it."""
import zlib

import numpy as np
import pytest

from conftest import sub

wh = sub("whisper")
WhisperConfig = sub("config").WhisperConfig


# ------------------------------------------------------------------------------------------------ pure functions
def test_avg_logprob_ended_cut_off_and_empty():
    row = np.array([-0.5, -1.5, -1.0, -9.0], np.float32)         # three emitted picks, then the stop pick or whatever followed
    assert wh.avg_logprob(row, 3, True) == pytest.approx((-0.5 - 1.5 - 1.0 - 9.0) / 4)         # OpenAI: sum_logprobs / (len + 1), the stop pick summed
    assert wh.avg_logprob(row, 3, False) == pytest.approx(-1.0)                               # cut off at the limit: the emitted picks only
    assert wh.avg_logprob(row, 0, True) == pytest.approx(-0.5)                                # an empty utterance that ended: the stop pick alone
    assert wh.avg_logprob(row, 0, False) == 0.0 and wh.avg_logprob(np.zeros(0, np.float32), 0, False) == 0.0
    assert wh.avg_logprob(np.array([-1.0, -np.inf], np.float32), 1, True) == -np.inf
    with pytest.raises(AssertionError):
        wh.avg_logprob(row, 4, True)                              # more picks than scores: the pairing is broken, not averaged over


def test_compression_ratio_tells_a_loop_from_speech():
    plain = "the quick brown fox jumps over the lazy dog while nobody watches"
    looped = "thank you. " * 40
    for text in (plain, looped, "été 中文"):
        raw = text.encode("utf-8")
        assert wh.compression_ratio(text) == len(raw) / len(zlib.compress(raw))
    assert wh.compression_ratio(plain) < 2.4 < wh.compression_ratio(looped)


def test_word_probability_is_the_mean_over_the_words_tokens():
    pieces = [" Hel", "lo", ",", " wor", "ld", None, "!"]        # None: an id that ends inside a character, counted with the one that completes it
    times = [(0.1 * i, 0.1 * i + 0.1) for i in range(len(pieces))]
    lps = np.log(np.array([0.5, 0.25, 1.0, 0.8, 0.4, 0.2, 0.6]))
    counts = wh.split_words(pieces)
    words = wh.word_times(pieces, times, lps)
    assert [w["tokens"] for w in words] == counts and sum(counts) == len(pieces)
    at = 0
    for w in words:
        assert w["probability"] == pytest.approx(np.exp(lps[at:at + w["tokens"]]).mean()) and 0.0 < w["probability"] <= 1.0
        at += w["tokens"]
    assert all("probability" not in w for w in wh.word_times(pieces, times))      # without scores the words are what they were
    with pytest.raises(AssertionError):
        wh.word_times(pieces, times, lps[:-1])


# ------------------------------------------------------------------------------------------------ the fallback loop over a scripted session
CFG = WhisperConfig()
LIMIT = 6
EOT = CFG.eot_id


class FakeSession:
    """Scripted WhisperSession: attempt k (the k-th full-prompt prefill) generates script[k][b] = (ids, scores of the picks incl. the stop pick)."""
    audio_dtype = np.float32

    def __init__(self, script, no_speech=None):
        self.script, self.no_speech = script, no_speech
        self.calls, self.attempt, self.head = [], -1, {"penalty": None, "sampling": None, "scores": False, "timestamps": False}
        self.batch = 0

    def encode(self, audios):
        self.batch = len(audios)
        self.calls.append(("encode", len(audios)))

    def set_penalty(self, value, range_):
        self.head["penalty"] = (value, range_)

    def set_sampling(self, enable, temperature=0.8, top_k=10, top_p=0.95, repetition_penalty=1.0, seed=0):
        self.head["sampling"] = (bool(enable), temperature, top_k, top_p, repetition_penalty, seed)

    def set_timestamps(self, enable, max_initial_index=50):
        self.head["timestamps"] = bool(enable)

    def set_token_scores(self, enable):
        self.head["scores"] = bool(enable)

    def prefill(self, prompt, want_logits=True):
        prompt = np.asarray(prompt)
        if prompt.shape[1] == 1:                                  # the [SOT] probe
            self.calls.append(("probe", dict(self.head)))
            return np.zeros(prompt.shape[0], np.int32), np.zeros((prompt.shape[0], CFG.vocab), np.float32)
        self.attempt += 1
        self.calls.append(("prefill", dict(self.head)))
        return np.zeros(prompt.shape[0], np.int32), None

    def no_speech_prob(self, no_speech_id):
        return np.asarray(self.no_speech, np.float32)

    def generate(self, max_new, eos_id):
        assert self.head["scores"], "the fallback reads scores: the mode must be on while the ids are generated"
        return [np.asarray(ids, np.int32) for ids, _ in self.script[self.attempt]]

    def token_scores(self):
        assert self.head["scores"]
        width = max(len(s) for _, s in self.script[self.attempt])
        out = np.full((self.batch, width), -50.0, np.float32)     # a finished sequence keeps picking while the others go on
        for b, (_, s) in enumerate(self.script[self.attempt]):
            out[b, :len(s)] = s
        return out


def _utt(ids, logprob):
    """ids that ended before the limit, every pick (the stop pick included) at `logprob`"""
    return list(ids), [logprob] * (len(ids) + 1)


GOOD, BAD = -0.2, -3.0
TEMPS = (0.2, 0.4, 0.6)


def _run(script, no_speech=None, **kw):
    sess = FakeSession(script, no_speech)
    tr = wh.WhisperTranscriber(CFG, sess, detect_language=False, no_speech_detection=no_speech is not None, top_k=7, top_p=0.9,
                               sampling_repetition_penalty=1.1, seed=100, repeat_penalty=0.8, temperature_fallback=TEMPS, **kw)
    B = len(script[0])
    out, _ = tr.transcribe([np.zeros(1600, np.int16)] * B, max_new=LIMIT)
    prefills = [h for what, h in sess.calls if what == "prefill"]
    return sess, out, prefills


def test_fallback_attempts_seeds_temperatures_and_who_keeps_what():
    # utterance 0 passes at attempt 0, utterance 1 at attempt 2, utterance 2 never: every attempt of the list runs and utterance 2 keeps the last
    script = [
        [_utt([1, 2, 3], GOOD), _utt([4, 4, 4], BAD), _utt([7, 7], BAD)],
        [_utt([9, 9, 9], GOOD), _utt([4, 4, 5], BAD), _utt([7, 8], BAD)],
        [_utt([9, 9, 8], BAD), _utt([4, 5, 6], GOOD), _utt([8, 8], BAD)],
        [_utt([9, 8, 8], BAD), _utt([5, 5, 5], BAD), _utt([8, 9], BAD)],
    ]
    sess, out, prefills = _run(script)
    assert len(prefills) == 4                                     # utterance 2 never passes: the list is exhausted
    assert prefills[0]["sampling"] == (False, 0.8, 7, 0.9, 1.1, 100) and prefills[0]["penalty"] == (0.8, 20)       # attempt 0: the configured head
    for k in (1, 2, 3):
        assert prefills[k]["sampling"] == (True, TEMPS[k - 1], 7, 0.9, 1.1, 100 + k), k
    assert all(h["scores"] for h in prefills)
    assert [o["tokens"].tolist() for o in out] == [[1, 2, 3], [4, 5, 6], [8, 9]]        # 0 keeps attempt 0, 1 takes attempt 2, 2 keeps the last
    assert [o["temperature"] for o in out] == [0.0, 0.4, 0.6]
    assert [o["avg_logprob"] for o in out] == pytest.approx([GOOD, GOOD, BAD])
    for o in out:
        assert len(o["token_logprobs"]) == len(o["tokens"]) and o["compression_ratio"] is None
    assert sess.head["sampling"] == (False, 0.8, 7, 0.9, 1.1, 100) and sess.head["penalty"] == (0.8, 20) and not sess.head["scores"]


def test_fallback_stops_when_nobody_needs_it():
    script = [[_utt([1, 2], GOOD), _utt([3], BAD)], [_utt([5, 5], BAD), _utt([6], GOOD)], [_utt([0], BAD), _utt([0], BAD)]]
    sess, out, prefills = _run(script)
    assert len(prefills) == 2 and [o["tokens"].tolist() for o in out] == [[1, 2], [6]] and [o["temperature"] for o in out] == [0.0, 0.2]
    sess, out, prefills = _run([[_utt([1, 2], GOOD), _utt([3], GOOD)]])
    assert len(prefills) == 1 and [o["temperature"] for o in out] == [0.0, 0.0]


def test_a_skipped_utterance_is_never_retried():
    script = [[_utt([1], GOOD), _utt([3, 3], BAD)], [_utt([2], BAD), _utt([4], BAD)]]
    sess, out, prefills = _run(script, no_speech=[0.1, 0.9])
    assert len(prefills) == 1                                     # the only bad decode belongs to a clip skipped for no speech
    assert out[1]["skipped"] and out[1]["tokens"].size == 0 and out[1]["token_logprobs"].size == 0 and out[1]["avg_logprob"] == 0.0
    assert out[0]["tokens"].tolist() == [1] and not out[0]["skipped"]
    probe = [h for what, h in sess.calls if what == "probe"]
    assert len(probe) == 1 and not probe[0]["scores"] and probe[0]["sampling"][0] is False


def test_compression_ratio_triggers_the_fallback_and_thresholds_are_arguments():
    decode = lambda ids: "".join("thank you. " if i == 4 else "word%d " % i for i in ids)
    looped, fine = _utt([4] * LIMIT, GOOD), _utt([1, 2, 3], GOOD)
    looped = (looped[0], looped[1][:LIMIT])                       # cut off at the limit: no stop pick
    assert wh.compression_ratio(decode([4] * LIMIT)) > 2.4
    sess, out, prefills = _run([[looped], [fine]], piece_decoder=decode)
    assert len(prefills) == 2 and out[0]["tokens"].tolist() == [1, 2, 3] and out[0]["temperature"] == 0.2
    assert out[0]["compression_ratio"] == pytest.approx(wh.compression_ratio(decode([1, 2, 3])))
    sess, out, prefills = _run([[looped], [fine]], piece_decoder=decode, compression_ratio_threshold=None)
    assert len(prefills) == 1 and out[0]["tokens"].tolist() == [4] * LIMIT
    sess, out, prefills = _run([[_utt([1], BAD)], [_utt([2], GOOD)]], logprob_threshold=-5.0)
    assert len(prefills) == 1


def test_token_scores_without_fallback_and_the_refusals():
    ids = [1, 2, 3] * 3
    assert len(wh.remove_repeated_parts(ids, 3, len(ids))) < len(ids)
    sess = FakeSession([[_utt(ids, GOOD)]])
    tr = wh.WhisperTranscriber(CFG, sess, detect_language=False, no_speech_detection=False, token_scores=True)
    out, _ = tr.transcribe([np.zeros(1600, np.int16)], max_new=len(ids) + 1)
    assert out[0]["tokens"].tolist() == ids                       # the repeat guard is not applied: it would break the pairing
    assert out[0]["token_logprobs"].tolist() == pytest.approx([GOOD] * len(ids)) and out[0]["temperature"] == 0.0
    assert out[0]["avg_logprob"] == pytest.approx(GOOD)
    plain = wh.WhisperTranscriber(CFG, FakeSession([[_utt(ids, GOOD)]]), detect_language=False, no_speech_detection=False)
    assert not plain.token_scores and plain.temperature_fallback == ()
    for kw in (dict(temperature_fallback=TEMPS), dict(token_scores=True)):
        with pytest.raises(ValueError):
            wh.WhisperTranscriber(CFG, sess, beam_size=2, **kw)
    with pytest.raises(ValueError):
        wh.WhisperTranscriber(CFG, sess, temperature_fallback=(0.0, 0.2))
