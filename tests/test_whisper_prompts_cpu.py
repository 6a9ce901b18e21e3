"""CPU: the host side of Whisper's text prompts -- build_prompt, the special id per geometry, the max_new clamp, the prompt list of
WhisperTranscriber.transcribe and transcribe_file(condition_on_previous_text=True) over a scripted session that records every prompt it is
given, and the arguments of tools/transcribe.py."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import sub

wh = sub("whisper")
cfgm = sub("config")
CFG = cfgm.whisper_tiny_test()                  # max_target_positions 64: build_prompt keeps 31 previous ids
HEAD = [CFG.sot_id, CFG.first_language_id, CFG.transcribe_id, CFG.no_timestamps_id]
WINDOW = 16000


def test_sot_prev_id_of_the_four_geometries():
    assert cfgm.whisper_large_v3().sot_prev_id == 50362
    assert cfgm.whisper_tiny_test().sot_prev_id == 562
    assert cfgm.whisper_mid_test().sot_prev_id == 4992
    assert cfgm.whisper_d256_test().sot_prev_id == 2992
    for c in (cfgm.whisper_large_v3(), cfgm.whisper_tiny_test(), cfgm.whisper_mid_test(), cfgm.whisper_d256_test()):
        assert c.eot_id < c.sot_prev_id < c.no_speech_id < c.no_timestamps_id      # a special id, next to its neighbours of the real vocabulary
        assert cfgm.WhisperConfig(**c.to_dict()) == c


def test_build_prompt_keeps_the_last_half_context():
    keep = CFG.max_target_positions // 2 - 1
    assert wh.build_prompt(CFG, HEAD, []) == HEAD and wh.build_prompt(CFG, HEAD, None) == HEAD
    assert wh.build_prompt(CFG, HEAD, [7, 8]) == [CFG.sot_prev_id, 7, 8] + HEAD
    prev = list(range(100, 100 + keep))
    assert wh.build_prompt(CFG, HEAD, prev) == [CFG.sot_prev_id] + prev + HEAD
    assert wh.build_prompt(CFG, HEAD, [5] + prev) == [CFG.sot_prev_id] + prev + HEAD           # one too many: the oldest goes
    long = list(range(200))
    got = wh.build_prompt(CFG, HEAD[:3], long)
    assert got == [CFG.sot_prev_id] + long[-keep:] + HEAD[:3] and len(got) <= CFG.max_target_positions // 2 + 3


class FakeSession:
    """Scripted WhisperSession: the k-th full-prompt prefill decodes script[k] = per sequence (ids, temperature the decode is scored to need).
    A decode whose temperature is above the sampler's current one scores badly (the fallback tries again), otherwise well."""
    audio_dtype = np.float32

    def __init__(self, script, no_speech=None):
        self.script, self.no_speech = script, list(no_speech or [])
        self.prompts, self.calls, self.limits = [], [], []
        self.batch, self.turn, self.sampling, self.probes = 0, -1, (False, 0.0), 0
        self.good = None

    def encode(self, audios):
        self.batch = len(audios)
        self.calls.append(("encode", len(audios)))

    def set_penalty(self, value, range_):
        pass

    def set_sampling(self, enable, temperature=0.8, *rest):
        self.sampling = (bool(enable), float(temperature) if enable else 0.0)

    def set_timestamps(self, enable, max_initial_index=50):
        pass

    def set_token_scores(self, enable):
        pass

    def _full(self, prompts):
        self.prompts.append([np.asarray(p).tolist() for p in prompts])
        if self.sampling[1] == 0.0 or self.good is None:
            self.turn += 1                                        # attempt 0 of the next batch: the next script entry
        self.good = [self.sampling[1] >= need for _, need in self.script[self.turn]]
        return np.zeros(len(prompts), np.int32), None

    def prefill(self, prompt, want_logits=True):
        prompt = np.asarray(prompt)
        if prompt.shape[1] == 1:
            self.probes += 1
            self.calls.append(("probe", prompt.shape[0]))
            return np.zeros(prompt.shape[0], np.int32), np.zeros((prompt.shape[0], CFG.vocab), np.float32)
        self.calls.append(("prefill", prompt.shape))
        return self._full(list(prompt))

    def prefill_prompts(self, prompts, want_logits=True):
        self.calls.append(("prefill_prompts", [len(p) for p in prompts]))
        return self._full(prompts)

    def no_speech_prob(self, no_speech_id):
        return np.asarray([self.no_speech.pop(0) for _ in range(self.batch)], np.float32)

    def generate(self, max_new, eos_id):
        self.limits.append(max_new)
        return [np.asarray(ids[:max_new], np.int32) for ids, _ in self.script[self.turn]]

    def token_scores(self):
        width = max(len(ids) for ids, _ in self.script[self.turn]) + 1
        out = np.full((self.batch, width), -0.1, np.float32)
        for b, ok in enumerate(self.good):
            if not ok:
                out[b] = -5.0
        return out


def _tr(sess, **kw):
    kw.setdefault("detect_language", False)
    kw.setdefault("no_speech_detection", False)
    return wh.WhisperTranscriber(CFG, sess, remove_repeats=False, **kw)


def test_transcribe_takes_ragged_prompts_and_clamps_max_new():
    sess = FakeSession([[([1, 2, 3], 0.0), ([4], 0.0), ([5, 6], 0.0)]])
    tr = _tr(sess, initial_prompt=[90, 91])
    prev = [[], list(range(10, 50)), None]
    out, _ = tr.transcribe([np.zeros(WINDOW, np.int16)] * 3, prompts=prev)
    keep = CFG.max_target_positions // 2 - 1
    want = [[CFG.sot_prev_id, 90, 91] + HEAD, [CFG.sot_prev_id] + ([90, 91] + prev[1])[-keep:] + HEAD, [CFG.sot_prev_id, 90, 91] + HEAD]
    assert sess.prompts == [want] and sess.calls[-1] == ("prefill_prompts", [len(p) for p in want])
    assert [o["prompt_len"] for o in out] == [len(p) for p in want]
    assert sess.limits == [CFG.max_target_positions - len(want[1])]          # the longest prompt bounds the batch
    assert [o["tokens"].tolist() for o in out] == [[1, 2, 3], [4], [5, 6]]
    # max_new below the clamp stands; no prompts at all: the plain uniform prefill, as before
    sess = FakeSession([[([1, 2, 3], 0.0)]])
    out, _ = _tr(sess).transcribe([np.zeros(WINDOW, np.int16)], max_new=2)
    assert sess.limits == [2] and sess.calls[-1] == ("prefill", (1, 4)) and sess.prompts == [[HEAD]] and out[0]["prompt_len"] == 4
    with pytest.raises(ValueError):
        _tr(FakeSession([])).transcribe([np.zeros(WINDOW, np.int16)], prompts=[[1], [2]])
    with pytest.raises(ValueError):
        _tr(FakeSession([]), initial_prompt="some text")                     # text needs prompt_encoder
    with pytest.raises(ValueError):
        _tr(FakeSession([]), initial_prompt=[CFG.sot_id])                    # text ids only
    assert _tr(FakeSession([]), initial_prompt="ab", prompt_encoder=lambda t: [len(t), 7]).initial_prompt == [3, 7]


def test_transcribe_file_without_conditioning_puts_initial_prompt_on_every_window_in_one_batch():
    sess = FakeSession([[([1], 0.0), ([2], 0.0), ([3], 0.0)]])
    res, _ = _tr(sess, initial_prompt=[90]).transcribe_file(np.zeros(3 * WINDOW, np.int16), input_audio_length=WINDOW)
    p = [CFG.sot_prev_id, 90] + HEAD
    assert sess.prompts == [[p, p, p]] and sess.calls[0] == ("encode", 3) and res["windows"] == [[1], [2], [3]] and res["prompt_len"] == [6, 6, 6]


def test_transcribe_file_conditions_each_window_on_the_text_before_it():
    # window 0 clean; window 1 clean; window 2 needs temperature 0.6 (> 0.5: its text is not carried on); window 3 sees the initial prompt alone;
    # window 4 has no speech (skipped: nothing decoded, nothing added); window 5 sees window 3's text
    script = [[([11, 12], 0.0)], [([13], 0.0)], [([14, 15], 0.6)], [([16], 0.2)], [([17], 0.0)]]
    sess = FakeSession(script, no_speech=[0.0, 0.0, 0.0, 0.0, 0.9, 0.0])
    tr = _tr(sess, no_speech_detection=True, initial_prompt=[90], condition_on_previous_text=True, temperature_fallback=(0.2, 0.6, 1.0))
    res, _ = tr.transcribe_file(np.zeros(6 * WINDOW, np.int16), input_audio_length=WINDOW)
    first = [p[0] for p in sess.prompts]                          # every attempt's prompt, in order (batches of one)
    P = lambda prev: ([CFG.sot_prev_id, 90] + prev + HEAD)
    want = [P([]), P([11, 12]), P([11, 12, 13]), P([11, 12, 13]), P([11, 12, 13]), P([]), P([]), P([16])]
    #       w0     w1           w2 attempt 0     w2 at 0.2        w2 at 0.6        w3     w3 at 0.2  w5
    assert first == want
    assert res["windows"] == [[11, 12], [13], [14, 15], [16], [], [17]]
    assert res["prompt_len"] == [6, 8, 9, 6, 0, 7]
    assert [s["temperature"] for s in res["window_scores"]] == [0.0, 0.0, 0.6, 0.2, 0.0, 0.0]
    assert [c for c in sess.calls if c[0] == "encode"] == [("encode", 1)] * 6 and sess.probes == 6      # in order, one window at a time
    assert res["tokens"].tolist() == [11, 12, 13, 14, 15, 16, 17]
    # without a fallback list the temperature never rises: nothing is ever reset
    sess = FakeSession([[([1], 0.0)], [([2], 0.9)], [([3], 0.0)]])
    res, _ = _tr(sess, condition_on_previous_text=True).transcribe_file(np.zeros(3 * WINDOW, np.int16), input_audio_length=WINDOW)
    assert [p[0] for p in sess.prompts] == [HEAD, [CFG.sot_prev_id, 1] + HEAD, [CFG.sot_prev_id, 1, 2] + HEAD]
    # the clamp follows every window's own prompt
    long = list(range(100, 140))
    sess = FakeSession([[(long, 0.0)], [([1], 0.0)]])
    _tr(sess, condition_on_previous_text=True).transcribe_file(np.zeros(2 * WINDOW, np.int16), input_audio_length=WINDOW)
    keep = CFG.max_target_positions // 2 - 1
    assert sess.limits == [CFG.max_target_positions - 4, CFG.max_target_positions - (1 + keep + 4)]


def _tool():
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    spec = importlib.util.spec_from_file_location("transcribe_tool_prompts", os.path.join(root, "tools", "transcribe.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_transcribe_tool_arguments(tmp_path):
    tool = _tool()
    base = ["run", "--family", "whisper", "--model", "m", "--wav", "a.wav", "--out", "o.json"]
    a = tool.build_parser().parse_args(base)
    assert a.initial_prompt_ids is None and a.condition_on_previous_text is False
    f = tmp_path / "ids.txt"
    f.write_text("10, 11\n12 13\n")
    a = tool.build_parser().parse_args(base + ["--initial-prompt-ids", str(f), "--condition-on-previous-text"])
    assert a.condition_on_previous_text is True and tool.parse_prompt_ids_file(a.initial_prompt_ids) == [10, 11, 12, 13]
    (tmp_path / "empty.txt").write_text("\n")
    with pytest.raises(SystemExit):
        tool.parse_prompt_ids_file(str(tmp_path / "empty.txt"))
    a = tool.build_parser().parse_args(["run", "--family", "sensevoice", "--model", "m", "--wav", "a.wav", "--out", "o.json", "--condition-on-previous-text"])
    with pytest.raises(SystemExit, match="whisper only"):
        tool.run(a)
