"""GPU: INT16 / F16 exports through the onnxruntime-API shim and the reference-shaped host loops.

An export made with `input_audio_dtype="INT16"` / `"F16"` declares that type on its `audio` input, refuses any other, and returns exactly what the
default (F32) export of the same checkpoint returns for the corresponding float audio -- both sides are this engine and the arithmetic is identical
(tests/test_pcm_ingest_gpu.py), so every case is compared with np.array_equal. The host loops read the type off the session by themselves."""
import json

import numpy as np
import pytest

from conftest import sub
from helpers import golden_cases, kaldi_audio, load_golden, sensevoice_setup
from test_oracle_paraformer import paraformer_setup
from test_oracle_paraformer_streaming import streaming_cases, streaming_setup
from test_oracle_qwen_asr import qwen_setup, unit_audio
from test_oracle_whisper import whisper_setup
from test_qwen_aligner_cpu import aligner_setup, clip_audio
from test_shim_paraformer_streaming_gpu import host_loop as stream_host_loop
from test_shim_qwen_gpu import LANGS, SPECIAL, HostLoop as QwenHost
from test_shim_whisper_gpu import HostLoop as _WhisperHostF32

pytestmark = pytest.mark.gpu

F32 = 1
DTYPES = {"F32": np.float32, "INT16": np.int16, "F16": np.float16}
ORT_TYPE = {"F32": "tensor(float)", "INT16": "tensor(int16)", "F16": "tensor(float16)"}
KALDI = ("sensevoice", "paraformer", "paraformer_streaming")


def _pcm(family, c):
    """The int16 clip of one golden case: the golden set's own audio rounded to PCM."""
    if family == "paraformer_streaming":
        return np.round(kaldi_audio(c["audio_seed"], int(c["n_chunks"]) * 8000)).astype(np.int16)
    if family in KALDI:
        return np.round(kaldi_audio(c["audio_seed"], c["n_samples"])).astype(np.int16)
    return np.clip(np.round(unit_audio(c["audio_seed"], c["n_samples"]) * 32768.0), -32768, 32767).astype(np.int16)


def _feed(family, pcm, name):
    """What an export of type `name` is fed for this PCM, and the float audio of the F32 export that must give the same result."""
    f32 = pcm.astype(np.float32) if family in KALDI else pcm.astype(np.float32) * np.float32(1.0 / 32768.0)
    if name == "INT16":
        return pcm, f32
    if name == "F16":
        return f32.astype(np.float16), f32.astype(np.float16).astype(np.float32)
    return f32, f32


class WhisperHost(_WhisperHostF32):
    """The Whisper host loop of tests/test_shim_whisper_gpu.py with the audio bound in the graph's own type, as the reference's loop does
    (Inference_Whisper_ONNX.py:103-126 feeds prepare_audio_input's result); the parent class writes float32 out."""

    def probe_prefill(self, audio, ids):
        plan, binding, keep = self.plans["probe"], self.probe.io_binding(), []
        a = self.io.array_for(plan["meta"]["audio"], np.ascontiguousarray(audio).reshape(1, 1, -1), axes={0: 1, 1: 1, 2: int(np.asarray(audio).size)})
        binding.bind_ortvalue_input("audio", self.ort.OrtValue.ortvalue_from_numpy(a, "cuda", 0))
        self._common_prefill_inputs(binding, plan, ids, keep)
        self.probe.run_with_iobinding(binding, run_options=self.run_options)
        outs = dict(zip(plan["outputs"], binding.get_outputs()))
        return outs, {n.replace("encoder_", "", 1): outs[n] for n in plan["cross_outputs"]}


class Setup:
    """One family: its tiny golden set, an exporter for a folder of a given audio type, the session that has the `audio` input."""

    def __init__(self, family):
        self.family = family
        if family == "sensevoice":
            self.g = load_golden("sensevoice_tiny")
            self.cfg, self.ck = sensevoice_setup("sensevoice_tiny")
        elif family == "paraformer":
            self.g = load_golden("paraformer_tiny")
            self.cfg, self.ck = paraformer_setup(str(self.g["cfg_name"]), int(self.g["ckpt_seed"]))
            self.vocab = ["<blank>", "<s>", "</s>"] + [f"t{i}" for i in range(3, self.cfg.vocab)]
        elif family == "paraformer_streaming":
            self.g = load_golden("paraformer_streaming_tiny")
            self.cfg, self.ck = streaming_setup(self.g)
            self.chunk = int(self.g["chunk"])
            assert self.chunk == 8000
        elif family == "whisper":
            self.g = load_golden("whisper_tiny")
            self.cfg, self.ck, self.sup, self.beg = whisper_setup(str(self.g["cfg_name"]), int(self.g["ckpt_seed"]))
        elif family == "qwen_asr":
            self.g = load_golden("qwen_asr_tiny")
            self.cfg, self.ck = qwen_setup(self.g)
            self.meta = {"audio_pcm_scale": "32768", "max_seq_len": str(self.cfg.max_seq_len), "special_token_ids": json.dumps(SPECIAL),
                         "supported_languages": json.dumps(LANGS)}
        else:
            self.g = load_golden("qwen_aligner_tiny")
            self.cfg, self.ck = aligner_setup(self.g)
            self.special = json.loads(str(self.g["special"]))
            self.meta = sub("qwen_aligner").aligner_metadata(self.cfg, self.special)
        if family == "paraformer_streaming":
            self.cases = [c for _, c in streaming_cases(self.g)]
        else:
            self.cases = [c for _, c in golden_cases(self.g)]

    def export(self, folder, name):
        f, kw = self.family, {"input_audio_dtype": name}
        if f == "sensevoice":
            sub("sensevoice").export_sensevoice(folder, self.cfg, self.ck, precision=F32, **kw)
        elif f == "paraformer":
            sub("paraformer").export_paraformer(folder, self.cfg, self.ck, self.vocab, "zh", "zh", precision=F32, **kw)
        elif f == "paraformer_streaming":
            meta = {"sample_rate": "16000", "audio_pcm_scale": "1", "special_token_ids": '{"stop": [2]}', "supported_languages": "{}"}
            sub("ort_shim_paraformer_streaming").export_paraformer_streaming_folder(folder, self.cfg, self.ck, meta, precision=F32, chunk=self.chunk, **kw)
        elif f == "whisper":
            sub("ort_shim_whisper").export_whisper(folder, self.cfg, self.ck, precision=F32, suppress_tokens=self.sup, begin_suppress_tokens=self.beg,
                                                   gelu_tanh=False, **kw)
        elif f == "qwen_asr":
            sub("ort_shim_qwen").export_qwen_asr_folder(folder, self.cfg, self.ck, self.meta, precision=F32, **kw)
        else:
            sub("ort_shim_qwen").export_qwen_aligner_folder(folder, self.cfg, self.ck, self.meta, F32, **kw)
        return folder

    def audio_graph(self, folder):
        stem = {"sensevoice": "SenseVoiceSmall", "paraformer": "Paraformer", "paraformer_streaming": sub("ort_shim_paraformer_streaming").ENCODER_FILE,
                "whisper": sub("ort_shim_whisper").GRAPH_FILES["probe_prefill_greedy"], "qwen_asr": sub("ort_shim_qwen").GRAPH_FILES["prefill_greedy"],
                "qwen_aligner": sub("ort_shim_qwen").ALIGNER_MERGED_FILE}[self.family]
        return sub("ort_shim").InferenceSession(f"{folder}/{stem}.onnx")

    def weights(self, folder):
        stem = {"paraformer_streaming": sub("ort_shim_paraformer_streaming").WEIGHTS_FILE, "whisper": sub("ort_shim_whisper").WEIGHTS_FILE,
                "qwen_asr": sub("ort_shim_qwen").WEIGHTS_FILE, "qwen_aligner": sub("ort_shim_qwen").ALIGNER_MERGED_FILE}[self.family]
        return f"{folder}/{stem}.asrmodel"

    # ---- the graph(s) behind the reference's call order, on one clip already in the export's type -> list of arrays
    def run_graphs(self, folder, audio, case):
        f, ort = self.family, sub("ort_shim")
        if f in ("sensevoice", "paraformer", "qwen_aligner"):
            sess = self.audio_graph(folder)
            b = sess.io_binding()
            b.bind_ortvalue_input("audio", ort.OrtValue.ortvalue_from_numpy(audio.reshape(1, 1, -1), "cuda", 0))       # device-resident audio OrtValue
            if f == "sensevoice":
                b.bind_cpu_input("language_idx", np.asarray([int(case["lang"])], np.int32))
            if f == "qwen_aligner":
                b.bind_cpu_input("input_ids", case["input_ids"].reshape(1, -1).astype(np.int32))
            for o in sess.get_outputs():
                b.bind_output(o.name)
            sess.run_with_iobinding(b)
            return [o.numpy() for o in b.get_outputs()]
        if f == "paraformer_streaming":
            toks, fired, _ = stream_host_loop(folder, audio, self.chunk)
            return [toks, np.asarray(fired)]
        if f == "whisper":
            host = WhisperHost(folder, "greedy")
            probe, cross = host.probe_prefill(audio, np.array([[self.cfg.sot_id]], np.int32))
            outs = host.prefill(case["prompt"].reshape(1, -1).astype(np.int32), cross)
            logits0 = outs[[m.name for m in host.prefill_s.get_outputs()].index("logits")].numpy()
            toks, steps = host.decode_tokens(outs, cross, 8, stop_tokens=set())
            return [probe["logits"].numpy(), logits0, np.asarray(toks), np.asarray(steps)]
        host = QwenHost(folder, "greedy")
        toks, ids_len, steps = host.transcribe(audio, case["query_ids"].tolist(), case["language_tail_ids"].tolist(), int(case["ids_len"]) + 10 + 8, stop=set())
        return [np.asarray(toks), np.asarray([ids_len, steps])]

    # ---- the reference-shaped host loop, opened on a folder, on int16 clips -> (input_audio_dtype, list of arrays, texts)
    def run_host_loop(self, folder, clips):
        f, eng = self.family, sub("engine")
        if f == "sensevoice":
            tr = sub("sensevoice").SenseVoiceTranscriber(folder, "en", device_type="cuda")
            res = [tr.transcribe(p) for p in clips]
            return tr.input_audio_dtype, [np.concatenate([np.asarray(w).reshape(-1) for w in r["token_ids"]]) for r in res], [r["text"] for r in res]
        if f == "paraformer":
            tr = sub("paraformer").ParaformerTranscriber(folder, device_type="cuda")
            res = [tr.transcribe(p) for p in clips]
            return tr.input_audio_dtype, [np.concatenate([np.asarray(w).reshape(-1) for w in r["token_ids"]]) for r in res], [r["text"] for r in res]
        sess = eng.load_session(self.weights(folder))
        if f == "paraformer_streaming":
            vocab = [f"t{i}" for i in range(self.cfg.vocab)]
            tr = sub("paraformer_streaming").ParaformerStreamTranscriber(sess, vocab, stop_token_ids=[2], decode_mode="zh")
            res = [tr.transcribe(p)[0] for p in clips]
            return tr.input_audio_dtype, [r["token_ids"] for r in res], [r["text"] for r in res]
        if f == "whisper":
            tr = sub("whisper").WhisperTranscriber(self.cfg, sess, suppress_tokens=self.sup)
            res, _ = tr.transcribe(clips, max_new=8)
            return tr.input_audio_dtype, [r["tokens"] for r in res] + [np.asarray([r["language_id"] for r in res])], [str(r["skipped"]) for r in res]
        if f == "qwen_asr":
            tr = sub("qwen_asr").QwenAsrTranscriber(self.cfg, sess, self.meta)
            res, _ = tr.transcribe(clips, max_new=8)
            return tr.input_audio_dtype, [r["tokens"] for r in res], [r["text"] for r in res]
        tr = sub("qwen_aligner").QwenForcedAligner(self.cfg, sess, self.meta)
        transcripts = []
        for c in self.cases:
            ids, at = [], 0
            for n in c["word_lens"]:
                ids.append(c["word_ids"][at:at + n].tolist())
                at += n
            transcripts.append(list(zip(c["words"].tolist(), ids)))
        out = tr.align(clips, transcripts, "English")
        return (tr.input_audio_dtype, [np.asarray([[r["start_time"], r["end_time"]] for r in o], np.int64).reshape(-1, 2) for o in out],
                [" ".join(r["text"] for r in o) for o in out])


FAMILIES = ["sensevoice", "paraformer", "paraformer_streaming", "whisper", "qwen_asr", "qwen_aligner"]


def _zero_binding(sess, overrides):
    """Every input bound (fresh state: zero-length histories, batch 1), so that the run reaches the audio check."""
    io, b = sub("ort_io"), sess.io_binding()
    for m in sess.get_inputs():
        shape = [d if isinstance(d, int) else (1 if ax == 0 else 0) for ax, d in enumerate(m.shape)]
        b.bind_cpu_input(m.name, overrides.get(m.name, np.zeros(shape, io.numpy_dtype(m))))
    for o in sess.get_outputs():
        b.bind_output(o.name)
    return b


@pytest.mark.parametrize("family", FAMILIES)
def test_exports_declare_their_audio_type_refuse_others_and_equal_the_f32_export(family, tmp_path):
    s = Setup(family)
    base = s.export(str(tmp_path / "F32"), "F32")
    ref_in = s.audio_graph(base).get_inputs()
    ref_audio = next(a for a in ref_in if a.name == "audio")
    assert ref_audio.type == "tensor(float)"
    for name in ("INT16", "F16"):
        folder = s.export(str(tmp_path / name), name)
        sess = s.audio_graph(folder)
        audio_arg = next(a for a in sess.get_inputs() if a.name == "audio")
        assert audio_arg.type == ORT_TYPE[name] and audio_arg.shape == ref_audio.shape
        assert [(a.name, a.type, a.shape) for a in sess.get_inputs() if a.name != "audio"] == [(a.name, a.type, a.shape) for a in ref_in if a.name != "audio"]
        n = s.chunk if family == "paraformer_streaming" else 8000
        with pytest.raises(ValueError, match=r"audio must be " + ORT_TYPE[name].replace("(", r"\(").replace(")", r"\)") + r".*got tensor\(float\)"):
            sess.run_with_iobinding(_zero_binding(sess, {"audio": np.zeros((1, 1, n), np.float32)}))
        for i, c in enumerate(s.cases):
            typed, f32 = _feed(family, _pcm(family, c), name)
            assert typed.dtype == DTYPES[name]
            got, want = s.run_graphs(folder, typed, c), s.run_graphs(base, f32, c)
            assert len(got) == len(want)
            for k, (a, b) in enumerate(zip(got, want)):
                assert a.shape == b.shape and np.array_equal(a, b), (family, name, i, k)


@pytest.mark.parametrize("family", FAMILIES)
def test_host_loops_pick_the_audio_type_up_from_the_folder(family, tmp_path):
    s = Setup(family)
    clips = [_pcm(family, c) for c in s.cases]
    assert all(p.dtype == np.int16 for p in clips)
    name32, ids32, text32 = s.run_host_loop(s.export(str(tmp_path / "F32"), "F32"), clips)
    name16, ids16, text16 = s.run_host_loop(s.export(str(tmp_path / "INT16"), "INT16"), clips)
    assert (name32, name16) == ("F32", "INT16")
    assert len(ids16) == len(ids32) and text16 == text32
    for i, (a, b) in enumerate(zip(ids16, ids32)):
        assert a.shape == b.shape and np.array_equal(a, b), (family, i)
    assert sum(a.size for a in ids32) > 0


def test_streaming_loop_pads_a_short_clip_in_the_session_dtype():
    """pad_to_chunks fills the tail with white noise cast to the audio type (Inference_Paraformer_Streaming_ONNX.py:356-362), which truncates differently
    per type: the streaming loops are compared on whole-chunk clips above, and here the padded tail only has to have the session's type."""
    ps, sv = sub("paraformer_streaming"), sub("sensevoice")
    short = np.round(kaldi_audio(77, 8000 + 123)).astype(np.int16).reshape(1, 1, -1)
    for name, dt in DTYPES.items():
        prepared = sv.prepare_audio_input(short, name, audio_pcm_scale=1)
        padded = ps.pad_to_chunks(prepared, 8000, np.random.default_rng(0))
        assert prepared.dtype == dt and padded.dtype == dt and padded.shape[-1] == 16000 and np.array_equal(padded[..., :8123], prepared)
        assert np.abs(padded[0, 0, 8123:].astype(np.float32)).max() > 0
