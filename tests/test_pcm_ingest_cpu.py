"""int16 / f16 audio ingest, the parts that need no GPU: the two C-ABI functions, the `input_audio_dtype` every exporter records in the
bundle header, and -- against the live reference where it is mounted -- the identity the GPU tests rest on: a 2^-15 input scale commutes
with every f32 rounding of the reference's STFT, so raw PCM scaled at the load equals pre-scaled float audio bit for bit."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, sub
from helpers import kaldi_audio, load_golden
from test_oracle_paraformer import paraformer_setup
from test_oracle_paraformer_streaming import streaming_setup
from test_oracle_qwen_asr import qwen_setup
from test_oracle_whisper import whisper_setup
from test_qwen_aligner_cpu import aligner_setup

F32 = 1


def test_audio_dtype_functions_are_exported_declared_and_guard_a_null_session():
    _lib = sub("_lib")
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "asr_mi355x.h"), "r", encoding="utf-8") as f:
        header = f.read()
    assert re.search(r"enum\s+asr_audio_dtype\s*\{\s*ASR_AUDIO_F32\s*=\s*0\s*,\s*ASR_AUDIO_I16\s*=\s*1\s*,\s*ASR_AUDIO_F16\s*=\s*2\s*\}", header)
    for name in ("asr_session_set_audio_dtype", "asr_session_audio_dtype"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*asr_session\s*\*", header), name
    assert "#define ASR_ABI_VERSION 1" in header and lib.asr_abi_version() == 1
    for entry in ("asr_sensevoice_run", "asr_paraformer_run", "asr_paraformer_stream_step", "asr_whisper_encode", "asr_qwen_prefill", "asr_qwen_align"):
        assert re.search(r"\bint\s+" + entry + r"\s*\(\s*asr_session\s*\*\s*s\s*,\s*const\s+void\s*\*\s*audio\b", header), entry
    invalid = 1                                                             # ASR_STATUS_INVALID
    assert lib.asr_session_set_audio_dtype(None, 1) == invalid
    assert b"null session" in lib.asr_last_error()
    out = C.c_int(-1)
    assert lib.asr_session_audio_dtype(None, C.byref(out)) == invalid and out.value == -1
    assert b"null" in lib.asr_last_error()


def _exports(tmp_path, dtype):
    """Every exporter once, with `input_audio_dtype=dtype` (None: the default call) -> {family: (bundle path with the audio input, metadata bundle)}."""
    kw = {} if dtype is None else {"input_audio_dtype": dtype}
    out = {}
    d = tmp_path / "sv"
    cfg = sub("config").sensevoice_tiny()
    sub("sensevoice").export_sensevoice(str(d), cfg, sub("checkpoints").synth_sensevoice_checkpoint(cfg, 0), precision=F32, **kw)
    out["sensevoice"] = (d / "SenseVoiceSmall.asrmodel", d / "ASR_Metadata.asrmodel")
    d = tmp_path / "pf"
    cfg, ck = paraformer_setup("paraformer_tiny")
    sub("paraformer").export_paraformer(str(d), cfg, ck, ["<blank>", "<s>", "</s>"] + [f"t{i}" for i in range(3, cfg.vocab)], "zh", "zh", precision=F32, **kw)
    out["paraformer"] = (d / "Paraformer.asrmodel", d / "ASR_Metadata.asrmodel")
    d = tmp_path / "ps"
    g = load_golden("paraformer_streaming_tiny")
    cfg, ck = streaming_setup(g)
    ws = sub("ort_shim_paraformer_streaming")
    ws.export_paraformer_streaming_folder(str(d), cfg, ck, {"sample_rate": "16000", "audio_pcm_scale": "1"}, precision=F32, chunk=int(g["chunk"]), **kw)
    out["paraformer_streaming"] = (d / (ws.WEIGHTS_FILE + ".asrmodel"), d / "ASR_Metadata.asrmodel")
    d = tmp_path / "wh"
    cfg, ck, sup, beg = whisper_setup("whisper_tiny_test")
    wg = sub("ort_shim_whisper")
    wg.export_whisper(str(d), cfg, ck, precision=F32, suppress_tokens=sup, begin_suppress_tokens=beg, **kw)
    out["whisper"] = (d / (wg.WEIGHTS_FILE + ".asrmodel"), d / (wg.METADATA_FILE + ".asrmodel"))
    g = load_golden("qwen_asr_tiny")
    cfg, ck = qwen_setup(g)
    meta = {"audio_pcm_scale": "32768", "max_seq_len": str(cfg.max_seq_len), "special_token_ids": json.dumps({"stop": [1]}), "supported_languages": "{}"}
    wq = sub("ort_shim_qwen")
    d = tmp_path / "qw"
    wq.export_qwen_asr_folder(str(d), cfg, ck, meta, precision=F32, **kw)
    out["qwen_asr_folder"] = (d / (wq.WEIGHTS_FILE + ".asrmodel"), d / (wq.METADATA_FILE + ".asrmodel"))
    p = tmp_path / "qwen_single.asrmodel"
    sub("qwen_asr").export_qwen_asr(cfg, ck, str(p), meta, F32, **kw)
    out["qwen_asr"] = (p, p)
    g = load_golden("qwen_aligner_tiny")
    cfg, ck = aligner_setup(g)
    ameta = sub("qwen_aligner").aligner_metadata(cfg, json.loads(str(g["special"])))
    d = tmp_path / "al"
    wq.export_qwen_aligner_folder(str(d), cfg, ck, ameta, F32, **kw)
    out["qwen_aligner_folder"] = (d / (wq.ALIGNER_MERGED_FILE + ".asrmodel"), d / (wq.METADATA_FILE + ".asrmodel"))
    p = tmp_path / "aligner_single.asrmodel"
    sub("qwen_aligner").export_qwen_aligner(cfg, ck, str(p), ameta, F32, **kw)
    out["qwen_aligner"] = (p, p)
    return out


PCM_SCALE = {"sensevoice": "1", "paraformer": "1", "paraformer_streaming": "1", "whisper": "32768", "qwen_asr_folder": "32768", "qwen_asr": "32768",
             "qwen_aligner_folder": "32768", "qwen_aligner": "32768"}


@pytest.mark.parametrize("dtype", [None, "F32", "INT16", "F16"])
def test_exporters_record_the_input_audio_dtype(tmp_path, dtype):
    shim = sub("ort_shim")
    want = {None: np.float32, "F32": np.float32, "INT16": np.int16, "F16": np.float16}[dtype]
    for family, (bundle, meta_bundle) in _exports(tmp_path, dtype).items():
        info, _ = shim.load_model(str(bundle))
        assert info.get("input_audio_dtype", "F32") == (dtype or "F32"), family
        assert shim.bundle_audio_dtype(info) == np.dtype(want), family
        minfo, _ = shim.load_model(str(meta_bundle))
        assert minfo["metadata"]["audio_pcm_scale"] == PCM_SCALE[family], family       # what the reference writes: independent of the type


def test_a_bundle_without_the_field_is_f32_and_a_bad_value_raises(tmp_path):
    shim = sub("ort_shim")
    p = str(tmp_path / "old.asrmodel")
    shim.save_model(p, "metadata", None, None, {"k": "v"})                  # the header an older writer produced: no field
    info, _ = shim.load_model(p)
    assert "input_audio_dtype" not in info and shim.bundle_audio_dtype(info) == np.float32
    cfg = sub("config").sensevoice_tiny()
    ck = sub("checkpoints").synth_sensevoice_checkpoint(cfg, 0)
    for bad in ("int16", "I16", "F64", 1):
        with pytest.raises(ValueError, match="input_audio_dtype"):
            sub("sensevoice").export_sensevoice(str(tmp_path / "bad"), cfg, ck, precision=F32, input_audio_dtype=bad)
    wcfg, wck, sup, beg = whisper_setup("whisper_tiny_test")
    with pytest.raises(ValueError, match="input_audio_dtype"):
        sub("ort_shim_whisper").export_whisper(str(tmp_path / "badw"), wcfg, wck, precision=F32, input_audio_dtype="PCM")
    eng = sub("engine")
    assert eng.audio_dtype_name(np.int16) == "INT16" and eng.audio_np_dtype("F16") == np.float16
    with pytest.raises(ValueError):
        eng.audio_np_dtype(np.float64)


def _pcm_clip():
    """48 000 int16 samples: Kaldi-range noise rounded to PCM, both ends of the range included."""
    pcm = np.round(kaldi_audio(7, 48000)).astype(np.int16)
    pcm[100], pcm[101], pcm[4097], pcm[-1] = -32768, 32767, -32768, 32767
    return pcm


def test_live_reference_stft_scale_commutes_and_f16_legs_are_not_vacuous():
    oracle = pytest.importorskip("oracle.reference_harness")
    if not oracle.reference_available() or not os.path.isfile(os.path.join(oracle.REFERENCE_ROOT, "Whisper", "STFT_Process.py")):
        pytest.skip("reference tree not mounted")
    import torch
    sys.path.insert(0, os.path.join(oracle.REFERENCE_ROOT, "Whisper"))
    try:
        from STFT_Process import STFT_Process                              # the real, unmodified reference module
    finally:
        sys.path.pop(0)

    def stft(scale):
        return STFT_Process("stft_B_power", n_fft=400, win_length=400, hop_len=160, max_frames=0, window_type="hann", pad_mode="reflect",
                            center_pad=True, input_scale=scale, drop_last_frame=True).eval()

    pcm = _pcm_clip()
    x = torch.from_numpy(pcm.astype(np.float32)).reshape(1, 1, -1)
    with torch.inference_mode():
        folded = stft(1.0 / 32768.0)(x)                                     # INT16 export: 1/32768 inside the window (STFT_Process.py:143)
        plain = stft(1.0)(x * torch.tensor(2.0 ** -15, dtype=torch.float32))   # F32 export fed pcm / 32768
    assert folded.shape == plain.shape and torch.equal(folded, plain), float((folded - plain).abs().max())
    # the F16 legs: int16 -> f16 -> f32 really rounds a Kaldi-range clip (|x| > 2048 is not representable) and stays finite at full scale
    half = pcm.astype(np.float16).astype(np.float32)
    assert np.isfinite(half).all() and not np.array_equal(half, pcm.astype(np.float32))
    assert np.abs(pcm.astype(np.int32)).max() == 32768 and (np.abs(pcm.astype(np.int32)) > 2048).mean() > 0.1
    assert half.min() == -32768.0 and half.max() == 32768.0                 # 32767 rounds to 2^15: finite (f16 max is 65504)
