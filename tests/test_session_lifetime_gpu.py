"""Sessions give back every device byte they took: after a session of each model family has been created, run down its main paths (captured graphs,
the SANM block and tile kernels' weight packs, grown KV pools, beam search) and closed, the process-wide count of device bytes held by workspaces and
owned weight arenas (asr_probe_live_device_bytes) is exactly where it started."""
import gc

import numpy as np
import pytest

from conftest import sub
from helpers import kaldi_audio, load_golden, sensevoice_setup
from test_oracle_paraformer_streaming import streaming_setup
from test_oracle_qwen_asr import qwen_setup
from test_oracle_qwen_asr import unit_audio as qwen_audio
from test_oracle_whisper import unit_audio, whisper_setup

pytestmark = pytest.mark.gpu

BF16 = 0


def _live():
    gc.collect()                      # sessions other tests left to the garbage collector go first
    return sub("_probe").live_device_bytes()


def _sensevoice(n_windows, path):
    cfg, ck = sensevoice_setup("sensevoice_small")
    sess = sub("engine").SenseVoiceSession.from_checkpoint(cfg, ck, precision=BF16)
    audios = [kaldi_audio(900 + i, 16000 + 4000 * (i % 5)) for i in range(n_windows)]
    langs = [i % 7 for i in range(n_windows)]
    for _ in range(3):                # eager, captured, replayed
        sess.run(audios, langs)
    sess.profile(True)
    sess.run(audios, langs)
    assert path in sess.profile_read()
    sess.close()


def _paraformer_streaming():
    g = load_golden("paraformer_streaming_tiny")
    cfg, ck = streaming_setup(g)
    chunk = int(g["chunk"])
    sess = sub("engine").ParaformerStreamSession(cfg, ck, precision=BF16, chunk=chunk, max_streams=3)
    audio = [kaldi_audio(950 + i, 4 * chunk) for i in range(3)]
    for k in range(4):
        sess.step(np.stack([a[k * chunk:(k + 1) * chunk] for a in audio]), [0, 1, 2])
    sess.close()


def _whisper():
    cfg, ck, sup, beg = whisper_setup("whisper_tiny_test")
    sess = sub("engine").WhisperSession.from_checkpoint(cfg, ck, precision=BF16, suppress_tokens=sup, begin_suppress_tokens=beg)
    audios = [unit_audio(960 + i, n) for i, n in enumerate((26240, 12640))]
    prompt = np.array([[cfg.sot_id, cfg.first_language_id, cfg.transcribe_id, cfg.no_timestamps_id]] * len(audios), np.int32)
    sess.encode(audios)
    sess.prefill(prompt)
    for _ in range(8):                # device-fed single-token steps: eager, captured, then replays
        sess.decode(None)
    sess.prefill(prompt, want_logits=False)
    sess.beam_search(2, 6, -1)
    sess.close()


def _qwen():
    g = load_golden("qwen_asr_tiny")
    cfg, ck = qwen_setup(g)
    sess = sub("engine").QwenAsrSession.from_checkpoint(cfg, ck, precision=BF16)
    audios = [qwen_audio(970 + i, n) for i, n in enumerate((30000, 9000))]
    head, tail, suffix = g["head_ids"].tolist(), g["tail_ids"].tolist(), g["suffix_ids"].tolist()
    pre, post = [head + suffix] * len(audios), [tail] * len(audios)
    sess.prefill(audios, pre, post)
    for _ in range(8):
        sess.decode(None)
    sess.prefill(audios, pre, post)
    sess.beam_search(2, 6)
    sess.close()


def test_every_session_returns_its_device_memory():
    start = _live()
    _sensevoice(12, "sanm_block")     # >= 12 windows: the block kernel and its per-session weight pack
    assert _live() == start
    _sensevoice(2, "sanm_tiles")      # small batches: the tile kernel and its pack
    assert _live() == start
    _paraformer_streaming()
    assert _live() == start
    _whisper()
    assert _live() == start
    _qwen()
    assert _live() == start
