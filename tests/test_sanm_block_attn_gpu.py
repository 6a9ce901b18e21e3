"""The attention half of the SANM block kernel at every window length where it takes another path, pinned bit for bit.

tests/golden/sanm_block_attn_parent.npz (tools/record_sanm_block_attn_fixture.py) holds what the block kernel computed at the commit named inside the file,
before the K image got its own swizzle and before the shared ninth query tile was scored once per workgroup: neither change touches the arithmetic or its
order, so `enc_out` and the tokens must stay equal bit for bit. Window lengths: 128 (no shared tile), 129 (one valid row in it), 130, 137, 143, 144 (a full
ninth tile), 113 / 97 / 33 (4 / 3 / 2 sub-tiles of 32 keys), 5 (a single tile). The comparison with the four-launch path keeps the fixture from pinning a
bug of the recording commit at lengths no other test covers.
"""
import numpy as np
import pytest

from conftest import sub
from helpers import kaldi_audio, load_golden, sensevoice_setup

pytestmark = pytest.mark.gpu

BF16 = 0
FIXTURE = "sanm_block_attn_parent"


def _batch():
    g = load_golden(FIXTURE)
    lens = [int(n) for n in g["lens"]]
    audios = [kaldi_audio(s, n) for s, n in zip(g["seeds"], lens)]
    return g, lens, audios, [int(x) for x in g["langs"]]


def _session(monkeypatch, block, scatter):
    cfg, ck = sensevoice_setup("sensevoice_small")
    monkeypatch.setenv("ASR_SANM_BLOCK", block)
    monkeypatch.setenv("ASR_SANM_BLOCK_MIN", "1")               # (by default only batches of >= 12 windows take the block kernel)
    monkeypatch.setenv("ASR_SANM_BLOCK_SCATTER", scatter)
    return sub("engine").SenseVoiceSession.from_checkpoint(cfg, ck, precision=BF16)


@pytest.mark.parametrize("scatter", ["0", "1"])
def test_block_kernel_attention_equals_the_recorded_parent_bit_for_bit(monkeypatch, scatter):
    """Eager (with the `enc_out` tap) and as the captured graph (tokens), clusters on one XCD and spread over four."""
    g, lens, audios, langs = _batch()
    sess = _session(monkeypatch, "1", scatter)
    rows = sess.utterance_rows(lens)
    assert [T for _, T in rows] == [int(t) for t in g["window_rows"]]
    sess.taps(True)
    eager = sess.run(audios, langs)
    enc = sess.tap("enc_out")
    sess.taps(False)
    sess.run(audios, langs)                               # eager again (captures), then the graph replays
    graph = sess.run(audios, langs)
    sess.profile(True)
    sess.profile_reset()
    sess.run(audios, langs)
    assert "sanm_block" in set(sess.profile_read())
    for i, (r0, T) in enumerate(rows):
        assert np.array_equal(enc[r0:r0 + min(16, T)], g[f"w{i}_head"]), (i, T, "first rows")
        assert np.array_equal(enc[r0 + max(0, T - 16):r0 + T], g[f"w{i}_tail"]), (i, T, "last rows")
        assert np.array_equal(eager[i], g[f"w{i}_tokens"]), (i, T, "tokens, eager")
        assert np.array_equal(graph[i], g[f"w{i}_tokens"]), (i, T, "tokens, captured graph")


def test_block_kernel_attention_lengths_against_the_four_launch_path(monkeypatch):
    """Same batch, one launch per block against four launches per block: other K orders, so bf16 accumulation noise and not bits -- the bounds of
    test_block_kernel_equals_separate_launches_ragged (logits within 0.12 after 69 blocks, frame arg-max equal on more than 97 % of the rows)."""
    _, lens, audios, langs = _batch()
    out = {}
    for flag in ("1", "0"):
        sess = _session(monkeypatch, flag, "0")
        sess.taps(True)
        sess.run(audios, langs)
        out[flag] = sess.tap("logits")
        sess.taps(False)
        sess.profile(True)
        sess.profile_reset()
        sess.run(audios, langs)
        assert ("sanm_block" in set(sess.profile_read())) == (flag == "1")
    same = total = 0
    for r0, T in sess.utterance_rows(lens):
        a, b = out["1"][r0:r0 + T], out["0"][r0:r0 + T]
        assert np.abs(a - b).max() < 0.12, (T, float(np.abs(a - b).max()))
        same += int((a.argmax(1) == b.argmax(1)).sum())
        total += T
    assert same / total > 0.97, same / total
