"""The beam-search ranking pass (launch_beam_select, shared by the Qwen3-ASR and Whisper searches) through the probe library: the ancestry
table it writes must name, for every generated slot, a row of the hypothesis's own utterance that wrote that slot -- also for an utterance
that has already finished, whose rows still run through the decoder and write their own slot every pass."""
import numpy as np
import pytest

from conftest import sub

pytestmark = pytest.mark.gpu

STALE = 999                                          # what the other (double-buffered) table may still hold from an earlier search


def _state(n_utt, beam, K, ld, n_prev, rng):
    N = n_utt * beam
    src_in = np.full((N, ld), STALE, np.int32)
    tok_in = np.full((N, ld), STALE, np.int32)
    for r in range(N):
        b = r // beam
        src_in[r, :n_prev] = b * beam + rng.integers(0, beam, n_prev)
        tok_in[r, :n_prev] = rng.integers(0, 500, n_prev)
    topv = -np.sort(rng.uniform(0.1, 3.0, (N, K)).astype(np.float32), axis=1)
    topi = rng.integers(0, 500, (N, K)).astype(np.int32)
    cum = -np.sort(rng.uniform(1.0, 5.0, N).astype(np.float32).reshape(n_utt, beam), axis=1).reshape(-1)
    return src_in, tok_in, topv, topi, cum


@pytest.mark.parametrize("beam", [1, 3, 8])
def test_every_written_ancestry_entry_names_a_row_of_the_utterance(beam):
    rng = np.random.default_rng(beam)
    n_utt, K, ld, n_prev = 3, beam, 12, 4
    N = n_utt * beam
    src_in, tok_in, topv, topi, cum = _state(n_utt, beam, K, ld, n_prev, rng)
    done = np.array([1, 0, 0], np.int32)             # utterance 0 finished before this pass; 1 and 2 are live
    fin = np.zeros(N, np.int32)
    fin[2 * beam:] = 1 if beam > 1 else 0            # utterance 2: its best hypothesis is live, the others ended (beam > 1)
    fin[2 * beam] = 0
    fin[0] = 1                                       # utterance 0 is finished because its best hypothesis ended
    length = np.full(N, n_prev, np.int32)
    nxt = topi[:, 0].copy()
    st = sub("_probe").beam_select(beam, K, n_prev + 1, topv, topi, cum, fin, length, nxt, done, src_in, tok_in,
                                   np.full((N, ld), STALE, np.int32), np.full((N, ld), STALE, np.int32))
    src = st["src_out"]
    for r in range(N):
        b = r // beam
        written = src[r, :n_prev + 1]
        assert ((written >= b * beam) & (written < (b + 1) * beam)).all(), (r, written.tolist())
        parent = int(src[r, n_prev])                 # the row that wrote the slot of this pass: the hypothesis's parent
        assert src[r, :n_prev].tolist() == src_in[parent, :n_prev].tolist(), r
    # the finished utterance stands as it was: its rows are their own parents, scores and lengths unchanged
    for r in range(beam):
        assert src[r, n_prev] == r and st["cum"][r] == cum[r] and st["len"][r] == n_prev
    assert st["done"][0] == 1
