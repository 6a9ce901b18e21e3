"""Every implementation of the SANM block against the float64 reference of the block (tests/sanm_block_ref.py), per path and per window.

One bf16 SenseVoiceSession per path (the dispatch switches are re-read at session creation), block 0 + one block ("one", n_tp = 0: after_norm and
tp_norm follow the block directly) or block 0 + three blocks, after_norm, two tp blocks ("deep": the hand-over of row statistics from block to block
inside a persistent launch, and the run that starts behind the stand-alone after_norm without statistics). The checkpoint carries planted attention
(heads 0..2 attend along permutations with top probabilities near 0.9), the batch is ten truncations of one clip with the window lengths at which the
block kernel changes path. The run is eager with taps on; exact_stack is computed from the session's OWN `block0` rows, so the front end and block 0 do
not enter. Per window and statistic (worst row's RMS, max abs):

    stat(enc_out - exact) <= 3 x E_round,     E_round = stat(exact - rounded), from the two references alone

and the profile of the very same run must show the intended kernel and none of the others behind block 0 (block 0 itself always runs q|k|v + attention
+ FSMN as `sanm_fused` unless that kernel is switched off).

A note on the two four-launch rows: the session evaluates the LayerNorms inside the projections only together with the fused attention kernel
(`alg` in SvSession::enqueue needs use_fused), so with ASR_SANM_FUSED=0 the ASR_LN_FUSED=1 row dispatches the same kernels as the ASR_LN_FUSED=0 row.
The folded LayerNorms of the tiled GEMMs (out-projection statistics into FFN-1, FFN-2 statistics into the next block) are what the "fused attention
half" row runs; "fused_separate_ln" adds the remaining combination (fused kernel on separately normalised rows).

The margin of 3 covers what rounded_stack does not model (f32 summation order, the f16 image of the FFN-2 partials, the hardware exp, statistics from
bf16-rounded sums, flips of single roundings). Measured stat / E_round on an MI355X, worst window of each class (RMS ratio, then max-abs ratio) -- a
kernel's distance from the exact reference IS the rounding noise, no path and no window class stands out, and none needed a further rounding point:

    case path                      T 129..144   T 128       T 33..113   T 5
    one  four_launch_separate_ln   1.01 1.24    0.97 0.89   1.00 1.09   0.92 0.99
    one  four_launch_folded_ln     1.01 1.24    0.97 0.89   1.00 1.09   0.92 0.99
    one  fused_attention_half      1.01 1.06    0.98 0.95   1.00 1.12   1.05 1.18
    one  fused_separate_ln         1.01 1.12    1.01 0.91   1.00 1.06   0.92 0.99
    one  tile_kernel               1.02 1.07    1.00 1.10   1.06 1.41   0.79 0.79
    one  block_kernel              1.01 1.06    0.99 0.96   1.01 1.12   1.06 1.16
    one  block_kernel_ffnk0        1.01 1.06    0.99 0.96   1.00 1.12   1.05 1.18
    one  block_kernel_scatter      1.01 1.06    0.99 0.96   1.01 1.12   1.06 1.16
    deep four_launch_folded_ln     1.02 1.05    1.00 0.97   1.01 1.18   0.97 0.95
    deep tile_kernel               1.02 1.02    1.00 1.38   1.04 1.15   1.07 1.10
    deep block_kernel              1.00 1.11    0.99 1.04   1.05 1.16   0.78 0.91
    deep block_kernel_per_block    1.00 1.11    0.99 1.04   1.05 1.16   0.78 0.91
    the 5-row window alone / second of two behind the 144-row window: tile_kernel 0.91 0.78 / 0.91 0.84, block_kernel 1.01 1.02 / 1.05 1.07

Planted mistakes (once, off the GPU, on the recorded rows of four paths of the one-block case, with the mistake in the reference side of the comparison):
exact_stack with key T - 1 masked, with FSMN tap -5 of row T - 1 dropped, with eight hidden columns of row T - 1 zeroed made the comparison fail on every
window they apply to; the smallest failing statistics were 18.9 / 11.2 (masked key), 29.6 / 20.9 (tap) and 11.8 / 9.1 (hidden columns) x E_round.
"""
import hashlib

import numpy as np
import pytest

import sanm_block_ref as R
from conftest import sub

pytestmark = pytest.mark.gpu

BF16 = 0
# every dispatch switch of the SANM session, at its default; a path overrides some
DEFAULTS = {"ASR_SANM_BLOCK": "1", "ASR_SANM_TILES": "1", "ASR_SANM_FUSED": "1", "ASR_LN_FUSED": "1", "ASR_SANM_BLOCK_MIN": "12", "ASR_SANM_BLOCK_FFNK": "1",
            "ASR_SANM_BLOCK_SCATTER": "0", "ASR_SANM_BLOCK_PERSIST": "1"}
UNSET = ("ASR_SANM_BLOCK8_OPT", "ASR_SANM_TILES_OPT", "ASR_SANM_BLOCK_DBG", "ASR_SANM_TILES_DBG", "ASR_SANM_BLOCK_FAULT", "ASR_NO_GRAPH", "ASR_SKINNY_M144")
FOUR = {"ASR_SANM_BLOCK": "0", "ASR_SANM_TILES": "0", "ASR_SANM_FUSED": "0"}
BLOCK = {"ASR_SANM_BLOCK": "1", "ASR_SANM_BLOCK_MIN": "1"}
# name -> (environment, the kernel that runs the blocks behind block 0 or None for the four launches, batches)
ALL, TWO_FIVES = (tuple(range(10)),), (tuple(range(5)), tuple(range(5, 10)))
PATHS = {
    "four_launch_separate_ln": ({**FOUR, "ASR_LN_FUSED": "0"}, None, ALL),
    "four_launch_folded_ln": ({**FOUR, "ASR_LN_FUSED": "1"}, None, ALL),
    "fused_attention_half": ({"ASR_SANM_BLOCK": "0", "ASR_SANM_TILES": "0"}, "sanm_fused", ALL),
    "fused_separate_ln": ({"ASR_SANM_BLOCK": "0", "ASR_SANM_TILES": "0", "ASR_LN_FUSED": "0"}, "sanm_fused", ALL),
    "tile_kernel": ({"ASR_SANM_BLOCK": "0"}, "sanm_tiles", TWO_FIVES),              # 72 tiles in all, the kernel takes 64: two batches of five
    "block_kernel": (BLOCK, "sanm_block", ALL),
    "block_kernel_ffnk0": ({**BLOCK, "ASR_SANM_BLOCK_FFNK": "0"}, "sanm_block", ALL),
    "block_kernel_scatter": ({**BLOCK, "ASR_SANM_BLOCK_SCATTER": "1"}, "sanm_block", ALL),
    "block_kernel_per_block": ({**BLOCK, "ASR_SANM_BLOCK_PERSIST": "0"}, "sanm_block", ALL),
}
ONE_PATHS = [p for p in PATHS if p != "block_kernel_per_block"]
DEEP_PATHS = ["four_launch_folded_ln", "tile_kernel", "block_kernel", "block_kernel_per_block"]

_arenas, _refs = {}, {}


def _arena(case):
    if case not in _arenas:
        cfg, ck = R.case(case)
        _arenas[case] = sub("arena").build_sensevoice_arena(cfg, ck, BF16)
    return _arenas[case]


def _reference(case, x0):
    """(exact_stack, E_round) of one window's rows behind block 0, shared by the paths whose block 0 gives the same rows."""
    key = (case, x0.shape[0], hashlib.sha1(np.ascontiguousarray(x0).tobytes()).hexdigest())
    if key not in _refs:
        cfg, ck = R.case(case)
        exact = R.exact_stack(cfg, ck, x0)
        _refs[key] = (exact, R.e_round(cfg, ck, x0, exact))
    return _refs[key]


def _session(monkeypatch, case, path):
    for k in UNSET:
        monkeypatch.delenv(k, raising=False)
    for k, v in {**DEFAULTS, **PATHS[path][0]}.items():
        monkeypatch.setenv(k, v)
    cfg, _ = R.case(case)
    return cfg, sub("engine").SenseVoiceSession(cfg, _arena(case), precision=BF16)


def _run(sess, audios):
    """One eager run with taps and the profile on: (rows, block0, enc_out, profile of this run)."""
    sess.taps(True)
    sess.profile(True)
    sess.profile_reset()
    sess.run(audios, [R.LANG] * len(audios))
    rows = sess.utterance_rows([a.size for a in audios])
    return rows, sess.tap("block0"), sess.tap("enc_out"), sess.profile_read()


def _check_kernels(cfg, path, prof):
    """The intended kernel ran the blocks behind block 0, the others did not."""
    env, kernel, _ = PATHS[path]
    n = lambda k: prof.get(k, {}).get("launches", 0)
    runs = 1 if cfg.n_tp == 0 else 2                       # blocks 1 .. n_main - 1, then (behind after_norm) the tp blocks
    want = {"sanm_fused": 1, "sanm_tiles": 0, "sanm_block": 0}                # block 0 on the fused kernel
    if kernel is None:
        want["sanm_fused"] = 0
        assert n("attention") == cfg.n_blocks and n("fsmn") == cfg.n_blocks and n("gemm_qkv") == cfg.n_blocks, prof
    elif kernel == "sanm_fused":
        want["sanm_fused"] = cfg.n_blocks
        assert n("attention") == 0 and n("fsmn") == 0, prof
    elif kernel == "sanm_tiles":
        want["sanm_tiles"] = runs
    else:
        want["sanm_block"] = runs if env.get("ASR_SANM_BLOCK_PERSIST", "1") == "1" else cfg.n_blocks - 1
    if kernel in ("sanm_tiles", "sanm_block"):
        assert n("gemm_ffn1") == 1 and n("gemm_out") == 1 and n("attention") == 0, prof         # block 0's own launches, nothing else
    assert {k: n(k) for k in want} == want, (path, prof)


def _compare(case, path, rows, lens, b0, enc, report):
    cfg, _ = R.case(case)
    for (r0, T), n in zip(rows, lens):
        assert T == cfg.seq_len(n)
        got = enc[r0:r0 + T].astype(np.float64)
        assert np.isfinite(got).all(), (path, T)
        exact, e = _reference(case, b0[r0:r0 + T])
        s = R.stat(got - exact)
        ratio = (s[0] / e[0], s[1] / e[1])
        print(f"{case:4s} {path:24s} T={T:3d} rms {s[0]:.5f} / E {e[0]:.5f} = {ratio[0]:.2f}   max {s[1]:.5f} / E {e[1]:.5f} = {ratio[1]:.2f}")
        report.append((T, s, e, ratio))


def _path_against_the_reference(monkeypatch, case, path):
    cfg, sess = _session(monkeypatch, case, path)
    audios = R.window_audios()
    report = []
    for batch in PATHS[path][2]:
        clips = [audios[i] for i in batch]
        rows, b0, enc, prof = _run(sess, clips)
        assert [T for _, T in rows] == [R.WINDOWS[i] for i in batch]
        _check_kernels(cfg, path, prof)
        _compare(case, path, rows, [a.size for a in clips], b0, enc, report)
    assert sess.sanm_stats()["giveups"] == 0
    assert len(report) == len(R.WINDOWS)
    over = [(T, s, e) for T, s, e, ratio in report if s[0] > R.MARGIN * e[0] or s[1] > R.MARGIN * e[1]]
    assert not over, (path, over)


@pytest.mark.parametrize("path", ONE_PATHS)
def test_one_block_against_the_float64_reference(monkeypatch, path):
    _path_against_the_reference(monkeypatch, "one", path)


@pytest.mark.parametrize("path", DEEP_PATHS)
def test_five_blocks_across_after_norm_against_the_float64_reference(monkeypatch, path):
    _path_against_the_reference(monkeypatch, "deep", path)


@pytest.mark.parametrize("path", ["tile_kernel", "block_kernel"])
def test_a_window_does_not_depend_on_its_neighbours(monkeypatch, path):
    """The full batch of the path (the tile kernel: its batch of five) in its own order and reversed: every window gets another row offset, another
    cluster / tile slot and other neighbours (the 5-row window moves from the last place, behind the 33-row window, to the first). The same kernels run
    both (asserted) and block 0 hands over the same rows (asserted), so every window's `enc_out` must be equal bit for bit.

    The 5-row window alone and as the second of two behind the 144-row window are NOT compared bit for bit with the full batch, because block 0 itself is
    dispatched by the batch's row count: the projections evaluate the LayerNorms inside the GEMM only when the rows fill 144-row tiles to 94 %
    (gemm_ln_fusable: 16 and 160 rows do not), so block 0 normalises separately, its rows differ from the full batch's by bf16 rounding (0.007 on the
    first element), and the block kernel derives the row statistics itself instead of taking them from block 0's FFN-2; the GEMM tilings differ with the
    row count as well (last bits). The kernel under test is the same (asserted), its input is not. These two runs -- one cluster / one tile with every
    other slot idle, and the smallest ragged batch -- are held to the float64 reference of their own rows instead."""
    cfg, sess = _session(monkeypatch, "one", path)
    audios = R.window_audios()
    i5, i144 = R.WINDOWS.index(5), R.WINDOWS.index(144)
    full = list(PATHS[path][2][-1])
    got = {}
    for name, batch in (("full", full), ("reversed", full[::-1])):
        rows, b0, enc, prof = _run(sess, [audios[i] for i in batch])
        _check_kernels(cfg, path, prof)
        got[name] = {i: (b0[r0:r0 + T].copy(), enc[r0:r0 + T].copy()) for i, (r0, T) in zip(batch, rows)}
    for i in full:
        assert np.array_equal(got["full"][i][0], got["reversed"][i][0]), (path, R.WINDOWS[i], "block 0 rows differ: not the same input")
        assert np.array_equal(got["full"][i][1], got["reversed"][i][1]), (path, R.WINDOWS[i], float(np.abs(got["full"][i][1] - got["reversed"][i][1]).max()))
    report = []
    for name, batch in (("alone", [i5]), ("pair", [i144, i5])):
        clips = [audios[i] for i in batch]
        rows, b0, enc, prof = _run(sess, clips)
        _check_kernels(cfg, path, prof)
        assert rows[-1] == ((0, 5) if name == "alone" else (144, 5))
        _compare("one", f"{path} {name}", rows, [a.size for a in clips], b0, enc, report)
    assert sess.sanm_stats()["giveups"] == 0
    over = [(T, s, e) for T, s, e, ratio in report if s[0] > R.MARGIN * e[0] or s[1] > R.MARGIN * e[1]]
    assert len(report) == 3 and not over, (path, over)
