"""GPU: decode_gemm_kernel<MT, NT, FOLD, WQ> (csrc/decode_gemm.hip) through asr_probe_decode_gemm_desc against the float64 statement of lowbit_ref.py.

The hook forces the plan (column tiles, K splits, row blocks) through launch_decode_gemm_planned, so every case names the instance and grid it runs instead of
taking what the CU count of the machine makes of it, and asserts
  (1) the launched (mt, nt, splits, row_blocks);
  (2) stray == 0: A has exactly M rows followed by NaN rows, both outputs are NaN-filled buffers of 64 + 16 rows, and no word outside M rows x N columns changed;
  (3) within() at margin 3 on "f32" and "lo", every row divided by the scale it was drawn at, E_round from the float32 evaluations alone ("seq", "lib" and the
      kernel's own K partition as three column granules see it);
  (4) out_lo == bf16(out_f32) bit for bit where both are stored;
  (5) a second launch into the same buffers, workspace and tickets gives the same bits (the partials hold NaN before the first launch);
  (6) every ticket reads 0 afterwards;
and, in tests of their own, (7) byte and nibble weights equal the bf16 kernel over the dequantised copy bit for bit under the same forced plan with every
epilogue term on, a 64-row 16-split launch before a 1-row launch on the same workspace changes nothing, plan_M, ws == nullptr, padded pitches and the refusals.

Shapes: N in {32, 64, 96} (six column granules at nt = 1, so the wave -> share rotation takes six values); K = 256 without a split, 288 in 2 splits (9 steps: uneven
shares, waves without a step), 512 in 4 and 8, 576 in 9 (the last arriver's second batch of eight), 1024 in 16; M over {1, 15, 16, 17, 31, 32, 33, 48, 49, 63, 64}.
Each of the six instances runs without a split, with one, and -- <1, *> at 17..32 rows, <2, *> at 33..64 -- as two row blocks, for the three weight kinds and the
four epilogues the sessions launch: q|k|v / cross-q (bias, fold -> bf16), out-proj / fc2 (bias + residual -> f32 + bf16), fc1 (bias, fold, erf-GELU -> bf16) of
whisper.hip and o_proj / down_proj (residual, no bias -> f32 + bf16) of qwen.hip.

The fold. Rows are drawn with a mean of 0, 0.3 and 3 standard deviations; the budget comes from the float32 evaluation of the one-pass variance
(sum x^2 / K - mean^2, clamped at 0) in the same orders. Measured on the CPU reference (33 x 64, f32 output, one-pass float32 forms judged against the budget of
the two-pass float32 forms, margin 3): in the kernel's order the one-pass variance fits up to |mean| / std = 100 at K = 256 and K = 1024 (ratio 0.2 .. 0.9,
1.6 at K = 256 and 100: beyond that a bf16 row holds its mean and little else); as ONE running sum it fits at K = 256 throughout but leaves the margin from
|mean| / std = 10 at K = 1024 (3.6; 9.1 at 30). The sequential order is also the one order that can set the budget alone (5 x the others at K = 1024 and 3
standard deviations, test_lowbit_ref_cpu.py), so the cases at 3 standard deviations are drawn at K <= 576. Nobody has measured |mean| / std on a real residual
stream: the synthetic checkpoints of the suite do not tell what a trained pre-LN decoder carries there.

Measured on an MI355X, stat / E_round (worst row's RMS, max abs), worst case per instance class; the margin is 3. A bf16 store is dominated by its own rounding,
which is part of E_round (a correct kernel sits at 1.00 there); the planted faults of test_lowbit_ref_cpu.py sit above 30.

  class (launches)                                     f32 store       f32 store: fold + residual + GELU     bf16 store
  one block, no split, <1|2|4, 1|2> (72 + 12)          1.00  1.00      0.99  0.90                            1.00  1.00
  K in 2, 4, 8, 9, 16 splits, <1|2|4, 1|2> (72 + 12)   1.00  1.00      0.81  0.80                            1.00  1.00
  two row blocks, <1|2, 1|2> (48 + 8)                  0.99  1.00      0.91  0.82                            1.00  1.00
  ReLU / erf-GELU / tanh-GELU behind the residual (9)  1.05  1.00      --                                    1.00  1.00
  plan_M = 64 at 10 rows, forced and free (9)          0.97  1.00      --                                    1.00  1.00
  ws == nullptr (4)                                    0.87  0.64      --                                    1.00  1.00
  1 row, with and without 64 rows x 16 splits before   0.26  0.27      --                                    1.00  1.00
  padded pitches (18)                                  1.00  1.00      --                                    1.00  1.00
  by weight kind: bf16 0.79 0.89, e4m3 0.99 1.00, MXFP4 1.05 1.00 (f32 store)

A 1.00 in the f32 column is not a coincidence of size: where the kernel's own partition is the float32 form that sets E_round, the kernel reproduces that
evaluation (32-element dot products entering an f32 accumulator one by one, waves 0..7, splits in order), so its statistic IS E_round.

N = 96 and nt: the plan's rule is N % (16 nt) == 0, which 96 passes for nt = 2 (three granules of 32); the table keeps nt = 2 to N = 32 and 64 and runs all six
granule rotations of N = 96 at nt = 1.
"""
import functools

import numpy as np
import pytest

import lowbit_ref as L
from conftest import sub

pytestmark = pytest.mark.gpu

SPLIT = [(288, 2), (512, 4), (512, 8), (576, 9), (1024, 16)]
ROWS = {1: (1, 15, 16), 2: (17, 31, 32), 4: (33, 48, 49, 63, 64)}
# epilogue -> (bias, fold, add, act, outputs)
EPI = {"qkv": (True, True, False, 0, ("lo",)), "out": (True, False, True, 0, ("f32", "lo")), "fc1": (True, True, False, 2, ("lo",)),
       "qwen": (False, False, True, 0, ("f32", "lo")), "act": (True, False, True, None, ("f32", "lo")), "all": (True, True, True, 2, ("f32", "lo"))}
WKIND = ("bf16", "w8", "w4")
INSTANCES = [(mt, nt, mode) for mt in (1, 2, 4) for nt in (1, 2) for mode in ("plain", "split", "blocks") if not (mt == 4 and mode == "blocks")]


def _shape(i, mt, nt, mode):
    """The i-th draw of (M, N, K, splits, row_blocks) for an instance and a mode; i walks the row counts, the widths and the split shapes."""
    N = ((32, 64, 96) if nt == 1 else (32, 64))[i % (3 if nt == 1 else 2)]
    if mode == "blocks":                                          # <mt, nt> twice: 2 x 16 rows at 17..32, 2 x 32 rows at 33..64
        return ROWS[2 * mt][i % len(ROWS[2 * mt])], N, (256, 512)[i % 2], 1, 2
    M = ROWS[mt][i % len(ROWS[mt])]
    if mode == "plain":
        return M, N, (256, 288, 576)[i % 3], 1, 1
    K, splits = SPLIT[i % len(SPLIT)]
    return M, N, K, splits, 1


def _cases():
    out, i = [], 0
    for mt, nt, mode in INSTANCES:
        for wkind in range(3):
            for epi in ("qkv", "out", "fc1", "qwen"):
                M, N, K, splits, rb = _shape(i, mt, nt, mode)
                offset = ((0.0, 0.3) if K == 1024 else (0.0, 0.3, 3.0))[i % (2 if K == 1024 else 3)]
                out.append(pytest.param(mt, nt, mode, wkind, epi, M, N, K, splits, rb, offset, i, id=f"{mode}-{mt}x{nt}-{WKIND[wkind]}-{epi}-{M}x{N}x{K}s{splits}"))
                i += 1
    return out


CASES = _cases()


def test_the_case_table_covers_what_it_says():
    seen = [c.values for c in CASES]
    assert {v[5] for v in seen} == {1, 15, 16, 17, 31, 32, 33, 48, 49, 63, 64} and {v[6] for v in seen} == {32, 64, 96}
    assert {(v[7], v[8]) for v in seen} >= set(SPLIT) | {(256, 1)}
    for mt, nt, mode in INSTANCES:
        mine = [v for v in seen if v[:3] == (mt, nt, mode)]
        assert {(v[3], v[4]) for v in mine} == {(w, e) for w in range(3) for e in ("qkv", "out", "fc1", "qwen")}
    assert {v[10] for v in seen if v[4] in ("qkv", "fc1")} == {0.0, 0.3, 3.0}
    assert all(v[7] <= 576 for v in seen if v[10] == 3.0)


def _bf16(x):
    return L.np_bf16(x)


@functools.lru_cache(maxsize=8)
def _operands(M, N, K, seed, fold, offset, wkind):
    return L.decode_inputs(M, N, K, seed, fold, offset, wkind)


def _launched_mt(M, rb):
    if rb == 2 and M > 16:
        return 1 if M <= 32 else 2
    return 1 if M <= 16 else 2 if M <= 32 else 4


def _run(M, N, K, nt, splits, rb, wkind, epi, seed, offset=0.0, act=None, tag="", check=True, dense=False, **kw):
    """One forced launch + assertions 1 .. 6; dense: the bf16 kernel over the dequantised copy of the same weights. -> outputs."""
    probe = sub("_probe")
    has_bias, fold, has_add, epi_act, want = EPI[epi]
    act = epi_act if act is None else act
    a, wk, bias, add, s = _operands(M, N, K, seed, fold, offset, wkind)
    spec = dict(bias=bias if has_bias else None, add=add if has_add else None, act=act, fold=fold)
    ops = dict(w=wk["w"]) if dense else wk
    out = probe.decode_gemm_desc(a, **ops, **spec, want=want, nt=nt, splits=splits, row_blocks=rb, **kw)
    if nt:
        assert out["plan"] == (_launched_mt(M, rb), nt, splits, rb if M > 16 else 1), out["plan"]
    assert out["stray"] == 0, out["stray"]
    assert out["tickets_zero"]
    if "lo" in out and "f32" in out:
        assert np.array_equal(out["lo"], _bf16(out["f32"]))
    if not check:
        return out
    exact, rounded = L.decode_forms(a, wk["w"], splits=out["plan"][2], w_scale=None if dense else wk.get("w_scale"), **spec)
    for key in want:
        ok, ratio = L.judge(out[key], exact, rounded, key, s)
        print(f"RATIO {tag} {WKIND[wkind]} {epi} act={act} {M}x{N}x{K} splits={out['plan'][2]} off={offset} {key} rms={ratio[0]:.3f} max={ratio[1]:.3f}")
        assert ok, (tag, key, ratio)
    return out


def _same(x, y, keys=("f32", "lo")):
    return all(np.array_equal(x[k], y[k], equal_nan=True) for k in keys if k in x or k in y)


@pytest.mark.parametrize("mt,nt,mode,wkind,epi,M,N,K,splits,rb,offset,seed", CASES)
def test_every_instance_against_float64(mt, nt, mode, wkind, epi, M, N, K, splits, rb, offset, seed):
    assert _launched_mt(M, rb) == mt
    one = _run(M, N, K, nt, splits, rb, wkind, epi, seed, offset, tag=f"{mode}<{mt},{nt}>")
    two = _run(M, N, K, nt, splits, rb, wkind, epi, seed, offset, check=False, repeats=2)
    assert _same(one, two)                                       # split order, self-resetting tickets, nothing stale read from the workspace


@pytest.mark.parametrize("wkind", [1, 2])
@pytest.mark.parametrize("i", range(len(INSTANCES)))
def test_byte_and_nibble_weights_equal_the_bf16_kernel_bit_for_bit(i, wkind):
    """Same forced plan, every epilogue term on (bias, fold, residual, erf-GELU, both outputs): the low-bit path may differ from the bf16 kernel over the
    dequantised copy in nothing but where the weights come from."""
    mt, nt, mode = INSTANCES[i]
    M, N, K, splits, rb = _shape(i + wkind, mt, nt, mode)
    low = _run(M, N, K, nt, splits, rb, wkind, "all", 100 + i, 0.3, tag=f"all {mode}<{mt},{nt}>")
    dense = _run(M, N, K, nt, splits, rb, wkind, "all", 100 + i, 0.3, check=False, dense=True)
    assert _same(low, dense)


@pytest.mark.parametrize("wkind", [0, 1, 2])
@pytest.mark.parametrize("act", [1, 2, 3])
def test_activations_come_after_the_residual(act, wkind):
    M, N, (K, splits) = (15, 31, 63)[act - 1], (64, 96, 32)[wkind], ((256, 1), (512, 4), (288, 2))[(act + wkind) % 3]
    _run(M, N, K, 1, splits, 1, wkind, "act", 200 + act, act=act, tag="act")


@pytest.mark.parametrize("wkind", [0, 1, 2])
def test_plan_rows_above_the_launched_rows(wkind):
    """plan_M = 64 with 10 rows: the partition is planned for 64 rows (slabs of 64 rows in the workspace) and the <1, nt> instance runs on it; the bits are those
    of the same split count planned for 10 rows, and what the cost model picks for plan_M = 64 is a plan of one row tile too."""
    planned = _run(10, 64, 512, 1, 4, 1, wkind, "out", 300, plan_M=64, tag="plan_M")
    own = _run(10, 64, 512, 1, 4, 1, wkind, "out", 300, check=False)
    assert _same(planned, own)
    blocks = _run(10, 64, 512, 2, 1, 2, wkind, "qkv", 301, 0.3, plan_M=64, tag="plan_M")          # a two-block plan at <= 16 rows launches one block
    assert blocks["plan"] == (1, 2, 1, 1)
    free = _run(10, 64, 512, 0, 0, 0, wkind, "out", 300, plan_M=64, tag="plan_M free")
    assert free["plan"][0] == 1 and free["plan"][3] == 1


@pytest.mark.parametrize("M", [1, 17, 40, 64])
def test_without_a_workspace_nothing_is_split(M):
    probe, lib = sub("_probe"), sub("_lib")
    out = _run(M, 96, 1024, 0, 0, 0, M % 3, "out", 400 + M, with_ws=False, tag="no_ws")
    assert out["plan"][2] == 1
    a, wk, bias, add, _ = _operands(M, 96, 1024, 400 + M, False, 0.0, M % 3)
    with pytest.raises(lib.AsrError, match="not admissible"):
        probe.decode_gemm_desc(a, **wk, bias=bias, with_ws=False, nt=1, splits=2, row_blocks=1)


@pytest.mark.parametrize("wkind", [0, 1, 2])
@pytest.mark.parametrize("M,nt,K,splits,rb", [(15, 1, 288, 2, 1), (33, 2, 576, 9, 1), (49, 1, 256, 1, 2)])
def test_padded_pitches_equal_the_contiguous_run(M, nt, K, splits, rb, wkind):
    """lda, ldw and every ld_add / ld_out above the extents (the gaps of A, W and add hold NaN): the same bits, nothing written into a gap."""
    for epi, off in (("out", 0.0), ("fc1", 0.3)):
        tight = _run(M, 64, K, nt, splits, rb, wkind, epi, 500 + M, off, tag="pitch")
        wide = _run(M, 64, K, nt, splits, rb, wkind, epi, 500 + M, off, check=False, lda=K + 8, ldw=K + 32, ld_add=64 + 4, ld_out_f32=64 + 8, ld_out_lo=64 + 12)
        assert _same(tight, wide)


@pytest.mark.parametrize("epi,offset", [("out", 0.0), ("qkv", 0.3)])
def test_a_64_row_16_split_launch_before_does_not_change_a_1_row_launch(epi, offset):
    """The 1-row launch finds 64-row slabs of 16 splits and their statistics in the workspace, and tickets that must have been re-armed."""
    for splits in (16, 2, 1):
        alone = _run(1, 96, 1024, 1, splits, 1, 0, epi, 600, offset, tag="after64")
        after = _run(1, 96, 1024, 1, splits, 1, 0, epi, 600, offset, check=False, pre_M=64, pre_splits=16)
        assert _same(alone, after)


def test_forced_plans_outside_the_plan_rules_are_refused():
    probe, lib = sub("_probe"), sub("_lib")
    a, wk, bias, add, _ = _operands(40, 96, 256, 700, False, 0.0, 0)
    for plan in (dict(nt=3, splits=1, row_blocks=1), dict(nt=1, splits=8, row_blocks=1), dict(nt=1, splits=17, row_blocks=1), dict(nt=1, splits=2, row_blocks=2),
                 dict(nt=1, splits=1, row_blocks=3)):
        with pytest.raises(lib.AsrError, match="not admissible"):
            probe.decode_gemm_desc(a, **wk, bias=bias, **plan)
    with pytest.raises(lib.AsrError, match="not admissible"):     # row blocks need more than 16 planned rows
        probe.decode_gemm_desc(a[:16], **wk, bias=bias, nt=1, splits=1, row_blocks=2)
    a, wk, bias, add, _ = _operands(8, 48, 256, 701, False, 0.0, 0)
    with pytest.raises(lib.AsrError, match="unsupported shape"):
        probe.decode_gemm_desc(a, **wk, bias=bias)
