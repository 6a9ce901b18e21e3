"""GPU: every reachable (kernel family, epilogue instance) of launch_gemm_bf16 / launch_gemm_f32 through asr_probe_gemm against the float64 statement of
gemm_ref.py, at the smallest shapes that still cross a tile, row-fragment or K-split edge.

Every case asserts (1) the kernel family the dispatcher reported, (2) stray == 0: no word outside valid rows x valid columns of the NaN-filled output
buffers changed (rows >= min(M, *m_dev), pitch gaps, rows up to round_up(M, 128)), (3) within(): worst row's RMS and max abs of got - exact, each
<= 3 x E_round with E_round from the float32 evaluations of gemm_ref.ORDERS alone, every row divided by the scale its inputs were drawn at (0.1 .. 10) so
that small-valued rows are judged on their own, (4) out_lo == bf16(out_f32) bit for bit where both are stored. Layout-only terms (slabs, pitches, m_dev,
repeats, a large call before a small one) are compared bit for bit between two runs of the same kernel; st_out against the returned bf16 values; arg-max
ids exactly (ties: the lowest index; planted winners: every row, after the float64 margins are asserted to exceed 2 x 3 x E_round).

Measured on an MI355X, stat / E_round (worst row's RMS, max abs), worst case per family x output class; the margin is 3. An operand-dtype store is
dominated by its own rounding, which is part of E_round: a correct kernel sits at 1.00 there, and the planted faults of test_gemm_ref_cpu.py sit above 30.

  family (cases)                         f32 store        f32 store, act / add2     bf16 store     statistics (sum, sum of squares)
  pipe, variants 1 .. 4                  1.00  1.03       1.03  1.00                1.00  1.00     1.00  1.00
  pipe, run-time-checked <-1, -1>        --               0.85  0.83                1.00  1.00     --
  t144, 4-stage / 2-stage ring           1.01  1.00       0.90  0.98 (generic)      1.00  1.00     1.00  1.00
  t144, LayerNorm fold                   --               --                        1.00  1.00     --
  big                                    0.93  0.95       0.66  0.77                1.00  1.00     --
  pp (persistent and per tile)           0.88  0.77       1.00  1.00                1.00  1.00     --
  skinny, 1 / 2 row tiles (+ no ws)      0.40  0.31       0.70  0.85                1.00  1.00     --
  skinny, 4 row tiles (+ hand-over)      0.32  0.23       0.64  0.44                1.00  1.00     --
  skinny, 9 row tiles with hand-over     0.33  0.27       --                        1.00  1.00     --
  skinny, RMSNorm fold                   0.33  0.30       --                        1.00  1.00     --
  tiled split-K + reduce                 0.29  0.26       0.34  0.35                1.00  1.00     1.00  1.00   (rms_out: 1.00  1.00)
  f32 kernel                             1.02  1.00       1.00  1.00                (f32 out_lo: the same)
  f32 split-K                            0.28  0.26       0.17  0.16
  transposed store (pipe, pp, f32)       --               --                        1.00  1.00
  lo_group slabs (pipe, big, pp, f32)    --               --                        1.00  1.00

Not compared here, and why:
  * t144w, t288w, t288w_amax, pp_amax and the heuristic choice of pp / big: their thresholds (hundreds of 144- or 256-row tiles, M >= 1024 / 2048) lie
    far above a few-second case. test_ops_gpu.py dispatches to them at their real sizes; its LayerNorm-fold and producer-epilogue value checks now also
    go through within(). Here variants 7, 8 and 136 run the same big / pp kernels, arg-max instance included, at small shapes.
  * The E_LSE arg-max instances (third partial, sum of exponentials): asr_probe_ctc_head and test_ctc_head_lse_gpu.py own them.
  * The decode GEMM (csrc/decode_gemm.hip, launch_decode_gemm: every Whisper decode step, Qwen3-ASR o_proj / down_proj) is not a launch_gemm_bf16 family:
    test_decode_gemm_ref_gpu.py owns it -- all 36 instances under a forced plan, bf16 / e4m3 / MXFP4 weights, against the float64 statement of lowbit_ref.py.
  * skinny_ln (ln_x prologue), skinny_w8 / skinny_w4 and the two-granule (N / 16 > 256) instance: operands the hook does not carry; test_ops_gpu.py,
    test_qwen_fp8_gpu.py, test_whisper_mxfp4_gpu.py and test_qwen_asr_gpu.py hold them (the byte / nibble files assert that the low-bit path equals the bf16
    path of the same kernel, under a whole-matrix budget: no float64 statement of skinny_w8 / skinny_w4 exists yet).
  * The ping-pong tuning instances (variants 9 .. 135) and the timing switches (GemmArgs::dbg): bench hooks, not product paths.
  * rms_out / st_out / m_dev in f32 mode: launch_gemm_f32 has no such term (the hook refuses them instead of returning unwritten buffers).
"""
import numpy as np
import pytest

import gemm_ref as R
from conftest import sub

pytestmark = pytest.mark.gpu

NAME = {1: "pipe", 2: "pipe", 3: "pipe", 4: "pipe", 5: "t144", 6: "t144", 7: "big", 8: "pp", 136: "pp"}
# epilogue letters: b bias, a add, 2 add2, r add2 through a row table, f f32 store, l operand-dtype store, s row statistics
PIPE = [(0, "bl"), (1, "bl"), (2, "bl"), (3, "bl"), (0, "a2f"), (0, "af"), (0, "baf"), (0, "a2fl"), (0, "afl"), (0, "bafl"), (0, "a2fls"), (0, "afls"),
        (0, "bafls"), (0, "bf"), (0, "f"), (4, "l"), (1, "bf"), (2, "b2f"), (3, "b2f")]            # ASR_GEMM_CASE (the two arg-max instances: test_argmax_*)
T144 = [(0, "bl"), (0, "f"), (4, "l"), (3, "bl"), (2, "bl"), (1, "bl"), (0, "a2f"), (0, "af"), (0, "baf"), (0, "a2fl"), (0, "afl"), (0, "bafl"),
        (0, "a2fls"), (0, "afls"), (0, "bafls")]                                                        # ASR_T144_CASE (E_LN: test_t144_layernorm_fold)
BIG = [(0, "bl"), (2, "bl"), (3, "bl"), (0, "baf"), (0, "f"), (4, "l"), (0, "af"), (0, "bf"), (1, "bf")]                                  # ASR_BIG_CASE
PP = [(0, "bl"), (2, "bl"), (3, "bl"), (0, "baf"), (0, "f"), (4, "l"), (0, "af"), (0, "bf"), (1, "bl"), (2, "b2f"), (3, "b2f")]            # ASR_PP_CASE
RAGGED = (137, 129, 65, 145, 257, 300, 127, 33)


def _run(M, N, K, kernel, epi, act=0, seed=0, tag="", check=True, **kw):
    """One launch + its assertions; -> (outputs, exact, rounded, row scales)."""
    probe = sub("_probe")
    rows = "r" in epi
    a, w, bias, add, add2, s = R.inputs(M, N, K, seed, table_rows=M + 9 if rows else 0)
    tab = np.array([(7 * m + 3) % (M + 9) for m in range(M)], np.int32) if rows else None
    if rows:
        tab[M // 2], tab[M - 1] = tab[0], M + 8                   # a repeat, and the table's last row at the clamped tail
    want = tuple(k for k, c in (("lo", "l"), ("f32", "f"), ("stats", "s"), ("t", "t"), ("rms", "n")) if c in epi)
    f32 = bool(kw.get("precision", 0))
    spec = dict(act=act, operand="f32" if f32 else "bf16")
    call = dict(act=act, want=want, **kw)
    if "b" in epi:
        spec["bias"] = call["bias"] = bias
    if "a" in epi:
        spec["add"] = call["add"] = add
    if "2" in epi or rows:
        spec["add2"] = call["add2"] = add2
        if rows:
            spec["add2_rows"] = call["add2_rows"] = tab
    if "n" in epi:
        spec["rms_eps"] = call["rms_eps"] = 1e-6
    if kw.get("ln"):
        spec["ln_dim"], spec["ln_eps"] = K, kw.get("ln_eps", 1e-5)
    if kw.get("a_rms_eps"):
        spec["a_rms_eps"] = kw["a_rms_eps"]
    out, kern = probe.gemm(a, w, **call)
    assert kern == kernel, (kern, kernel)
    assert out["stray"] == 0, out["stray"]
    if not check:
        return out, None, None, s
    exact, rounded = R.forms(a, w, **spec)
    Mv = M if kw.get("m_dev") is None else min(M, kw["m_dev"])
    for key in want:
        if key == "stats":
            _check_stats(out, tag)
            continue
        got = out[key]
        ref = {"t": "lo"}.get(key, key)
        if key == "t":
            got = got.T
        elif key == "lo" and kw.get("lo_group"):
            got = R.unlay_slabs(got, Mv)
        ex, ro = {ref: exact[ref][:Mv]}, [{ref: r[ref][:Mv]} for r in rounded]
        ok, ratio = R.judge(got, ex, ro, ref, s[:Mv])
        print(f"RATIO {tag or kernel} act={act} epi={epi} {M}x{N}x{K} {key} rms={ratio[0]:.3f} max={ratio[1]:.3f}")
        assert ok, (tag, key, ratio)
    if "lo" in out and "f32" in out and not f32 and not kw.get("lo_group"):
        assert np.array_equal(out["lo"], _bf16(out["f32"]))
    return out, exact, rounded, s


def _bf16(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def _check_stats(out, tag):
    """st_out against the float64 sums of the bf16 values the same launch returned; rounded forms: float32 sums of those 32 values in three orders."""
    lo = out["lo"]
    exact = R.stats_of(lo)
    forms = [R.stats_of(lo, np.float32, o) for o in ("seq", "pair", "lib")]
    for i, name in enumerate(("sum", "sumsq")):
        ok, ratio = R.within(out["stats"][..., i], exact[..., i], [f[..., i] for f in forms])
        print(f"RATIO {tag} stats {name} rms={ratio[0]:.3f} max={ratio[1]:.3f}")
        assert ok, (tag, name, ratio)


def _same(x, y):
    return all(np.array_equal(x[k], y[k], equal_nan=True) for k in x if k != "stray") and x.keys() == y.keys()


# ---- the compile-time instance lists, one case per listed instance at a ragged M ---------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(PIPE)))
def test_pipe_instances(i):
    """gemm_bf16_pipe: the four (tile width, ring depth) forms in turn, N = 128 / 384 (one and three column tiles), K = 64 / 192 / 576 (1, 3, 9 steps)."""
    act, epi = PIPE[i]
    v = 1 + i % 4
    _run(RAGGED[i % 6], (128, 384)[i % 2], (64, 192, 576)[i % 3], "pipe", epi, act, seed=i, variant=v, tag=f"pipe{v}")


def test_pipe_runtime_checked_instance_and_refusals():
    """An epilogue outside ASR_GEMM_CASE runs the <-1, -1> instance; statistics have no run-time-checked form; the 128-row tiles have no LayerNorm fold."""
    _run(137, 128, 192, "pipe", "bafl", act=1, variant=4, tag="pipe_generic")
    _run(129, 384, 64, "pipe", "2l", act=3, variant=1, tag="pipe_generic")
    probe, lib = sub("_probe"), sub("_lib")
    a, w, bias, add, _, _ = R.inputs(137, 128, 64, 0)
    with pytest.raises(lib.AsrError, match="statistics"):
        probe.gemm(a, w, bias, act=1, variant=4, want=("lo", "stats"))
    with pytest.raises(lib.AsrError, match="LayerNorm"):
        probe.gemm(a, w, bias, act=1, ln=True, variant=4)


@pytest.mark.parametrize("i", range(len(T144)))
def test_t144_instances(i):
    """gemm_bf16_t144 with the 4- and the 2-stage ring (variants 5 / 6): one ragged 144-row tile, two tiles, K halves summed through LDS."""
    act, epi = T144[i]
    v = 5 + i % 2
    _run((137, 145, 257, 300)[i % 4], (128, 384)[(i // 2) % 2], (64, 192, 576)[i % 3], "t144", epi, act, seed=i, variant=v, tag=f"t144_{v}")


@pytest.mark.parametrize("variant,M", [(-1, 137), (6, 137), (5, 280)])
def test_t144_layernorm_fold(variant, M):
    """ReLU(LayerNorm(x) W^T + b) with the statistics handed over per 32 columns and the column sums of the bf16 weights (E_BIAS | E_LO | E_LN)."""
    _run(M, 128, 192, "t144", "bl", act=1, seed=M + variant + 1, variant=variant, ln=True, tag="t144_ln")


def test_t144_runtime_checked_instance_and_refusals():
    _run(145, 128, 192, "t144", "bafl", act=1, variant=5, tag="t144_generic")
    probe, lib = sub("_probe"), sub("_lib")
    a, w, bias, add, _, _ = R.inputs(137, 128, 64, 0)
    with pytest.raises(lib.AsrError, match="no instance"):
        probe.gemm(a, w, bias, act=1, variant=5, want=("lo", "stats"))
    with pytest.raises(lib.AsrError, match="does not support"):
        probe.gemm(a, w, bias, variant=6, want=("t",))


@pytest.mark.parametrize("i", range(len(BIG)))
def test_big_instances(i):
    act, epi = BIG[i]
    _run((129, 257, 300)[i % 3], (256, 512)[i % 2], (64, 192, 576)[i % 3], "big", epi, act, seed=i, variant=7, tag="big")


def test_big_refuses_what_it_does_not_implement():
    probe, lib = sub("_probe"), sub("_lib")
    a, w, bias, add, _, _ = R.inputs(129, 256, 64, 0)
    for kw in (dict(act=1), dict(want=("lo", "stats")), dict(m_dev=5), dict(want=("t",))):
        with pytest.raises(lib.AsrError, match="variant 7"):
            probe.gemm(a, w, bias, variant=7, **kw)


@pytest.mark.parametrize("variant", [8, 136])
@pytest.mark.parametrize("i", range(len(PP)))
def test_pp_instances(i, variant):
    """The ping-pong 256 x 256 kernel, persistent (8) and one workgroup per tile (136): N % 256, K % 128."""
    act, epi = PP[i]
    _run((129, 257, 300)[i % 3], (256, 512)[i % 2], (128, 384)[i % 2], "pp", epi, act, seed=i, variant=variant, tag=f"pp{variant}")


def test_pp_refuses_an_unlisted_instance():
    probe, lib = sub("_probe"), sub("_lib")
    a, w, bias, add, _, _ = R.inputs(129, 256, 128, 0)
    for kw in (dict(act=1, add=add, want=("f32",)), dict(m_dev=5)):
        with pytest.raises(lib.AsrError, match="variant 8"):
            probe.gemm(a, w, bias, variant=8, **kw)


# ---- the weight-streaming kernel: run-time epilogue, row tiles 1 / 2 / 4 / 9 ----------------------------------------------------------------------------
SKINNY = [(1, 128, 256, 0, "bl"), (15, 48, 256, 2, "bfl"), (17, 128, 512, 3, "b2f"), (17, 80, 256, 0, "arf"), (15, 128, 256, 4, "l"),
          (17, 384, 256, 1, "bafl"), (16, 128, 256, 0, "f")]


@pytest.mark.parametrize("M,N,K,act,epi", SKINNY)
def test_skinny_one_and_two_row_tiles(M, N, K, act, epi):
    _run(M, N, K, "skinny", epi, act, seed=M, tag="skinny12")
    _run(M, N, K, "skinny", epi, act, seed=M, with_ws=False, tag="skinny12_no_ws")


@pytest.mark.parametrize("M,N,K,act,epi", [(33, 128, 512, 0, "bfl"), (64, 384, 256, 2, "brf"), (33, 80, 256, 4, "l")])
def test_skinny_four_row_tiles(M, N, K, act, epi, monkeypatch):
    """33 .. 64 rows stream weights without a workspace, with ASR_SKINNY_MAX_M=64 (then with the split-K hand-over), and for the RMSNorm fold."""
    _run(M, N, K, "skinny", epi, act, seed=M, with_ws=False, tag="skinny4_no_ws")
    monkeypatch.setenv("ASR_SKINNY_MAX_M", "64")
    one, *_ = _run(M, N, K, "skinny", epi, act, seed=M, tag="skinny4_splitk")
    two, *_ = _run(M, N, K, "skinny", epi, act, seed=M, check=False)
    assert _same(one, two)                                       # the hand-over sums in split order and re-arms its tickets


@pytest.mark.parametrize("M", [1, 15, 17, 33, 64])
def test_skinny_rmsnorm_fold(M):
    """a_rms_eps: sum(x^2) from the streamed fragments of all eight K slices, the output rows scaled before bias / add."""
    _run(M, 128, 512, "skinny", "baf", seed=M, a_rms_eps=1e-6, tag="skinny_rms")
    _run(M, 128, 256, "skinny", "l", act=4, seed=M, a_rms_eps=1e-6, tag="skinny_rms")


def test_rmsnorm_fold_is_refused_above_64_rows():
    probe, lib = sub("_probe"), sub("_lib")
    a, w, bias, _, _, _ = R.inputs(65, 128, 256, 0)
    with pytest.raises(lib.AsrError, match="weight-streaming"):
        probe.gemm(a, w, bias, a_rms_eps=1e-6)


def test_skinny_nine_row_tiles(monkeypatch):
    monkeypatch.setenv("ASR_SKINNY_M144", "1")
    _run(137, 128, 256, "skinny", "bafl", act=1, tag="skinny9")
    _run(65, 80, 512, "skinny", "brf", act=2, tag="skinny9")
    monkeypatch.setenv("ASR_SKINNY_SPLITK", "1")
    one, *_ = _run(137, 128, 512, "skinny", "bfl", tag="skinny9_splitk")
    two, *_ = _run(137, 128, 512, "skinny", "bfl", check=False)
    assert _same(one, two)


def test_skinny_honours_the_device_side_row_count():
    """Rows >= *m_dev stay untouched on the weight-streaming kernel too, and the rows below it do not change."""
    full, *_ = _run(17, 128, 256, "skinny", "bfl", tag="skinny_m_dev")
    for md in (0, 1, 16, 17, 40):
        part, *_ = _run(17, 128, 256, "skinny", "bfl", m_dev=md, check=md > 0, tag="skinny_m_dev")
        assert all(np.array_equal(part[k], full[k][:md]) for k in ("lo", "f32"))


def test_statistics_at_few_rows_take_the_tiled_kernels():
    """The weight-streaming kernel has no statistics epilogue: a producer with st_out is routed to the 128-row tiles at any row count."""
    _run(17, 128, 256, "pipe", "afls", tag="pipe_stats_small")
    _run(33, 128, 1024, "pipe_splitk", "bafls", tag="splitk_stats_small")


# ---- split-K across workgroups ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,act,epi", [(65, 128, 1024, 0, "bl"), (129, 384, 2048, 2, "b2f"), (300, 128, 1024, 1, "bafl"), (137, 384, 1024, 0, "afls"),
                                           (145, 128, 2048, 3, "bl"), (129, 1024, 1024, 0, "afn"), (65, 1024, 2048, 0, "bafln")])
def test_tiled_split_k_and_its_reduce(M, N, K, act, epi):
    one, *_ = _run(M, N, K, "pipe_splitk", epi, act, seed=K, tag="splitk")
    two, *_ = _run(M, N, K, "pipe_splitk", epi, act, seed=K, check=False)
    assert _same(one, two)


def test_rms_out_is_refused_where_the_reduce_does_not_run():
    probe, lib = sub("_probe"), sub("_lib")
    a, w, bias, _, _, _ = R.inputs(129, 1024, 192, 0)
    with pytest.raises(lib.AsrError, match="gemm_reduce_can_norm"):
        probe.gemm(a, w, bias, want=("f32", "rms"))
    a, w, bias, _, _, _ = R.inputs(129, 384, 1024, 0)
    with pytest.raises(lib.AsrError, match="gemm_reduce_can_norm"):
        probe.gemm(a, w, bias, want=("f32", "rms"))


# ---- the exact-f32 kernel ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,act,epi,kernel", [(137, 128, 80, 1, "bl", "f32"), (129, 384, 192, 2, "b2f", "f32"), (300, 128, 64, 3, "bafl", "f32"),
                                                  (65, 128, 48, 4, "l", "f32"), (17, 128, 64, 0, "arfl", "f32"), (137, 128, 512, 0, "bafl", "f32_splitk"),
                                                  (129, 384, 2048, 2, "b2f", "f32_splitk"), (33, 128, 1024, 1, "bl", "f32_splitk")])
def test_f32_kernel_and_its_split_k(M, N, K, act, epi, kernel):
    one, *_ = _run(M, N, K, kernel, epi, act, seed=K, precision=1, tag=kernel)
    two, *_ = _run(M, N, K, kernel, epi, act, seed=K, precision=1, check=False)
    assert _same(one, two)
    if kernel == "f32_splitk":
        _run(M, N, K, "f32", epi, act, seed=K, precision=1, with_ws=False, tag="f32_no_ws")


# ---- the transposed store --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [129, 130, 131, 137, 300])
@pytest.mark.parametrize("variant", [1, 2, 3, 4, 8, 136, "f32"])
def test_transposed_store(M, variant):
    """out_t[n][m] with the per-column bias: the un-swapped orientation, the m0 + 3 < M vector / scalar split at every M % 4, ld_out_t above M
    (the words between M and the pitch must keep their NaN: stray == 0)."""
    pp = variant in (8, 136)
    kw = dict(precision=1) if variant == "f32" else dict(variant=variant)
    N, K = (256, 128) if pp else (128, 192)
    _run(M, N, K, "f32" if variant == "f32" else NAME[variant], "bt", seed=M, ld_out_t=(M + 3) // 4 * 4 + 12, tag=f"out_t_{variant}", **kw)
    _run(M, N, K, "f32" if variant == "f32" else NAME[variant], "t", seed=M + 1, tag=f"out_t_{variant}", **kw)


# ---- layout-only identities, bit for bit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [1, 4, 7, 8, 136, "f32"])
@pytest.mark.parametrize("M,group", [(137, 64), (300, 128), (129, 32)])
def test_lo_group_slabs_equal_the_plain_store(variant, M, group):
    """Per-head slabs [N / group][Mpad][group] == the row-major out_lo re-laid, rows >= M of every slab untouched, slab stride wider than Mpad x group."""
    kw = dict(precision=1) if variant == "f32" else dict(variant=variant)
    name = "f32" if variant == "f32" else NAME[variant]
    N, K = (256, 128)
    plain, *_ = _run(M, N, K, name, "bl", seed=M, tag=f"slabs_{variant}", **kw)
    slabs, *_ = _run(M, N, K, name, "bl", seed=M, lo_group=group, pad_out=16, tag=f"slabs_{variant}", **kw)
    assert np.array_equal(R.unlay_slabs(slabs["lo"], M), plain["lo"])
    assert np.isnan(slabs["lo"][:, M:]).all()


PITCH = [("pipe", dict(variant=2), 137, 128, 192, "bafls", 0), ("pipe", dict(variant=3), 129, 384, 64, "brf", 2), ("t144", dict(variant=5), 145, 128, 192, "a2fls", 0),
         ("big", dict(variant=7), 257, 256, 192, "baf", 0), ("pp", dict(variant=8), 300, 256, 128, "b2f", 3), ("pp", dict(variant=136), 129, 256, 128, "l", 4),
         ("skinny", dict(), 17, 80, 256, "barfl", 1), ("skinny", dict(with_ws=False), 64, 128, 256, "l", 4), ("pipe_splitk", dict(), 137, 1024, 1024, "bafln", 0),
         ("f32", dict(precision=1, with_ws=False), 137, 128, 80, "barfl", 2), ("f32_splitk", dict(precision=1), 129, 128, 512, "bafl", 0)]


@pytest.mark.parametrize("kernel,kw,M,N,K,epi,act", PITCH, ids=[f"{p[0]}-{i}" for i, p in enumerate(PITCH)])
def test_padded_pitches_equal_the_contiguous_run(kernel, kw, M, N, K, epi, act):
    """lda, ldw and every ld_out / ld_add / ld_add2 wider than the matrix (the gaps of A and W hold NaN): the same bits, nothing written into a gap."""
    tight, *_ = _run(M, N, K, kernel, epi, act, seed=M, tag="pitch", **kw)
    wide, *_ = _run(M, N, K, kernel, epi, act, seed=M, check=False, pad_a=8, pad_w=16, pad_out=8, **kw)
    assert _same(tight, wide)


@pytest.mark.parametrize("kernel,kw,M,N,K,epi", [("pipe", dict(variant=4), 300, 128, 192, "bafl"), ("pipe", dict(variant=1), 300, 384, 64, "brf"),
                                                 ("pipe", dict(), 300, 128, 1024, "bl"), ("t144", dict(variant=5), 300, 128, 192, "afls"),
                                                 ("t144", dict(variant=6), 280, 128, 192, "bl")])
def test_device_side_row_count(kernel, kw, M, N, K, epi):
    """m_dev in {0, 1, 129, M} (and above M): rows >= *m_dev untouched, rows below it bit-identical to the full run."""
    full, *_ = _run(M, N, K, kernel, epi, seed=M, tag="m_dev", m_dev=M, **kw)
    for md in (0, 1, 129, M + 50):
        part, *_ = _run(M, N, K, kernel, epi, seed=M, check=False, m_dev=md, **kw)
        for k in part:
            if k != "stray":
                assert np.array_equal(part[k], full[k][:md]), (k, md)


def test_argmax_under_a_device_side_row_count():
    probe = sub("_probe")
    a, w, bias, _, _, _ = R.inputs(300, 256, 192, 3)
    full, kern = probe.gemm(a, w, bias, argmax=True, n_valid=200, variant=2)
    assert kern == "pipe" and full["stray"] == 0
    for md in (0, 1, 129, 300):
        part, kern = probe.gemm(a, w, bias, argmax=True, n_valid=200, variant=2, m_dev=md)
        assert kern == "pipe" and part["stray"] == 0 and np.array_equal(part["ids"], full["ids"][:md])


@pytest.mark.parametrize("kernel,kw,N,K,epi", [("pipe", dict(variant=3), 128, 192, "bafl"), ("skinny", dict(), 128, 512, "bfl"),
                                               ("f32", dict(precision=1, with_ws=False), 128, 64, "bl")])
def test_a_large_call_before_does_not_change_a_small_one(kernel, kw, N, K, epi):
    alone, *_ = _run(17, N, K, kernel, epi, seed=5, tag="sequence", **kw)
    big_kw = dict(kw, variant=kw.get("variant", 4)) if kernel == "skinny" else kw
    _run(300, N, K, NAME.get(big_kw.get("variant"), kernel), epi, seed=6, check=False, **big_kw)
    after, *_ = _run(17, N, K, kernel, epi, seed=5, check=False, **kw)
    assert _same(alone, after)


def test_a_split_k_call_before_does_not_change_a_smaller_one():
    alone, *_ = _run(65, 128, 1024, "pipe_splitk", "bafl", seed=5, tag="sequence")
    _run(300, 384, 2048, "pipe_splitk", "bafl", seed=6, check=False)
    after, *_ = _run(65, 128, 1024, "pipe_splitk", "bafl", seed=5, check=False)
    assert _same(alone, after)


# ---- the fused row arg-max ------------------------------------------------------------------------------------------------------------------------------
AMAX_N, AMAX_K = 512, 128
AMAX = [("pipe", 1), ("pipe", 2), ("pp", 8), ("pp", 136)]
PAIRS = ((8, 9), (17, 26), (33, 100), (40, 300))                # one register quad, two lanes, two 64-column slabs, two column tiles


def _amax_margin(exact, rounded, dup):
    """Per row: the float64 winner minus the best column that is not one of its copies, and 2 x 3 x E_round (max-abs statistic) of the logits."""
    e = R.e_round(exact["f32"], [r["f32"] for r in rounded])[1]
    z = exact["f32"].copy()
    for m in range(z.shape[0]):
        z[m, dup[m]] = -np.inf
    return exact["f32"][np.arange(z.shape[0]), exact["ids"]] - z.max(axis=1), 2 * R.MARGIN * e


@pytest.mark.parametrize("n_valid", [AMAX_N, AMAX_N - 1, 449, 65])
@pytest.mark.parametrize("kernel,variant", AMAX)
def test_argmax_ties_go_to_the_lowest_index(kernel, variant, n_valid):
    """Duplicate weight rows and biases: equal maxima in one register quad, in two lanes, in two slabs, in two column tiles, and at n_valid - 1 against a
    LARGER copy at n_valid (masked). Every row's winner is planted; the id must be the lowest copy, exactly, on every row."""
    probe = sub("_probe")
    M = 137
    a, w, bias, _, _, _ = R.inputs(M, AMAX_N, AMAX_K, n_valid, scale_rows=False, col_offset=False)
    a, w, bias = a.copy(), w.copy(), bias.copy()
    for lo, hi in PAIRS:
        w[hi], bias[hi] = w[lo], bias[lo]
    last = n_valid - 1
    w[last + 1 if last + 1 < AMAX_N else last] = w[last]
    if last + 1 < AMAX_N:
        bias[last + 1] = bias[last] + 1.0
    targets = [p[0] for p in PAIRS] + [last]
    copies = {p[0]: list(p) for p in PAIRS}
    copies[last] = [last, min(last + 1, AMAX_N - 1)]
    tgt = np.array([targets[m % 5] for m in range(M)])
    a += 40.0 * w[tgt] / (w[tgt] ** 2).sum(1, keepdims=True)
    exact, rounded = R.forms(a, w, bias=bias, n_valid=n_valid)
    assert np.array_equal(exact["ids"], tgt)                      # the float64 statement itself: first index, copies behind n_valid masked
    margin, need = _amax_margin(exact, rounded, [copies[t] for t in tgt])
    assert (margin > need).all(), (margin.min(), need)
    out, kern = probe.gemm(a, w, bias, argmax=True, n_valid=n_valid, variant=variant)
    assert kern == kernel and out["stray"] == 0
    assert np.array_equal(out["ids"], tgt)


@pytest.mark.parametrize("n_valid", [AMAX_N, AMAX_N - 1, 449, 65])
@pytest.mark.parametrize("kernel,variant", AMAX)
def test_argmax_planted_winner_on_every_row(kernel, variant, n_valid):
    probe = sub("_probe")
    M = 300
    a, w, bias, _, _, _ = R.inputs(M, AMAX_N, AMAX_K, n_valid + 1, scale_rows=False, col_offset=False)
    tgt = np.array([(37 * m + 11) % n_valid for m in range(M)])
    a = a + 40.0 * w[tgt] / (w[tgt] ** 2).sum(1, keepdims=True)
    exact, rounded = R.forms(a, w, bias=bias, n_valid=n_valid)
    assert np.array_equal(exact["ids"], tgt)
    assert (exact["margin"] > 2 * R.MARGIN * R.e_round(exact["f32"], [r["f32"] for r in rounded])[1]).all()      # EVERY row is margin-safe
    out, kern = probe.gemm(a, w, bias, argmax=True, n_valid=n_valid, variant=variant)
    assert kern == kernel and out["stray"] == 0
    assert np.array_equal(out["ids"], tgt)
