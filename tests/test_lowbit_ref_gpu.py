"""GPU: the low-bit kernels that no test reached directly -- the FP8 cross-K/V quantiser, LayerNorm -> e4m3 operand rows, and the FP8 matrix-pipe GEMM at
M < 256, with pitches, non-unit scales, every activation, group_m and the saturation count -- against the references of lowbit_ref.py.

Tolerances. Quantiser scales, bytes and dequantisations are exact. A value stored as e4m3 is bounded per element, without a cap:
|decode(byte) - clamp(y)| <= half an e4m3 ulp at y + 3 x E_round, y the float64 value before the clamp and E_round the worst |exact - float32 form| of the
element's row (lowbit_ref.fp8_store_bound). The f32 output of the matrix-pipe GEMM is judged by within() at margin 3 against the float64 product of the decoded
bytes, E_round from the float32 orders in steps of 128. sat_count is compared exactly, after the test has asserted that no exact value lies within 3 x E_round of
+-448: the saturating values are planted through the bias (two columns, far outside), the others stay far inside.

A limit of the contract, found by these tests: the FP8 matrix instruction does not add its 128 products in float32. On general e4m3 operands (normal values at
scale 4, products up to 324) the f32 output differs from the float64 product by up to 430 float32 ulps of the sum (140 .. 230 x E_round of the float32 orders, up
to 1.5e-5 of sum |a||w| + 1, mean error negative: the products are aligned to the largest of the instruction and the bits below are dropped), while operands of one
binade and whole-number operands give float32(exact sum) bit for bit at every shape here. No float32 summation order describes that, so the float32 budget holds
only where the pipe is exact: the within() and half-ulp cases use whole-number operands -8 .. 8 (all exact in e4m3; bias, scales, residual and activation stay
general, so the epilogue, the pitches, the row guard, group_m and sat_count are tested in full), and the same launches run on general operands under the bound
test_whisper_fp8_gpu.py has always put on this kernel, 2e-5 of sum |a||w| + 1, with the float32 ratio printed. Fp8GemmArgs (csrc/gemm.h) now says so.

Measured on an MI355X, worst case per class (an e4m3 store sits at its own rounding, 1.00, as a bf16 store does in test_gemm_ref_gpu.py):

  class (cases)                                                    figure
  cross-K/V quantiser, row quantisers at ld > K                    exact (scales, bytes, dequantisation, gap rows)
  LayerNorm -> e4m3, 11 cases                                      error / bound 1.000; error / half ulp alone 0.9999 (no element needs the 3 x E_round part)
  FP8 GEMM f32 store, whole-number operands (5)                    stat / E_round 1.00  1.00   (|err| <= 1.5e-7 of sum |a||w| + 1)
  FP8 GEMM f32 store, general operands (5)                         stat / E_round 134 .. 155 (RMS), 140 .. 231 (max); |err| <= 1.45e-5 of sum |a||w| + 1, bound 2e-5
  FP8 GEMM byte store, whole-number operands, act 0..3 (20)        error / bound 1.000
  FP8 GEMM byte store, general operands, act 0..3 (20)             error / (half ulp + 3 E_round) up to 1.95: elements next to a rounding tie that the pipe moves across it
  sat_count (40)                                                   equal to the reference's count
"""
import numpy as np
import pytest
import torch

import lowbit_ref as L
from conftest import sub

pytestmark = pytest.mark.gpu


# ---- the FP8 cross-K/V cache ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dq_in_place", [False, True])
def test_crosskv_quantiser_scales_bytes_dequantisation_and_gaps(dq_in_place):
    probe = sub("_probe")
    x, row_off, n_lfr = L.crosskv_slabs()
    q, sc, after = probe.quantize_crosskv_fp8(x, row_off, n_lfr, dq_in_place)
    want_q, want_sc, want_after = L.crosskv_ref(x, row_off, n_lfr, dq_in_place)
    assert np.array_equal(sc, want_sc)                          # one power-of-two scale per (slab, sequence); 1 for the empty sequence
    covered = np.zeros(x.shape[1], bool)
    for s in range(x.shape[0]):
        for b, (r0, n) in enumerate(zip(row_off, n_lfr)):
            covered[r0:r0 + n] = True
            if n:
                amax = np.abs(x[s, r0:r0 + n]).max()
                assert 224.0 < amax / sc[s, b] <= 448.0
                t8 = torch.from_numpy(x[s, r0:r0 + n] / sc[s, b]).to(torch.float8_e4m3fn)
                assert np.array_equal(q[s, r0:r0 + n], t8.view(torch.uint8).numpy())          # torch's OCP e4m3fn conversion of value / scale
                if dq_in_place:
                    assert np.array_equal(after[s, r0:r0 + n], t8.to(torch.float32).numpy() * sc[s, b])
    assert np.array_equal(q, want_q) and np.array_equal(after.astype(np.float64), want_after)
    assert (q[:, ~covered] == L.SENTINEL).all() and np.array_equal(after[:, ~covered], x[:, ~covered])      # gap rows: bytes and bf16 untouched
    if not dq_in_place:
        assert np.array_equal(after, x)


# ---- the row quantisers with a row pitch above K ---------------------------------------------------------------------------------------------------------------
def _weights(N, K, seed):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((N, K)) * np.exp(rng.uniform(-6, 3, (N, 1)))).astype(np.float32)
    w[3] = 0.0
    w[5, K - 8:] = [448.0, -448.0, 6.0, -6.0, 0.25, 0.75, 464.0, 1e-4]          # the last columns of a row: what sits next to the gap
    return w


@pytest.mark.parametrize("ld", [512 + 8, 512 + 40])
def test_fp8_row_quantiser_with_a_row_pitch_above_k(ld):
    """The gap holds 1.7e38: a quantiser that read past K would take its scale from it. Bytes, scales and the dequantisation are the reference's and the
    contiguous run's."""
    probe = sub("_probe")
    w = _weights(48, 512, 5)
    q, sc, dq = probe.quantize_fp8(w, ld=ld)
    want_q, want_sc, want_dq = L.fp8_rows_reference(L.np_bf16(w))
    assert np.array_equal(sc, want_sc) and np.array_equal(q, want_q) and np.array_equal(dq.astype(np.float64), want_dq)
    assert all(np.array_equal(x, y) for x, y in zip((q, sc, dq), probe.quantize_fp8(w)))


@pytest.mark.parametrize("ld", [256 + 8, 256 + 40])
def test_mxfp4_block_quantiser_with_a_row_pitch_above_k(ld):
    probe = sub("_probe")
    w = _weights(40, 256, 11)
    q, sc, dq = probe.quantize_mxfp4(w, ld=ld)
    want_code, want_sc, want_dq = L.mxfp4_reference(L.np_bf16(w))
    got_code = np.stack([q & 15, q >> 4], axis=2).reshape(q.shape[0], -1)
    zero = (want_code & 7) == 0                                               # (the sign of a zero code carries no value)
    assert np.array_equal(sc, want_sc) and np.array_equal(got_code & 7, want_code & 7) and np.array_equal((got_code >> 3)[~zero], (want_code >> 3)[~zero])
    assert np.array_equal(dq.astype(np.float64), want_dq)
    assert all(np.array_equal(x, y) for x, y in zip((q, sc, dq), probe.quantize_mxfp4(w)))


# ---- LayerNorm -> e4m3 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,rows,inv", L.LN_CASES)
def test_layernorm_fp8_per_element(D, rows, inv):
    probe = sub("_probe")
    ld_x, ld_out = D + 8, D + 12
    x = L.ln_input(rows, D, ld_x, 1)
    out = probe.layernorm_fp8(x, D, 1e-5, inv, ld_out)
    assert (out[rows:] == L.SENTINEL).all() and (out[:, D:] == L.SENTINEL).all()
    y = L.layernorm_fp8_ref(x, D, 1e-5, inv)
    forms = [L.layernorm_fp8_ref(x, D, 1e-5, inv, rounded="f32", order=o) for o in L.LN_ORDERS]
    assert (np.abs(y) > 448.0).any() == L.ln_saturates(D, inv)
    got = L.e4m3_decode(out[:rows, :D])
    assert not np.isnan(got).any()
    excess = np.abs(got - L.clamp448(y)) / L.fp8_store_bound(y, forms)
    half = np.abs(got - L.clamp448(y)) / (0.5 * L.e4m3_ulp(y))
    print(f"RATIO layernorm_fp8 D={D} rows={rows} inv={inv} error / bound max={excess.max():.3f}  error / half ulp max={half.max():.4f}")
    assert (excess <= 1.0).all(), excess.max()


# ---- the FP8 matrix-pipe GEMM --------------------------------------------------------------------------------------------------------------------------------
FP8_SHAPES = [(1, 256, 256), (255, 256, 256), (257, 512, 256), (300, 256, 512), (3841, 256, 256)]


def _fp8_operands(M, N, K, seed, integer=False):
    """General operands: asymmetric normal values at scale 4 rounded to e4m3. integer: whole numbers -8 .. 8 (exact in e4m3; every product and every partial sum
    is a whole number below 2^14, which the matrix pipe's adder holds exactly)."""
    rng = np.random.default_rng([M, N, K, seed])
    if integer:
        a8 = L.e4m3_encode(np.clip(rng.integers(-7, 8, (M, K)) + np.sign(np.linspace(-1, 1, K))[None, :], -8, 8))
        w8 = L.e4m3_encode(np.clip(rng.integers(-7, 8, (N, K)) + (np.arange(N) % 2)[:, None], -8, 8))
    else:
        a8 = L.e4m3_encode((rng.standard_normal((M, K)) + np.linspace(-0.5, 0.5, K)[None, :]) * 4.0)
        w8 = L.e4m3_encode((rng.standard_normal((N, K)) + np.linspace(0, 0.5, N)[:, None]) * 4.0)
    w_scale = (2.0 ** rng.integers(-8, -5, N)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    add = (rng.standard_normal((M, N)) * 3.0).astype(np.float32)
    return a8, w8, w_scale, bias, add


PITCH = dict(lda=16, ldw=32, ld_add=16, ld_out=8)


def _fp8_f32(M, N, K, integer):
    probe = sub("_probe")
    a8, w8, w_scale, bias, add = _fp8_operands(M, N, K, 0, integer)
    a_scale = 0.25
    out, _ = probe.gemm_fp8_v2(a8, w8, w_scale, bias, a_scale=a_scale, add=add, lda=K + PITCH["lda"], ldw=K + PITCH["ldw"], ld_add=N + PITCH["ld_add"],
                               ld_out=N + PITCH["ld_out"])
    assert np.isnan(out[M:]).all() and np.isnan(out[:, N:]).all()          # rows past M and the pitch gap are untouched
    exact = L.gemm_fp8_ref(a8, w8, w_scale, a_scale, bias, add=add)["f32"]
    forms = [L.gemm_fp8_ref(a8, w8, w_scale, a_scale, bias, add=add, rounded="f32", order=o)["f32"] for o in L.FP8_ORDERS]
    ok, ratio = L.within(out[:M, :N], exact, forms)
    mag = (np.abs(L.e4m3_decode(a8)) @ np.abs(L.e4m3_decode(w8)).T) * (w_scale.astype(np.float64) * a_scale)[None, :] + 1.0
    rel = (np.abs(out[:M, :N] - exact) / mag).max()
    print(f"RATIO gemm_fp8 f32 {'integer' if integer else 'general'} {M}x{N}x{K} rms={ratio[0]:.3f} max={ratio[1]:.3f}  |err| / (sum |a||w| + 1) max={rel:.2e}")
    return ok, ratio, rel


@pytest.mark.parametrize("M,N,K", FP8_SHAPES)
def test_fp8_gemm_f32_output(M, N, K):
    """within() at margin 3 against the float64 product, on operands whose sums the matrix pipe holds exactly (see the module text): rows below the 256-row tile,
    pitches on every operand, non-unit a_scale, the group_m walk of the 3841-row case."""
    ok, ratio, _ = _fp8_f32(M, N, K, integer=True)
    assert ok, ratio


@pytest.mark.parametrize("M,N,K", FP8_SHAPES)
def test_fp8_gemm_f32_output_on_general_operands(M, N, K):
    """The same launches on general e4m3 operands, under the bound test_whisper_fp8_gpu.py has always put on this kernel at M >= 256 (2e-5 of sum |a||w| + 1);
    the stat / E_round ratio against the float32 orders is printed, not asserted: the matrix pipe does not add in float32 (module text)."""
    _, _, rel = _fp8_f32(M, N, K, integer=False)
    assert rel < 2e-5, rel


def _fp8_bytes(M, N, K, act, integer):
    """One byte-output launch: sentinels, the saturation count (exactly), -> (|decode(byte) - clamp(y)|, the half-ulp + 3 x E_round bound, inv x (sum |a||w| + 1))."""
    probe = sub("_probe")
    a8, w8, w_scale, bias, _ = _fp8_operands(M, N, K, 1 + act, integer)
    a_scale, inv = 0.5, 8.0
    bias = bias.copy()
    bias[5], bias[N - 3] = 600.0 / inv, -700.0 / inv                       # two columns far outside +-448 (the negative one only where the activation keeps it)
    exact = L.gemm_fp8_ref(a8, w8, w_scale, a_scale, bias, act=act, out_inv_scale=inv)
    forms = [L.gemm_fp8_ref(a8, w8, w_scale, a_scale, bias, act=act, out_inv_scale=inv, rounded="f32", order=o) for o in L.FP8_ORDERS]
    if act == 2:
        forms.append(L.gemm_fp8_ref(a8, w8, w_scale, a_scale, bias, act=act, out_inv_scale=inv, rounded="f32", order="seq", gelu="fast"))
    y = exact["y"]
    e = L.e_round(y, [f["y"] for f in forms])[1]
    mag = inv * ((np.abs(L.e4m3_decode(a8)) @ np.abs(L.e4m3_decode(w8)).T) * (w_scale.astype(np.float64) * a_scale)[None, :] + 1.0)
    edge = L.MARGIN * e + (0.0 if integer else 1.13 * 2e-5 * mag)
    assert (np.abs(np.abs(y) - 448.0) > edge).all()                        # no exact value near the edge: the count is decided
    assert exact["sat"] == M * (2 if act == 0 else 1) and all(f["sat"] == exact["sat"] for f in forms)
    out, sat = probe.gemm_fp8_v2(a8, w8, w_scale, bias, a_scale=a_scale, act=act, out_inv_scale=inv, lda=K + PITCH["lda"], ldw=K + PITCH["ldw"],
                                 ld_out=N + PITCH["ld_out"])
    assert (out[M:] == L.SENTINEL).all() and (out[:, N:] == L.SENTINEL).all()
    assert sat == exact["sat"], (sat, exact["sat"])
    got = L.e4m3_decode(out[:M, :N])
    assert not np.isnan(got).any()
    return np.abs(got - L.clamp448(y)), L.fp8_store_bound(L.clamp448(y), [L.clamp448(f["y"]) for f in forms]), mag


@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("M,N,K", FP8_SHAPES)
def test_fp8_gemm_byte_output_and_saturation_count(M, N, K, act):
    """Every element within half an e4m3 ulp + 3 x E_round, sat_count exact, rows past M and the pitch gap untouched -- on operands whose sums the matrix pipe
    holds exactly (module text)."""
    err, bound, _ = _fp8_bytes(M, N, K, act, integer=True)
    print(f"RATIO gemm_fp8 bytes integer act={act} {M}x{N}x{K} error / bound max={(err / bound).max():.3f}")
    assert (err <= bound).all(), (err / bound).max()


@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("M,N,K", FP8_SHAPES)
def test_fp8_gemm_byte_output_on_general_operands(M, N, K, act):
    """General operands: the bound grows by what the matrix pipe may lose before the epilogue, 2e-5 of sum |a||w| + 1 (the bound of test_whisper_fp8_gpu.py) times
    out_inv_scale and the largest slope of an activation (1.13, the erf-GELU's); sat_count stays exact. The ratio to the bound without that term is printed."""
    err, bound, mag = _fp8_bytes(M, N, K, act, integer=False)
    print(f"RATIO gemm_fp8 bytes general act={act} {M}x{N}x{K} error / (half ulp + 3 E_round) max={(err / bound).max():.3f}")
    assert (err <= bound + 1.13 * 2e-5 * mag).all()
