"""CPU: the references of lowbit_ref.py are themselves checked -- the K partition against a transcription of the kernel's index arithmetic, the float32 orders
against each other, the codecs against torch and exhaustively, and every planted fault against the budget of the inputs the GPU tests use: a fault must land
above 3 x E_round by a factor of at least 10, or the comparison would not notice it."""
import numpy as np
import pytest
import torch

import gemm_ref as R
import lowbit_ref as L

FACTOR = 10.0


def _admissible():
    for K in range(256, 1025, 32):
        for splits in range(1, 17):
            if splits == 1 or (K >> 5) >= 2 * splits:
                yield K, splits


def test_decode_partition_is_the_kernels_index_arithmetic():
    """Every wave of every workgroup walks its K-steps as the kernel's loop does (k_begin, kslice, trips of U steps guarded by k + 32 u < kslice), for both trip
    lengths: every step of K is visited exactly once, in the share decode_partition names, and empty shares are empty."""
    n = 0
    for K, splits in _admissible():
        parts = L.decode_partition(K, splits)
        steps = K >> 5
        seen = np.zeros(steps, np.int64)
        for ks in range(splits):
            wg_lo = steps * ks // splits
            wg_n = steps * (ks + 1) // splits - wg_lo
            assert wg_n >= 2
            for kw in range(8):
                w_lo, w_hi = wg_lo + wg_n * kw // 8, wg_lo + wg_n * (kw + 1) // 8
                k_begin, kslice = w_lo * 32, (w_hi - w_lo) * 32
                for U in (8, 4):
                    visited = []
                    k = 0
                    while k < kslice:
                        visited += [k_begin + k + u * 32 for u in range(U) if k + u * 32 < kslice]
                        k += 32 * U
                    lo, hi = parts[ks][kw]
                    assert visited == list(range(lo, hi, 32)), (K, splits, ks, kw, U)
                seen[w_lo:w_hi] += 1
        assert (seen == 1).all(), (K, splits)
        flat = [p for wg in parts for p in wg]
        assert flat[0][0] == 0 and flat[-1][1] == K and all(a[1] == b[0] for a, b in zip(flat, flat[1:]))
        n += 1
    assert n > 100
    assert sum(lo == hi for wg in L.decode_partition(288, 2) for lo, hi in wg) >= 7          # 9 steps over 2 x 8 waves: waves without a step


@pytest.mark.parametrize("fold", [False, True])
def test_statement_is_gemm_ref_restricted(fold):
    a, wk, bias, add, _ = L.decode_inputs(17, 64, 288, 1, fold, 0.3)
    mine = L.decode_gemm_ref(a, wk["w"], bias=bias, add=add, act=2, fold=fold)
    ref = R.gemm_ref(a, wk["w"], bias=bias, add=add, act=2, ln_dim=288 if fold else 0, only=("f32", "lo"))
    for k in ("f32", "lo"):
        assert np.abs(mine[k] - ref[k]).max() <= 1e-12 * np.abs(ref[k]).max()


@pytest.mark.parametrize("M,N,K,splits,fold,offset,wkind", [(17, 64, 288, 2, False, 0.0, 0), (33, 96, 576, 9, True, 0.3, 1), (64, 32, 1024, 16, True, 0.3, 2),
                                                             (1, 96, 256, 1, True, 0.0, 0), (48, 64, 512, 8, False, 0.0, 2), (49, 64, 576, 9, True, 3.0, 2),
                                                             (31, 32, 512, 4, True, 3.0, 1)])
def test_no_float32_order_sets_the_budget_alone(M, N, K, splits, fold, offset, wkind):
    """Each float32 evaluation, judged as if it were a kernel against the budget of the OTHERS, stays within the margin: E_round is not one outlier order.
    (With the fold at K = 1024 and a row mean of 3 standard deviations it would be: one running sum over 1024 terms puts the sequential order at 5 x the
    others. The fold cases of test_decode_gemm_ref_gpu.py at 3 standard deviations are therefore drawn at K <= 576.)"""
    a, wk, bias, add, s = L.decode_inputs(M, N, K, M + K, fold, offset, wkind)
    spec = dict(bias=bias, add=None if fold else add, fold=fold, w_scale=wk.get("w_scale"))
    exact, rounded = L.decode_forms(a, wk["w"], splits=splits, **spec)
    for i, r in enumerate(rounded):
        others = rounded[:i] + rounded[i + 1:]
        for key in ("f32", "lo"):
            ok, ratio = L.judge(r[key], exact, others, key, s)
            assert ok, (i, key, ratio)


def _fault_ratio(a, w_exact, w_mut, s, splits, keys=("f32", "lo"), mut=None, **spec):
    exact, rounded = L.decode_forms(a, w_exact, splits=splits, **spec)
    bad = L.decode_gemm_ref(a, w_mut, mut=mut, splits=splits, **spec)
    out = {}
    for key in keys:
        ok, ratio = L.judge(bad[key], exact, rounded, key, s)
        assert not ok
        out[key] = max(ratio) / L.MARGIN
    return out


FAULTS = [("drop_split", dict(M=17, N=64, K=1024, splits=16, wkind=0, epi="out")),
          ("drop_split", dict(M=64, N=96, K=288, splits=2, wkind=1, epi="qwen")),
          ("stats_first_split", dict(M=33, N=64, K=512, splits=4, wkind=0, epi="qkv", offset=0.3)),
          ("stats_first_split", dict(M=1, N=32, K=576, splits=9, wkind=2, epi="fc1", offset=0.0)),
          ("w8_scale_late", dict(M=16, N=96, K=512, splits=4, wkind=1, epi="qkv", offset=0.3)),
          ("w8_scale_late", dict(M=49, N=32, K=256, splits=1, wkind=1, epi="fc1", offset=3.0)),
          ("row_block", dict(M=20, N=64, K=256, splits=1, wkind=0, epi="out", block_rows=16)),
          ("row_block", dict(M=33, N=32, K=256, splits=1, wkind=0, epi="qkv", offset=0.3, block_rows=32)),
          ("act_before_add", dict(M=15, N=64, K=256, splits=1, wkind=0, epi="act", act=1)),
          ("act_before_add", dict(M=31, N=96, K=512, splits=4, wkind=1, epi="act", act=2)),
          ("act_before_add", dict(M=63, N=32, K=288, splits=2, wkind=2, epi="act", act=3)),
          ("nibble_swap", dict(M=32, N=64, K=512, splits=8, wkind=2, epi="out")),
          ("scale_neighbour", dict(M=48, N=96, K=576, splits=9, wkind=2, epi="qkv", offset=0.3))]


@pytest.mark.parametrize("mut,case", FAULTS, ids=[f"{m}-{i}" for i, (m, _) in enumerate(FAULTS)])
def test_planted_decode_gemm_faults_land_far_above_the_budget(mut, case):
    fold = case["epi"] in ("qkv", "fc1")
    a, wk, bias, add, s = L.decode_inputs(case["M"], case["N"], case["K"], 7, fold, case.get("offset", 0.0), case["wkind"])
    spec = dict(bias=None if case["epi"] == "qwen" else bias, add=None if fold else add, fold=fold, w_scale=wk.get("w_scale"),
                act=case.get("act", 2 if case["epi"] == "fc1" else 0))
    w_mut, m = wk["w"], mut
    if mut == "scale_neighbour":
        w_mut, m = L.mxfp4_dequant(wk["wq"], wk["w_scale8"], mut="scale_neighbour").astype(np.float32), None
        assert np.array_equal(L.mxfp4_dequant(wk["wq"], wk["w_scale8"]), wk["w"])
    if mut == "nibble_swap":                                     # the two spellings of the fault are the same fault
        assert np.array_equal(L.mxfp4_dequant(wk["wq"], wk["w_scale8"], mut="nibble_swap"), wk["w"].reshape(case["N"], -1, 2)[:, :, ::-1].reshape(case["N"], -1))
    if mut == "row_block":
        spec["block_rows"] = case["block_rows"]
    ratio = _fault_ratio(a, wk["w"], w_mut, s, case["splits"], mut=m, **spec)
    print(mut, case, ratio)
    assert all(r >= FACTOR for r in ratio.values()), ratio


def test_codecs_round_trip_every_code():
    codes = np.arange(256, dtype=np.uint8)
    ok = ~np.isnan(L.E4M3)
    assert (~ok).sum() == 2 and not ok[0x7F] and not ok[0xFF]
    back = L.e4m3_encode(L.E4M3[ok])
    zero = L.E4M3[ok] == 0
    assert np.array_equal(back[~zero], codes[ok][~zero]) and np.array_equal(back[zero] & 0x7F, np.zeros(zero.sum(), np.uint8))
    assert np.array_equal(L.e4m3_encode(np.array([-0.0]))[0:1], np.array([0x80], np.uint8))
    assert L.e4m3_encode(np.array([np.nan]))[0] == 0x7F and np.array_equal(L.e4m3_encode(np.array([1e9, -1e9, 464.0])), np.array([0x7E, 0xFE, 0x7E], np.uint8))
    t8 = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float64).numpy()
    assert np.array_equal(t8[ok], L.E4M3[ok]) and np.isnan(t8[~ok]).all()
    c4 = np.arange(16, dtype=np.uint8)
    v4 = L.e2m1_decode(c4)
    assert np.array_equal(np.abs(v4[:8]), L.E2M1_LEVELS) and np.array_equal(v4[8:], -v4[:8])
    nz = (c4 & 7) != 0
    assert np.array_equal(L.e2m1_encode(v4)[nz], c4[nz]) and np.array_equal(L.e2m1_encode(v4)[~nz] & 7, np.zeros(2, np.uint8))
    assert np.array_equal(L.e2m1_encode(np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 7.0, -5.0])), np.array([0, 2, 2, 4, 4, 6, 6, 7, 14], np.uint8))      # ties to even
    assert np.array_equal(L.e8m0_decode(np.array([127, 1, 254])), np.array([1.0, 2.0 ** -126, 2.0 ** 127]))
    p = L.mxfp4_pack(np.array([[1, 10, 7, 0]], np.uint8))
    assert np.array_equal(p, np.array([[0xA1, 0x07]], np.uint8))


def test_reference_quantisers_agree_with_torch():
    rng = np.random.default_rng(3)
    x = np.clip(rng.standard_normal(200000) * np.exp(rng.uniform(-9, 6.2, 200000)), -448, 448).astype(np.float32)
    want = torch.from_numpy(x).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(L.e4m3_encode(x.astype(np.float64)), want)
    grid = L.E4M3[:0x7F]
    mids = 0.5 * (grid[1:] + grid[:-1])                          # every tie of the format (exact in f32)
    want = torch.from_numpy(mids.astype(np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(L.e4m3_encode(mids), want)
    w = L.np_bf16(rng.standard_normal((24, 256)) * np.exp(rng.uniform(-6, 3, (24, 1))))
    w[3] = 0.0
    q, s, dq = L.fp8_rows_reference(w)
    amax = np.abs(w).max(axis=1)
    assert s[3] == 1.0 and (((amax / s > 224.0) & (amax / s <= 448.0)) | (amax == 0)).all()
    t8 = torch.from_numpy(w / s[:, None]).to(torch.float8_e4m3fn)
    assert np.array_equal(q, t8.view(torch.uint8).numpy()) and np.array_equal(dq, t8.to(torch.float64).numpy() * s[:, None])
    assert np.array_equal(L.np_bf16(dq), dq.astype(np.float32))          # the dequantisation is exact in bf16
    codes, sb, dq4 = L.mxfp4_reference(w)
    assert np.array_equal(L.mxfp4_dequant(L.mxfp4_pack(codes), sb), dq4) and np.array_equal(L.np_bf16(dq4), dq4.astype(np.float32))


def test_crosskv_reference_and_its_planted_fault():
    x, row_off, n_lfr = L.crosskv_slabs()
    for dq in (False, True):
        q, sc, after = L.crosskv_ref(x, row_off, n_lfr, dq)
        assert sc.shape == (3, 4) and (sc[:, 0] == 1.0).all()
        for s in range(3):
            for b, (r0, n) in enumerate(zip(row_off, n_lfr)):
                if n:
                    amax = np.abs(x[s, r0:r0 + n]).max()
                    assert 224.0 < amax / sc[s, b] <= 448.0
                    t8 = torch.from_numpy(x[s, r0:r0 + n] / sc[s, b]).to(torch.float8_e4m3fn)
                    assert np.array_equal(q[s, r0:r0 + n], t8.view(torch.uint8).numpy())
        covered = np.zeros(240, bool)
        for r0, n in zip(row_off, n_lfr):
            covered[r0:r0 + n] = True
        assert (q[:, ~covered] == L.SENTINEL).all() and np.array_equal(after[:, ~covered], x[:, ~covered])
        assert np.array_equal(after, x) != dq
    bad = L.crosskv_ref(x, row_off, n_lfr, mut="scale_over_slab")
    good = L.crosskv_ref(x, row_off, n_lfr)
    assert (bad[1][:, 1:3] != good[1][:, 1:3]).all() and not np.array_equal(bad[0], good[0])          # exact assertions: any difference is a failure


@pytest.mark.parametrize("D,rows,inv", L.LN_CASES)
def test_layernorm_fp8_reference_budget_and_planted_fault(D, rows, inv):
    x = L.ln_input(rows, D, D + 8, 0)
    y = L.layernorm_fp8_ref(x, D, 1e-5, inv)
    forms = [L.layernorm_fp8_ref(x, D, 1e-5, inv, rounded="f32", order=o) for o in L.LN_ORDERS]
    bound = L.fp8_store_bound(y, forms)
    for f in forms:                                              # every float32 form, stored as e4m3, meets the bound it helps to set
        got = L.e4m3_decode(L.e4m3_encode(L.clamp448(f)))
        assert (np.abs(got - L.clamp448(y)) <= bound).all()
    assert (np.abs(y) > 448.0).any() == L.ln_saturates(D, inv)
    bad = L.e4m3_decode(L.e4m3_encode(L.clamp448(L.layernorm_fp8_ref(x, D, 1e-5, inv, mut="no_mean"))))
    excess = np.abs(bad - L.clamp448(y)) / bound
    assert excess.max() >= FACTOR, excess.max()


def test_gemm_fp8_reference_orders_agree():
    rng = np.random.default_rng(2)
    a8 = L.e4m3_encode(rng.standard_normal((5, 256)) * 4)
    w8 = L.e4m3_encode(rng.standard_normal((256, 256)) * 4)
    sc, bias = np.full(256, 2.0 ** -6, np.float32), rng.standard_normal(256).astype(np.float32)
    exact = L.gemm_fp8_ref(a8, w8, sc, 0.5, bias, act=2, out_inv_scale=4.0)
    forms = [L.gemm_fp8_ref(a8, w8, sc, 0.5, bias, act=2, out_inv_scale=4.0, rounded="f32", order=o) for o in L.FP8_ORDERS]
    for i, f in enumerate(forms):
        ok, ratio = L.within(f["y"], exact["y"], [g["y"] for j, g in enumerate(forms) if j != i])
        assert ok, (i, ratio)
    assert exact["sat"] == int((np.abs(exact["y"]) > 448).sum())
