"""CPU: the float64 GEMM statement of gemm_ref.py against torch's own operators on every epilogue, every float32 order inside E_round, and the planted
faults of the GemmArgs checklist rejected by within() on the smallest shapes test_gemm_ref_gpu.py runs."""
import numpy as np
import pytest
import torch

import gemm_ref as R

F = torch.nn.functional
M, N, K = 17, 128, 64            # the smallest shape of the GPU grid: one ragged row tile (M % 4 == 1), one column tile, one bf16 K step


def _b(x):
    return torch.from_numpy(np.asarray(x, np.float32)).to(torch.bfloat16).double()


def _d(x):
    return torch.from_numpy(np.asarray(x, np.float64))


@pytest.fixture(scope="module")
def data():
    return R.inputs(M, N, K, 1, table_rows=M + 7)


def _close(x, y):
    return np.allclose(np.asarray(x), np.asarray(y), rtol=1e-11, atol=1e-11)


def test_statement_matches_torch_on_every_epilogue(data):
    a, w, bias, add, add2, _ = data
    rows = np.array([(5 * m + 3) % (M + 7) for m in range(M)])
    rows[1], rows[4] = rows[0], M + 6                       # a repeat and the last row of the table: arbitrary, non-monotone
    lin = F.linear(_b(a), _b(w), _d(bias))
    assert _close(R.gemm_ref(a, w, bias)["f32"], lin)
    assert _close(R.gemm_ref(a, w, bias, act=1)["f32"], torch.relu(lin))
    assert _close(R.gemm_ref(a, w, bias, add=add, act=2, add2=add2, add2_rows=rows)["f32"], F.gelu(lin + _d(add)) + _d(add2)[rows])
    assert _close(R.gemm_ref(a, w, bias, act=3, add2=add2)["f32"], F.gelu(lin, approximate="tanh") + _d(add2)[:M])
    z = F.linear(_b(a), _b(w))
    assert _close(R.gemm_ref(a, w, act=4)["f32"], F.silu(z[:, 0::2]) * z[:, 1::2])
    assert _close(R.gemm_ref(a, w, operand="f32")["f32"], F.linear(_d(a), _d(w)))
    ln = F.linear(F.layer_norm(_b(a), (K,), None, None, 1e-5), _b(w), _d(bias))
    assert np.allclose(R.gemm_ref(a, w, bias, act=1, ln_dim=K)["f32"], torch.relu(ln), rtol=1e-9, atol=1e-9)
    x = _b(a)
    rms = F.linear(x * torch.rsqrt((x * x).mean(1, keepdim=True) + 1e-6), _b(w))
    assert np.allclose(R.gemm_ref(a, w, a_rms_eps=1e-6)["f32"], rms, rtol=1e-10, atol=1e-10)
    full = R.gemm_ref(a, w, bias, lo_group=64, rms_eps=1e-6, n_valid=N - 1)
    assert _close(full["t"], lin.t()) and _close(full["slabs"], lin.reshape(M, 2, 64).permute(1, 0, 2))
    assert _close(R.unlay_slabs(full["slabs"], M), lin)
    assert _close(full["rms"], lin * torch.rsqrt((lin * lin).mean(1, keepdim=True) + 1e-6))
    lo = _b(lin.numpy()).reshape(M, N // 32, 32)
    assert _close(full["stats"][..., 0], lo.sum(-1)) and _close(full["stats"][..., 1], (lo * lo).sum(-1))
    assert np.array_equal(full["ids"], lin[:, :N - 1].argmax(1).numpy())


def test_argmax_takes_the_first_index_and_respects_n_valid():
    v = np.zeros((3, 8))
    v[0, [2, 5]] = 1.0
    v[1, 7] = 9.0
    v[2, [6, 7]] = (4.0, 5.0)
    ids, margin = R.argmax_first(v, 7)
    assert ids.tolist() == [2, 0, 6] and margin.tolist() == [0.0, 0.0, 4.0]


@pytest.mark.parametrize("spec", [dict(act=1), dict(act=2, add2=True), dict(act=4), dict(ln_dim=K, act=1), dict(a_rms_eps=1e-6), dict(operand="f32")])
def test_every_float32_order_is_inside_its_own_e_round(data, spec):
    a, w, bias, add, add2, s = data
    spec = dict(spec)
    if spec.pop("add2", False):
        spec["add2"] = add2
    if spec.get("act") != 4:
        spec["bias"] = bias
    exact, rounded = R.forms(a, w, **spec)
    assert len(rounded) >= 8                                  # seq, lib and the blockings that divide K = 64
    for key in ("f32", "lo"):
        e = R.e_round(exact[key], [r[key] for r in rounded])
        assert e[0] > 0 and e[1] > 0
        for r in rounded:
            ok, ratio = R.judge(r[key], exact, rounded, key, s)
            assert ok and max(ratio) <= 1.0 + 1e-12, (key, ratio)


FAULTS = {
    "drop_k16": (dict(bias=True, act=1), "lo"),
    "swap_cols": (dict(bias=True), "lo"),
    "no_bias_group": (dict(bias=True, act=2), "lo"),
    "add2_before_act": (dict(bias=True, act=2, add2=True), "f32"),
    "gate_up_swapped": (dict(act=4), "lo"),
    "row_shift": (dict(bias=True), "f32"),
    "t_tail_stale": (dict(bias=True), "t"),
    "slab_off_by_one": (dict(bias=True, lo_group=64), "slabs"),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_within_rejects_planted_fault(data, fault):
    a, w, bias, add, add2, s = data
    flags, key = FAULTS[fault]
    spec = {k: v for k, v in flags.items() if k not in ("bias", "add2")}
    if flags.get("bias"):
        spec["bias"] = bias
    if flags.get("add2"):
        spec["add2"] = add2
    exact, rounded = R.forms(a, w, **spec)
    lay = (lambda x: x.T) if key == "t" else (lambda x: R.unlay_slabs(x, M)) if key == "slabs" else (lambda x: x)
    ex, ro = {key: lay(exact[key])}, [{key: lay(r[key])} for r in rounded]
    for order in ("seq", (32, 2)):
        good = R.gemm_ref(a, w, rounded="f32", order=order, **spec)
        bad = R.gemm_ref(a, w, rounded="f32", order=order, mut=fault, **spec)
        assert R.judge(lay(good[key]), ex, ro, key, s)[0]
        ok, ratio = R.judge(lay(bad[key]), ex, ro, key, s)
        assert not ok and max(ratio) > 10 * R.MARGIN, (fault, ratio)      # not a near miss: an order of magnitude outside the margin


def test_within_rejects_statistics_of_the_unrounded_values(data):
    a, w, bias, add, add2, _ = data
    got = R.gemm_ref(a, w, bias, add=add, rounded="f32", order="seq")
    bad = R.gemm_ref(a, w, bias, add=add, rounded="f32", order="seq", mut="stats_unrounded")
    exact = R.stats_of(got["lo"])                             # float64 sums of the bf16 values the launch returned
    rounded = [R.stats_of(got["lo"], np.float32, o) for o in ("seq", "pair")]
    for i in (0, 1):
        assert R.within(got["stats"][..., i], exact[..., i], [r[..., i] for r in rounded])[0]
        assert not R.within(bad["stats"][..., i], exact[..., i], [r[..., i] for r in rounded])[0]


def test_a_tie_resolved_to_the_higher_index_is_seen(data):
    a, w, bias, _, _, _ = data
    w, bias = w.copy(), bias.copy()
    a = a + 2.0 * w[5][None, :] * np.linspace(1, 2, M, dtype=np.float32)[:, None] * K        # column 5 wins every row ...
    w[70], bias[70] = w[5], bias[5]                                                           # ... and column 70 ties with it
    exact = R.gemm_ref(a, w, bias, n_valid=N)
    assert (exact["ids"] == 5).all() and (exact["margin"] == 0).all()
    bad = R.gemm_ref(a, w, bias, n_valid=N, rounded="f32", order="seq", mut="tie_high")
    assert (bad["ids"] == 70).all() and not np.array_equal(bad["ids"], exact["ids"])
    assert np.array_equal(R.gemm_ref(a, w, bias, n_valid=N, rounded="f32", order="lib")["ids"], exact["ids"])
