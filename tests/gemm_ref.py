"""Float64 statement of what GemmArgs (csrc/gemm.h) means, its float32 evaluations in the summation orders the kernels use along K (they exist ONLY to
measure the rounding noise E_round = stat(exact - rounded)), the inputs on which GEMM faults show, and planted faults that prove the comparison.

gemm_ref(a, w, ...) in the order gemm.h documents the terms:

  operands   a [M][K], w [N][K] rounded to the operand dtype (bf16, or kept for the f32 kernel), then C = A W^T
  LayerNorm  folded (ln_dim): C = rstd (x W^T - mean colsum), statistics of the first ln_dim columns of the rounded rows, colsum[n] = sum_k W[n][k]
  RMSNorm    folded (a_rms_eps): C = rsqrt(mean_k x^2 + eps) (x W^T)
  epilogue   + bias + add, activation (0 none, 1 ReLU, 2 erf-GELU, 3 tanh-GELU, 4 SwiGLU over interleaved gate / up columns -> N / 2 outputs),
             + add2[add2_rows[m]] AFTER the activation
  outputs    "f32" the value; "lo" the value rounded to the operand dtype; "t" = lo transposed; "slabs" = lo as [N / lo_group][M][lo_group];
             "stats" (sum, sum of squares) per 32 columns of the bf16-ROUNDED values; "rms" = value * rsqrt(mean_n value^2 + rms_eps) (operand dtype);
             "ids" the row arg-max over n < n_valid, first index on ties, with "margin" = top-1 minus top-2

rounded=None states the function in float64 (only the operands are rounded: "lo" is then the unrounded value, so that the output rounding is part of
E_round and not of the statement); rounded="f32" evaluates it in float32 with the product summed in `order` and the stores rounded.
"""
import os
import re

import numpy as np
import torch

from front_end_ref import MARGIN, e_round, stat, within  # noqa: F401  (the comparison is the front ends': imported, not copied)

F = torch.nn.functional
F64, F32 = torch.float64, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACT_NONE, ACT_RELU, ACT_GELU_ERF, ACT_GELU_TANH, ACT_SWIGLU = 0, 1, 2, 3, 4

# float32 summation orders along K. "seq": one running sum, k ascending; "lib": the library's blocked product; (B, ways): the matrix pipe's shape -- K in
# `ways` contiguous parts (K halves of the 144-row tiles, the eight waves of the weight-streaming kernel, split-K passes), each part a running f32 sum of
# B-long dot products (one MFMA K-step: 16, 32 or 64 elements enter the accumulator together), the parts then added in order
ORDERS = ("seq", "lib") + tuple((b, ways) for b in (16, 32, 64) for ways in (1, 2, 4, 8))


def bf16(t):
    return t.to(F32).to(torch.bfloat16).to(t.dtype)


def _t(x, dt):
    return torch.as_tensor(np.asarray(x)).to(dt)


def mm32(a, w, order):
    """a [M][K] x w [N][K]^T in float32, summed along K in `order`; None when the order does not divide K."""
    assert a.dtype == F32 and w.dtype == F32
    M, K = a.shape
    if order == "lib":
        return a @ w.t()
    if order == "seq":
        acc = torch.zeros(M, w.shape[0], dtype=F32)
        for k in range(K):
            acc += a[:, k:k + 1] * w[:, k].unsqueeze(0)
        return acc
    b, ways = order
    if K % (b * ways) != 0:
        return None
    part, tot = K // ways, None
    a64, w64 = a.to(F64), w.to(F64)
    for h in range(ways):
        acc = torch.zeros(M, w.shape[0], dtype=F32)
        for k in range(h * part, (h + 1) * part, b):
            acc += (a64[:, k:k + b] @ w64[:, k:k + b].t()).to(F32)          # a B-long dot product enters the accumulator as one rounded term
        tot = acc if tot is None else tot + acc
    return tot


def _fast_gelu_coef():
    """The constants of gelu_erf_fast2 as they stand in csrc/gemm_dev.h (the regular expressions of test_formulas_cpu.py)."""
    src = open(os.path.join(ROOT, "automatic-speech-recognition-asr-onnx_amd", "csrc", "gemm_dev.h")).read()
    body = src[src.index("void gelu_erf_fast2"):src.index("float gelu_erf_fast(float v)")]
    lead = re.search(r"q = a \* ([-0-9.e+]+)f \+ ([-0-9.e+]+)f;", body)
    rest = re.findall(r"q = q \* a \+ ([-0-9.e+]+)f;", body)
    clamp = float(re.search(r"fminf\(fabsf\(v0\), ([0-9.]+)f\)", body).group(1))
    return [np.float32(lead.group(1)), np.float32(lead.group(2))] + [np.float32(c) for c in rest], np.float32(clamp)


def fast_gelu32(v):
    """gelu_erf_fast2 in float32: max(v, 0) - a 2^q(a), a = min(|v|, clamp), Horner from the highest order."""
    coef, clamp = _fast_gelu_coef()
    x = v.numpy().astype(np.float32)
    a = np.minimum(np.abs(x), clamp)
    q = coef[0] * a + coef[1]
    for c in coef[2:]:
        q = q * a + c
    return torch.from_numpy((np.maximum(x, np.float32(0)) - a * np.exp2(q)).astype(np.float32))


def _act(v, act, gelu, mut):
    if act == ACT_RELU:
        return torch.relu(v)
    if act == ACT_GELU_ERF:
        return fast_gelu32(v) if gelu == "fast" else F.gelu(v)
    if act == ACT_GELU_TANH:
        return F.gelu(v, approximate="tanh")
    if act == ACT_SWIGLU:
        gate, up = (v[:, 1::2], v[:, 0::2]) if mut == "gate_up_swapped" else (v[:, 0::2], v[:, 1::2])
        return F.silu(gate) * up
    assert act == ACT_NONE, act
    return v


def relay_slabs(lo, group):
    """[M][N] -> [N / group][M][group] (GemmArgs::lo_group)."""
    M, N = lo.shape
    return np.ascontiguousarray(lo.reshape(M, N // group, group).transpose(1, 0, 2))


def unlay_slabs(slabs, M):
    """[N / group][>= M][group] -> [M][N]."""
    return np.ascontiguousarray(slabs[:, :M].transpose(1, 0, 2).reshape(M, -1))


def stats_of(lo, dtype=np.float64, order="seq"):
    """(sum, sum of squares) per 32-column group of the given (already rounded) values -> [M][N / 32][2]; float32 orders: "seq" ascending, "pair" the
    epilogue's shape (8 per lane, then the four lanes of a row)."""
    x = np.asarray(lo, dtype).reshape(lo.shape[0], -1, 32)
    if dtype == np.float64 or order == "lib":
        return np.stack([x.sum(-1), (x * x).sum(-1)], -1).astype(np.float64)
    if order == "seq":
        s1, s2 = np.zeros(x.shape[:2], dtype), np.zeros(x.shape[:2], dtype)
        for k in range(32):
            s1 = s1 + x[..., k]
            s2 = s2 + x[..., k] * x[..., k]
        return np.stack([s1, s2], -1).astype(np.float64)
    x8 = x.reshape(x.shape[0], x.shape[1], 4, 8)
    s1, s2 = np.zeros(x8.shape[:3], dtype), np.zeros(x8.shape[:3], dtype)
    for k in range(8):
        s1 = s1 + x8[..., k]
        s2 = s2 + x8[..., k] * x8[..., k]
    p = lambda s: (s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])
    return np.stack([p(s1), p(s2)], -1).astype(np.float64)


def argmax_first(v, n_valid):
    """Row arg-max over n < n_valid with the first index on ties -> (ids [M], top-1 minus top-2 [M])."""
    z = np.array(v, dtype=np.float64)
    z[:, n_valid:] = -np.inf
    ids = z.argmax(axis=1)                     # numpy returns the first maximum
    top2 = np.sort(z, axis=1)[:, -2:]
    return ids.astype(np.int32), top2[:, 1] - top2[:, 0]


def gemm_ref(a, w, bias=None, add=None, act=0, add2=None, add2_rows=None, ln_dim=0, ln_eps=1e-5, a_rms_eps=0.0, rms_eps=None, lo_group=0, n_valid=None,
             operand="bf16", rounded=None, order="seq", gelu="lib", mut=None, only=None):
    """-> dict of float64 arrays (see the module text), or None when `order` does not divide K. mut plants a fault (test_gemm_ref_cpu.py):
    "drop_k16" a K step of 16 left out, "swap_cols" columns 9 and 10 exchanged, "no_bias_group" bias missing on columns 8 .. 15, "add2_before_act",
    "gate_up_swapped", "row_shift" row 1 holds row 2, "t_tail_stale" the M % 4 tail rows of the transpose left zero, "slab_off_by_one" every slab one
    place on, "stats_unrounded" statistics of the values before the bf16 rounding, "tie_high" the arg-max takes the LAST maximum."""
    assert operand in ("bf16", "f32") and rounded in (None, "f32")
    dt = F64 if rounded is None else F32
    rnd = (lambda t: bf16(t)) if operand == "bf16" else (lambda t: t.to(F32).to(t.dtype))
    with torch.inference_mode():
        A, W = rnd(_t(a, F64)), rnd(_t(w, F64))
        M, K = A.shape
        N = W.shape[0]
        Am = A.clone()
        if mut == "drop_k16":
            Am[:, 16:32] = 0.0
        if rounded is None:
            c = Am @ W.t()
        else:
            c = mm32(Am.to(F32), W.to(F32), order)
            if c is None:
                return None
        if ln_dim:
            x = A[:, :ln_dim].to(dt)
            mean = x.sum(1, keepdim=True) / ln_dim
            var = ((x * x).sum(1, keepdim=True) / ln_dim - mean * mean).clamp(min=0.0) if rounded else ((x - mean) ** 2).mean(1, keepdim=True)
            colsum = W.sum(1).to(dt)                                      # the f32 table is the float64 sum rounded once
            c = (c - mean * colsum.unsqueeze(0)) * torch.rsqrt(var + ln_eps)
        if a_rms_eps > 0.0:
            x = A.to(dt)
            c = c * torch.rsqrt((x * x).sum(1, keepdim=True) / K + a_rms_eps)
        if bias is not None:
            b = _t(bias, dt).clone()
            if mut == "no_bias_group":
                b[8:16] = 0.0
            c = c + b
        if add is not None:
            c = c + _t(add, dt)
        t2 = None
        if add2 is not None:
            t2 = _t(add2, dt)
            t2 = t2[torch.as_tensor(np.asarray(add2_rows), dtype=torch.long)] if add2_rows is not None else t2[:M]
        if t2 is not None and mut == "add2_before_act":
            c = c + t2
        v = _act(c, act, gelu, mut)
        if t2 is not None and mut != "add2_before_act":
            v = v + t2
        if mut == "swap_cols":
            v = v.clone()
            v[:, [9, 10]] = v[:, [10, 9]]
        if mut == "row_shift":
            v = v.clone()
            v[1] = v[2]
        lo = v if rounded is None else rnd(v)
        if only is not None:                                      # large matrices: just the named matrix outputs ("f32" / "lo")
            return {k: (v if k == "f32" else lo).to(F64).numpy() for k in only}
        out = {"f32": v.to(F64).numpy()}
        lo_np = lo.to(F64).numpy()
        out["lo"] = lo_np
        t = lo_np.T.copy()
        if mut == "t_tail_stale" and M % 4:
            t[:, M - M % 4:] = 0.0
        out["t"] = t
        if lo_group:
            s = relay_slabs(lo_np, lo_group)
            out["slabs"] = np.roll(s, 1, axis=0) if mut == "slab_off_by_one" else s
        if N % 32 == 0 and act != ACT_SWIGLU:
            out["stats"] = stats_of((v if mut == "stats_unrounded" else bf16(v)).to(F64).numpy())
        if rms_eps is not None:
            out["rms"] = rnd(v * torch.rsqrt((v * v).mean(1, keepdim=True) + rms_eps)).to(F64).numpy() if rounded else \
                (v * torch.rsqrt((v * v).mean(1, keepdim=True) + rms_eps)).numpy()
        if n_valid is not None:
            ids, margin = argmax_first(out["f32"], n_valid)
            if mut == "tie_high":
                z = out["f32"].copy()
                z[:, n_valid:] = -np.inf
                ids = (z.shape[1] - 1 - z[:, ::-1].argmax(axis=1)).astype(np.int32)
            out["ids"], out["margin"] = ids, margin
        return out


def forms(a, w, orders=ORDERS, **spec):
    """(the float64 statement, its float32 evaluations in every order that divides K; for the erf-GELU with a bf16 store also the fast formula of
    gemm_dev.h in float32, in the sequential order)."""
    exact = gemm_ref(a, w, **spec)
    rounded = [r for r in (gemm_ref(a, w, rounded="f32", order=o, **spec) for o in orders) if r is not None]
    if spec.get("act", 0) == ACT_GELU_ERF and spec.get("operand", "bf16") == "bf16":
        rounded.append(gemm_ref(a, w, rounded="f32", order="seq", gelu="fast", **spec))
    return exact, rounded


def judge(got, exact, rounded, key, scale=None):
    """within() on output `key` in the [M][columns] orientation; scale [M]: every row divided by the scale its inputs were drawn at, so that a
    small-valued row weighs as much as a large one in both statistics. -> (ok, (rms ratio, max ratio))."""
    if scale is None:
        return within(got, exact[key], [r[key] for r in rounded])
    s = 1.0 / np.asarray(scale, np.float64)[:, None]
    return within(np.asarray(got, np.float64) * s, exact[key] * s, [r[key] * s for r in rounded])


def inputs(M, N, K, seed, scale_rows=True, table_rows=0, col_offset=True):
    """Asymmetric operands (row- and column-dependent offsets, as test_gemm_matches_torch draws them: transposed fragments and swapped C layouts change the
    result), rows at scales 0.1 .. 10 (the first three rows pin 10, 0.1, 1), bias, add and an add2 table of table_rows rows (default M) at scale 1.
    scale_rows / col_offset = False: unit rows, weights without the column offset (the arg-max tests plant their own winners)."""
    rng = np.random.default_rng([M, N, K, seed])
    s = 10.0 ** rng.uniform(-1, 1, M) if scale_rows else np.ones(M)
    if scale_rows:
        s[:3] = (10.0, 0.1, 1.0)[:min(M, 3)]
    a = (rng.standard_normal((M, K)) + np.linspace(-1, 1, K)[None, :]) * s[:, None]
    w = (rng.standard_normal((N, K)) + (np.linspace(0, 1.5, N)[:, None] if col_offset else 0.0)) / np.sqrt(K)
    bias = rng.standard_normal(N)
    add = rng.standard_normal((M, N)) * s[:, None]
    add2 = rng.standard_normal((table_rows or M, N))
    return tuple(x.astype(np.float32) for x in (a, w, bias, add, add2)) + (s,)
