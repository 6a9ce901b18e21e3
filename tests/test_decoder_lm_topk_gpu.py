"""launch_lm_topk (csrc/decoder_lm.hip) through the probe library: the M best (value, id) pairs of a logits row, value descending then id ascending, and the
row's log-sum-exp. Logits are on the 2^-10 grid, so the pairs and their order are compared exactly; the log-sum-exp within token_heads_ref's budget for
beam_topk_kernel's reduction, which this kernel repeats. Pad columns sit at PAD_LOGIT (+1e30): a kernel that lets one into a list or a sum fails visibly.

The planted rows assume the kernel's column assignment: 1024 threads, thread t reads the float4 groups at columns 4 t + 4096 j, wave w = t // 64. A thread
keeps a best-8 list, so more than 8 of the row's best in one thread's share is the layout the one-pass merge cannot rank on its own."""
import numpy as np
import pytest

import token_heads_ref as thr
from conftest import sub

pytestmark = pytest.mark.gpu
F32 = np.float32
MS = [1, 8, 9, 32]
TOP = F32(20.0)                        # above every N(0, 3^2) draw used here


def probe():
    return sub("_probe")


def reference(x, M, bias=None):
    v = np.asarray(x, F32) if bias is None else (np.asarray(x, F32) + np.asarray(bias, F32)[None, :]).astype(F32)
    rows = len(v)
    cv, ci, lse, mx = np.full((rows, M), -np.inf, F32), np.zeros((rows, M), np.int32), np.full(rows, -np.inf), np.full(rows, -np.inf)
    for r in range(rows):
        o = [int(c) for c in thr.order(v[r])[:M] if v[r, c] > -np.inf]
        cv[r, :len(o)], ci[r, :len(o)] = v[r, o], o
        fin = v[r][v[r] > -np.inf].astype(np.float64)
        if fin.size:
            mx[r] = fin.max()
            lse[r] = mx[r] + np.log(np.exp(fin - mx[r]).sum())
    return cv, ci, lse, mx


def check(x, M, bias=None, slow=None):
    got = probe().lm_topk(x, M, bias=bias)
    cv, ci, lse, mx = reference(x, M, bias)
    assert np.array_equal(got["cand_i"], ci)
    assert np.array_equal(got["cand_v"].view(np.uint32), cv.view(np.uint32))
    assert not np.isnan(got["lse"]).any()
    fin = np.isfinite(lse)
    assert np.array_equal(got["lse"][~fin], lse[~fin].astype(F32))
    if fin.any():
        bud = thr.beam_topv_budget(x.shape[1], mx[fin], lse[fin], 0.0)
        worst = float((np.abs(got["lse"][fin] - lse[fin]) / bud).max())
        print(f"log-sum-exp error / budget {worst:.3f}, strict-order rows {got['slow_rows']}")
        assert worst <= 1.0
    if slow is not None:
        assert (got["slow_rows"] > 0) == slow, got["slow_rows"]
    return got


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("n", [5, 129, 4097])
@pytest.mark.parametrize("rows", [1, 3, 65])
def test_grid_rows(rows, n, M):
    check(thr.grid_logits([rows, n, 61], rows, n), M)


@pytest.mark.parametrize("M", MS)
def test_the_large_vocabulary(M):
    n = 151936
    x = thr.grid_logits([n, 63], 3, n)
    bias = np.zeros(n, F32)
    bias[thr.order(x[0])[:3]] = -np.inf                   # BEGIN_SUPPRESS on row 0's best columns
    check(x, M, bias=bias, slow=False)


def _share(t, n):
    """The columns thread t reads, ascending."""
    cols = [4 * t + 4096 * j + e for j in range(-(-n // 4096)) for e in range(4)]
    return [c for c in cols if c < n]


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("n", [36869, 151936])
def test_all_best_in_one_threads_share(n, M):
    x = thr.grid_logits([n, 65], 3, n)
    for r, t in enumerate((0, 517, 1023)):
        cols = _share(t, n)
        assert len(cols) >= 33
        take = cols[::-1][:M + 1] if r == 1 else cols[:M + 1]      # one more than M: the (M + 1)-th must stay out; row 1 has them in descending id order
        x[r, take] = TOP + np.arange(len(take), 0, -1, dtype=F32) * F32(thr.GRID)
    check(x, M, slow=M > 8)                                # (M + 1 planted values in one share: from M = 9 on the list of 8 runs out before the M-th winner)


@pytest.mark.parametrize("M", MS)
def test_best_spread_one_per_wave(M):
    n = 4097 * 9
    x = thr.grid_logits([n, 67], 3, n)
    for r in range(3):
        cols = [4 * (64 * (k % 16) + (7 * k + r) % 64) + 4096 * (k // 16) for k in range(M)]
        x[r, cols] = TOP + F32(thr.GRID) * np.arange(M, 0, -1, dtype=F32)
    check(x, M, slow=False)


@pytest.mark.parametrize("M", MS)
def test_equal_maxima_go_to_the_lower_id(M):
    n = 12289
    x = thr.grid_logits([n, 69], 3, n)
    rng = np.random.default_rng(71)
    x[0, rng.choice(n, M + 5, replace=False)] = TOP        # more than M equal maxima, spread
    x[1, _share(3, n)[:12]] = TOP                          # ... and twelve of them in one thread's share
    x[2, :] = F32(1.5)                                     # a constant row: the first M ids
    check(x, M)


@pytest.mark.parametrize("M", MS)
def test_minus_inf_columns_ragged_width_and_short_rows(M):
    n = 4099                                               # not a multiple of 4: the last float4 holds one valid column and three pads
    x = thr.grid_logits([n, 73], 4, n)
    best = thr.order(x[0])[:6]
    x[0, best[[0, 2, 4]]] = -np.inf                        # -inf among the best
    x[0, n - 1] = TOP                                      # the very last valid column wins
    x[1, :] = -np.inf
    x[1, [5, 4098, 77]] = [F32(1.0), F32(1.0), F32(2.0)]   # fewer than M finite columns (from M = 8 on)
    x[2, :] = -np.inf                                      # nothing at all: no candidates, a score of -inf, never NaN
    got = check(x, M)
    assert (got["cand_v"][2] == -np.inf).all() and (got["cand_i"][2] == 0).all() and got["lse"][2] == -np.inf
    assert (got["cand_i"][:, :] < n).all()
