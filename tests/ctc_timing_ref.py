"""Numpy / plain-Python statement of the timed CTC head: the frame log-probability the GEMM epilogue and the row reduce produce (csrc/gemm_dev.h
epilogue_rows with E_LSE, csrc/gemm.hip argmax_lse_reduce_kernel), the collapse with spans (csrc/kernels.hip ctc_collapse_timed_kernel), and the error
budget of the former.

The log-soft-max is float64 (first maximum wins); the collapse is integers; the token score is restated in np.float32 in the kernel's own order (ascending
frames, then one division), so it is bit-defined.

The seeded operands the GPU head test uses are built here too, so the CPU test can check their planted structure without a GPU."""
import math

import numpy as np

U32 = 2.0 ** -24                       # half an f32 ulp, relative
F32 = np.float32


# ------------------------------------------------------------------------------------------------ frame log-probability
def frame_logprob(logits, n_valid=None):
    """(ids [rows] int32, logprob [rows] float64, spread [rows] float64) over the first n_valid columns: the first index of the row maximum, log soft-max
    there, and spread = sum_i p_i (max - v_i), the soft-max-weighted distance of the exponents from the maximum (what scales the exponentials' argument error)."""
    v = np.asarray(logits, np.float64)
    if n_valid is not None:
        v = v[:, :n_valid]
    ids = np.argmax(v, axis=1).astype(np.int32)                 # numpy: the first occurrence
    m = v.max(axis=1, keepdims=True)
    e = np.exp(v - m)
    tot = e.sum(axis=1)
    spread = ((m - v) * e).sum(axis=1) / tot
    return ids, -np.log(tot), spread


def budget(n_valid, logprob, spread, K=0, abs_dot=0.0, vmax=0.0):
    """Bound on |frame_logprob_gpu - logprob| for one row, from the operation counts of the epilogue and the reduce.

    frame_logprob = -logf(tot), tot = sum_s S_s expf(best_s - best_row), S_s = sum_{n in slab s} __expf(v_n - best_s); the relative error of tot is the
    absolute error of its logarithm.
    1. the exponentials: v_exp_f32 is good to one ulp (2 ulp = 2^-22 granted); its argument (v - best) log2(e) carries the subtraction's, the
       constant's and the product's rounding, 3 * 2^-24 relative, i.e. 3 * 2^-24 |x| relative in exp(x). The two levels' |x| (inside the slab, slab to row)
       add up to max - v_n, and every term enters tot with weight p_n: 3 * 2^-24 * spread. (expf of the reduce: one ulp, inside the 2^-22.)
    2. the f32 additions, all terms positive, 2^-24 relative per addition on a term's path: 16 columns per lane, 2 lane merges, the product S_s * exp, ceil(n_slabs / 64)
       slabs per lane of the reduce, 6 lane merges.
    3. logf: one ulp of the result, 2 * 2^-24 |logprob|.
    4. K > 0 -- the reference is the float64 product of the bf16 operands, not the stored logits: every logit carries the f32 accumulation of the MFMA chain
       (K / 16 sequential accumulator updates at the shortest instruction the bf16 kernels could use, 5 levels inside one, each 2^-24 of at most
       abs_dot = max_n sum_k |a_k| |w_nk|) and the bias addition (2^-24 vmax). log soft-max at the arg-max is v_max - LSE(v), 1-Lipschitz in each: twice that."""
    n_slabs = -(-int(n_valid) // 64)
    depth = 16 + 2 + 1 + -(-n_slabs // 64) + 6
    b = 2.0 ** -22 + 3 * U32 * np.asarray(spread, np.float64) + depth * U32 + 2 * U32 * np.abs(np.asarray(logprob, np.float64))
    if K > 0:
        b = b + 2 * ((K // 16 + 5) * U32 * abs_dot + U32 * vmax)
    return b


# ------------------------------------------------------------------------------------------------ collapse with spans
def mean_f32(values):
    """The kernel's token score: f32 sum in ascending order, one f32 division by the f32 count."""
    s = F32(0.0)
    for x in np.asarray(values, F32):
        s = F32(s + x)
    return F32(s / F32(len(values)))


def collapse_timed(ids, frame_lp, blank_id=0):
    """(token ids, first frames, last frames, scores) of one utterance under the reference's circular rule: frame t is kept when id[t] != id[(t + 1) mod T]
    and id[t] != blank; first = start of the maximal LINEAR run of equal ids ending at t (no wrap); score = mean_f32 of frame_lp over first..t."""
    ids = [int(i) for i in ids]
    T = len(ids)
    tok, first, last, score = [], [], [], []
    start = 0
    for t in range(T):
        if t > 0 and ids[t] != ids[t - 1]:
            start = t
        if ids[t] != ids[(t + 1) % T] and ids[t] != blank_id:
            tok.append(ids[t]); first.append(start); last.append(t); score.append(mean_f32(frame_lp[start:t + 1]))
    return np.asarray(tok, np.int32), np.asarray(first, np.int32), np.asarray(last, np.int32), np.asarray(score, F32)


def runs(*pairs):
    """[(id, length), ...] -> frame ids."""
    return np.concatenate([np.full(n, i, np.int32) for i, n in pairs])


# Hand-written sequences for every edge of the collapse (blank = 0): name -> (frame ids, expected [(id, first, last), ...]).
COLLAPSE_CASES = {
    "T1_blank": (runs((0, 1)), []),
    "T1_token": (runs((5, 1)), []),                              # the circular rule compares the only frame with itself: nothing is kept
    "all_blank": (runs((0, 300)), []),
    "run_1": (runs((0, 3), (7, 1), (0, 3)), [(7, 3, 3)]),
    "run_2": (runs((0, 3), (7, 2), (0, 3)), [(7, 3, 4)]),
    "run_64": (runs((0, 1), (7, 64), (0, 2)), [(7, 1, 64)]),
    "run_65": (runs((0, 1), (7, 65), (0, 2)), [(7, 1, 65)]),
    "run_256": (runs((0, 1), (7, 256), (0, 2)), [(7, 1, 256)]),
    "run_257": (runs((0, 1), (7, 257), (0, 2)), [(7, 1, 257)]),
    "run_600": (runs((0, 1), (7, 600), (0, 2)), [(7, 1, 600)]),
    "straddle_63_64": (runs((0, 60), (9, 8), (0, 4)), [(9, 60, 67)]),
    "straddle_255_256": (runs((0, 250), (9, 12), (0, 4)), [(9, 250, 261)]),
    "straddle_511_512_from_200": (runs((0, 200), (9, 320), (4, 3), (0, 2)), [(9, 200, 519), (4, 520, 522)]),
    "same_id_twice": (runs((0, 2), (6, 3), (0, 1), (6, 2), (0, 2)), [(6, 2, 4), (6, 6, 7)]),
    "last_run_equals_frame0": (runs((5, 3), (0, 2), (8, 2), (5, 4)), [(5, 0, 2), (8, 5, 6)]),       # the tail run of 5 wraps into frame 0: it emits nothing
    "last_run_differs": (runs((5, 3), (0, 2), (8, 4)), [(5, 0, 2), (8, 5, 8)]),                      # emitted at T - 1
    "dense": (np.array([3, 3, 0, 3, 4, 4, 4, 0, 0, 9, 1, 1, 0], np.int32), [(3, 0, 1), (3, 3, 3), (4, 4, 6), (9, 9, 9), (1, 10, 11)]),
}


def case_logprob(seed, T):
    """Frame log-probabilities for a collapse case: negative, irregular mantissas, a few exact zeros."""
    rng = np.random.default_rng(seed)
    lp = (-rng.gamma(0.7, 1.5, T)).astype(F32)
    lp[rng.random(T) < 0.05] = 0.0
    return lp


# ------------------------------------------------------------------------------------------------ operands of the head test
HEAD_K = 512
ROW_KINDS = ("random", "plant_slab0", "random", "plant_right", "plant_last", "plus90", "minus90", "equal", "dominant")
COL_TOP, COL_SLAB0, COL_RIGHT = 64 * 3 + 40, 17, 64 * 4 + 2      # the arg-max peak (slab 3), the planted peaks in slab 0 and in the slab to its right
PEAK, PLANT = 16.0, 15.75


def bf16_round(x):
    """Round-to-nearest-even to bf16, returned as f32."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return u.view(F32).reshape(np.shape(x)).copy()


def head_operands(seed, M, N, n_valid):
    """(a [M][K], w [N][K], bias [N], kinds [M]): a and w bf16-exact, bias bf16-exact f32. The first eight k are switches, zero in the random part:
      k = 0  per-row offset (w[:, 0] = 1);   k = 1..4  height of a peak on COL_TOP / COL_SLAB0 / COL_RIGHT / n_valid - 1 (the last partly valid slab);
      k = 5  cancels the bias (w[n, 5] = -bias[n]).
    The rest is a random product giving logits of a few units (sum of their exponentials ~ e^11 for ten thousand columns). Row m has kind
    ROW_KINDS[m % 9]; the LAST row of the matrix is always a plant_last row, so that the padded row tile is exercised by a sensitive row:
      plant_*   a peak of 16 on COL_TOP and one of 15.75 on a column of another slab over a background an eighth as wide (the peak columns have no bias):
                the two hold nearly all of the row's probability, about half each (whichever the background lifts higher is the arg-max), so losing
                either slab's partial moves the result by ~0.69;
      plus90 / minus90   every logit shifted by +-90;
      equal     every logit exactly 0: -log n_valid, id 0;
      dominant  every logit 0, COL_TOP 40: the result lies in (-1e-6, 0]."""
    assert n_valid - 1 > COL_RIGHT + 64 and N % 128 == 0 and n_valid <= N
    rng = np.random.default_rng(seed)
    K = HEAD_K
    a = bf16_round(rng.standard_normal((M, K), dtype=F32))
    w = bf16_round(rng.standard_normal((N, K), dtype=F32) * F32(2.0 / math.sqrt(K)))
    bias = bf16_round(rng.normal(0.0, 0.5, N))
    a[:, :8] = 0.0
    w[:, :8] = 0.0
    w[:, 0] = 1.0
    w[COL_TOP, 1] = w[COL_SLAB0, 2] = w[COL_RIGHT, 3] = w[n_valid - 1, 4] = 1.0
    bias[[COL_TOP, COL_SLAB0, COL_RIGHT, n_valid - 1]] = 0.0
    w[:, 5] = -bias
    kinds = [ROW_KINDS[m % len(ROW_KINDS)] for m in range(M)]
    kinds[M - 1] = "plant_last"
    for m, kind in enumerate(kinds):
        if kind.startswith("plant_"):
            a[m, 8:] *= F32(0.125)                   # a flat background, so that the two peaks stay level to within a few tenths
            a[m, 1] = PEAK
            a[m, {"plant_slab0": 2, "plant_right": 3, "plant_last": 4}[kind]] = PLANT
        elif kind == "plus90":
            a[m, 0] = 90.0
        elif kind == "minus90":
            a[m, 0] = -90.0
        elif kind in ("equal", "dominant"):
            a[m, :] = 0.0
            a[m, 5] = 1.0
            if kind == "dominant":
                a[m, 1] = 40.0
    return a, w, bias, kinds


def head_reference(a, w, bias, n_valid, rows=None):
    """float64 statement over the (bf16-exact) operands for the given rows (default all): (ids, logprob, spread, abs_dot, vmax), one entry per row."""
    a64 = np.asarray(a, np.float64) if rows is None else np.asarray(a, np.float64)[rows]
    w64 = np.asarray(w[:n_valid], np.float64)
    v = a64 @ w64.T + np.asarray(bias[:n_valid], np.float64)[None, :]
    ids, lp, spread = frame_logprob(v)
    abs_dot = (np.abs(a64) @ np.abs(w64).T).max(axis=1)
    return ids, lp, spread, abs_dot, np.abs(v).max(axis=1)
