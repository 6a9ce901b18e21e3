"""Reference statements of the CTC forced alignment (csrc/ctc_align.hip) and the inputs of its GPU tests.

The rule. A transcript of L targets has states s = 0 .. 2 L: even s is a blank, odd s = 2 j + 1 is target j. Row t of the emission matrix `em` holds, at
slot 0, the log-probability of the blank and, at slot j + 1, that of target j. With slot(s) = 0 for even s and (s + 1) / 2 for odd s,

    v_0[0] = em[0][0],  v_0[1] = em[0][1],  v_0[s] = -inf otherwise,
    v_t[s] = best(v_t-1[s], v_t-1[s - 1], v_t-1[s - 2]) + em[t][slot(s)],

where the s - 2 move exists only for odd s = 2 j + 1 with j >= 1 and target j != target j - 1. Ties go to the smaller move: s - 1 is taken only if strictly
greater than staying, s - 2 only if strictly greater than both. The path ends in state 2 L - 1 or 2 L, the odd one on a tie. The forward sum replaces best
by log-add-exp and gives the transcript's log-likelihood. No alignment exists (status 1) when the best end value is -inf.

Three statements: `align64` (float64, np.logaddexp) from the rule, `align32` (np.float32, the kernel's additions, comparisons and span means in its order)
and `brute` (every frame labelling, for tiny cases). `mutant` switches one rule off at a time, so that tests can show their inputs would notice.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
U32 = 2.0 ** -24                       # half an f32 ulp, relative
NINF = -np.inf
SENT_I, SENT_F = -77777, F32(-12345.5)          # what the GPU tests put into every output slot before a call


def _slots(L):
    """slot(s) for s = 0 .. 2 L."""
    s = np.arange(2 * L + 1)
    return np.where(s % 2 == 0, 0, (s + 1) // 2)


def _skip_mask(targets, repeat_rule=True):
    """True at odd s = 2 j + 1 whose s - 2 move exists."""
    L = len(targets)
    m = np.zeros(2 * L + 1, bool)
    for j in range(1, L):
        m[2 * j + 1] = (targets[j] != targets[j - 1]) or not repeat_rule
    return m


def _sweep(em, targets, dtype, repeat_rule=True, tie_ge=False, final_odd_on_tie=True, start_v1=True, forward=True):
    """Viterbi (and forward) sweep in `dtype`, vectorised over the states. Returns (v_end [S], f_end [S] or None, bp [T][S] uint8, fmax [T])."""
    em = np.asarray(em, dtype)
    T, L = em.shape[0], len(targets)
    S = 2 * L + 1
    slot, skip = _slots(L), _skip_mask(targets, repeat_rule)
    v = np.full(S, NINF, dtype)
    v[0] = em[0, 0]
    if L > 0 and start_v1:
        v[1] = em[0, 1]
    f = v.astype(np.float64) if forward else None
    bp = np.zeros((T, S), np.uint8)
    fmax = np.zeros(T)
    gt = (lambda a, b: a >= b) if tie_ge else (lambda a, b: a > b)
    ninf1, ninf2 = np.full(1, NINF, dtype), np.full(2, NINF, dtype)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            if t > 0:
                e = em[t, slot]
                s1 = np.concatenate([ninf1, v[:-1]])
                s2 = np.where(skip, np.concatenate([ninf2, v[:-2]])[:S], dtype(NINF))
                best, b = v.copy(), np.zeros(S, np.uint8)
                m = gt(s1, best)
                best, b = np.where(m, s1, best), np.where(m, 1, b)
                m = skip & gt(s2, best)
                best, b = np.where(m, s2, best), np.where(m, 2, b)
                v = (best + e).astype(dtype)
                bp[t] = b
                if forward:
                    f1 = np.concatenate([[NINF], f[:-1]])
                    f2 = np.where(skip, np.concatenate([[NINF, NINF], f[:-2]])[:S], NINF)
                    f = np.logaddexp(np.logaddexp(f, f1), f2) + em[t, slot].astype(np.float64)
            if forward:
                fin = np.isfinite(f)
                fmax[t] = np.abs(f[fin]).max() if fin.any() else 0.0
    return v, f, bp, fmax


def _finish(em, targets, v, f, bp, dtype, final_odd_on_tie=True):
    T, L = np.asarray(em).shape[0], len(targets)
    a = v[2 * L - 1] if L > 0 else dtype(NINF)
    b = v[2 * L]
    odd_end = L > 0 and (a >= b if final_odd_on_tie else a > b)
    score = a if odd_end else b
    out = {"status": 0 if score != NINF else 1, "path_score": dtype(score), "loglik": NINF, "states": None, "first": np.zeros(L, np.int32),
           "last": np.zeros(L, np.int32), "logprob": np.zeros(L, dtype)}
    if out["status"]:
        out["path_score"] = dtype(NINF)
        return out
    if f is not None:
        out["loglik"] = float(np.logaddexp(f[2 * L - 1] if L > 0 else NINF, f[2 * L]))
    s = 2 * L - 1 if odd_end else 2 * L
    states = np.zeros(T, np.int32)
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    out["states"] = states
    emd = np.asarray(em, dtype)
    for j in range(L):
        rows = np.nonzero(states == 2 * j + 1)[0]
        out["first"][j], out["last"][j] = rows[0], rows[-1]
        acc = dtype(0.0)                              # the kernel's token score: sum in ascending row order, one division by the count
        for t in range(rows[0], rows[-1] + 1):
            acc = dtype(acc + emd[t, j + 1])
        out["logprob"][j] = dtype(acc / dtype(rows[-1] - rows[0] + 1))
    return out


def align64(em, targets, **rules):
    """The float64 statement: {"status", "path_score", "loglik", "states" [T], "first", "last", "logprob" [L], "budget"}; rows count from 0 = em[0]."""
    final = rules.pop("final_odd_on_tie", True)
    v, f, bp, fmax = _sweep(em, targets, np.float64, **rules)
    out = _finish(em, targets, v, f, bp, np.float64, final)
    out["budget"] = budget(fmax)
    return out


def align32(em, targets, **rules):
    """The np.float32 restatement of the kernel's Viterbi sweep, walk back and span means (no forward sum: that one is budgeted against align64)."""
    final = rules.pop("final_odd_on_tie", True)
    v, _, bp, _ = _sweep(em, targets, F32, forward=False, **rules)
    return _finish(em, targets, v, None, bp, F32, final)


MUTANTS = {"no_repeat_rule": {"repeat_rule": False}, "tie_larger_move": {"tie_ge": True}, "tie_final_blank": {"final_odd_on_tie": False},
           "start_without_v1": {"start_v1": False}}


def mutant(name, em, targets):
    """align32 with one rule broken (MUTANTS)."""
    return align32(em, targets, **MUTANTS[name])


def budget(fmax):
    """Bound on |loglik_gpu - loglik| from the operation count of the forward chain. A row costs every state at most three steps -- two lae and the addition
    of the emission (`T * 3 lae steps per state chain`) -- and lae is a maximum plus log1pf(expf(-|a - b|)), 1-Lipschitz in its operands (sup norm), so the
    steps' own errors add up along the chain and are not amplified. One step, with |F| the largest finite forward value of the row:
      1. expf at 2 ulp, y = exp(x) <= 1, passed through log1p (slope 1 / (1 + y) <= 1) onto at most y / (1 + y) <= 1/2:          2^-23
      2. the rounding of the argument x = -|a - b|: 2^-24 |x| relative in y, |x| y <= 1 / e:                                      0.37 * 2^-24
      3. log1pf at 2 ulp of a result <= ln 2 (ulp 2^-24 below 1):                                                                 2^-23
      4. the addition max + log1p (or + em), rounded at |F|:                                                                      2^-24 |F|
    i.e. (5 + |F|) 2^-24 per step, three steps per row."""
    return float((3.0 * (5.0 + np.asarray(fmax, np.float64)) * U32).sum())


def brute(em, targets):
    """Every frame labelling of a tiny case, in float64: (best score, list of the state sequences that reach it, log-sum over all paths); (-inf, [], -inf)
    when there is none."""
    em = np.asarray(em, np.float64)
    T, L = em.shape[0], len(targets)
    slot, skip = _slots(L), _skip_mask(targets)
    best, arg, tot = NINF, [], NINF

    def labellings(prefix):                            # every state sequence the moves allow, one frame at a time
        if len(prefix) == T:
            if prefix[-1] >= 2 * L - 1:
                yield tuple(prefix)
            return
        for s in ([0, 1] if not prefix else [prefix[-1], prefix[-1] + 1, prefix[-1] + 2]):
            if s > 2 * L or (prefix and s - prefix[-1] == 2 and not skip[s]):
                continue
            yield from labellings(prefix + [s])

    for path in labellings([]):
        sc = sum(em[t, slot[s]] for t, s in enumerate(path))
        if sc == NINF:
            continue
        tot = np.logaddexp(tot, sc)
        if sc > best:
            best, arg = sc, [path]
        elif sc == best:
            arg.append(path)
    return best, arg, float(tot)


# ------------------------------------------------------------------------------------------------ emissions
def em_random(seed, T, L):
    """Log-probability-like emissions with irregular mantissas: the blank often likely, targets peaked here and there."""
    rng = np.random.default_rng(seed)
    em = (-rng.gamma(0.9, 2.5, (T, L + 1))).astype(F32)
    em[:, 0] = (-rng.gamma(0.6, 1.0, T)).astype(F32)
    return em


def em_grid(seed, T, L, step=2.0 ** -8, lo=-16.0):
    """Emissions on a grid of `step` inside [lo, 0]: with step 2^-8, |em| <= 16 and T <= 700 every partial sum is below 2^14 on a 2^-8 grid -- 22 bits -- and
    exact in f32, so the f32 and float64 sweeps agree and planted ties are ties in both."""
    rng = np.random.default_rng(seed)
    n = int(round(-lo / step))
    return (-(rng.integers(0, n + 1, (T, L + 1)) * step)).astype(F32)


def em_coarse(seed, T, L):
    """Whole numbers in -3 .. 0: ties everywhere."""
    return em_grid(seed, T, L, step=1.0, lo=-3.0)


def targets_random(seed, L, alphabet=6):
    """Ids 1 .. alphabet: adjacent equal targets occur about once in `alphabet`."""
    return np.random.default_rng(seed).integers(1, alphabet + 1, L).astype(np.int32)


# ------------------------------------------------------------------------------------------------ hand cases, one per tie rule
def hand_cases():
    """name -> (em, targets, states the rule demands)."""
    z = lambda *rows: np.asarray(rows, F32)
    return {
        # stay vs. step: rows 1 and 2 can hold the blank or the target at equal cost; staying wins backwards, so the target is entered as early as possible
        # seen from the end: t = 2 stays in state 1, t = 1 stays too, the start takes v[1] = v[0]: state 2 L - 1 = 1 wins the end tie and is never left.
        "stay_vs_step": (z([0, 0], [0, 0], [0, 0]), [3], [1, 1, 1]),
        # step 1 vs. step 2 into target 1 at t = 2: staying costs 9, coming from the blank (state 2) and from target 0 (state 1) cost the same: the blank wins
        "step1_vs_step2": (z([0, 0, 0], [0, 0, -9], [0, 0, 0]), [3, 4], [1, 2, 3]),
        # the end: states 2 L - 1 and 2 L tie; the odd state wins, so the last row is the target's, not a blank's
        "final_odd_vs_even": (z([0, -1], [-1, 0], [0, 0]), [3], [0, 1, 1]),
        # equal targets may not skip the blank between them: the blank costs 5 and is still taken
        "forbidden_skip": (z([-9, 0, -9], [-5, -1, -9], [-9, -9, 0]), [3, 3], [1, 2, 3]),
        # ... different targets at the same cost do skip it
        "allowed_skip": (z([-9, 0, -9], [-5, -9, 0], [-9, -9, 0]), [3, 4], [1, 3, 3]),
    }


# ------------------------------------------------------------------------------------------------ the GPU file's inputs
def _witnesses(seed):
    """Four small sequences that every group carries, so that a broken rule shows in every group (test_ctc_align_ref_cpu checks that it does)."""
    w_start = em_random(seed + 2, 9, 3)
    w_start[0, 0] = NINF                               # the path has to start in state 1
    return [("w_repeat", em_random(seed, 14, 6), np.asarray([5, 5, 7, 7, 7, 2], np.int32)),
            ("w_ties", np.zeros((9, 4), F32), np.asarray([1, 2, 3], np.int32)),
            ("w_final", np.asarray([[0, -1], [-1, 0], [0, 0]], F32), np.asarray([3], np.int32)),
            ("w_start", w_start, np.asarray([4, 5, 6], np.int32))]


def _seq(name, seed, T, L, kind="random", targets=None):
    em = {"random": em_random, "grid": em_grid, "coarse": em_coarse}[kind](seed, T, L)
    return (name, em, targets_random(seed + 1000, L) if targets is None else np.asarray(targets, np.int32))


def gpu_groups():
    """group -> [(name, em [T'][L + 1] f32, targets [L] int32)]: one op call per group and row0. The sizes cross every stride of the launch: a thread per
    target pair in workgroups of whole waves (L + 1 = 32, 33, 34 around half a wave is not a boundary; 64 and 128 threads are: L = 63 / 64 ride in
    `sizes_small`, 127 / 128 / 129 in `sizes_mid`), eight rows per backpointer word (T' = 2, 63, 64, 65), backpointers in LDS (small groups) and in the
    workspace (`sizes_big`)."""
    a = np.asarray
    g = {}
    g["edge"] = [_seq("L0", 1, 5, 0), _seq("T1_L1", 2, 1, 1), _seq("T_eq_L", 3, 6, 6, targets=[1, 2, 3, 4, 5, 6]), _seq("aa_T3", 4, 3, 2, targets=[9, 9]),
                 _seq("aa_T2_infeasible", 5, 2, 2, targets=[9, 9]), _seq("T2_L1", 6, 2, 1), _seq("T2_L0", 7, 2, 0), _seq("T_lt_L", 8, 3, 5)]
    g["sizes_small"] = [_seq("L31_T63", 10, 63, 31), _seq("L32_T64", 11, 64, 32), _seq("L33_T65", 12, 65, 33), _seq("L33_T65_coarse", 13, 65, 33, "coarse"),
                        _seq("L63_T64", 14, 64, 63), _seq("L64_T65", 15, 65, 64)]
    g["sizes_mid"] = [_seq("L127_T500", 20, 500, 127), _seq("L128_T500", 21, 500, 128, "grid"), _seq("L129_T700", 22, 700, 129)]
    g["sizes_big"] = [_seq("L511_T700", 30, 700, 511), _seq("L1023_T1100", 31, 1100, 1023), _seq("L1023_T700_infeasible", 32, 700, 1023),
                      _seq("L511_T700_grid", 33, 700, 511, "grid")]
    g["ragged"] = [_seq("T1", 40, 1, 1), _seq("T700", 41, 700, 40), _seq("T1_L0", 42, 1, 0), _seq("T700_grid", 43, 700, 90, "grid")]
    # -inf columns: a wall over rows 3..7 in target 1's slot forces it to wait behind blanks; a slot that is -inf in every row leaves no path at all; a blank
    # that is impossible everywhere forces the path through the targets alone
    wall = em_random(50, 14, 3); wall[3:8, 2] = NINF
    dead = em_random(51, 12, 3); dead[:, 2] = NINF
    noblank = em_random(52, 9, 4); noblank[:, 0] = NINF
    allinf = np.full((6, 3), NINF, F32)
    late = em_random(53, 10, 2); late[:7, 1] = NINF; late[:7, 0] = F32(-0.5)
    g["inf"] = [("wall", wall, a([1, 2, 3], np.int32)), ("dead_slot_infeasible", dead, a([1, 2, 3], np.int32)), ("no_blank", noblank, a([1, 2, 1, 2], np.int32)),
                ("all_inf_infeasible", allinf, a([1, 2], np.int32)), ("late_start", late, a([3, 3], np.int32))]
    g["ties"] = [(n, em, a(t, np.int32)) for n, (em, t, _) in hand_cases().items()] + [
        _seq("coarse_L5_T20", 60, 20, 5, "coarse"), _seq("coarse_L40_T130", 61, 130, 40, "coarse"), _seq("coarse_repeat", 62, 30, 8, "coarse", targets=[2, 2, 2, 3, 3, 2, 2, 4]),
        _seq("grid_L20_T64", 63, 64, 20, "grid"), ("all_zero", np.zeros((12, 5), F32), a([1, 1, 2, 3], np.int32))]
    for i, k in enumerate(g):
        g[k] = g[k] + _witnesses(900 + 10 * i)
    return g


def pack_group(seqs, row0):
    """The op call's operands for one group: (em [sum T][ld], seq_lens, targets). Rows in front of row0 and slots past a sequence's L + 1 hold NaN: the
    kernel must read neither."""
    ld = (max(len(t) for _, _, t in seqs) + 1 + 3) // 4 * 4
    blocks, lens = [], []
    for _, em, t in seqs:
        blk = np.full((em.shape[0] + row0, ld), np.nan, F32)
        blk[row0:, :len(t) + 1] = em
        blocks.append(blk)
        lens.append(blk.shape[0])
    return np.concatenate(blocks), np.asarray(lens, np.int32), [t for _, _, t in seqs]
