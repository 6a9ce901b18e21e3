"""Numpy / plain-Python statement of the timed Paraformer outputs, written from the rules in include/asr_mi355x.h (nothing of the oracle is used):

  fire_frames()        the offline CIF fire rows (csrc/kernels.hip cif_scan_kernel<true>): float64 running sum of the alphas and the tail threshold, rounded
                       ONCE to f32 after every row, floored; a token fires at the row where that floor rises (Export_Paraformer.py:505-507)
  stream_fire_steps()  the streaming integrate-and-fire (stream_cif_kernel<true>) restated in np.float32 in the kernel's operation order, with the weight
                       carried from chunk to chunk: only additions, subtractions and comparisons, so it is bit-defined
  token_times()        the build's own span rule (paraformer.token_times)

The scores have no statement of their own here: offline they are ctc_timing_ref.frame_logprob / budget (the GEMM epilogue's sum of exponentials), streaming
token_scores_ref.argmax_scores / fused_budget (launch_argmax_logprob_rows)."""
import numpy as np

F32 = np.float32


def fire_frames(alphas_f32, tail):
    """Rows t in [0, T] at which a token fires for the T alphas of one utterance; t == T is the tail threshold's row. int32, strictly increasing."""
    a = np.concatenate([np.asarray(alphas_f32, F32).reshape(-1), np.asarray([tail], F32)]).astype(np.float64)
    fl = np.floor(np.cumsum(a).astype(F32))                   # np.cumsum adds in order, as the kernel's loop does
    prev = np.concatenate([[F32(0.0)], fl[:-1]])
    return np.nonzero(fl > prev)[0].astype(np.int32)


def stream_fire_steps(alphas_f32, carried):
    """One chunk step of one stream: alphas_f32 = the n_int integrated rows' alphas, carried = the weight left by the previous step (f32; 0 after a reset).
    Returns (fire steps int32 -- -1 for the entry fire in front of the loop --, the weight carried on)."""
    one = F32(1.0)
    ca = F32(carried)
    steps = []
    cond_b = F32(0.0) if ca < one else one
    if cond_b != 0:
        steps.append(-1)
    ca = F32(ca - cond_b)
    for t, al in enumerate(np.asarray(alphas_f32, F32).reshape(-1)):
        thr = F32(one - ca)
        cond_b = F32(0.0) if al < thr else one
        if cond_b != 0:
            steps.append(t)
        ca = F32(ca + al)
        ca = F32(ca - cond_b)
    return np.asarray(steps, np.int32), ca


def absolute_rows(fire_step, chunk_index, rows_new, rows_carried):
    """Integration step t of a stream's chunk_index-th chunk since its reset -> absolute LFR row chunk_index * B + t - C, clipped at 0."""
    return np.maximum(int(chunk_index) * int(rows_new) + np.asarray(fire_step, np.int64) - int(rows_carried), 0)


def token_times(fire_frame, n_rows, row_seconds, max_token_rows=4):
    """[n, 2] (start, end) seconds: token k ends min(fire_k + 1, n_rows) rows in and starts at the later of the previous token's end (0 for the first)
    and end - max_token_rows."""
    out, prev_end = [], 0
    for f in np.asarray(fire_frame, np.int64).reshape(-1).tolist():
        end = min(f + 1, int(n_rows))
        start = max(prev_end, end - int(max_token_rows))
        out.append((start * row_seconds, end * row_seconds))
        prev_end = end
    return np.asarray(out, np.float64).reshape(-1, 2)


# hand cases of the offline scan: name -> (alphas, tail, expected fire rows)
NEAR_ONE = float(np.float32(1.0 - 2.0 ** -24))
FIRE_CASES = {
    "f32_rounding": ([1.0, NEAR_ONE], 0.0, [0, 1]),            # the f64 sum 2 - 2^-24 rounds to 2.0f: a float64 floor would give one token
    "halves": ([0.5] * 6, 0.0, [1, 3, 5]),
    "ones": ([1.0] * 5, 0.0, [0, 1, 2, 3, 4]),
    "T1_none": ([0.3], 0.45, []),
    "T1_tail": ([0.6], 0.45, [1]),
    "T1_row": ([1.0], 0.45, [0]),
    "tiny_terms": ([1e-30] * 3 + [0.999] + [1e-30] * 3 + [0.001], 0.0, [7]),
}


def ragged_alphas(seed=0, T=700):
    """Seeded alphas in (0.05, 0.9) for the long utterance of the ragged batch."""
    return np.random.default_rng(seed).uniform(0.05, 0.9, T).astype(F32)
