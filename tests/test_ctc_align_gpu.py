"""GPU, op level: the CTC forced-alignment trellis (asr_op_ctc_align -> ctc_align_kernel) against its statements in tests/ctc_align_ref.py.

Spans, status and path_score must equal the np.float32 restatement bit for bit (the Viterbi part is additions and comparisons only); token_logprob too (a
sequential f32 sum and one division). loglik is compared with the float64 forward sum within ctc_align_ref.budget (the operation count of the lae chain);
every case prints its observed error / budget. The groups, their sizes and the NaN in front of row0 and behind a sequence's slots are ctc_align_ref's
(test_ctc_align_ref_cpu shows that a broken rule changes the expected answer in every group). Outputs start out holding a sentinel: slots past a sequence's
length and every slot of a sequence without an alignment must keep it.

Measured on an MI355X (largest |loglik error| / budget per group, row0 = 0 and 4 alike): see DESIGN 4.3c."""
import ctypes as C
import functools

import numpy as np
import pytest

import ctc_align_ref as ref
from conftest import sub

pytestmark = pytest.mark.gpu

GROUPS = sorted(ref.gpu_groups())


@functools.lru_cache(maxsize=None)
def _expected(group):
    """name -> (f32 restatement, float64 statement), computed once and shared (row numbers count from the first aligned row)."""
    return {n: (ref.align32(em, t), ref.align64(em, t)) for n, em, t in ref.gpu_groups()[group]}


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("row0", [0, 4])
@pytest.mark.parametrize("group", GROUPS)
def test_trellis_equals_the_f32_restatement(group, row0):
    eng = sub("engine")
    seqs = ref.gpu_groups()[group]
    em, lens, targets = ref.pack_group(seqs, row0)
    max_t = max(1, max(len(t) for t in targets)) + 3                  # three spare slots per row
    first, last, tlp, path, lik, status = eng.op_ctc_align(em, lens, targets, row0=row0, max_tokens=max_t, fill=(ref.SENT_I, ref.SENT_F))
    worst = 0.0
    for b, (name, _, t) in enumerate(seqs):
        w32, w64 = _expected(group)[name]
        L = len(t)
        assert status[b] == w32["status"], (name, status[b])
        assert not np.isnan(path[b]) and not np.isnan(lik[b]), name
        n_kept = 0 if w32["status"] else L
        assert np.all(first[b, n_kept:] == ref.SENT_I) and np.all(last[b, n_kept:] == ref.SENT_I), name      # the caller's fill
        assert np.all(_bits(tlp[b, n_kept:]) == _bits(ref.SENT_F)), name
        if w32["status"]:
            assert path[b] == -np.inf and lik[b] == -np.inf, name
            continue
        assert _bits(path[b]) == _bits(w32["path_score"]), (name, path[b], w32["path_score"])
        assert np.array_equal(first[b, :L], w32["first"] + row0) and np.array_equal(last[b, :L], w32["last"] + row0), name
        assert np.array_equal(_bits(tlp[b, :L]), _bits(w32["logprob"])), name
        err = abs(float(lik[b]) - w64["loglik"])
        assert np.isfinite(lik[b]) and lik[b] >= path[b] - w64["budget"], name
        worst = max(worst, err / w64["budget"])
        assert err <= w64["budget"], (name, err, w64["budget"])
    print(f"ctc_align {group} row0={row0}: largest |loglik error| / budget = {worst:.3g}")


def test_nothing_outside_the_outputs_is_written():
    """The op call on arrays that sit inside larger sentinel-filled buffers: the words around every output keep the sentinel."""
    eng, lib = sub("engine"), sub("_lib")
    seqs = ref.gpu_groups()["edge"]
    em, lens, targets = ref.pack_group(seqs, 0)
    B, max_t, G = len(seqs), max(len(t) for t in targets), 64
    toff = np.zeros(B + 1, np.int32)
    toff[1:] = np.cumsum([len(t) for t in targets])
    tids = np.ascontiguousarray(np.concatenate(targets), np.int32)
    bufs = {k: np.full(2 * G + n, s, dt) for k, (n, s, dt) in {"first": (B * max_t, ref.SENT_I, np.int32), "last": (B * max_t, ref.SENT_I, np.int32),
                                                              "tlp": (B * max_t, ref.SENT_F, np.float32), "path": (B, ref.SENT_F, np.float32),
                                                              "lik": (B, ref.SENT_F, np.float32), "status": (B, ref.SENT_I, np.int32)}.items()}
    ptr = lambda k, ty: bufs[k][G:].ctypes.data_as(C.POINTER(ty))
    em_before, tids_before = em.copy(), tids.copy()
    lib.check(lib.load().asr_op_ctc_align(em.ctypes.data_as(C.POINTER(C.c_float)), em.shape[1], lens.ctypes.data_as(C.POINTER(C.c_int32)), B, 0,
                                          tids.ctypes.data_as(C.POINTER(C.c_int32)), toff.ctypes.data_as(C.POINTER(C.c_int32)), ptr("first", C.c_int32),
                                          ptr("last", C.c_int32), ptr("tlp", C.c_float), max_t, ptr("path", C.c_float), ptr("lik", C.c_float),
                                          ptr("status", C.c_int32)))
    for k, v in bufs.items():
        sent = ref.SENT_F if v.dtype == np.float32 else ref.SENT_I
        assert np.all(v[:G] == sent) and np.all(v[-G:] == sent), k
    assert np.array_equal(em, em_before, equal_nan=True) and np.array_equal(tids, tids_before)
    want = [_expected("edge")[n][0] for n, _, _ in seqs]
    assert list(bufs["status"][G:G + B]) == [w["status"] for w in want]
    first = bufs["first"][G:G + B * max_t].reshape(B, max_t)
    for b, w in enumerate(want):
        n = 0 if w["status"] else len(targets[b])
        assert np.array_equal(first[b, :n], w["first"][:n]) and np.all(first[b, n:] == ref.SENT_I)


def test_bad_arguments_are_errors():
    eng, lib = sub("engine"), sub("_lib")
    em = ref.em_random(1, 6, 2)
    with pytest.raises(lib.AsrError):
        eng.op_ctc_align(em, [6], [[1, 2]], row0=6)                  # no row left
    with pytest.raises(lib.AsrError):
        eng.op_ctc_align(em, [6], [[1, 2, 3]])                       # ld_em 3 holds two targets
    with pytest.raises(lib.AsrError):
        eng.op_ctc_align(np.zeros((6, 1028), np.float32), [6], [list(range(1, 1025))])      # 1024 targets: past the kernel's bound
