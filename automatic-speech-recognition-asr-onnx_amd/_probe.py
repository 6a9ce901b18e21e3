"""ctypes binding of libasr_mi355x_probe.so (include/asr_mi355x_probe.h): test / tuning hooks, NOT the product ABI.

Used by tests/ and tools/ only; the transcribers, the onnxruntime shim and bench.py's timed path never import this."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib

PROBE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libasr_mi355x_probe.so")
_fp, _ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)


class GemmDesc(C.Structure):
    _fields_ = [("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("a", _fp), ("w", _fp), ("bias", _fp), ("add", _fp),
                ("act", C.c_int32), ("ln", C.c_int32), ("ln_eps", C.c_float), ("argmax", C.c_int32), ("n_valid", C.c_int32),
                ("variant", C.c_int32), ("out_lo", _fp), ("out_f32", _fp), ("out_stats", _fp), ("out_ids", _ip),
                ("kernel", C.c_char * 32),
                ("precision", C.c_int32), ("add2", _fp), ("add2_table_rows", C.c_int32), ("add2_rows", _ip), ("a_rms_eps", C.c_float),
                ("m_dev", C.c_int32), ("lo_group", C.c_int32), ("out_t", _fp), ("ld_out_t", C.c_int32), ("out_rms", _fp), ("rms_eps", C.c_float),
                ("pad_a", C.c_int32), ("pad_w", C.c_int32), ("pad_out", C.c_int32), ("with_ws", C.c_int32), ("stray", C.c_int32)]


class DecodeAttnDesc(C.Structure):
    _fields_ = [("bf16", C.c_int32), ("cross", C.c_int32), ("B", C.c_int32), ("b0", C.c_int32), ("nb", C.c_int32), ("H", C.c_int32),
                ("n", C.c_int32), ("causal", C.c_int32), ("q", _fp), ("ld_q", C.c_int32), ("q_col0", C.c_int32), ("max_keys", C.c_int32),
                ("kv_new", _fp), ("k_hist", _fp), ("v_hist", _fp), ("hist", C.c_int32), ("hist_dev", C.c_int32), ("max_pos", C.c_int32),
                ("paged", C.c_int32), ("n_pages", C.c_int32), ("pages_per_seq", C.c_int32), ("page_table", _ip), ("k_after", _fp), ("v_after", _fp),
                ("k_slab", _fp), ("v_slab", _fp), ("rows", C.c_int32), ("row_off", _ip), ("n_lfr", _ip), ("fp8", C.c_int32),
                ("kv8", C.c_void_p), ("scale8", _fp), ("out", _fp), ("stray", C.c_int32), ("kernel", C.c_char * 32)]


class QwenAttnDesc(C.Structure):
    _fields_ = [("bf16", C.c_int32), ("step", C.c_int32), ("no_fuse", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("KV", C.c_int32),
                ("rows", C.c_int32), ("qkv", _fp), ("qn", _fp), ("kn", _fp), ("rope", _fp), ("rope_rows", C.c_int32), ("eps", C.c_float),
                ("hist", _ip), ("T", _ip), ("row_off", _ip), ("row_seq", _ip), ("row_t", _ip), ("S_max", C.c_int32), ("paged", C.c_int32),
                ("n_pages", C.c_int32), ("pps", C.c_int32), ("table", _ip), ("hist_ld", C.c_int32), ("k_hist", _fp), ("v_hist", _fp),
                ("after_ld", C.c_int32), ("k_after", _fp), ("v_after", _fp), ("beam", C.c_int32), ("ld_src", C.c_int32), ("S_hyp", C.c_int32),
                ("src", _ip), ("p0", _ip), ("ext_k", _fp), ("ext_v", _fp), ("q_out", _fp), ("k_rows_out", _fp), ("ctx", _fp),
                ("stray", C.c_int32), ("qt", C.c_int32), ("nw", C.c_int32), ("kernel", C.c_char * 32)]


class EncAttnDesc(C.Structure):
    _fields_ = [("bf16", C.c_int32), ("head_dim", C.c_int32), ("n_heads", C.c_int32), ("kv_group", C.c_int32), ("causal", C.c_int32), ("batch", C.c_int32),
                ("key_lens", _ip), ("q_lens", _ip), ("packed_qk", C.c_int32), ("slack_rows", C.c_int32), ("pad_fill_k", C.c_float), ("pad_fill_v", C.c_float),
                ("q", _fp), ("k", _fp), ("v", _fp), ("ctx", _fp),
                ("hd", C.c_int32), ("chunk", C.c_int32), ("qt", C.c_int32), ("waves", C.c_int32), ("grid_z", C.c_int32), ("n_qblocks", C.c_int32),
                ("stray", C.c_int32)]


class FsmnDesc(C.Structure):
    _fields_ = [("bf16", C.c_int32), ("batch", C.c_int32), ("channels", C.c_int32), ("lens", _ip), ("pad_fill", C.c_float),
                ("v", _fp), ("w", _fp), ("b", _fp), ("out", _fp), ("stray", C.c_int32)]


class BeamSelectDesc(C.Structure):
    _fields_ = [("n_utt", C.c_int32), ("beam", C.c_int32), ("K", C.c_int32), ("ld", C.c_int32), ("first", C.c_int32), ("n_slots", C.c_int32),
                ("n_stop", C.c_int32), ("topv", _fp), ("topi", _ip), ("cum", _fp), ("fin", _ip), ("len", _ip), ("next", _ip), ("done", _ip),
                ("stop", _ip), ("src_in", _ip), ("tok_in", _ip), ("src_out", _ip), ("tok_out", _ip)]


class TokenHeadDesc(C.Structure):
    _fields_ = [("op", C.c_int32), ("rows", C.c_int32), ("n_valid", C.c_int32), ("ld", C.c_int32), ("logits", _fp), ("vec", _fp),
                ("K", C.c_int32), ("ld_save", C.c_int32), ("n_saved", C.c_int32), ("n_saved_after", C.c_int32), ("save_ids", _ip),
                ("range", C.c_int32), ("partial", C.c_int32), ("value", C.c_float), ("next_in", _ip),
                ("temperature", C.c_float), ("top_p", C.c_float), ("repetition_penalty", C.c_float), ("noise", _fp), ("seed", C.c_uint64),
                ("no_speech_id", C.c_int32), ("out_v", _fp), ("out_i", _ip),
                ("steps", C.c_int32), ("track_history", C.c_int32), ("sampling", C.c_int32), ("change_step", C.c_int32), ("range2", C.c_int32),
                ("value2", C.c_float), ("picks", _ip),
                ("timestamps", C.c_int32), ("ts_begin", C.c_int32), ("no_timestamps_id", C.c_int32), ("eot_id", C.c_int32), ("max_initial", C.c_int32),
                ("n_saved_rows", _ip), ("scores", C.c_int32), ("logprob", _fp), ("timed", C.c_int32),
                ("head_ms", C.c_float)]


class WhisperAlignDesc(C.Structure):
    _fields_ = [("op", C.c_int32), ("bf16", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("n", C.c_int32), ("n_pairs", C.c_int32),
                ("max_rows", C.c_int32), ("ld", C.c_int32), ("q", _fp), ("k_slab", _fp), ("slab_rows", C.c_int32), ("row_off", _ip), ("n_lfr", _ip),
                ("sel", _ip), ("n_sel", C.c_int32), ("position", C.c_int32), ("p0", C.c_int32), ("n_rows", _ip), ("n_frames", _ip), ("width", C.c_int32),
                ("scores", _fp), ("stats", _fp), ("cost", _fp), ("frames", _ip), ("path", _ip), ("path_stride", C.c_int32), ("path_len", _ip)]


class HotwordDesc(C.Structure):
    _fields_ = [("op", C.c_int32), ("rows", C.c_int32), ("n_valid", C.c_int32), ("ld", C.c_int32), ("logits", _fp), ("vec", _fp),
                ("ids", _ip), ("offsets", _ip), ("n_phrases", C.c_int32), ("boost", C.c_float), ("node", _ip), ("n_saved", C.c_int32),
                ("next_in", _ip), ("root_save", _fp), ("n_root", C.c_int32), ("K", C.c_int32), ("topv", _fp), ("topi", _ip), ("lse", _fp)]


class HotwordHeadDesc(C.Structure):
    _fields_ = [("rows", C.c_int32), ("n_valid", C.c_int32), ("ld", C.c_int32), ("steps", C.c_int32), ("logits", _fp), ("vec", _fp),
                ("ld_save", C.c_int32), ("range", C.c_int32), ("partial", C.c_int32), ("value", C.c_float),
                ("sampling", C.c_int32), ("K", C.c_int32), ("temperature", C.c_float), ("top_p", C.c_float), ("repetition_penalty", C.c_float),
                ("seed", C.c_uint64), ("noise", _fp),
                ("timestamps", C.c_int32), ("ts_begin", C.c_int32), ("no_timestamps_id", C.c_int32), ("eot_id", C.c_int32), ("max_initial", C.c_int32),
                ("scores", C.c_int32), ("ids", _ip), ("offsets", _ip), ("n_phrases", C.c_int32), ("boost", C.c_float),
                ("picks", _ip), ("save_ids", _ip), ("n_saved_after", C.c_int32), ("nodes", _ip), ("logprob", _fp), ("logits_out", _fp),
                ("timed", C.c_int32), ("head_ms", C.c_float)]


class HotwordRankDesc(C.Structure):
    _fields_ = [("n_utt", C.c_int32), ("beam", C.c_int32), ("tab_ld", C.c_int32), ("first", C.c_int32), ("n_slots", C.c_int32), ("n_stop", C.c_int32),
                ("n_valid", C.c_int32), ("ld", C.c_int32), ("logits", _fp), ("vec", _fp),
                ("ids", _ip), ("offsets", _ip), ("n_phrases", C.c_int32), ("boost", C.c_float),
                ("cum", _fp), ("fin", _ip), ("len", _ip), ("next", _ip), ("done", _ip), ("stop", _ip),
                ("src_in", _ip), ("tok_in", _ip), ("src_out", _ip), ("tok_out", _ip), ("node_in", _ip), ("node_out", _ip), ("topv", _fp), ("topi", _ip),
                ("iters", C.c_int32), ("ms_topk", C.c_float), ("ms_rerank", C.c_float)]


class LmModel(C.Structure):
    _fields_ = [("image", _ip), ("n_words", C.c_int64), ("alpha", C.c_float), ("beta", C.c_float), ("oov_logprob", C.c_float), ("topk", C.c_int32),
                ("end_ids", _ip), ("n_end", C.c_int32)]


class LmTopkDesc(C.Structure):
    _fields_ = [("rows", C.c_int32), ("n_valid", C.c_int32), ("ld", C.c_int32), ("M", C.c_int32), ("logits", _fp), ("vec", _fp),
                ("cand_v", _fp), ("cand_i", _ip), ("lse", _fp), ("slow_rows", C.c_int32), ("iters", C.c_int32), ("ms_lm_topk", C.c_float),
                ("ms_beam_topk", C.c_float)]


class LmPickDesc(C.Structure):
    _fields_ = [("rows", C.c_int32), ("n_saved", C.c_int32), ("ld_save", C.c_int32), ("cand_v", _fp), ("cand_i", _ip), ("lse", _fp),
                ("state", _ip), ("next", _ip), ("logprob", _fp)]


class DecGemmDesc(C.Structure):
    _fields_ = [("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("plan_M", C.c_int32), ("lda", C.c_int32), ("ldw", C.c_int32), ("ld_add", C.c_int32),
                ("ld_out_f32", C.c_int32), ("ld_out_lo", C.c_int32), ("wkind", C.c_int32), ("a", C.c_void_p), ("w_bf16", C.c_void_p), ("wq", C.c_void_p),
                ("w_scale", _fp), ("w_scale8", C.c_void_p), ("bias", _fp), ("fold", C.c_int32), ("ln_eps", C.c_float), ("add", _fp), ("act", C.c_int32),
                ("out_f32", _fp), ("out_lo", _fp), ("with_ws", C.c_int32), ("repeats", C.c_int32), ("force_nt", C.c_int32), ("force_splits", C.c_int32),
                ("force_row_blocks", C.c_int32), ("pre_M", C.c_int32), ("pre_splits", C.c_int32), ("mt", C.c_int32), ("nt", C.c_int32), ("splits", C.c_int32),
                ("row_blocks", C.c_int32), ("stray", C.c_int32), ("tickets_zero", C.c_int32)]


SIGNATURES = {
    "asr_probe_decode_gemm_desc": (C.c_int, [C.POINTER(DecGemmDesc)]),
    "asr_probe_quantize_fp8_ld": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, _fp, C.c_void_p]),
    "asr_probe_quantize_mxfp4_ld": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "asr_probe_quantize_crosskv_fp8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ip, _ip, C.c_int, C.c_int, C.c_void_p, _fp]),
    "asr_probe_layernorm_fp8": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p]),
    "asr_probe_gemm_fp8_v2": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, _fp, C.c_float, _fp, _fp, C.c_int, C.c_int, C.c_float,
                                        C.c_void_p, C.c_int, _fp, C.c_int, C.POINTER(C.c_uint64)]),
    "asr_probe_gemm": (C.c_int, [C.POINTER(GemmDesc)]),
    "asr_probe_ctc_head": (C.c_int, [C.c_int] * 3 + [_fp, _fp, _fp, C.c_int, C.c_int, _ip, _fp, _ip, C.c_char_p]),
    "asr_probe_ctc_topk": (C.c_int, [C.c_int] * 3 + [_fp, _fp, _fp, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _fp, C.c_char_p]),
    "asr_probe_ctc_target_logprob": (C.c_int, [C.c_int] * 3 + [_fp, _fp, _fp, C.c_int, C.c_int, C.c_int, _ip, C.c_int, _ip, _ip, C.c_int, C.c_int, _fp, _ip, C.c_char_p]),
    "asr_probe_gemm_chain": (C.c_int, [C.c_int] * 6 + [_fp]),
    "asr_probe_last_kernel": (C.c_char_p, []),
    "asr_probe_quantize_fp8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, _fp, C.c_void_p]),
    "asr_probe_quantize_mxfp4": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "asr_probe_decode_gemm_mxfp4": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _fp, C.c_int, _fp]),
    "asr_probe_decode_gemm": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _fp, _fp, C.c_int, _fp]),
    "asr_probe_decode_attention": (C.c_int, [C.POINTER(DecodeAttnDesc)]),
    "asr_probe_qwen_attention": (C.c_int, [C.POINTER(QwenAttnDesc)]),
    "asr_probe_encoder_attention": (C.c_int, [C.POINTER(EncAttnDesc)]),
    "asr_probe_fsmn": (C.c_int, [C.POINTER(FsmnDesc)]),
    "asr_probe_beam_select": (C.c_int, [C.POINTER(BeamSelectDesc)]),
    "asr_probe_token_head": (C.c_int, [C.POINTER(TokenHeadDesc)]),
    "asr_probe_whisper_align": (C.c_int, [C.POINTER(WhisperAlignDesc)]),
    "asr_probe_hotword": (C.c_int, [C.POINTER(HotwordDesc)]),
    "asr_probe_hotword_head_steps": (C.c_int, [C.POINTER(HotwordHeadDesc)]),
    "asr_probe_hotword_rank": (C.c_int, [C.POINTER(HotwordRankDesc)]),
    "asr_probe_lm_topk": (C.c_int, [C.POINTER(LmTopkDesc)]),
    "asr_probe_lm_pick": (C.c_int, [C.POINTER(LmModel), C.POINTER(LmPickDesc)]),
    "asr_probe_lm_head_steps": (C.c_int, [C.POINTER(LmModel), C.POINTER(HotwordHeadDesc), _ip]),
    "asr_probe_lm_rank": (C.c_int, [C.POINTER(LmModel), C.POINTER(HotwordRankDesc), _ip, _ip]),
    "asr_probe_decode_attention_beam": (C.c_int, [C.c_int] * 8 + [_ip, C.c_int, _fp, _fp, _fp, _fp, _ip, C.c_char_p]),
    "asr_probe_decode_attention_ks": (C.c_int, [C.POINTER(DecodeAttnDesc), _ip]),
    "asr_probe_decode_attention_beam_ks": (C.c_int, [C.c_int] * 8 + [_ip, C.c_int, _fp, _fp, _fp, _fp, _ip, C.c_char_p, _ip]),
    "asr_probe_prompt_attention": (C.c_int, [C.POINTER(DecodeAttnDesc), _ip]),
    "asr_probe_gemm_counts": (C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    "asr_probe_live_device_bytes": (C.c_int, [C.POINTER(C.c_int64)]),
    "asr_probe_gemm_fp8": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, _fp, C.c_float, _fp, _fp, C.c_int, C.c_void_p, _fp, C.c_int, _fp]),
    "asr_probe_gemm_bench": (C.c_int, [C.c_int] * 6 + [_fp]),
    "asr_probe_grid_barrier": (C.c_int, [C.c_int, C.c_int, _fp]),
    "asr_probe_grid_barrier2": (C.c_int, [C.c_int, C.c_int, C.c_int, _fp]),
}
_plib = None


def load():
    global _plib
    if _plib is None:
        _lib.load()                       # the probe library resolves the product library's launchers
        if not os.path.isfile(PROBE_PATH):
            raise ImportError(f"{PROBE_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(PROBE_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _plib = lib
    return _plib


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def gemm(a, w, bias=None, add=None, act=0, ln=False, ln_eps=1e-5, argmax=False, n_valid=0, variant=-1, want=("lo",), precision=0, add2=None,
         add2_rows=None, a_rms_eps=0.0, m_dev=None, lo_group=0, ld_out_t=0, rms_eps=1e-6, pad_a=0, pad_w=0, pad_out=0, with_ws=True):
    """One GEMM through the product dispatcher (precision 0: operands rounded to bf16, launch_gemm_bf16; 1: launch_gemm_f32); returns
    (dict of outputs, kernel family name). want: "lo" ([M][N]; [M][N / 2] with act 4; with lo_group the slabs as laid out, [N / lo_group][round_up(M, 128)]
    [lo_group], unwritten rows NaN), "f32", "stats" ([M][N / 32][2]), "t" (the transposed store, [N][M]), "rms" ([M][N], the split-K reduce's second
    output). With m_dev (the device-side row count beside the launch bound M) the outputs hold min(M, m_dev) rows. add2 is a table [R][N] read at row
    add2_rows[m] (row m without add2_rows). pad_*: extra elements per row of A, W and of every output / add / add2 buffer; with_ws=False launches without
    the split-K workspace. out["stray"]: words outside the valid rows x valid columns of the NaN-filled output buffers that the launch changed."""
    a, w = _f32(a), _f32(w)
    M, K = a.shape
    N = w.shape[0]
    Mv = M if m_dev is None else min(M, int(m_dev))
    d = GemmDesc()
    d.M, d.N, d.K, d.act, d.ln, d.ln_eps, d.argmax, d.n_valid, d.variant = M, N, K, act, int(ln), ln_eps, int(argmax), n_valid, variant
    d.precision, d.a_rms_eps, d.m_dev, d.lo_group, d.ld_out_t, d.rms_eps = int(precision), a_rms_eps, -1 if m_dev is None else int(m_dev), lo_group, ld_out_t, rms_eps
    d.pad_a, d.pad_w, d.pad_out, d.with_ws, d.stray = pad_a, pad_w, pad_out, int(with_ws), -1
    keep = [a, w]
    d.a, d.w = a.ctypes.data_as(_fp), w.ctypes.data_as(_fp)
    if bias is not None:
        bias = _f32(bias); keep.append(bias); d.bias = bias.ctypes.data_as(_fp)
    if add is not None:
        add = _f32(add); keep.append(add); d.add = add.ctypes.data_as(_fp)
        assert add.shape == (M, N), add.shape
    if add2 is not None:
        add2 = _f32(add2); keep.append(add2); d.add2 = add2.ctypes.data_as(_fp); d.add2_table_rows = add2.shape[0]
        assert add2.shape[1] == N, add2.shape
        if add2_rows is not None:
            add2_rows = np.ascontiguousarray(add2_rows, dtype=np.int32); keep.append(add2_rows); d.add2_rows = add2_rows.ctypes.data_as(_ip)
            assert add2_rows.shape == (M,), add2_rows.shape
    out = {}

    def buf(key, shape, field):
        out[key] = np.zeros(shape, dtype=np.float32)
        setattr(d, field, out[key].ctypes.data_as(_fp))

    if argmax:
        out["ids"] = np.zeros((Mv,), dtype=np.int32); d.out_ids = out["ids"].ctypes.data_as(_ip)
    else:
        if "lo" in want:
            buf("lo", (N // lo_group, (M + 127) // 128 * 128, lo_group) if lo_group else (Mv, N // 2 if act == 4 else N), "out_lo")
        if "f32" in want:
            buf("f32", (Mv, N), "out_f32")
        if "stats" in want:
            buf("stats", (Mv, N // 32, 2), "out_stats")
        if "t" in want:
            buf("t", (N, Mv), "out_t")
        if "rms" in want:
            buf("rms", (Mv, N), "out_rms")
    _lib.check(load().asr_probe_gemm(C.byref(d)))
    out["stray"] = int(d.stray)
    return out, d.kernel.decode()


def ctc_head(a, w, bias, n_valid=0, variant=-1):
    """The CTC head with frame log-probabilities (arg-max GEMM with the sum-of-exponentials partial + row reduce) through the product dispatcher;
    returns (ids[M], frame_logprob[M], words written past row M, kernel family name)."""
    a, w, bias = _f32(a), _f32(w), _f32(bias)
    M, K = a.shape
    N = w.shape[0]
    ids, lp = np.zeros((M,), dtype=np.int32), np.zeros((M,), dtype=np.float32)
    stray, name = C.c_int32(-1), C.create_string_buffer(32)
    _lib.check(load().asr_probe_ctc_head(M, N, K, a.ctypes.data_as(_fp), w.ctypes.data_as(_fp), bias.ctypes.data_as(_fp), n_valid, variant,
                                         ids.ctypes.data_as(_ip), lp.ctypes.data_as(_fp), C.byref(stray), name))
    return ids, lp, stray.value, name.value.decode()


def ctc_topk(a, w, bias, topk, n_valid=0, variant=-1, precision=0):
    """The candidate kernel of the CTC prefix beam search behind the head of ctc_head (asr_probe_ctc_topk); precision 0 = bf16 operands, 1 = f32.
    Returns (ids[M, topk], logprob[M, topk], kernel family name of the head GEMM)."""
    a, w, bias = _f32(a), _f32(w), _f32(bias)
    M, K = a.shape
    N = w.shape[0]
    ids, lp = np.zeros((M, topk), dtype=np.int32), np.zeros((M, topk), dtype=np.float32)
    name = C.create_string_buffer(32)
    _lib.check(load().asr_probe_ctc_topk(M, N, K, a.ctypes.data_as(_fp), w.ctypes.data_as(_fp), bias.ctypes.data_as(_fp), n_valid, variant, precision, topk,
                                         ids.ctypes.data_as(_ip), lp.ctypes.data_as(_fp), name))
    return ids, lp, name.value.decode()


def ctc_target_logprob(a, w, bias, row_utt, targets, blank_id=0, n_valid=0, variant=-1, precision=0, ld_em=None):
    """The emission kernel of the CTC forced alignment behind the head of ctc_head (asr_probe_ctc_target_logprob); `targets` is one id list per transcript,
    row_utt[m] the transcript of row m (-1: none). Returns (em[M, ld_em], words written past row M, kernel family name of the head GEMM)."""
    a, w, bias = _f32(a), _f32(w), _f32(bias)
    M, K = a.shape
    N = w.shape[0]
    row_utt = np.ascontiguousarray(row_utt, dtype=np.int32)
    assert row_utt.shape == (M,)
    targets = [np.asarray(t, dtype=np.int32).reshape(-1) for t in targets]
    offs = np.zeros(len(targets) + 1, dtype=np.int32)
    offs[1:] = np.cumsum([t.size for t in targets])
    ids = np.ascontiguousarray(np.concatenate(targets + [np.zeros(1, np.int32)]), dtype=np.int32)
    if ld_em is None:
        ld_em = (max(t.size for t in targets) + 1 + 3) // 4 * 4
    em = np.zeros((M, ld_em), dtype=np.float32)
    stray, name = C.c_int32(-1), C.create_string_buffer(32)
    _lib.check(load().asr_probe_ctc_target_logprob(M, N, K, a.ctypes.data_as(_fp), w.ctypes.data_as(_fp), bias.ctypes.data_as(_fp), n_valid, variant, precision,
                                                   row_utt.ctypes.data_as(_ip), len(targets), ids.ctypes.data_as(_ip), offs.ctypes.data_as(_ip), blank_id, ld_em,
                                                   em.ctypes.data_as(_fp), C.byref(stray), name))
    return em, stray.value, name.value.decode()


def gemm_bench(M, N, K, variant=-1, epilogue=0, iters=50) -> float:
    """Average milliseconds per launch of the bf16 GEMM (device-resident operands)."""
    ms = C.c_float(0.0)
    _lib.check(load().asr_probe_gemm_bench(variant, M, N, K, epilogue, iters, C.byref(ms)))
    return ms.value


def gemm_set_variant(variant: int = -1) -> None:
    """Pin the bf16 GEMM kernel variant for the following op_gemm calls (-1 = heuristic)."""
    gemm_bench(1152, 256, 64, variant, 0, 1)


def gemm_counts(reset: bool = False) -> dict:
    """Launches per GEMM kernel family since the last reset (host-side; a hipGraph replay does not count)."""
    buf = C.create_string_buffer(1024)
    _lib.check(load().asr_probe_gemm_counts(int(reset), buf, 1024))
    return {k: int(v) for k, v in (kv.split("=") for kv in buf.value.decode().split(";") if kv)}


def live_device_bytes() -> int:
    """Device bytes held, process-wide, by session workspaces and the arenas they own (host-side counter)."""
    n = C.c_int64(0)
    _lib.check(load().asr_probe_live_device_bytes(C.byref(n)))
    return n.value


def gemm_chain(M, N, K, epilogue=0, cold_mb=768, replays=5):
    """(microseconds per launch, kernel family) of a captured chain of decode-shaped GEMMs over cold weights."""
    us = C.c_float(0.0)
    _lib.check(load().asr_probe_gemm_chain(M, N, K, epilogue, cold_mb, replays, C.byref(us)))
    return us.value, load().asr_probe_last_kernel().decode()


def decode_attention(q, bf16=True, n=1, B=None, b0=0, nb=0, ld_q=None, q_col0=0, max_keys=0,
                     kv_new=None, k_hist=None, v_hist=None, causal=True, hist_dev=False, max_pos=0, page_table=None, n_pages=0,
                     k_slab=None, v_slab=None, row_off=None, n_lfr=None, fp8=False, key_start=None, prompt=False, ks_entry=False):
    """One decoder attention call through launch_decode_attention (asr_mi355x_probe.h) on f32 host arrays (rounded to the element type on upload).

    Self mode (kv_new given): q [B n][ld_q], kv_new [B n][2 H 64] (k, then v), k_hist / v_hist [B][H][hist][64], a contiguous cache of max_pos
    positions or a paged one (page_table [B][pages_per_seq] over a pool of n_pages pages of 16 positions).
    Cross mode (k_slab given): slabs [H][rows][64], sequence b at rows row_off[b] ... + n_lfr[b]; fp8 routes the slabs through the product quantiser.

    key_start [B] (left-padded prompts): the single-token self forms with DecAttnArgs::key_start (asr_probe_decode_attention_ks), or -- prompt=True --
    the prompt-attention kernel (asr_probe_prompt_attention: any n, empty cache, key_start = the left pads, may be None).

    Returns (out [B n][H 64], after, kernel): `after` is the self cache gathered to (k [B][H][hist + n][64], v [...], stray element count) or,
    in FP8 cross mode, (bytes [2][H][rows][64] uint8, scales [2][H][B]); None otherwise."""
    q = _f32(q)
    d = DecodeAttnDesc()
    cross = k_slab is not None
    H = (k_slab.shape[0] if cross else kv_new.shape[1] // 128)
    if B is None:
        B = (len(n_lfr) if cross else k_hist.shape[0])
    d.bf16, d.cross, d.B, d.b0, d.nb, d.H, d.n = int(bf16), int(cross), B, b0, nb, H, n
    d.causal = int(causal and not cross)
    d.ld_q, d.q_col0, d.max_keys = (ld_q or q.shape[1]), q_col0, max_keys
    assert q.shape == (B * n, d.ld_q), q.shape
    keep = [q]
    d.q = q.ctypes.data_as(_fp)
    out = np.zeros((B * n, H * 64), np.float32)
    d.out = out.ctypes.data_as(_fp)
    after = None
    if not cross:
        kv_new, k_hist, v_hist = _f32(kv_new), _f32(k_hist), _f32(v_hist)
        hist = k_hist.shape[2]
        assert kv_new.shape == (B * n, 2 * H * 64) and k_hist.shape == v_hist.shape == (B, H, hist, 64)
        keep += [kv_new, k_hist, v_hist]
        d.kv_new, d.k_hist, d.v_hist = kv_new.ctypes.data_as(_fp), k_hist.ctypes.data_as(_fp), v_hist.ctypes.data_as(_fp)
        d.hist, d.hist_dev, d.max_pos = hist, int(hist_dev), max_pos
        if page_table is not None:
            pt = np.ascontiguousarray(page_table, np.int32)
            keep.append(pt)
            d.paged, d.n_pages, d.pages_per_seq, d.page_table = 1, n_pages, pt.shape[1], pt.ctypes.data_as(_ip)
        ka = np.zeros((B, H, hist + n, 64), np.float32)
        va = np.zeros_like(ka)
        d.k_after, d.v_after = ka.ctypes.data_as(_fp), va.ctypes.data_as(_fp)
    else:
        k_slab, v_slab = _f32(k_slab), _f32(v_slab)
        ro, nl = np.ascontiguousarray(row_off, np.int32), np.ascontiguousarray(n_lfr, np.int32)
        assert k_slab.shape == v_slab.shape and k_slab.shape[2] == 64 and ro.shape == nl.shape == (B,)
        keep += [k_slab, v_slab, ro, nl]
        d.k_slab, d.v_slab, d.rows = k_slab.ctypes.data_as(_fp), v_slab.ctypes.data_as(_fp), k_slab.shape[1]
        d.row_off, d.n_lfr, d.fp8 = ro.ctypes.data_as(_ip), nl.ctypes.data_as(_ip), int(fp8)
        if fp8:
            kv8 = np.zeros((2, H, k_slab.shape[1], 64), np.uint8)
            sc8 = np.zeros((2, H, B), np.float32)
            d.kv8, d.scale8 = kv8.ctypes.data, sc8.ctypes.data_as(_fp)
            after = (kv8, sc8)
    if prompt or ks_entry or key_start is not None:          # (ks_entry: asr_probe_decode_attention_ks even with a null key_start)
        ks = None if key_start is None else np.ascontiguousarray(key_start, np.int32)
        assert ks is None or ks.shape == (B,)
        entry = load().asr_probe_prompt_attention if prompt else load().asr_probe_decode_attention_ks
        _lib.check(entry(C.byref(d), None if ks is None else ks.ctypes.data_as(_ip)))
    else:
        _lib.check(load().asr_probe_decode_attention(C.byref(d)))
    if not cross:
        after = (ka, va, d.stray)
    return out, after, d.kernel.decode()


def decode_attention_beam(q, kv_new, ext, src, beam, p0, hist, bf16=True, hist_dev=False, key_start=None):
    """One "self_beam" call (asr_mi355x_probe.h): q [rows][H 64], kv_new [rows][2 H 64], ext [rows][2][H][S][64] (the rows' extents before the call),
    src [rows][ld_src] (row holding generated position p0 + j of row r). Returns (out [rows][H 64], ext after the call, stray element count, kernel)."""
    q, kv_new = _f32(q), _f32(kv_new)
    ext = np.array(ext, dtype=np.float32, order="C", copy=True)
    src = np.ascontiguousarray(src, np.int32)
    rows, _, H, S, _ = ext.shape
    assert q.shape == (rows, H * 64) and kv_new.shape == (rows, 2 * H * 64) and src.ndim == 2 and src.shape[0] == rows
    out = np.zeros((rows, H * 64), np.float32)
    stray = np.zeros(1, np.int32)
    kern = C.create_string_buffer(32)
    args = (int(bf16), rows, int(beam), H, S, int(p0), int(hist), int(hist_dev), src.ctypes.data_as(_ip), src.shape[1], q.ctypes.data_as(_fp),
            kv_new.ctypes.data_as(_fp), ext.ctypes.data_as(_fp), out.ctypes.data_as(_fp), stray.ctypes.data_as(_ip), kern)
    if key_start is not None:           # [rows / beam]: the utterances' left pads (asr_probe_decode_attention_beam_ks)
        ks = np.ascontiguousarray(key_start, np.int32)
        assert ks.shape == (rows // beam,)
        _lib.check(load().asr_probe_decode_attention_beam_ks(*args, ks.ctypes.data_as(_ip)))
    else:
        _lib.check(load().asr_probe_decode_attention_beam(*args))
    return out, ext, int(stray[0]), kern.value.decode()


def qwen_attention(qkv, H, KV, qn, kn, rope, eps, hist, T, S_max, bf16=True, step=False, no_fuse=False, row_off=None, k_hist=None, v_hist=None,
                   table=None, n_pages=0, beam=0, src=None, p0=None, ext_k=None, ext_v=None):
    """The attention stage of one Qwen3 decoder layer through launch_qwen_attention (asr_mi355x_probe.h) on f32 host arrays.

    qkv [rows][(H + 2 KV) 128]; sequence b appends T[b] positions at hist[b], its rows starting at row_off[b] (default: consecutive, each sequence at
    the next multiple of 16; a step: row b); rows no sequence owns are gap rows. k_hist / v_hist [seq][KV][>= max hist][128] are the cached rows;
    table [seq][pps] selects the paged layout over a pool of n_pages. beam > 0: rows are hypotheses with extents ext_k / ext_v [B][KV][S_hyp][128],
    ancestry src [B][ld_src] and prompt lengths p0 [B]; the cache is then the utterances' prompt cache.

    Returns dict(ctx, q [rows][H 128] (NaN where unwritten), k_rows [rows][KV 128], k_after / v_after [B][KV][max(hist + T)][128] (NaN past a sequence's
    positions), ext_k / ext_v (beam), stray, kernel, qt, nw, row_off)."""
    qkv = _f32(qkv)
    i32 = lambda x: np.ascontiguousarray(x, np.int32)
    hist, T = i32(hist), i32(T)
    B = hist.size
    rows = qkv.shape[0]
    if row_off is None:
        row_off = np.arange(B) if step else np.concatenate([[0], np.cumsum((T + 15) // 16 * 16)[:-1]])
    row_off = i32(row_off)
    row_seq, row_t = np.full(rows, -1, np.int32), np.zeros(rows, np.int32)
    for b in range(B):
        row_seq[row_off[b]:row_off[b] + T[b]] = b
        row_t[row_off[b]:row_off[b] + T[b]] = np.arange(T[b])
    qn, kn, rope = _f32(qn), _f32(kn), _f32(rope)
    assert qkv.shape == (rows, (H + 2 * KV) * 128) and qn.shape == kn.shape == (128,) and rope.ndim == 2 and rope.shape[1] == 128
    d = QwenAttnDesc()
    d.bf16, d.step, d.no_fuse, d.B, d.H, d.KV, d.rows, d.rope_rows, d.eps, d.S_max = int(bf16), int(step), int(no_fuse), B, H, KV, rows, rope.shape[0], eps, S_max
    keep = [qkv, qn, kn, rope, hist, T, row_off, row_seq, row_t]
    d.qkv, d.qn, d.kn, d.rope = (x.ctypes.data_as(_fp) for x in (qkv, qn, kn, rope))
    d.hist, d.T, d.row_off, d.row_seq, d.row_t = (x.ctypes.data_as(_ip) for x in (hist, T, row_off, row_seq, row_t))
    if k_hist is not None and k_hist.shape[2] > 0:
        k_hist, v_hist = _f32(k_hist), _f32(v_hist)
        assert k_hist.shape == v_hist.shape and k_hist.shape[1:] == (KV, k_hist.shape[2], 128)
        keep += [k_hist, v_hist]
        d.hist_ld, d.k_hist, d.v_hist = k_hist.shape[2], k_hist.ctypes.data_as(_fp), v_hist.ctypes.data_as(_fp)
    if table is not None:
        table = i32(table)
        keep.append(table)
        d.paged, d.n_pages, d.pps, d.table = 1, n_pages, table.shape[1], table.ctypes.data_as(_ip)
    out = dict(ctx=np.zeros((rows, H * 128), np.float32), q=np.zeros((rows, H * 128), np.float32), k_rows=np.zeros((rows, KV * 128), np.float32), row_off=row_off)
    d.ctx, d.q_out, d.k_rows_out = (out[k].ctypes.data_as(_fp) for k in ("ctx", "q", "k_rows"))
    if beam:
        src, p0 = i32(src), i32(p0)
        out["ext_k"], out["ext_v"] = (np.array(x, dtype=np.float32, order="C", copy=True) for x in (ext_k, ext_v))
        assert src.ndim == 2 and src.shape[0] == B and p0.shape == (B,) and out["ext_k"].shape == out["ext_v"].shape == (B, KV, ext_k.shape[2], 128)
        keep += [src, p0]
        d.beam, d.ld_src, d.S_hyp, d.src, d.p0 = beam, src.shape[1], ext_k.shape[2], src.ctypes.data_as(_ip), p0.ctypes.data_as(_ip)
        d.ext_k, d.ext_v = out["ext_k"].ctypes.data_as(_fp), out["ext_v"].ctypes.data_as(_fp)
    else:
        n_after = int((hist + T).max())
        out["k_after"], out["v_after"] = np.full((B, KV, n_after, 128), np.nan, np.float32), np.full((B, KV, n_after, 128), np.nan, np.float32)
        d.after_ld, d.k_after, d.v_after = n_after, out["k_after"].ctypes.data_as(_fp), out["v_after"].ctypes.data_as(_fp)
    _lib.check(load().asr_probe_qwen_attention(C.byref(d)))
    out.update(stray=d.stray, kernel=d.kernel.decode(), qt=d.qt, nw=d.nw)
    return out


def encoder_attention(q, k, v, key_lens, n_heads, head_dim, bf16=True, q_lens=None, kv_group=1, causal=False, packed_qk=False, slack_rows=128,
                      pad_fill_k=64.0, pad_fill_v=1e4):
    """The ragged encoder attention through the sessions' launchers (asr_probe_encoder_attention, asr_mi355x_probe.h): q [sum Tq][H hd],
    k / v [sum T][(H / kv_group) hd], dense. Returns dict(ctx [sum Tq][H hd], instance = (hd, chunk, qt, waves) of the bf16 kernel that ran,
    grid_z (f32: the gridDim.z chosen; bf16: 0), n_qblocks, stray)."""
    q, k, v = _f32(q), _f32(k), _f32(v)
    key_lens = np.ascontiguousarray(key_lens, np.int32)
    d = EncAttnDesc()
    d.bf16, d.head_dim, d.n_heads, d.kv_group, d.causal, d.batch = int(bf16), head_dim, n_heads, kv_group, int(causal), key_lens.size
    d.packed_qk, d.slack_rows, d.pad_fill_k, d.pad_fill_v = int(packed_qk), slack_rows, pad_fill_k, pad_fill_v
    d.key_lens = key_lens.ctypes.data_as(_ip)
    n_q = int(key_lens.sum())
    if q_lens is not None:
        q_lens = np.ascontiguousarray(q_lens, np.int32)
        assert q_lens.shape == key_lens.shape
        d.q_lens = q_lens.ctypes.data_as(_ip)
        n_q = int(q_lens.sum())
    dk = n_heads // kv_group * head_dim
    assert q.shape == (n_q, n_heads * head_dim) and k.shape == v.shape == (int(key_lens.sum()), dk), (q.shape, k.shape, v.shape)
    ctx = np.zeros((n_q, n_heads * head_dim), np.float32)
    d.q, d.k, d.v, d.ctx = (x.ctypes.data_as(_fp) for x in (q, k, v, ctx))
    d.stray = -1
    _lib.check(load().asr_probe_encoder_attention(C.byref(d)))
    return dict(ctx=ctx, instance=(d.hd, d.chunk, d.qt, d.waves), grid_z=d.grid_z, n_qblocks=d.n_qblocks, stray=int(d.stray))


def fsmn(v, w, b, lens, bf16=False, pad_fill=1e4):
    """launch_fsmn on v [sum T][C] with poisoned pad columns (asr_probe_fsmn) -> (out [sum T][C] f32, stray)."""
    v, w, b = _f32(v), _f32(w), _f32(b)
    lens = np.ascontiguousarray(lens, np.int32)
    C_ = v.shape[1]
    assert v.shape[0] == int(lens.sum()) and w.shape == (C_, 11) and b.shape == (C_,), (v.shape, w.shape, b.shape)
    out = np.zeros_like(v)
    d = FsmnDesc()
    d.bf16, d.batch, d.channels, d.pad_fill, d.stray = int(bf16), lens.size, C_, pad_fill, -1
    d.lens, d.v, d.w, d.b, d.out = lens.ctypes.data_as(_ip), v.ctypes.data_as(_fp), w.ctypes.data_as(_fp), b.ctypes.data_as(_fp), out.ctypes.data_as(_fp)
    _lib.check(load().asr_probe_fsmn(C.byref(d)))
    return out, int(d.stray)


def beam_select(beam, K, n_slots, topv, topi, cum, fin, length, nxt, done, src_in, tok_in, src_out, tok_out, stop=(), first=False):
    """One launch_beam_select pass (asr_mi355x_probe.h) on host arrays -> dict of the state and tables after it (inputs are not modified)."""
    f32 = lambda x: np.array(x, np.float32, order="C", copy=True)
    i32 = lambda x: np.array(x, np.int32, order="C", copy=True)
    st = dict(topv=f32(topv), topi=i32(topi), cum=f32(cum), fin=i32(fin), len=i32(length), next=i32(nxt), done=i32(done),
              stop=i32(list(stop) or [0]), src_in=i32(src_in), tok_in=i32(tok_in), src_out=i32(src_out), tok_out=i32(tok_out))
    d = BeamSelectDesc()
    d.n_utt, d.beam, d.K, d.ld, d.first, d.n_slots, d.n_stop = st["done"].size, beam, K, st["src_in"].shape[1], int(first), n_slots, len(stop)
    for k in ("topv", "cum"):
        setattr(d, k, st[k].ctypes.data_as(_fp))
    for k in ("topi", "fin", "len", "next", "done", "stop", "src_in", "tok_in", "src_out", "tok_out"):
        setattr(d, k, st[k].ctypes.data_as(_ip))
    _lib.check(load().asr_probe_beam_select(C.byref(d)))
    return st


PAD_LOGIT = np.float32(1e30)              # what token_head puts in the pad columns [n_valid, ld) of every logits row
_HEAD_OPS = {"argmax_rows": 0, "beam_topk": 1, "apply_penalty": 2, "append_ids": 3, "sample_topk_topp": 4, "no_speech_prob": 5, "timestamp_rules": 7,
             "argmax_logprob_rows": 8, "logprob_at_rows": 9}


def token_head(op, logits=None, vec=None, K=0, save_ids=None, n_saved=0, range_=0, value=1.0, partial=0, next_ids=None,
               temperature=1.0, top_p=1.0, repetition_penalty=1.0, noise=None, seed=0, no_speech_id=0, timestamps=None, logprob=None, ld_save=0):
    """One token-selection head (asr_mi355x_probe.h: asr_probe_token_head) through its product launcher; `op` is the launcher's name less "launch_".

    logits [rows][n_valid] are laid out with the sessions' leading dimension ld = roundup(n_valid, 128), the pad filled with PAD_LOGIT (+1e30: a kernel
    that lets a pad column into a maximum, a top-k list or a soft-max sum fails visibly); vec (extra / bias / penalty, [n_valid]) gets zeros there.
    timestamp_rules: timestamps = (ts_begin, no_timestamps_id, eot_id, max_initial); n_saved is one length for every row or an array of per-row lengths.
    argmax_logprob_rows / logprob_at_rows: logprob = the score history [rows][ld_save] as it stands before the call (the caller's fill pattern), n_saved the
    counter, next_ids the ids to score (logprob_at_rows); "ids" starts from a -1 fill, "logprob" comes back with whatever the kernel wrote.
    Returns a dict: the head's outputs (ids | topv, topi | next | prob), logits [rows][ld] after the call, save_ids (the whole table) and n_saved after it."""
    d = TokenHeadDesc()
    d.op = _HEAD_OPS[op]
    out, keep = {}, []
    if logits is not None:
        logits = _f32(logits)
        rows, n_valid = logits.shape
        ld = (n_valid + 127) // 128 * 128
        padded = np.full((rows, ld), PAD_LOGIT, np.float32)
        padded[:, :n_valid] = logits
        out["logits"] = padded
        d.logits, d.n_valid, d.ld = padded.ctypes.data_as(_fp), n_valid, ld
        if vec is not None:
            v = np.zeros(ld, np.float32)
            v[:n_valid] = _f32(vec)
            keep.append(v); d.vec = v.ctypes.data_as(_fp)
    else:
        rows, d.n_valid, d.ld = len(next_ids), 1, 128
    d.rows, d.K = rows, K
    if save_ids is not None:
        out["save_ids"] = np.array(save_ids, np.int32, order="C", copy=True)
        assert out["save_ids"].ndim == 2 and out["save_ids"].shape[0] == rows
        d.save_ids, d.ld_save = out["save_ids"].ctypes.data_as(_ip), out["save_ids"].shape[1]
        if np.ndim(n_saved) == 0:
            d.n_saved = int(n_saved)
        else:
            per_row = np.ascontiguousarray(n_saved, np.int32)
            assert op == "timestamp_rules" and per_row.shape == (rows,)
            keep.append(per_row); d.n_saved_rows = per_row.ctypes.data_as(_ip)
    if timestamps is not None:
        d.ts_begin, d.no_timestamps_id, d.eot_id, d.max_initial = (int(v) for v in timestamps)
    d.range, d.partial, d.value = range_, partial, value
    if next_ids is not None:
        nx = np.ascontiguousarray(next_ids, np.int32)
        keep.append(nx); d.next_in = nx.ctypes.data_as(_ip)
    d.temperature, d.top_p, d.repetition_penalty, d.seed, d.no_speech_id = temperature, top_p, repetition_penalty, seed, no_speech_id
    if noise is not None:
        noise = _f32(noise)
        assert noise.shape == (rows, K)
        d.noise = noise.ctypes.data_as(_fp)
    if op == "beam_topk":
        out["topv"], out["topi"] = np.zeros((rows, K), np.float32), np.zeros((rows, K), np.int32)
        d.out_v, d.out_i = out["topv"].ctypes.data_as(_fp), out["topi"].ctypes.data_as(_ip)
    elif op == "no_speech_prob":
        out["prob"] = np.zeros(rows, np.float32)
        d.out_v = out["prob"].ctypes.data_as(_fp)
    elif op in ("argmax_logprob_rows", "logprob_at_rows"):
        out["logprob"] = np.array(logprob, np.float32, order="C", copy=True)
        assert out["logprob"].ndim == 2 and out["logprob"].shape[0] == rows
        d.logprob, d.ld_save, d.n_saved = out["logprob"].ctypes.data_as(_fp), out["logprob"].shape[1], int(n_saved)
        if op == "argmax_logprob_rows":
            out["ids"] = np.full(rows, -1, np.int32)
            d.out_i = out["ids"].ctypes.data_as(_ip)
    elif op in ("argmax_rows", "sample_topk_topp"):
        key = "ids" if op == "argmax_rows" else "next"
        out[key] = np.full(rows, -1, np.int32)
        d.out_i = out[key].ctypes.data_as(_ip)
    _lib.check(load().asr_probe_token_head(C.byref(d)))
    if save_ids is not None:
        out["n_saved"] = d.n_saved_after
    return out


def head_steps(logits, steps, ld_save, range_, value, partial, bias=None, track_history=False, sampler=None, noise=None, change=None, timestamps=None,
               scores=False, timed=False):
    """A TokenHead (csrc/decode_head.h) driven through `steps` decoder steps on the same logits rows (asr_probe_token_head, op 6): step 0 is a prefill
    (`bias` added, no penalty), the others are decode steps. sampler: (temperature, top_k, top_p, repetition_penalty, seed) or None; noise: uniforms
    [rows][top_k] armed for step 0; change: (step, value, range) -- set_penalty before that step; timestamps: (ts_begin, no_timestamps_id, eot_id,
    max_initial) -- Whisper's timestamp mode on; scores: token scores on. Rows are padded as token_head pads them.
    Returns {"picks": [steps][rows], "save_ids": the final history [rows][ld_save], "n_saved": the counter} and, with scores, "logprob": the score history
    [rows][ld_save] (NaN where no step wrote). timed (plain arg-max head only): the rows are uploaded once and "head_ms" is the device time of the steps'
    launches, run back to back (tools/probes/token_scores_timing.py)."""
    logits = _f32(logits)
    rows, n_valid = logits.shape
    ld = (n_valid + 127) // 128 * 128
    padded = np.full((rows, ld), PAD_LOGIT, np.float32)
    padded[:, :n_valid] = logits
    d = TokenHeadDesc()
    d.op, d.rows, d.n_valid, d.ld, d.logits = 6, rows, n_valid, ld, padded.ctypes.data_as(_fp)
    if bias is not None:
        v = np.zeros(ld, np.float32)
        v[:n_valid] = _f32(bias)
        d.vec = v.ctypes.data_as(_fp)
    d.steps, d.ld_save, d.range, d.value, d.partial, d.track_history = steps, ld_save, range_, value, partial, int(track_history)
    if sampler is not None:
        d.sampling, (d.temperature, d.K, d.top_p, d.repetition_penalty, d.seed) = 1, sampler
    if noise is not None:
        noise = _f32(noise)
        assert noise.shape == (rows, d.K)
        d.noise = noise.ctypes.data_as(_fp)
    if change is not None:
        d.change_step, d.value2, d.range2 = change
    if timestamps is not None:
        d.timestamps, (d.ts_begin, d.no_timestamps_id, d.eot_id, d.max_initial) = 1, (int(v) for v in timestamps)
    out = {"picks": np.full((steps, rows), -1, np.int32), "save_ids": np.full((rows, ld_save), -1, np.int32)}
    d.picks, d.save_ids = out["picks"].ctypes.data_as(_ip), out["save_ids"].ctypes.data_as(_ip)
    if scores:
        out["logprob"] = np.zeros((rows, ld_save), np.float32)
        d.scores, d.logprob = 1, out["logprob"].ctypes.data_as(_fp)
    d.timed = int(timed)
    _lib.check(load().asr_probe_token_head(C.byref(d)))
    out["n_saved"] = d.n_saved_after
    if timed:
        out["head_ms"] = float(d.head_ms)
    return out


def _pad_rows(logits):
    """[..., n_valid] -> ([..., ld] with PAD_LOGIT in the pad columns, n_valid, ld): the sessions' leading dimension, as token_head pads."""
    logits = _f32(logits)
    n_valid = logits.shape[-1]
    ld = (n_valid + 127) // 128 * 128
    padded = np.full(logits.shape[:-1] + (ld,), PAD_LOGIT, np.float32)
    padded[..., :n_valid] = logits
    return padded, n_valid, ld


def _phrases(d, phrases, boost, keep):
    """Flatten token-id lists into the ids / offsets / n_phrases / boost fields of a hotword descriptor."""
    phrases = [np.asarray(p, np.int32).reshape(-1) for p in phrases]
    offs = np.zeros(len(phrases) + 1, np.int32)
    offs[1:] = np.cumsum([p.size for p in phrases])
    ids = np.ascontiguousarray(np.concatenate(phrases) if phrases else np.zeros(1, np.int32), np.int32)
    keep += [ids, offs]
    d.ids, d.offsets, d.n_phrases, d.boost = ids.ctypes.data_as(_ip), offs.ctypes.data_as(_ip), len(phrases), float(boost)


def hotword_op(op, phrases, boost, node, logits=None, n_saved=1, next_ids=None, bias=None, K=0, n_root=0):
    """One hotword kernel on host arrays (asr_probe_hotword). op "bias": logits [rows][n_valid] -> {"logits" [rows][ld] after the update, "root_save"
    [rows][n_root] when n_root > 0 (NaN where nothing was saved)}; "advance": next_ids -> {"node"}; "rerank": launch_beam_topk + launch_hotword_rerank ->
    {"topv", "topi" [rows][K], "lse" [rows]}. node [rows]: the rows' trie nodes; n_saved: the device counter (0: every row counts as at the root)."""
    d, keep, out = HotwordDesc(), [], {}
    d.op = {"bias": 0, "advance": 1, "rerank": 2}[op]
    node = np.array(node, np.int32, order="C", copy=True)
    d.rows, d.node, d.n_saved = node.size, node.ctypes.data_as(_ip), int(n_saved)
    _phrases(d, phrases, boost, keep)
    if logits is not None:
        out["logits"], d.n_valid, d.ld = _pad_rows(logits)
        d.logits = out["logits"].ctypes.data_as(_fp)
        if bias is not None:
            v = np.zeros(d.ld, np.float32)
            v[:d.n_valid] = _f32(bias)
            keep.append(v); d.vec = v.ctypes.data_as(_fp)
    if next_ids is not None:
        nx = np.ascontiguousarray(next_ids, np.int32)
        keep.append(nx); d.next_in = nx.ctypes.data_as(_ip)
    if op == "bias" and n_root:
        out["root_save"] = np.full((node.size, n_root), np.nan, np.float32)
        d.root_save, d.n_root = out["root_save"].ctypes.data_as(_fp), n_root
    if op == "rerank":
        out["topv"], out["topi"], out["lse"] = np.zeros((node.size, K), np.float32), np.zeros((node.size, K), np.int32), np.zeros(node.size, np.float32)
        d.K, d.topv, d.topi, d.lse = K, out["topv"].ctypes.data_as(_fp), out["topi"].ctypes.data_as(_ip), out["lse"].ctypes.data_as(_fp)
    _lib.check(load().asr_probe_hotword(C.byref(d)))
    out["node"] = node
    return out


def _lm_model(lm, keep):
    """lm = dict(image, alpha, beta, oov, topk, end_ids) -> the model descriptor of the LM hooks."""
    m = LmModel()
    img = np.ascontiguousarray(lm["image"], np.int32)
    ends = np.ascontiguousarray(list(lm.get("end_ids", ())) or [0], np.int32)
    keep += [img, ends]
    m.image, m.n_words, m.alpha, m.beta, m.oov_logprob = img.ctypes.data_as(_ip), img.size, float(lm["alpha"]), float(lm["beta"]), float(lm.get("oov", 0.0))
    m.topk, m.end_ids, m.n_end = int(lm["topk"]), ends.ctypes.data_as(_ip), len(lm.get("end_ids", ()))
    return m


def lm_topk(logits, M, bias=None, iters=0):
    """launch_lm_topk on logits [rows][n_valid], padded as token_head pads them (asr_probe_lm_topk) -> {"cand_v", "cand_i" [rows][M], "lse" [rows],
    "slow_rows": rows that took the strict-order passes}; iters > 0 adds "ms_lm_topk" / "ms_beam_topk" (beam_topk at K = min(M, 8)) per `iters` launches."""
    d, keep = LmTopkDesc(), []
    padded, n_valid, ld = _pad_rows(logits)
    rows = len(padded)
    d.rows, d.n_valid, d.ld, d.M, d.logits, d.iters = rows, n_valid, ld, int(M), padded.ctypes.data_as(_fp), int(iters)
    if bias is not None:
        v = np.zeros(ld, np.float32)
        v[:n_valid] = _f32(bias)
        keep.append(v); d.vec = v.ctypes.data_as(_fp)
    out = {"cand_v": np.full((rows, M), np.nan, np.float32), "cand_i": np.full((rows, M), -1, np.int32), "lse": np.full(rows, np.nan, np.float32)}
    d.cand_v, d.cand_i, d.lse = out["cand_v"].ctypes.data_as(_fp), out["cand_i"].ctypes.data_as(_ip), out["lse"].ctypes.data_as(_fp)
    _lib.check(load().asr_probe_lm_topk(C.byref(d)))
    out["slow_rows"] = int(d.slow_rows)
    if iters:
        out["ms_lm_topk"], out["ms_beam_topk"] = float(d.ms_lm_topk), float(d.ms_beam_topk)
    return out


def lm_pick(lm, cand_v, cand_i, lse, state, n_saved=1, ld_save=0):
    """launch_lm_pick on host candidates [rows][topk] (asr_probe_lm_pick) -> {"next", "state" [rows]} and "logprob" [rows][ld_save] (NaN where nothing was
    written) when ld_save > 0."""
    d, keep = LmPickDesc(), []
    m = _lm_model(lm, keep)
    cv, ci, ls = _f32(cand_v), np.ascontiguousarray(cand_i, np.int32), _f32(lse)
    rows = len(cv)
    assert cv.shape == ci.shape == (rows, m.topk) and ls.shape == (rows,)
    out = {"state": np.array(state, np.int32, order="C", copy=True), "next": np.full(rows, -1, np.int32)}
    d.rows, d.n_saved, d.ld_save = rows, int(n_saved), int(ld_save)
    d.cand_v, d.cand_i, d.lse = cv.ctypes.data_as(_fp), ci.ctypes.data_as(_ip), ls.ctypes.data_as(_fp)
    d.state, d.next = out["state"].ctypes.data_as(_ip), out["next"].ctypes.data_as(_ip)
    if ld_save:
        out["logprob"] = np.full((rows, ld_save), np.nan, np.float32)
        d.logprob = out["logprob"].ctypes.data_as(_fp)
    _lib.check(load().asr_probe_lm_pick(C.byref(m), C.byref(d)))
    return out


def hotword_head_steps(logits, phrases, boost, ld_save, range_=4, value=1.0, partial=0, bias=None, sampler=None, noise=None, timestamps=None, scores=False,
                       want_logits=False, timed=0, lm=None):
    """A TokenHead with hotwords driven through logits [steps][rows][n_valid], a different row per step (asr_probe_hotword_head_steps): step 0 is a prefill
    (`bias` added, no penalty). sampler: (temperature, top_k, top_p, repetition_penalty, seed); noise [steps][rows][top_k]: caller uniforms for every step;
    timestamps: (ts_begin, no_timestamps_id, eot_id, max_initial). An empty phrase list leaves the mode off.
    Returns {"picks" [steps][rows], "save_ids" [rows][ld_save], "n_saved", "nodes" [steps][rows] (-1 with the mode off)} and "logprob" [rows][ld_save] with
    scores, "logits" [steps][rows][ld] with want_logits. timed = N > 0 (arg-max head): logits holds one step's rows [1][rows][n_valid], reused by N steps
    whose launches run back to back between two device events -> "head_ms" (tools/probes/hotword_timing.py); picks and histories are not results then.
    lm: dict(image, alpha, beta, oov, topk, end_ids) -- the model is set after the hotwords (asr_probe_lm_head_steps) and "states" [steps][rows] comes back."""
    d, keep = HotwordHeadDesc(), []
    padded, n_valid, ld = _pad_rows(logits)
    steps, rows = padded.shape[:2]
    if timed:
        assert steps == 1
        steps = int(timed)
    d.rows, d.n_valid, d.ld, d.steps, d.logits = rows, n_valid, ld, steps, padded.ctypes.data_as(_fp)
    if bias is not None:
        v = np.zeros(ld, np.float32)
        v[:n_valid] = _f32(bias)
        keep.append(v); d.vec = v.ctypes.data_as(_fp)
    d.ld_save, d.range, d.partial, d.value = ld_save, range_, partial, value
    if sampler is not None:
        d.sampling, (d.temperature, d.K, d.top_p, d.repetition_penalty, d.seed) = 1, sampler
    if noise is not None:
        noise = _f32(noise)
        assert noise.shape == (steps, rows, d.K)
        d.noise = noise.ctypes.data_as(_fp)
    if timestamps is not None:
        d.timestamps, (d.ts_begin, d.no_timestamps_id, d.eot_id, d.max_initial) = 1, (int(v) for v in timestamps)
    _phrases(d, phrases, boost, keep)
    out = {"picks": np.full((steps, rows), -1, np.int32), "save_ids": np.full((rows, ld_save), -1, np.int32), "nodes": np.full((steps, rows), -1, np.int32)}
    d.picks, d.save_ids, d.nodes = (out[k].ctypes.data_as(_ip) for k in ("picks", "save_ids", "nodes"))
    if scores:
        out["logprob"] = np.zeros((rows, ld_save), np.float32)
        d.scores, d.logprob = 1, out["logprob"].ctypes.data_as(_fp)
    if want_logits:
        out["logits"] = np.zeros_like(padded)
        d.logits_out = out["logits"].ctypes.data_as(_fp)
    d.timed = int(bool(timed))
    if lm is not None:
        out["states"] = np.full((steps, rows), -1, np.int32)
        _lib.check(load().asr_probe_lm_head_steps(C.byref(_lm_model(lm, keep)), C.byref(d), out["states"].ctypes.data_as(_ip)))
    else:
        _lib.check(load().asr_probe_hotword_head_steps(C.byref(d)))
    out["n_saved"] = d.n_saved_after
    if timed:
        out["head_ms"] = float(d.head_ms)
    return out


def hotword_rank(logits, phrases, boost, beam, n_slots, cum, fin, length, nxt, done, src_in, tok_in, node_in, stop=(), first=False, bias=None, iters=0, lm=None,
                 state_in=None):
    """One ranking pass of the beam search with hotwords (asr_probe_hotword_rank): beam_topk + re-rank + select with the node hand-over, on logits
    [rows][n_valid] ([n_utt][n_valid] when first). Returns the state, the tables written (from a -1 fill), "node_out" and the re-ranked "topv" / "topi".
    lm: dict(image, alpha, beta, oov, topk, end_ids) -- the pass with the model on (asr_probe_lm_rank: lm_topk + lm_rerank + select; the phrase list may be
    empty), state_in [rows] the rows' LM states; "state_out" comes back."""
    d, keep = HotwordRankDesc(), []
    f32 = lambda x: np.array(x, np.float32, order="C", copy=True)
    i32 = lambda x: np.array(x, np.int32, order="C", copy=True)
    padded, n_valid, ld = _pad_rows(logits)
    st = dict(cum=f32(cum), fin=i32(fin), len=i32(length), next=i32(nxt), done=i32(done), stop=i32(list(stop) or [0]), src_in=i32(src_in), tok_in=i32(tok_in),
              node_in=i32(node_in))
    st["src_out"], st["tok_out"] = np.full_like(st["src_in"], -1), np.full_like(st["tok_in"], -1)
    st["node_out"] = np.full_like(st["node_in"], -1)
    st["topv"], st["topi"] = np.zeros((len(padded), beam), np.float32), np.zeros((len(padded), beam), np.int32)
    d.n_utt, d.beam, d.tab_ld, d.first, d.n_slots, d.n_stop = st["done"].size, beam, st["src_in"].shape[1], int(first), n_slots, len(stop)
    d.n_valid, d.ld, d.logits = n_valid, ld, padded.ctypes.data_as(_fp)
    if bias is not None:
        v = np.zeros(ld, np.float32)
        v[:n_valid] = _f32(bias)
        keep.append(v); d.vec = v.ctypes.data_as(_fp)
    _phrases(d, phrases, boost, keep)
    for k in ("cum", "topv"):
        setattr(d, k, st[k].ctypes.data_as(_fp))
    for k in ("fin", "len", "next", "done", "stop", "src_in", "tok_in", "src_out", "tok_out", "node_in", "node_out", "topi"):
        setattr(d, k, st[k].ctypes.data_as(_ip))
    d.iters = int(iters)
    if lm is not None:
        sin = i32(state_in if state_in is not None else np.zeros(st["node_in"].size, np.int32))
        st["state_out"] = np.full_like(sin, -1)
        _lib.check(load().asr_probe_lm_rank(C.byref(_lm_model(lm, keep)), C.byref(d), sin.ctypes.data_as(_ip), st["state_out"].ctypes.data_as(_ip)))
    else:
        _lib.check(load().asr_probe_hotword_rank(C.byref(d)))
    if iters:
        st["ms_topk"], st["ms_rerank"] = float(d.ms_topk), float(d.ms_rerank)
    return st


def _bf16_bits(x):
    """f32 array -> bf16 bit patterns (round to nearest even), as uint16."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def _bf16_to_f32(bits):
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def _pitched(wb, ld):
    """[N][K] bf16 bits -> [N][ld] with 0x7f00 (1.7e38) in the gap: a quantiser that read it would take its scale from it."""
    out = np.full((wb.shape[0], ld), 0x7F00, np.uint16)
    out[:, :wb.shape[1]] = wb
    return out


def quantize_fp8(w, ld=0):
    """Row quantiser of the FP8 mode on an f32 array (rounded to bf16 first): (bytes [N][K] uint8, scale [N] f32, dequantised f32 [N][K]). ld > K: the rows are
    uploaded with that pitch, the gap holding 1.7e38."""
    wb = _bf16_bits(w)
    N, K = wb.shape
    q = np.zeros((N, K), np.uint8); sc = np.zeros((N,), np.float32); dq = np.zeros((N, K), np.uint16)
    if ld:
        wp = _pitched(wb, ld)
        _lib.check(load().asr_probe_quantize_fp8_ld(wp.ctypes.data, ld, N, K, q.ctypes.data, sc.ctypes.data_as(_fp), dq.ctypes.data))
    else:
        _lib.check(load().asr_probe_quantize_fp8(wb.ctypes.data, N, K, q.ctypes.data, sc.ctypes.data_as(_fp), dq.ctypes.data))
    return q, sc, _bf16_to_f32(dq)


def quantize_mxfp4(w, ld=0):
    """Block quantiser of the MXFP4 mode on an f32 array (rounded to bf16 first): (nibbles [N][K / 2] uint8, e8m0 scales [N][K / 32] uint8, dequantised f32 [N][K]).
    ld > K: as quantize_fp8."""
    wb = _bf16_bits(w)
    N, K = wb.shape
    q = np.zeros((N, K // 2), np.uint8); sc = np.zeros((N, K // 32), np.uint8); dq = np.zeros((N, K), np.uint16)
    if ld:
        wp = _pitched(wb, ld)
        _lib.check(load().asr_probe_quantize_mxfp4_ld(wp.ctypes.data, ld, N, K, q.ctypes.data, sc.ctypes.data, dq.ctypes.data))
    else:
        _lib.check(load().asr_probe_quantize_mxfp4(wb.ctypes.data, N, K, q.ctypes.data, sc.ctypes.data, dq.ctypes.data))
    return q, sc, _bf16_to_f32(dq)


def decode_gemm_mxfp4(a, w4, scale8, w_dq=None, bias=None, fold=False):
    """Decode GEMM (<= 64 rows) over MXFP4 weights; w_dq (f32, exact in bf16) supplies the column sums of the LayerNorm fold."""
    ab = _bf16_bits(a)
    M, K = ab.shape
    N = w4.shape[0]
    out = np.zeros((M, N), np.float32)
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    dq = None if w_dq is None else _bf16_bits(w_dq)
    q, s = np.ascontiguousarray(w4, np.uint8), np.ascontiguousarray(scale8, np.uint8)
    _lib.check(load().asr_probe_decode_gemm_mxfp4(M, N, K, ab.ctypes.data, q.ctypes.data, s.ctypes.data, None if dq is None else dq.ctypes.data,
                                                  None if b is None else b.ctypes.data_as(_fp), int(fold), out.ctypes.data_as(_fp)))
    return out


def decode_gemm(a, w=None, w8=None, scale=None, bias=None, fold=False):
    """Decode GEMM (<= 64 rows) on host arrays: a [M][K] f32 (rounded to bf16), weights either f32 `w` (rounded to bf16) or (w8, scale)."""
    ab = _bf16_bits(a)
    M, K = ab.shape
    wb = None if w is None else _bf16_bits(w)
    N = (wb if wb is not None else w8).shape[0]
    out = np.zeros((M, N), np.float32)
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    s = None if scale is None else np.ascontiguousarray(scale, np.float32)
    q = None if w8 is None else np.ascontiguousarray(w8, np.uint8)
    _lib.check(load().asr_probe_decode_gemm(M, N, K, ab.ctypes.data, None if wb is None else wb.ctypes.data, None if q is None else q.ctypes.data,
                                            None if s is None else s.ctypes.data_as(_fp), None if b is None else b.ctypes.data_as(_fp), int(fold),
                                            out.ctypes.data_as(_fp)))
    return out


def decode_gemm_desc(a, w, wq=None, w_scale=None, w_scale8=None, bias=None, fold=False, ln_eps=1e-5, add=None, act=0, want=("f32",), plan_M=0, lda=0, ldw=0,
                     ld_add=0, ld_out_f32=0, ld_out_lo=0, with_ws=True, repeats=1, nt=0, splits=0, row_blocks=0, pre_M=0, pre_splits=0):
    """The decode GEMM with every DecGemmArgs term (asr_probe_decode_gemm_desc). a [M][K], w [N][K] f32, both exact in bf16 after rounding here; w is the weight
    matrix, or with wq its dequantised copy: (wq [N][K] uint8, w_scale [N]) = e4m3 bytes, (wq [N][K / 2], w_scale8 [N][K / 32]) = e2m1 nibbles + e8m0.
    nt / splits / row_blocks force the plan (0: decode_gemm_plan). -> dict: "f32" / "lo" [M][N], "plan" = (mt, nt, splits, row_blocks) as launched, "stray",
    "tickets_zero"."""
    ab, wb = _bf16_bits(a), _bf16_bits(w)
    (M, K), N = ab.shape, wb.shape[0]
    d = DecGemmDesc(M=M, N=N, K=K, plan_M=plan_M, lda=lda, ldw=ldw, ld_add=ld_add, ld_out_f32=ld_out_f32, ld_out_lo=ld_out_lo, fold=int(fold), ln_eps=ln_eps,
                    act=act, with_ws=int(with_ws), repeats=repeats, force_nt=nt, force_splits=splits, force_row_blocks=row_blocks, pre_M=pre_M, pre_splits=pre_splits)
    keep = [ab, wb]
    d.a, d.w_bf16 = ab.ctypes.data, wb.ctypes.data
    if wq is not None:
        q = np.ascontiguousarray(wq, np.uint8); keep.append(q); d.wq = q.ctypes.data
        if w_scale8 is not None:
            s8 = np.ascontiguousarray(w_scale8, np.uint8); keep.append(s8); d.w_scale8 = s8.ctypes.data; d.wkind = 2
            assert q.shape == (N, K // 2) and s8.shape == (N, K // 32)
        else:
            sc = _f32(w_scale); keep.append(sc); d.w_scale = sc.ctypes.data_as(_fp); d.wkind = 1
            assert q.shape == (N, K) and sc.shape == (N,)
    if bias is not None:
        bias = _f32(bias); keep.append(bias); d.bias = bias.ctypes.data_as(_fp)
    if add is not None:
        add = _f32(add); keep.append(add); d.add = add.ctypes.data_as(_fp)
        assert add.shape == (M, N)
    out = {}
    for key in want:
        out[key] = np.zeros((M, N), np.float32)
        setattr(d, {"f32": "out_f32", "lo": "out_lo"}[key], out[key].ctypes.data_as(_fp))
    _lib.check(load().asr_probe_decode_gemm_desc(C.byref(d)))
    out["plan"], out["stray"], out["tickets_zero"] = (d.mt, d.nt, d.splits, d.row_blocks), d.stray, bool(d.tickets_zero)
    return out


def quantize_crosskv_fp8(slabs, row_off, n_lfr, dq_in_place=False):
    """launch_quantize_crosskv_fp8 on an f32 array [n_slabs][rows][64] (rounded to bf16 first): (bytes [n_slabs][rows][64], 0xa5 where nothing was written;
    scale [n_slabs][batch]; the slabs after the launch as f32)."""
    sb = _bf16_bits(slabs)
    S, R, hd = sb.shape
    assert hd == 64
    ro, nl = _i32(row_off), _i32(n_lfr)
    q = np.zeros((S, R, 64), np.uint8); sc = np.zeros((S, ro.size), np.float32)
    _lib.check(load().asr_probe_quantize_crosskv_fp8(sb.ctypes.data, S, R, _ptr(ro, _ip), _ptr(nl, _ip), ro.size, int(dq_in_place), q.ctypes.data, _ptr(sc, _fp)))
    return q, sc, _bf16_to_f32(sb)


def layernorm_fp8(x, D, eps, inv_scale, ld_out):
    """launch_layernorm_fp8 on x [rows][ld_x] f32 (the first D columns are the row): bytes [rows + 4][ld_out], 0xa5 where nothing was written."""
    x = _f32(x)
    rows, ld_x = x.shape
    out = np.zeros((rows + 4, ld_out), np.uint8)
    _lib.check(load().asr_probe_layernorm_fp8(_ptr(x, _fp), ld_x, rows, D, eps, inv_scale, ld_out, out.ctypes.data))
    return out


def gemm_fp8_v2(a8, w8, w_scale, bias, a_scale=1.0, add=None, act=0, out_inv_scale=1.0, lda=0, ldw=0, ld_add=0, ld_out=0):
    """FP8 matrix-pipe GEMM with pitches (0: the extent), out_inv_scale and the saturation count: -> (out as laid out, [M + 8][ld_out], uint8 with 0xa5 where nothing
    was written / float32 with NaN there when `add` is given; sat_count)."""
    a8, w8 = np.ascontiguousarray(a8, np.uint8), np.ascontiguousarray(w8, np.uint8)
    (M, K), N = a8.shape, w8.shape[0]
    sc, b = _f32(w_scale), _f32(bias)
    ld_out = ld_out or N
    sat = C.c_uint64(0)
    if add is None:
        out = np.zeros((M + 8, ld_out), np.uint8)
        _lib.check(load().asr_probe_gemm_fp8_v2(M, N, K, a8.ctypes.data, lda or K, w8.ctypes.data, ldw or K, _ptr(sc, _fp), a_scale, _ptr(b, _fp), None, 0, act,
                                                out_inv_scale, out.ctypes.data, ld_out, None, 0, C.byref(sat)))
    else:
        r = _f32(add)
        out = np.zeros((M + 8, ld_out), np.float32)
        _lib.check(load().asr_probe_gemm_fp8_v2(M, N, K, a8.ctypes.data, lda or K, w8.ctypes.data, ldw or K, _ptr(sc, _fp), a_scale, _ptr(b, _fp), _ptr(r, _fp),
                                                ld_add or N, act, out_inv_scale, None, 0, _ptr(out, _fp), ld_out, C.byref(sat)))
    return out, int(sat.value)


def e4m3_table():
    """The 256 OCP e4m3 values (index = byte; 0x7f / 0xff are NaN)."""
    t = np.zeros(256, np.float64)
    for v in range(256):
        s, e, m = v >> 7, (v >> 3) & 15, v & 7
        x = (m / 8.0) * 2.0 ** -6 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7)
        if e == 15 and m == 7:
            x = np.nan
        t[v] = -x if s else x
    return t


def gemm_fp8(a8, w8, w_scale, bias, a_scale=1.0, add=None, act=0, iters=0):
    """FP8 matrix-pipe GEMM on host arrays: a8 [M][K], w8 [N][K] uint8 (e4m3). Returns (out, us): out uint8 [M][N] (bytes of act(...)) without `add`,
    else float32 [M][N]."""
    a8, w8 = np.ascontiguousarray(a8, np.uint8), np.ascontiguousarray(w8, np.uint8)
    M, K = a8.shape
    N = w8.shape[0]
    sc, b = _f32(w_scale), _f32(bias)
    us = C.c_float(0.0)
    if add is None:
        out = np.zeros((M, N), np.uint8)
        _lib.check(load().asr_probe_gemm_fp8(M, N, K, a8.ctypes.data, w8.ctypes.data, sc.ctypes.data_as(_fp), a_scale, b.ctypes.data_as(_fp), None, act,
                                             out.ctypes.data, None, iters, C.byref(us)))
    else:
        r = _f32(add)
        out = np.zeros((M, N), np.float32)
        _lib.check(load().asr_probe_gemm_fp8(M, N, K, a8.ctypes.data, w8.ctypes.data, sc.ctypes.data_as(_fp), a_scale, b.ctypes.data_as(_fp), r.ctypes.data_as(_fp), act,
                                             None, out.ctypes.data_as(_fp), iters, C.byref(us)))
    return out, us.value


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _ptr(a, typ):
    return a.ctypes.data_as(typ)


def whisper_align_scores(q, k_slab, row_off, n_lfr, sel, scores, position, p0, n=1, bf16=False):
    """launch_align_scores on host arrays: q [B n][H 64], k_slab [H][rows][64], sel [(head, slot)], scores [B][n_pairs][max_rows][ld] (returned updated)."""
    q, k = _f32(q), _f32(k_slab)
    ro, nl, sl = _i32(row_off), _i32(n_lfr), _i32(sel).reshape(-1, 2)
    out = _f32(scores).copy()
    B, P, R, ld = out.shape
    d = WhisperAlignDesc(op=0, bf16=int(bf16), B=B, H=k.shape[0], n=n, n_pairs=P, max_rows=R, ld=ld, q=_ptr(q, _fp), k_slab=_ptr(k, _fp), slab_rows=k.shape[1],
                         row_off=_ptr(ro, _ip), n_lfr=_ptr(nl, _ip), sel=_ptr(sl, _ip), n_sel=sl.shape[0], position=int(position), p0=int(p0), scores=_ptr(out, _fp))
    assert q.shape == (B * n, k.shape[0] * 64) and k.shape[2] == 64 and ro.size == nl.size == B
    _lib.check(load().asr_probe_whisper_align(C.byref(d)))
    return out


def whisper_align_op(op, n_rows, n_frames, scores=None, stats=None, cost=None, width=7):
    """One of the four alignment launches on host arrays. op "softmax" -> scores; "colstats" -> stats [B][n_pairs][2][ld]; "cost" (scores, stats, width) -> cost
    [B][max_rows][ld] (`cost` given: what the kernel leaves alone comes back unchanged); "dtw" (cost) -> (frames [B][max_rows], paths: per utterance [(row, frame)]
    in path order)."""
    code = {"softmax": 1, "colstats": 2, "cost": 3, "dtw": 4}[op]
    nr, nf = _i32(n_rows), _i32(n_frames)
    d = WhisperAlignDesc(op=code, n_rows=_ptr(nr, _ip), n_frames=_ptr(nf, _ip), width=int(width))
    if code <= 3:
        sc = _f32(scores).copy()
        B, P, R, ld = sc.shape
        d.scores = _ptr(sc, _fp)
    else:
        co = _f32(cost).copy()
        (B, R, ld), P = co.shape, 1
    d.B, d.n_pairs, d.max_rows, d.ld = B, P, R, ld
    assert nr.size == nf.size == B
    if code == 1:
        _lib.check(load().asr_probe_whisper_align(C.byref(d)))
        return sc
    if code == 2:
        st = np.full((B, P, 2, ld), np.nan, np.float32)
        d.stats = _ptr(st, _fp)
        _lib.check(load().asr_probe_whisper_align(C.byref(d)))
        return st
    if code == 3:
        st = _f32(stats)
        co = np.full((B, R, ld), np.nan, np.float32) if cost is None else _f32(cost).copy()
        d.stats, d.cost = _ptr(st, _fp), _ptr(co, _fp)
        _lib.check(load().asr_probe_whisper_align(C.byref(d)))
        return co
    frames = np.full((B, R), -1, np.int32)
    stride = R + ld
    path = np.full((B, stride, 2), -1, np.int32)
    plen = np.zeros(B, np.int32)
    d.cost, d.frames, d.path, d.path_stride, d.path_len = _ptr(co, _fp), _ptr(frames, _ip), _ptr(path, _ip), stride, _ptr(plen, _ip)
    _lib.check(load().asr_probe_whisper_align(C.byref(d)))
    return frames, [path[b, :plen[b]][::-1].copy() for b in range(B)]
