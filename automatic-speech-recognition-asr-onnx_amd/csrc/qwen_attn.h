// The attention stage of one Qwen3 decoder layer (csrc/qwen.hip): everything between the q|k|v GEMM and the o_proj GEMM. QwSession::decoder_pass
// calls it once per layer; the probe library calls it on host arrays (asr_probe_qwen_attention), so the kernels are tested through the session's own
// selection rule and launch geometry.
#pragma once
#include "engine.h"
#include "kernels.h"

// Where position s of (sequence b, kv head) lives. Two layouts of a layer's cache:
//   extents (table == nullptr): [seq][kv head][S_max][128] -- beam-search hypothesis rows, the persistent decode kernel, ASR_QWEN_KV_PAGED=0;
//   pages (the default): 16 positions per page behind a block table [seq][pps] of page ids, one pool for all layers laid out page-major
//   [page][layer][kv head][16][128] (`base` carries the layer's offset, page_stride the elements between consecutive pages), so a sequence holds
//   pages for the positions it has, not for max_seq_len, and a finished sequence's pages go back to the free list (host: QwSession::kv_*).
struct KvAddr { const int32_t* table; int pps; size_t page_stride; int S_max; };

// One layer's attention over `rows` packed rows of `B` sequences (T new positions per sequence, appended at hist[b]). Element type T of the session
// (float or bf16_t) types q, kc, vc, ctx, k_rows, vt, kc_p, vc_p.
struct QwAttnArgs {
  bool bf16 = false, step = false, no_fuse = false;      // bf16 session; single-position step (rows == B); ASR_QWEN_NO_FUSE
  const float* qkv = nullptr;                             // [rows][(H + 2 KV) 128]: q heads, k heads, v heads
  int rows = 0, B = 0, H = 0, KV = 0;
  const float *qn = nullptr, *kn = nullptr, *rope = nullptr; float eps = 0.0f;     // folded per-head norm weights [128], rope table [position][cos 64 | sin 64]
  const int32_t *hist = nullptr, *row_seq = nullptr, *row_t = nullptr;            // positions already cached [B]; per row: sequence (< 0: gap row) and t
  const UttPlan* plan = nullptr;                          // per sequence: T, row_off
  void *q = nullptr, *kc = nullptr, *vc = nullptr, *ctx = nullptr;               // operand rows [rows][H 128], this layer's cache, context rows [rows][H 128]
  KvAddr ka{nullptr, 0, 0, 0};
  int S = 0;                                              // cache positions per sequence: bounds the scalar prefill's score buffer
  // bf16 prefill through the MFMA kernel (n_qb > 0): row-major copy of the new keys, V^T [KV 128][ld_vt], query-block tables and geometry
  void* k_rows = nullptr; const void* vt = nullptr; int ld_vt = 0;
  const int32_t *qb_utt = nullptr, *qb_q0 = nullptr; int n_qb = 0, qt = 0, nw = 0, max_T = 0;
  // beam search: rows are hypotheses, kc / vc their extents (ka.S_max slots), the prompt is read from the utterances' prefill cache kc_p / vc_p (kap)
  const int32_t *beam_src = nullptr, *beam_p0 = nullptr; int ld_src = 0, beam = 1;
  const void *kc_p = nullptr, *vc_p = nullptr; KvAddr kap{nullptr, 0, 0, 0};
};

enum QwAttnForm { QW_ATTN_FUSED_DECODE, QW_ATTN_FUSED_BEAM, QW_ATTN_ROPE_MFMA, QW_ATTN_ROPE_SCALAR };
// the form launch_qwen_attention will take for these arguments (the MFMA form needs a.vt filled before the launch)
QwAttnForm qwen_attention_form(const QwAttnArgs& a);
// launches the stage on stream s (prof: the session's profiler) and returns the form that ran: "fused_g1" / "fused_g2" / "fused_g4", "beam_g1" / "beam_g2" /
// "beam_g4", "rope_mfma", "rope_scalar"
template <typename T>
const char* launch_qwen_attention(const QwAttnArgs& a, Profiler& prof, hipStream_t s);
