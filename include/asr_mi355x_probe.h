/* Probe / test hooks of the MI355X ASR engine -- libasr_mi355x_probe.so.
 *
 * NOT part of the product C ABI (include/asr_mi355x.h): nothing here is what the reference's onnxruntime binding for the
 * hot path would call. These entries exist for tests/ (kernel-selection parity at the benchmarked sizes) and tools/
 * (tuning probes); the product library libasr_mi355x.so does not export them. */
#ifndef ASR_MI355X_PROBE_H
#define ASR_MI355X_PROBE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* One bf16 GEMM C[M][N] = A[M][K] W[N][K]^T through the product's dispatcher with the epilogues of the batch-64 SANM path.
 * Operands are rounded to bf16 on upload. Outputs are host arrays; `kernel` receives the kernel family that ran. */
typedef struct asr_probe_gemm_desc {
  int32_t M, N, K;
  const float* a;          /* [M][K] */
  const float* w;          /* [N][K] */
  const float* bias;       /* [N] or NULL */
  const float* add;        /* [M][N] f32 additive term or NULL */
  int32_t act;             /* 0 none, 1 relu, 2 gelu(erf), 3 gelu(tanh) */
  int32_t ln;              /* 1: C = LayerNorm_noaffine(bf16(A)) W^T + bias evaluated inside the GEMM (row statistics + column sums) */
  float ln_eps;
  int32_t argmax;          /* 1: fused row arg-max over n < n_valid -> out_ids[M] (no matrix output) */
  int32_t n_valid;
  int32_t variant;         /* -1 heuristic; pins a kernel (csrc/gemm.hip): 1..4 pipe, 5 / 6 t144, 7 big, 8 pp, 136 pp with one workgroup per tile */
  float* out_lo;           /* [M][N] bf16 results widened to f32, or NULL */
  float* out_f32;          /* [M][N] f32 results, or NULL */
  float* out_stats;        /* [M][N/32][2] (sum, sum of squares) of the bf16 outputs per 32-column group, or NULL */
  int32_t* out_ids;        /* [M] when argmax */
  char kernel[32];         /* out: "t288w", "t288w_amax", "t144w", "t144", "big", "pp", "pp_amax", "pipe", "pipe_splitk", "skinny", "skinny_ln",
                            * "skinny_w8", "skinny_w4"; precision 1: "f32", "f32_splitk" */
  /* ---- every GemmArgs term at op level. The behaviour above: all zero except m_dev = -1 and with_ws = 1. */
  int32_t precision;       /* 0: operands rounded to bf16, launch_gemm_bf16; 1: operands kept, launch_gemm_f32 (out_lo / out_t / rms_out elements are then f32) */
  const float* add2;       /* [add2_table_rows][N] f32 term added AFTER the activation, or NULL */
  int32_t add2_table_rows; /* rows of the add2 table (>= M without add2_rows) */
  const int32_t* add2_rows;/* [M] row of the table per output row (any order, repeats allowed), or NULL: row m */
  float a_rms_eps;         /* > 0: RMSNorm of the A rows folded into the product (weight-streaming kernel) */
  int32_t m_dev;           /* >= 0: uploaded as the device-side row count beside the launch bound M (0 is a row count); < 0: none */
  int32_t lo_group;        /* > 0: out_lo is [N / lo_group][round_up(M, 128)][lo_group], returned as laid out (unwritten rows hold NaN) */
  float* out_t;            /* [N][M] transposed result in the operand dtype, or NULL; stored with pitch ld_out_t */
  int32_t ld_out_t;        /* 0: round_up(M, 4) + pad_out; else >= M, a multiple of 4 */
  float* out_rms;          /* [M][N] second output of the split-K reduce (RMS-normalised rows), or NULL; needs gemm_reduce_can_norm */
  float rms_eps;
  int32_t pad_a, pad_w;    /* extra elements per row of A / W (16-byte multiples); the gap holds NaN */
  int32_t pad_out;         /* extra elements per row of every output, of add and of add2 (a multiple of 8) */
  int32_t with_ws;         /* 0: launch without sk_ws / sk_cnt (the paths the dispatcher takes for callers without a workspace) */
  /* out: 32-bit (f32 / index) or 16-bit (bf16) words of the output buffers outside valid rows x valid columns that no longer hold the NaN pattern they
   * were filled with. Buffers reach round_up(M, 128) rows plus the pitch gap; valid rows are m < min(M, m_dev). */
  int32_t stray;
} asr_probe_gemm_desc;
int asr_probe_gemm(asr_probe_gemm_desc* d);
/* The CTC head with frame log-probabilities through the same dispatcher: operands as asr_probe_gemm with `argmax` (bias required), the arg-max epilogue also
 * writes the per-slab sum of exponentials and the row reduce merges the three partials. out_ids[M]: first index of the row maximum over n < n_valid (0 = N);
 * out_logprob[M]: log soft-max of the row at that index. `variant` as above. *stray (nullable): words of the padded rows >= M that the launches wrote.
 * kernel32 (nullable, 32 bytes): the GEMM kernel family that ran. */
int asr_probe_ctc_head(int M, int N, int K, const float* a, const float* w, const float* bias, int n_valid, int variant, int32_t* out_ids,
                       float* out_logprob, int32_t* stray, char* kernel32);

/* The candidate kernel of the CTC prefix beam search behind the same head: per row the topk (1..16) best columns n < n_valid and their log soft-max,
 * recomputed from the topk slabs with the largest maxima. precision: ASR_PRECISION_BF16 (operands rounded to bf16, `variant` as above) or ASR_PRECISION_F32
 * (the f32 GEMM, variant ignored). out_ids / out_logprob [M][topk], higher value first, lower id on ties. */
int asr_probe_ctc_topk(int M, int N, int K, const float* a, const float* w, const float* bias, int n_valid, int variant, int precision, int topk,
                       int32_t* out_ids, float* out_logprob, char* kernel32);

/* The emission kernel of asr_sensevoice_align behind the same head: operands, `variant` and `precision` as asr_probe_ctc_topk. row_utt [M] names every row's
 * transcript (0 .. n_utts - 1, or -1: the row is left alone); transcript u = target_ids[target_offsets[u] .. target_offsets[u + 1]), ids < n_valid.
 * out_em [M][ld_em]: slot 0 the log soft-max at blank_id, slot j at the transcript's target j - 1, slots past its length -inf (ld_em > the longest transcript).
 * *stray: words written to rows at or past M. */
int asr_probe_ctc_target_logprob(int M, int N, int K, const float* a, const float* w, const float* bias, int n_valid, int variant, int precision,
                                 const int32_t* row_utt, int n_utts, const int32_t* target_ids, const int32_t* target_offsets, int blank_id, int ld_em,
                                 float* out_em, int32_t* stray, char* kernel32);

/* Decode-shaped GEMM (M <= 64 rows) as a captured chain of dependent launches over `cold_mb` megabytes of weight copies (larger than
 * the Infinity Cache => every launch streams its weights from HBM, like a decoder stack does once per token): microseconds per launch.
 * epilogue: 0 bias -> bf16, 1 bias + GELU -> bf16, 2 bias + residual -> f32, 3 LayerNorm prologue (f32 rows in) -> bf16. */
int asr_probe_gemm_chain(int M, int N, int K, int epilogue, int cold_mb, int replays, float* us_per_launch);
const char* asr_probe_last_kernel(void);      /* kernel family of the last asr_probe_gemm_chain */

/* FP8 mode (ASR_PRECISION_FP8W). Row quantiser: w_bf16[N][K] -> e4m3 bytes out8[N][K], power-of-two scale[N], optional exact bf16
 * dequantisation dq_bf16[N][K]. Decode GEMM on host arrays: out[M][N] f32 = a[M][K] (bf16, M <= 64) x either w_bf16 or (w8, scale);
 * fold != 0 applies the folded LayerNorm (column sums from w_bf16: pass the dequantised copy next to byte weights). */
int asr_probe_quantize_fp8(const uint16_t* w_bf16, int N, int K, uint8_t* out8, float* scale, uint16_t* dq_bf16);
/* MXFP4 mode: block quantiser (out4 [N][K / 2] nibbles, scale8 [N][K / 32] e8m0 bytes, dq the exact bf16 dequantisation) and the decode GEMM over them */
int asr_probe_quantize_mxfp4(const uint16_t* w_bf16, int N, int K, uint8_t* out4, uint8_t* scale8, uint16_t* dq_bf16);
/* the two row quantisers over w_bf16 [N][ld], ld >= K a multiple of 8: K columns of every row are read, the gap is the caller's */
int asr_probe_quantize_fp8_ld(const uint16_t* w_bf16, int ld, int N, int K, uint8_t* out8, float* scale, uint16_t* dq_bf16);
int asr_probe_quantize_mxfp4_ld(const uint16_t* w_bf16, int ld, int N, int K, uint8_t* out4, uint8_t* scale8, uint16_t* dq_bf16);
int asr_probe_decode_gemm_mxfp4(int M, int N, int K, const uint16_t* a, const uint8_t* w4, const uint8_t* scale8, const uint16_t* w_dq, const float* bias,
                                int fold, float* out);
int asr_probe_decode_gemm(int M, int N, int K, const uint16_t* a, const uint16_t* w_bf16, const uint8_t* w8, const float* scale,
                          const float* bias, int fold, float* out);

/* FP8 matrix-pipe GEMM (precision mode ASR_PRECISION_FP8MM) on host arrays: out = act((a8 w8^T) a_scale w_scale[n] + bias) as e4m3 bytes (out8), or
 * (a8 w8^T) a_scale w_scale[n] + bias + add as f32 (out_f32). iters > 0 also times the launch (microseconds in *us). */
int asr_probe_gemm_fp8(int M, int N, int K, const uint8_t* a8, const uint8_t* w8, const float* w_scale, float a_scale, const float* bias,
                       const float* add, int act, uint8_t* out8, float* out_f32, int iters, float* us);

/* The decode GEMM (csrc/decode_gemm.hip) with every DecGemmArgs term on host arrays. A holds exactly M rows followed by NaN rows, the pitch gaps of A, W and
 * add hold NaN, both outputs are NaN-filled buffers of 64 + 16 rows, the split-K partials hold NaN and the tickets 0 before the first launch.
 * force_*: 0 = what decode_gemm_plan says; a forced plan that breaks the plan's admissibility rules (N % (16 nt), one finishing wave per tile, K / 32 >= 2 splits,
 * the workspace size, row blocks only without a split and above 16 planned rows) is refused. */
typedef struct asr_probe_dec_gemm_args {
  int32_t M, N, K, plan_M;
  int32_t lda, ldw, ld_add, ld_out_f32, ld_out_lo;   /* elements; 0 = the extent (K / K / N / N / N) */
  int32_t wkind;           /* 0 bf16 weights, 1 e4m3 bytes + one f32 scale per output column, 2 e2m1 nibbles + one e8m0 byte per (column, 32 k) */
  const uint16_t* a;       /* [M][K] bf16 bits */
  const uint16_t* w_bf16;  /* [N][K] bf16 bits: the weights (wkind 0) or their dequantised copy (the column sums of the fold come from it) */
  const uint8_t* wq;       /* wkind 1: [N][K] bytes; wkind 2: [N][K / 2], element 2 i in the low nibble of byte i */
  const float* w_scale;    /* wkind 1: [N] */
  const uint8_t* w_scale8; /* wkind 2: [N][K / 32] */
  const float* bias;       /* [N] or NULL */
  int32_t fold;            /* 1: the affine-free LayerNorm of the rows of A folded in (colsum) */
  float ln_eps;
  const float* add;        /* [M][N] or NULL */
  int32_t act;             /* 0 none, 1 relu, 2 gelu(erf), 3 gelu(tanh) */
  float* out_f32;          /* [M][N] or NULL */
  float* out_lo;           /* [M][N] bf16 results widened to f32, or NULL */
  int32_t with_ws;         /* 0: ws == cnt == NULL */
  int32_t repeats;         /* >= 1 launches into the same buffers, workspace and tickets */
  int32_t force_nt, force_splits, force_row_blocks;
  int32_t pre_M, pre_splits; /* pre_M > 0: first a launch of pre_M rows (row i = row i % M) with pre_splits splits on the same workspace, into scratch outputs */
  /* out */
  int32_t mt, nt, splits, row_blocks;  /* the instance <mt, nt> and the grid (K splits, row blocks) of the last launch */
  int32_t stray;           /* words of the two output buffers outside M rows x N columns that no longer hold the NaN pattern */
  int32_t tickets_zero;    /* 1: every ticket word reads 0 after the launches */
} asr_probe_dec_gemm_args;
int asr_probe_decode_gemm_desc(asr_probe_dec_gemm_args* d);

/* launch_quantize_crosskv_fp8 (the FP8 cross-K/V cache) on host arrays: slabs [n_slabs][rows][64] bf16 bits, updated in place by dq_in_place; sequence b holds
 * rows [row_off[b], row_off[b] + n_lfr[b]) of every slab (row_off on 16-row boundaries). out8 [n_slabs][rows][64] holds 0xa5 where nothing was written;
 * scale [n_slabs][batch]. */
int asr_probe_quantize_crosskv_fp8(uint16_t* slabs, int n_slabs, int rows, const int32_t* row_off, const int32_t* n_lfr, int batch, int dq_in_place,
                                   uint8_t* out8, float* scale);
/* launch_layernorm_fp8 on host arrays: x [rows][ld_x] -> out [rows + 4][ld_out] e4m3 bytes; every byte of out is 0xa5 before the launch. */
int asr_probe_layernorm_fp8(const float* x, int ld_x, int rows, int D, float eps, float inv_scale, int ld_out, uint8_t* out);
/* asr_probe_gemm_fp8 with a pitch on every operand, out_inv_scale and the saturation count. Either out8 [M + 8][ld_out8] (0xa5 before the launch; *sat_count
 * receives Fp8GemmArgs::sat_count) or out_f32 [M + 8][ld_out_f32] (every byte 0xff before the launch; needs add [M][N], uploaded with pitch ld_add). */
int asr_probe_gemm_fp8_v2(int M, int N, int K, const uint8_t* a8, int lda, const uint8_t* w8, int ldw, const float* w_scale, float a_scale, const float* bias,
                          const float* add, int ld_add, int act, float out_inv_scale, uint8_t* out8, int ld_out8, float* out_f32, int ld_out_f32,
                          uint64_t* sat_count);

/* One Whisper decoder attention call through the product dispatcher (launch_decode_attention<bf16 | f32>, head_dim 64) on host arrays.
 * Operands are rounded to the element type on upload. Sequences [b0, b0 + nb) of a batch of B are launched (nb = 0: B - b0).
 *   self  (cross = 0): q [B n][ld_q] (head h at q_col0 + h 64), kv_new [B n][2 H 64] (k columns, then v), cached rows k_hist / v_hist
 *         [B][H][hist][64]; the cache is a contiguous extent of max_pos positions per (sequence, head), or (paged = 1) pages of 16 positions
 *         (n_pages of them, laid out as whisper.hip's pool: K page of every head, then V) addressed by page_table [B][pages_per_seq].
 *         k_after / v_after [B][H][hist + n][64] receive the cache after the call. hist_dev = 1: the history length travels in device memory.
 *   cross (cross = 1): slabs k_slab / v_slab [H][rows][64], sequence b at rows [row_off[b], row_off[b] + n_lfr[b]); fp8 = 1 (bf16 only):
 *         the slabs go through the product's FP8 quantiser first, whose bytes ([2][H][rows][64], K then V) and scales ([2][H][B]) come back
 *         in kv8 / scale8 when non-null.
 * out [B n][H 64] (rows of sequences outside the launch stay 0); `kernel` receives the form that ran. */
typedef struct asr_probe_decode_attn_desc {
  int32_t bf16;            /* 1 bf16, 0 f32 */
  int32_t cross, B, b0, nb, H, n, causal;
  const float* q; int32_t ld_q, q_col0;
  int32_t max_keys;        /* the launch's max_keys (0: max_pos / pages_per_seq 16 / the longest extent) */
  /* self */
  const float* kv_new;
  const float* k_hist; const float* v_hist;
  int32_t hist, hist_dev, max_pos;
  int32_t paged, n_pages, pages_per_seq;
  const int32_t* page_table;
  float* k_after; float* v_after;
  /* cross */
  const float* k_slab; const float* v_slab;
  int32_t rows;
  const int32_t* row_off; const int32_t* n_lfr;
  int32_t fp8;
  uint8_t* kv8; float* scale8;
  float* out;
  int32_t stray;           /* out (self): cache elements outside positions [0, hist + n) of the batch's (sequence, head) extents that changed */
  char kernel[32];         /* out: "self_wave", "cross_1pass", "cross_1pass_fp8", "general_n1", "general_n8", "general_n1_fp8", "general_n8_fp8" */
} asr_probe_decode_attn_desc;
int asr_probe_decode_attention(asr_probe_decode_attn_desc* d);
/* One beam-search self-attention call ("self_beam": single-token, hypothesis rows with per-row extents and an ancestry table) through the same
 * dispatcher. rows = utterances x beam (utterance-major), all at position hist (hist_dev = 1: read from device memory). ext [rows][2][H][S][64] holds
 * every row's extent (K, then V; slot = position): uploaded (rounded to the element type) before the call and overwritten with the extents after it.
 * Positions below p0 are read from the row's own extent, position p0 <= p < hist from the extent of row src[r][p - p0] (src [rows][ld_src]).
 * q [rows][H 64], kv_new [rows][2 H 64] (k, then v), out [rows][H 64]; stray (nullable) = elements outside slot `hist` that changed;
 * kernel (32 bytes) receives the form that ran. */
int asr_probe_decode_attention_beam(int bf16, int rows, int beam, int H, int S, int p0, int hist, int hist_dev, const int32_t* src, int ld_src,
                                    const float* q, const float* kv_new, float* ext, float* out, int32_t* stray, char* kernel);

/* Left-padded prompts (asr_whisper_prefill_prompts). The descriptor is the one of asr_probe_decode_attention.
 *   asr_probe_decode_attention_ks: the same call with DecAttnArgs::key_start = key_start (host [B], 0 .. hist each; null: the plain entry): single-token
 *         self-attention only; sequence b sees cached keys key_start[b] .. hist - 1 and its new row. `kernel`: "self_wave_ks", "general_n1_ks".
 *   asr_probe_decode_attention_beam_ks: the beam form with key_start [rows / beam] ("self_beam_ks").
 *   asr_probe_prompt_attention: the call goes to launch_prompt_attention (csrc/prompt_attn.hip) instead -- any n up to 1536, the whole batch (b0 = nb = 0),
 *         self: hist = 0 (the cache image starts as NaN everywhere; k_after / v_after [B][H][n][64] and stray as above), query slot i of sequence b sees key
 *         slots key_start[b] .. i and the slots below key_start[b] write zeros; cross: unmasked over the plan, pad slots write zeros.
 *         `kernel`: "prompt_self" / "prompt_cross". */
int asr_probe_decode_attention_ks(asr_probe_decode_attn_desc* d, const int32_t* key_start);
int asr_probe_decode_attention_beam_ks(int bf16, int rows, int beam, int H, int S, int p0, int hist, int hist_dev, const int32_t* src, int ld_src,
                                       const float* q, const float* kv_new, float* ext, float* out, int32_t* stray, char* kernel, const int32_t* key_start);
int asr_probe_prompt_attention(asr_probe_decode_attn_desc* d, const int32_t* key_start);

/* The attention stage of one Qwen3 decoder layer through the session's launcher (launch_qwen_attention, csrc/qwen_attn.h; head_dim 128) on host arrays:
 * per-head RMSNorm of q and k, RoPE, cache write, causal GQA attention. Which kernels run follows from bf16 / step / no_fuse / H / KV exactly as in a session:
 * "fused_g1|2|4" (a step), "beam_g1|2|4" (a step with beam > 0), "rope_mfma" (bf16 prefill), "rope_scalar" (f32, no_fuse). Cache operands are rounded to
 * the element type on upload; qkv, qn, kn and rope are f32 as in a session.
 *   rows / plan : qkv [rows][(H + 2 KV) 128] (q heads, k heads, v heads); sequence b has T[b] new positions at rows row_off[b] .. (a multiple of 16 unless
 *                 step; step: T = 1, row_off = b, rows = B), appended at position hist[b]; row_seq / row_t [rows] name each row's sequence (-1: gap row) and t.
 *   cache       : extents [seq][KV][S_max][128], or (paged = 1) pages of 16 positions [page][2 layers][KV][16][128] addressed by table [seq][pps] -- the call
 *                 works on the second layer, so the page stride is not the layer size. k_hist / v_hist [seq][KV][hist_ld][128] supply positions below hist[b];
 *                 every other slot is NaN before the call. k_after / v_after [B][KV][after_ld][128] receive positions below hist[b] + T[b] after it.
 *   beam > 0    : the B rows are hypotheses, `beam` per utterance; the cache above is the utterances' prompt cache (seq = B / beam, positions below p0[b]);
 *                 ext_k / ext_v [B][KV][S_hyp][128] are the rows' extents (slot j = position p0 + j), uploaded as given and overwritten with their state after
 *                 the call; generated position p0[b] + j of row b is read from row src[b][j] (src [B][ld_src]).
 * q_out [rows][H 128] (nullable) and k_rows_out [rows][KV 128] (nullable; the MFMA form's key copy) come back NaN where nothing was written; ctx [rows][H 128].
 * stray: cache and extent elements outside positions [hist[b], hist[b] + T[b]) (beam: outside slot hist[b] - p0[b] of row b) whose bits changed.
 * qt / nw: the MFMA form's query-block geometry (0 when it was not set up). */
typedef struct asr_probe_qwen_attn_desc {
  int32_t bf16, step, no_fuse;
  int32_t B, H, KV, rows;
  const float* qkv; const float* qn; const float* kn; const float* rope;
  int32_t rope_rows; float eps;
  const int32_t* hist; const int32_t* T; const int32_t* row_off; const int32_t* row_seq; const int32_t* row_t;
  int32_t S_max;           /* the session's max_seq_len */
  int32_t paged, n_pages, pps;
  const int32_t* table;
  int32_t hist_ld; const float* k_hist; const float* v_hist;
  int32_t after_ld; float* k_after; float* v_after;
  int32_t beam, ld_src, S_hyp;
  const int32_t* src; const int32_t* p0;
  float* ext_k; float* ext_v;
  float* q_out; float* k_rows_out; float* ctx;
  int32_t stray, qt, nw;
  char kernel[32];
} asr_probe_qwen_attn_desc;
int asr_probe_qwen_attention(asr_probe_qwen_attn_desc* d);

/* The ragged encoder attention (launch_attention_bf16_hd128 / _hd64 / launch_attention_f32, csrc/kernels.hip) in every form a session launches, on host
 * arrays laid out as a session lays them out: utterance b's rows start at the sum of the earlier lengths rounded up to 16, V is stored transposed with
 * the packed row count as its leading dimension, and the query blocks hold 16 qt waves rows from attention_geometry(longest utterance) (f32: 64).
 *   q [sum Tq][n_heads hd], k / v [sum T][(n_heads / kv_group) hd], ctx [sum Tq][n_heads hd] (dense, utterance after utterance; rounded to bf16 on upload).
 *   key_lens [batch]; q_lens null: the self form; else the cross form (q_plan, ld_q != ld_qk) with q_lens[b] <= key_lens[b]: the query blocks are laid over
 *   the key rows, as the Paraformer decoder's are.   causal, kv_group: bf16 only.   packed_qk: q and k share one buffer of 2 n_heads hd columns, k at column
 *   n_heads hd, as the Qwen3 audio encoder launches it (self form, kv_group 1).
 *   slack_rows: rows allocated behind the last utterance's 16-row boundary (0 or a multiple of 8): n_rows_alloc == ld_vt == sum of the rounded lengths + slack.
 *   pad_fill_k / pad_fill_v: FINITE values in every K (and Q) row / every V^T column that belongs to no key -- rows T .. roundup16(T) of every utterance and
 *   the slack -- and in the guard bytes in front of and behind every buffer (ctx: pad_fill_v), so that a stray read is a wrong number and not a fault.
 * Out: hd, chunk, qt, waves: the bf16 instance that ran (grid_z 0); f32: hd, waves 4, grid_z = the gridDim.z chosen (chunk, qt 0). n_qblocks. stray: context
 * elements outside the query rows, guards included, whose bits changed. */
typedef struct asr_probe_enc_attn_desc {
  int32_t bf16, head_dim, n_heads, kv_group, causal, batch;
  const int32_t* key_lens; const int32_t* q_lens;
  int32_t packed_qk, slack_rows;
  float pad_fill_k, pad_fill_v;
  const float* q; const float* k; const float* v;
  float* ctx;
  int32_t hd, chunk, qt, waves, grid_z, n_qblocks, stray;
} asr_probe_enc_attn_desc;
int asr_probe_encoder_attention(asr_probe_enc_attn_desc* d);

/* launch_fsmn (11 taps) on v [sum T][channels] as a session lays it out (V^T [channels][round_up(rows, 128)], rows rounded up to 16 per utterance), every
 * element of V^T that belongs to no utterance row and the guards around both buffers = pad_fill (finite). w [channels][11], b [channels],
 * out [sum T][channels] (f32). stray: guard elements whose bits changed + output elements of pad rows that are not zero. */
typedef struct asr_probe_fsmn_desc {
  int32_t bf16, batch, channels;
  const int32_t* lens;
  float pad_fill;
  const float* v; const float* w; const float* b;
  float* out;
  int32_t stray;
} asr_probe_fsmn_desc;
int asr_probe_fsmn(asr_probe_fsmn_desc* d);

/* One pass of the beam-search ranking (launch_beam_select, shared by the Qwen3-ASR and Whisper searches) on host arrays. Hypotheses of utterance b
 * are rows b * beam + r. topv / topi: the rows' K best (log-prob, id) pairs, [rows][K] ([n_utt][K] when first = 1); cum / fin / len / next [rows] and
 * done [n_utt] are the search state, updated in place; stop [n_stop]; src_in / tok_in [rows][ld] the tables the pass reads, src_out / tok_out [rows][ld]
 * the tables it writes (uploaded as given, so entries the pass leaves alone come back unchanged). n_slots: generated cache slots after the pass. */
typedef struct asr_probe_beam_select_desc {
  int32_t n_utt, beam, K, ld, first, n_slots, n_stop;
  const float* topv; const int32_t* topi;
  float* cum; int32_t* fin; int32_t* len; int32_t* next; int32_t* done;
  const int32_t* stop;
  const int32_t* src_in; const int32_t* tok_in;
  int32_t* src_out; int32_t* tok_out;
} asr_probe_beam_select_desc;
int asr_probe_beam_select(asr_probe_beam_select_desc* d);

/* One call of a token-selection head through its product launcher on host arrays. op: 0 launch_argmax_rows, 1 launch_beam_topk, 2 launch_apply_penalty,
 * 3 launch_append_ids, 4 launch_sample_topk_topp, 5 launch_no_speech_prob, 7 launch_timestamp_rules, 8 / 9 the token-score kernels; 6 "head steps", below. Rows keep their real leading dimension (ld, a multiple of 128, >= n_valid): the
 * caller fills the pad columns, so a kernel that reads them shows. n_saved is put in device memory, as the sessions keep it; the logits, the whole save_ids
 * table and the counter come back as they stand after the call (penalty and sampler work in place). Fields an op does not use are ignored.
 * op 6 drives a TokenHead (csrc/decode_head.h) as a session does: configured from value / range / partial / ld_save / track_history (+ the sampler fields when
 * sampling != 0), restarted, then `steps` times enqueue + consumed on a fresh copy of the same logits rows -- step 0 with `vec` as the bias and without the
 * penalty (a prefill), later steps without bias and with it (decode steps). `noise`, when set, is armed before step 0. Before step change_step (> 0) the penalty
 * is set to value2 / range2. With timestamps != 0 the head runs in Whisper's timestamp mode (ts_begin / no_timestamps_id / eot_id / max_initial). Out: picks
 * [steps][rows], save_ids (the final history table), n_saved_after (the counter); logits are not written back.
 * ops 8 / 9 are the token-score kernels: 8 launch_argmax_logprob_rows (-> out_i [rows], uploaded as given), 9 launch_logprob_at_rows (ids = next_in [rows], any
 * value); both write column n_saved of `logprob` [rows][ld_save] (the counter in device memory; n_saved >= ld_save writes nothing). op 6 with scores != 0 runs
 * the head in scores mode and returns its score history in `logprob` (columns no step wrote are NaN); steps may then exceed ld_save when value == 1 and no
 * change is scheduled (the overflow is dropped).
 * op 7 masks the logits in place by the history save_ids [rows][ld_save] and its length: n_saved for every row (one shared device counter), or n_saved_rows
 * [rows] when set (per-row counters, as the beam ranker keeps them). Every entry of the table must be a valid id. */
typedef struct asr_probe_token_head_desc {
  int32_t op, rows, n_valid, ld;
  float* logits;             /* [rows][ld], in / out (ops 0 1 2 4 5) */
  const float* vec;          /* [ld]: extra (0, 4), bias (1), nullable; penalty (5) */
  int32_t K;                 /* beam_topk: pairs per row; sampler: top_k */
  int32_t ld_save, n_saved;  /* history table geometry and the device counter's value (2 3 4) */
  int32_t n_saved_after;     /* out: the device counter after the call */
  int32_t* save_ids;         /* [rows][ld_save], in / out (2 3 4) */
  int32_t range, partial;    /* apply_penalty */
  float value;
  const int32_t* next_in;    /* [rows] append_ids */
  float temperature, top_p, repetition_penalty;   /* sampler */
  const float* noise;        /* [rows][K] uniforms, or NULL: the counter-based generator keyed by seed */
  uint64_t seed;
  int32_t no_speech_id;
  float* out_v;              /* topv [rows][K] (1), prob [rows] (5) */
  int32_t* out_i;            /* ids [rows] (0), topi [rows][K] (1), next [rows] (4) */
  int32_t steps, track_history, sampling, change_step, range2;   /* head steps (6) */
  float value2;
  int32_t* picks;            /* out [steps][rows] (6) */
  int32_t timestamps;        /* head steps (6): timestamp mode on */
  int32_t ts_begin, no_timestamps_id, eot_id, max_initial;   /* timestamp rules (6 7) */
  const int32_t* n_saved_rows;   /* [rows] per-row history lengths, or NULL: n_saved for all (7) */
  int32_t scores;            /* head steps (6): token scores on */
  float* logprob;            /* the score history [rows][ld_save]: in / out (8 9: uploaded as given, so what the kernel leaves alone comes back unchanged), out (6) */
  int32_t timed;             /* head steps (6), plain arg-max head only: upload the rows once, run the steps' launches back to back between two device events */
  float head_ms;             /* out (6, timed): the device time between the two events */
} asr_probe_token_head_desc;
int asr_probe_token_head(asr_probe_token_head_desc* d);

/* Hotword boosting of the autoregressive decoders (csrc/hotword.hip, launchers in csrc/kernels.h). The phrases -- ids / offsets [n_phrases + 1], as
 * asr_whisper_set_hotwords takes them -- are turned into the product's trie image (nodes breadth first, children by token: tests/ctc_beam_ref.py numbers
 * them the same way); every id must lie in [0, n_valid).
 * asr_probe_hotword, one kernel on host arrays. node [rows] in (each inside the trie), n_saved the device counter's value (0: every row counts as at the root).
 *   op 0 launch_hotword_bias: logits [rows][ld] in / out; root_save (nullable) [rows][n_root], n_root = the root's child count, uploaded as given and read back.
 *   op 1 launch_hotword_advance: next_in [rows] (any value) -> node out.
 *   op 2 launch_beam_topk (with lse_out) + launch_hotword_rerank: logits, vec (bias, nullable), K -> topv / topi [rows][K], lse [rows] (nullable). */
typedef struct asr_probe_hotword_desc {
  int32_t op, rows, n_valid, ld;
  float* logits; const float* vec;
  const int32_t* ids; const int32_t* offsets; int32_t n_phrases; float boost;
  int32_t* node; int32_t n_saved;
  const int32_t* next_in;
  float* root_save; int32_t n_root;
  int32_t K; float* topv; int32_t* topi; float* lse;
} asr_probe_hotword_desc;
int asr_probe_hotword(asr_probe_hotword_desc* d);

/* "Hotword head steps": a TokenHead (csrc/decode_head.h) driven as a session drives it -- configured (penalty value / range / partial, the sampler fields when
 * sampling != 0, Whisper's timestamp mode when timestamps != 0, token scores when scores != 0, then set_hotwords; n_phrases == 0: the mode stays off),
 * reserved, restarted, then `steps` times enqueue + consumed, step i on rows logits[i] ([steps][rows][ld], a different row per step) -- step 0 with `vec` as
 * the bias and without the penalty (a prefill), later steps without bias and with it. noise (nullable) [steps][rows][K]: armed before every step. Out: picks
 * [steps][rows], save_ids [rows][ld_save] (the final history), n_saved_after, nodes [steps][rows] (the node table after every step; untouched with the
 * mode off), logprob [rows][ld_save] with scores (NaN where no step wrote), logits_out (nullable) [steps][rows][ld]: every step's rows after the head ran.
 * timed (arg-max head only): logits holds ONE step's rows [rows][ld], uploaded once and reused by all `steps` steps (the bias accumulates: a timing, not a
 * result); the steps' launches run back to back between two device events (head_ms); nodes / logits_out are not written. */
typedef struct asr_probe_hotword_head_desc {
  int32_t rows, n_valid, ld, steps;
  const float* logits; const float* vec;
  int32_t ld_save, range, partial; float value;
  int32_t sampling, K; float temperature, top_p, repetition_penalty; uint64_t seed; const float* noise;
  int32_t timestamps, ts_begin, no_timestamps_id, eot_id, max_initial;
  int32_t scores;
  const int32_t* ids; const int32_t* offsets; int32_t n_phrases; float boost;
  int32_t* picks; int32_t* save_ids; int32_t n_saved_after; int32_t* nodes; float* logprob; float* logits_out;
  int32_t timed; float head_ms;
} asr_probe_hotword_head_desc;
int asr_probe_hotword_head_steps(asr_probe_hotword_head_desc* d);

/* One ranking pass of the beam search with hotwords on, as BeamRanker runs it: launch_beam_topk (K = beam, lse_out) on logits ([rows][ld]; [n_utt][ld] and
 * `vec` as the bias when first != 0), launch_hotword_rerank, launch_beam_select with the node hand-over. The search state and the tables are those of
 * asr_probe_beam_select (tab_ld their row stride); node_in [rows] the rows' nodes before the pass, node_out [rows] uploaded as given and read back. topv / topi
 * come back as the re-rank left them. iters > 0: afterwards launch_beam_topk alone (ms_topk) and launch_beam_topk with lse_out + the re-rank (ms_rerank)
 * are timed, `iters` launches each back to back between two device events. */
typedef struct asr_probe_hotword_rank_desc {
  int32_t n_utt, beam, tab_ld, first, n_slots, n_stop, n_valid, ld;
  const float* logits; const float* vec;
  const int32_t* ids; const int32_t* offsets; int32_t n_phrases; float boost;
  float* cum; int32_t* fin; int32_t* len; int32_t* next; int32_t* done;
  const int32_t* stop;
  const int32_t* src_in; const int32_t* tok_in; int32_t* src_out; int32_t* tok_out;
  const int32_t* node_in; int32_t* node_out;
  float* topv; int32_t* topi;
  int32_t iters; float ms_topk, ms_rerank;
} asr_probe_hotword_rank_desc;
int asr_probe_hotword_rank(asr_probe_hotword_rank_desc* d);

/* n-gram LM fusion of the autoregressive decoders (csrc/decoder_lm.hip, launchers in csrc/kernels.h). The model of every hook: an image as
 * asr_whisper_set_lm takes it (checked against n_valid as the vocabulary), the weights, the candidate width topk (1..32) and the end ids. */
typedef struct asr_probe_lm_model {
  const int32_t* image; int64_t n_words;
  float alpha, beta, oov_logprob;
  int32_t topk;
  const int32_t* end_ids; int32_t n_end;
} asr_probe_lm_model;
/* launch_lm_topk on host arrays: logits [rows][ld], vec (bias, nullable) -> cand_v / cand_i [rows][M], lse [rows], slow_rows = the rows that took the
 * strict-order passes. iters > 0: afterwards launch_lm_topk (ms_lm_topk) and launch_beam_topk at K = min(M, 8) with lse_out (ms_beam_topk) are timed, `iters`
 * launches each back to back between two device events. */
typedef struct asr_probe_lm_topk_desc {
  int32_t rows, n_valid, ld, M;
  const float* logits; const float* vec;
  float* cand_v; int32_t* cand_i; float* lse;
  int32_t slow_rows;
  int32_t iters; float ms_lm_topk, ms_beam_topk;
} asr_probe_lm_topk_desc;
int asr_probe_lm_topk(asr_probe_lm_topk_desc* d);
/* launch_lm_pick on host arrays: candidates cand_v / cand_i [rows][topk] and lse [rows] as launch_lm_topk leaves them (ids inside the image's vocabulary),
 * state [rows] in / out, n_saved the device counter's value (0: every row counts as at start_node) -> next [rows], logprob (nullable) [rows][ld_save]. */
typedef struct asr_probe_lm_pick_desc {
  int32_t rows, n_saved, ld_save;
  const float* cand_v; const int32_t* cand_i; const float* lse;
  int32_t* state; int32_t* next; float* logprob;
} asr_probe_lm_pick_desc;
int asr_probe_lm_pick(const asr_probe_lm_model* m, asr_probe_lm_pick_desc* d);
/* asr_probe_hotword_head_steps with the model set on the head after the hotwords (TokenHead::set_lm); states [steps][rows]: the state table after every
 * step. n_phrases == 0 leaves the hotwords off. */
int asr_probe_lm_head_steps(const asr_probe_lm_model* m, asr_probe_hotword_head_desc* d, int32_t* states);
/* asr_probe_hotword_rank with the model on, as BeamRanker runs it: launch_lm_topk (M = topk), launch_lm_rerank, launch_beam_select with the node and the
 * state hand-over. n_phrases == 0: no trie (node_in / node_out are not used). state_in [rows] the rows' states before the pass (not read when first != 0),
 * state_out [rows] uploaded as given and read back. iters > 0: ms_topk times the pass without a model (launch_beam_topk at K = beam, + lse_out and
 * launch_hotword_rerank with a trie), ms_rerank launch_lm_topk + launch_lm_rerank. */
int asr_probe_lm_rank(const asr_probe_lm_model* m, asr_probe_hotword_rank_desc* d, const int32_t* state_in, int32_t* state_out);

/* One kernel of the Whisper token-timestamp path (csrc/whisper_align.hip, launchers in csrc/kernels.h) on host arrays. Every extent a kernel follows is checked
 * here first. op:
 *   0 launch_align_scores: q [B n][H 64] and the K slabs k_slab [H][slab_rows][64] (rounded to bf16 on upload when bf16 != 0), sequence b at slab rows
 *     [row_off[b], row_off[b] + n_lfr[b]); sel [n_sel][2] = (head, slot); the row written is position + n - 1 - p0 (position travels in device memory);
 *   1 launch_align_softmax, 2 launch_align_colstats (-> stats [B][n_pairs][2][ld]: mean, 1 / std), 3 launch_align_cost (reads scores and stats, width =
 *     medfilt width -> cost [B][max_rows][ld]), 4 launch_align_dtw (reads cost -> frames [B][max_rows], path [B][path_stride][2] from the end backwards, path_len [B]).
 * scores [B][n_pairs][max_rows][ld] is uploaded as given and read back after ops 0 and 1; cost likewise after op 3 (what a kernel leaves alone comes back unchanged). */
typedef struct asr_probe_whisper_align_desc {
  int32_t op, bf16;
  int32_t B, H, n, n_pairs, max_rows, ld;
  /* op 0 */
  const float* q; const float* k_slab;
  int32_t slab_rows;
  const int32_t* row_off; const int32_t* n_lfr;
  const int32_t* sel; int32_t n_sel;
  int32_t position, p0;
  /* ops 1-4 */
  const int32_t* n_rows; const int32_t* n_frames;
  int32_t width;
  float* scores; float* stats; float* cost;
  int32_t* frames; int32_t* path; int32_t path_stride; int32_t* path_len;
} asr_probe_whisper_align_desc;
int asr_probe_whisper_align(asr_probe_whisper_align_desc* d);

/* launches per GEMM kernel family since the last reset, as "family=count;..." (host-side counters: hipGraph replays do not
 * count, so reset, run a session once on a new batch geometry, read). reset != 0 clears the counters after the read. */
int asr_probe_gemm_counts(int reset, char* buf, int cap);

/* device bytes held, process-wide, by the sessions' workspaces (DeviceBuffer) and the weight arenas they copied in: back at its
 * earlier value once every session created since has been destroyed */
int asr_probe_live_device_bytes(int64_t* bytes);

/* Tuning hook: time `iters` launches of the bf16 GEMM on device-resident pseudo-random operands.
 * variant: -1 heuristic, 0..7 kernel variants (csrc/gemm.hip). epilogue: 0 bias->lo, 1 bias+relu->lo,
 * 2 bias+residual->f32, 3 two residual terms->f32, 4 transposed store, 5 LayerNorm-folded FFN-1, 6 producer epilogue. */
int asr_probe_gemm_bench(int variant, int M, int N, int K, int epilogue, int iters, float* avg_ms);
/* microseconds per grid-wide barrier of a cooperative launch with n_workgroups x 512 threads (single counter + __threadfence) */
int asr_probe_grid_barrier(int n_workgroups, int iters, float* us_per_barrier);
/* hierarchical barrier (per-XCD arrival counters, relaxed agent-scope atomics, no fence): mode 1 = one release flag, 2 = one flag
 * per XCD; also checks that an sc1 payload written before a barrier is visible after it. mode + 16 * KiB makes every workgroup
 * also read KiB kibibytes of one shared buffer per round through sc1 loads (+ 8: through plain cached loads). */
int asr_probe_grid_barrier2(int n_workgroups, int iters, int mode, float* us_per_barrier);

#ifdef __cplusplus
}
#endif
#endif /* ASR_MI355X_PROBE_H */
