// Non-GEMM kernels of the ASR hot path (gfx950).
#pragma once
#include <vector>

#include "common.h"
#include "ngram_lm.h"

// Per-utterance geometry, built on the host for every run and uploaded with one copy.
struct UttPlan {
  int64_t audio_off;   // first sample in the packed audio buffer (a sample index whatever the sample type)
  int32_t n_samples;
  int32_t n_frames;    // fbank / STFT frames
  int32_t frame_off;   // first row in the packed mel buffer
  int32_t n_lfr;       // low-frame-rate rows (SenseVoice/Paraformer) or encoder positions (Whisper)
  int32_t T;           // encoder sequence length (n_lfr + prompts)
  int32_t row_off;     // first row in the packed activation matrices (multiple of 16)
  int32_t lang;        // language selector index
  int32_t blk0;        // first front-end workgroup of this utterance
};

// ---- Kaldi fbank: frames -> |DFT|^2 -> mel -> ln  (SenseVoice/Export_SenseVoice.py:139-160,275-278)
// dft_packed / mel_packed are MFMA-fragment-ordered constant tables built by arena.py.
enum { AUDIO_F32 = 0, AUDIO_I16 = 1, AUDIO_F16 = 2 };           // asr_audio_dtype of the C ABI
inline size_t audio_elt_bytes(int audio_dtype) { return audio_dtype == AUDIO_F32 ? 4 : 2; }
struct FbankArgs {
  const void* audio;           // packed samples of type audio_dtype
  const UttPlan* plan;
  const int32_t* blk_utt;      // per workgroup: utterance
  const int32_t* blk_f0;       // per workgroup: first frame (multiple of 64)
  const float* dft_packed;     // [n_bin_tiles][2][n_kchunks][64 lanes][4]
  const float* mel_packed;     // [n_mel_tiles][n_bin_tiles][64 lanes][4]
  float* mel_out;              // [total_frames][n_mels]
  int n_bin_tiles;             // ceil((nfft/2+1)/16)
  int n_kchunks;               // win_length / 16
  int n_mel_tiles;             // n_mels / 16
  int n_mels;
  int win, hop;
  float log_floor;             // FLT_EPSILON (Kaldi) / 1e-10 (Whisper)
  // Whisper variant (Whisper/STFT_Process.py:224-246): reflect pad nfft/2 left, nfft/2 - hop right (last frame dropped),
  // log10 instead of ln, and the per-workgroup maximum written to blk_max for the per-utterance clamp
  int whisper;
  int dbg = 0;                 // ASR_FBANK_DBG (fbank_split_kernel, timing-only ablations; results are garbage by design): 1 no DFT steps, 2 no mel projection, 4 no audio loads, 8 no basis refills
  float* blk_max;
  // bf16 sessions: the DFT on the bf16 matrix pipe with split operands (launch_fbank_split_table): null = exact-f32 MFMA
  const void* dft_split = nullptr;
  // log10 / ln of log_floor, rounded once from double on the host: a bin at the floor (digital silence) gets exactly the value the reference's CPU
  // graph gives (-10 for Whisper), not the device logarithm's last-bit approximation of it
  float log_at_floor = 0.0f;
  // sample type of `audio`: the kernels are instantiated per type and launch_fbank dispatches (kept last: the kernels never read it, and the
  // offsets of the fields they do read stay what they were)
  int audio_dtype = AUDIO_F32;
};
void launch_fbank(const FbankArgs& a, int n_blocks, hipStream_t s);
// three-term bf16 split (hi + mid + lo = the f32 value to 2^-24) of the packed DFT basis, as 16x16x32 fragments:
// out[(bin tile * 2 + re/im) * ceil(win / 32) + k chunk][term][lane] x 16 bytes; rows k >= win are zero
size_t fbank_split_table_bytes(int n_bin_tiles, int win);
void launch_fbank_split_table(const float* dft_packed, int n_bin_tiles, int n_kchunks16, void* out, hipStream_t s);

// ---- resampler (resample.hip): packed frames of any rate and channel count -> model-rate mono f32, in front of the fbank launch.
// A polyphase Kaiser-windowed sinc (beta 9, 32 zero crossings a side, cutoff 0.945 of the narrower Nyquist). With g = gcd(rate_in, rate_model), L = rate_model / g,
// M = rate_in / g, fc = 0.945 min(1, L / M), W = ceil(32 / fc), T = 2 W + 1:   c[p][k] = fc sinc(t) I0(9 sqrt(1 - (t / 32)^2)) / I0(9),  t = ((k - W) - p / L) fc
// (0 at |t| >= 32), and output n of an utterance of n_in frames (n_out = ceil(n_in L / M)) is   sum_k c[(n M) mod L][k] x[floor(n M / L) - W + k]   with x zero
// outside the utterance and, for C interleaved channels, x[i] = (x[i][0] + ... + x[i][C - 1]) (1 / C) in f32 after Pcm<S>::widen. rate_in == rate_model is the pure
// down-mix L = M = T = 1, W = 0.
struct ResampleDesign {
  int L, M, W, T;
  int tile;                    // outputs per workgroup (1024, 512 or 256: the largest whose input span fits the LDS budget)
  int span_max;                // LDS floats of a tile: ((L - 1) + (tile - 1) M) / L + T
};
// INVALID (with a message) for a rate < 1, L > 1024, or a ratio whose smallest tile does not fit in LDS (rate_in beyond ~40 x rate_model)
ResampleDesign resample_design(int rate_in, int rate_model);
void resample_table(const ResampleDesign& d, float* coeffs);                        // [L][T], computed in double and rounded once
inline int64_t resample_n_out(int64_t n_in, const ResampleDesign& d) { return (n_in * d.L + d.M - 1) / d.M; }
struct RsUtt {
  int64_t in_off;              // first input frame in the packed buffer (a frame = `channels` interleaved samples)
  int64_t out_off;             // first output sample in the packed f32 buffer
  int32_t n_in, n_out;
};
struct ResampleArgs {
  const void* audio;           // packed interleaved samples of type audio_dtype
  const RsUtt* utt;
  const int32_t* tile_utt;     // per workgroup: utterance
  const int32_t* tile_n0;      // per workgroup: first output sample (multiple of d.tile)
  const float* tab_t;          // the coefficients TRANSPOSED, [T][L]: at tap k the lanes of a wave read one row of L floats, whatever their phases
  float* out;
  ResampleDesign d;
  int channels;
  float scale;                 // int16 only: 2^-15 where the front end behind is the Whisper / Qwen one (Pcm<int16_t>::widen), else 1
  int audio_dtype = AUDIO_F32;
};
void launch_resample(const ResampleArgs& a, int n_tiles, hipStream_t s);

// ---- the streaming form (asr_mi355x.h "streaming input format"): step c of a stream (c = 0, 1, .. since its reset) produces outputs
// [c S, (c + 1) S) of the signal above, S = chunk. hi(c) = floor(((c + 1) S - 1) M / L) + W is the last input frame they read; the step consumes the stream's
// frames [A(c), A(c + 1)), A(0) = 0, A(c) = hi(c - 1) + 1, and reaches back at most 2 W frames before A(c). Host and device use these definitions.
__host__ __device__ inline int64_t resample_stream_hi(const ResampleDesign& d, int chunk, int64_t c) { return ((c + 1) * chunk - 1) * d.M / d.L + d.W; }
__host__ __device__ inline int64_t resample_stream_start(const ResampleDesign& d, int chunk, int64_t c) { return c <= 0 ? 0 : resample_stream_hi(d, chunk, c - 1) + 1; }
__host__ __device__ inline int resample_stream_need(const ResampleDesign& d, int chunk, int64_t c) {
  return (int)(resample_stream_hi(d, chunk, c) + 1 - resample_stream_start(d, chunk, c));
}
// Frames a stream carries from step to step. A(c) - (floor(c S M / L) - W), the reach of step c's first output, is 2 W when outputs c S - 1 and c S have different
// centre frames -- always when M >= L -- and 2 W + 1 when they share one, which up-sampling allows (8 kHz with an odd chunk). The pure down-mix carries nothing.
__host__ __device__ inline int resample_stream_keep(const ResampleDesign& d) { return d.M < d.L ? 2 * d.W + 1 : 2 * d.W; }
inline int resample_stream_pitch(const ResampleDesign& d, int chunk) {        // frames per row of a step's audio: need(0), or a later step's largest count
  const int64_t later = (int64_t)chunk * d.M / d.L + 1, first = resample_stream_need(d, chunk, 0);
  return (int)(first > later ? first : later);
}
// Slot i of a launch is stream sid[i * sid_stride]; its geometry comes from count[stream] on the device, so the launch arguments depend on n only. Two launches:
// the tiles (offline geometry: at most d.tile outputs and d.span_max frames of span per workgroup, the span staged from the stream's carried frames and the
// slot's row), then one workgroup per slot that writes the last 2 W frames of (carried | row[0, need)) into the OTHER half of hist and advances the count.
struct ResampleStreamArgs {
  const void* audio;           // [n][pitch][channels] samples of audio_dtype; slot i reads the first need(c_i) frames of row i
  const int32_t* sid;          // slot -> stream, at a stride of sid_stride words (the lang field of the step's UttPlan array, or a plain list)
  int sid_stride;
  int32_t* count;              // [streams] steps since the stream's reset
  float* hist;                 // [2][streams][2 W] mono f32 (widened and averaged as the kernel stages them): step c reads half c & 1
  int streams;
  const float* tab_t;          // [T][L]
  float* out;                  // [n][chunk]
  int32_t* need_out;           // nullable [n]: the frames each slot's step read
  ResampleDesign d;
  int chunk, pitch, channels;
  float scale;
  int audio_dtype = AUDIO_F32;
};
void launch_resample_stream(const ResampleStreamArgs& a, int n, hipStream_t s);

// ---- energy VAD (vad.hip): packed frames of any rate and channel count -> speech segments, per utterance of a ragged batch (the statement: asr_mi355x.h).
// Stage 1 (one launch, a tile list over (utterance, first analysis frame)): e[f] = sum of x^2 over the H input frames of analysis frame f, its level q[f], and the
// utterance's 1024-bin level histogram. Stage 2 (one launch, one workgroup per utterance, the mask as bits in LDS): floor / peak / thr, the mask, the three run rules,
// the cuts of long runs; its segments land in the utterance's own range of seg_tmp and vad_pack_kernel (one launch) packs the batch's in order.
constexpr int VAD_TILE_F = 256;              // analysis frames per stage-1 workgroup
constexpr int VAD_MAX_F = 1 << 20;           // analysis frames per utterance: the mask is 128 KiB of LDS
constexpr int VAD_LEVELS = 1024;
struct VadUtt {
  int64_t in_off;              // first input frame in the packed buffer, from the buffer's start
  int64_t abs_off;             // the caller's offset of that frame (what segments are reported in)
  int64_t f_off;               // first analysis frame in the packed e[] / q[] (and first slot in seg_tmp)
  int32_t n, F;                // input frames, analysis frames = ceil(n / H)
  int32_t need;                // ceil(p_floor F): the cumulative count the floor level reaches
  int32_t pad_;
};
struct VadRules { int32_t margin, peak_drop, abs_level, min_speech, min_pause, pad, max_frames; };
struct VadArgs {
  const void* audio;           // packed interleaved samples of type audio_dtype
  const VadUtt* utt;
  const int32_t* tile_utt;     // per stage-1 workgroup: utterance
  const int32_t* tile_f0;      // per stage-1 workgroup: first analysis frame (multiple of VAD_TILE_F)
  float* energy;               // [sum F]
  int32_t* level;              // [sum F]
  int32_t* hist;               // [batch][VAD_LEVELS], zero before stage 1
  int32_t* seg_tmp;            // [sum F][2]: utterance u's segments in analysis frames, from slot f_off
  int32_t* seg_count;          // [batch]
  int32_t* stats;              // [batch][3] floor, peak, thr
  int64_t* seg_out;            // [seg_cap][2]
  int32_t* seg_utt;            // [seg_cap]
  int64_t seg_cap;
  VadRules r;
  int H, channels, batch, max_F;
  int audio_dtype = AUDIO_F32;
};
inline int vad_hop(int rate) { const int h = (rate + 50) / 100; return h < 1 ? 1 : h; }
// (bits(max(e, 2^-40)) >> 20) - (bits(2^-40) >> 20), at most 1023: host and device use this one definition
__host__ __device__ inline int vad_level(float e) {
  const float m = e > 0x1p-40f ? e : 0x1p-40f;         // (a NaN takes the floor)
  const int q = (int)(__builtin_bit_cast(uint32_t, m) >> 20) - (int)((87u << 23) >> 20);
  return q > 1023 ? 1023 : q;
}
void launch_vad(const VadArgs& a, int n_tiles, hipStream_t s);      // the memset of hist, stage 1, stage 2, the pack: four nodes on s, no host work between

// ---- Whisper log-mel finish (Export_Whisper.py:425-427): max(x, utterance_max - 8), (x + 4) / 4, written in the
// GAPPED time-major layout the conv stem reads: utterance b owns rows [2*row_off_b, 2*row_off_b + 2*rows_b); row
// 2*row_off_b is the conv's left zero pad, frame f sits at row 2*row_off_b + 1 + f, everything else is zero.
template <typename T>
void launch_whisper_mel_finish(const float* mel, const float* blk_max, const UttPlan* plan, const int32_t* grow_utt,
                               int n_gapped_rows, int n_mels, T* out, hipStream_t s);
// zero the rows of a gapped-layout matrix that are not frames (conv zero padding after conv1)
// dst row m (row space of `to`, utterance row_utt[m]) = src row of the same (utterance, position) in the row space of `from`; pad rows zero
void launch_compact_rows(const float* src, const UttPlan* from, const UttPlan* to, const int32_t* row_utt, int rows, int d, float* dst, hipStream_t s);
template <typename T>
void launch_zero_gap_rows(T* buf, int ld, int n_cols, const UttPlan* plan, const int32_t* grow_utt, int n_gapped_rows,
                          hipStream_t s);

// affine-free LayerNorm of f32 rows written as OCP e4m3 bytes of y * inv_scale (saturating): operand rows of the FP8 matrix-pipe GEMM (csrc/gemm_fp8.hip)
void launch_layernorm_fp8(const float* x, int ld_x, int rows, int D, float eps, float inv_scale, unsigned char* out, int ld_out, hipStream_t s);

// ---- decoder token + position embedding: x[b*n + i] = embed[ids[b*n + i]] + pos[hist + i]   (Export_Whisper.py:450-497)
// kstart (nullable, device [sequences]): left-padded prompts -- slot hist + i of sequence b = row / kstart_rows (0: n) is position hist + i - kstart[b]; a
// pad slot (below kstart[b]) takes position 0 and the id staged for it, so it reads inside both tables (its row is never attended by a real one).
template <typename T>
void launch_embed_pos(const int32_t* ids, int rows, int n, int hist, const int32_t* hist_dev, const T* embed, const float* pos, int d,
                      float* x, hipStream_t s, const int32_t* kstart = nullptr, int kstart_rows = 0);
void launch_add_scalar(int32_t* p, int v, hipStream_t s);      // *p += v (device-side history counter)

// ---- decoder attention, head_dim 64, n <= 8 new queries per sequence. Keys/values are rows of 64:
//   self : cache [b][h][S_max][64]; the n new rows are appended from `kv_new` (fused qkv GEMM output) and attended
//          with the reference's additive -128 causal mask (Export_Whisper.py:468-480,640-647)
//   cross: per-(layer, head) slabs [row][64] written by the encoder's cross-KV GEMM; no mask (:654-660)
struct DecAttnArgs {
  const void* q; int ld_q; int q_col0;
  const void* kv_new; int ld_new; int k_col0, v_col0;          // null for cross
  void* k_base; void* v_base;
  int64_t stride_b, stride_h;                                  // element strides of (b, h) inside k_base / v_base
  const UttPlan* plan;                                         // cross: row_off / n_lfr per sequence; null for self
  int hist, n, n_heads, causal;
  int max_keys = 0;                                            // upper bound of keys per sequence (sizes the LDS score buffer)
  int sc_ld = 0;                                               // (set by the launcher)
  const int32_t* hist_dev;                                     // when set, the history length is read from device memory (graph replay)
  void* out; int ld_out;
  const float* k_scale = nullptr; const float* v_scale = nullptr;   // FP8 cross-K/V: k_base / v_base hold e4m3 bytes, scale[head][sequence] per slab
  // paged self-KV cache (block table; stride_b / stride_h unused): position s of (sequence b, head h) lives at
  //   k_base + page_table[b * pages_per_seq + (s >> 4)] * page_stride + h * 1024 + (s & 15) * 64       (pages of 16 positions x 64 dims per head)
  const int32_t* page_table = nullptr; int pages_per_seq = 0; int64_t page_stride = 0;
  // a launch over the sub-batch [b0, b0 + grid.x) of the session's batch (the decode chains of whisper.hip): every per-sequence index is b0 + blockIdx.x;
  // scale_ld = sequences per head row of k_scale / v_scale (0: the launch's own grid.x)
  int b0 = 0, scale_ld = 0;
  // beam search ("self_beam": single-token self-attention of hypothesis rows, `batch` = rows = utterances x beam, utterance-major): row r's cache is an
  // extent k_base + r * stride_b + h * stride_h (slot = position); positions below beam_p0 (the prompt, copied into every row) are read from the row's own
  // extent, position p >= beam_p0 from the extent of row beam_src[r * ld_src + p - beam_p0] (its ancestry). The new row goes to the row's own slot `hist`.
  const int32_t* beam_src = nullptr; int ld_src = 0, beam_p0 = 0, beam = 1;
  // left-padded prompts (asr_whisper_prefill_prompts): single-token self-attention ("self_wave", "general_n1", "self_beam") of sequence b sees cached keys
  // key_start[b] .. hist - 1 only (the beam form reads key_start[row / beam]); the slots below are never loaded. Null: every key, and the kernels are
  // the instances they were before the field existed.
  const int32_t* key_start = nullptr;
};

// ---- prompt attention, head_dim 64, any number n of query rows per sequence (prefills of more than 8 ids or of ragged lengths; csrc/prompt_attn.hip).
// One workgroup per (sequence, head, tile of query rows: 16 for f32, 64 for bf16); keys go through LDS in blocks of 64 under an online soft-max (exp2 on
// pre-scaled scores).
//   self : q / k / v are rows b * n + slot of the fused q|k|v GEMM output; query slot i of sequence b sees key slots key_start[b] .. i. Later keys are
//          SKIPPED (the reference adds -128 to them, Export_Whisper.py:468-480: exp(-128) of an f32 soft-max at |score| << 100 is below half an ulp of
//          the sum, so the two are indistinguishable). All n K / V rows are written to the cache (contiguous or paged, as decode_attn_kernel does);
//          a query row without a visible key (a pad slot) writes zeros.
//   cross: keys / values are the per-(layer, head) slabs [row][64] through the plan (row_off, n_lfr), unmasked; pad slots write zeros too.
// bf16: QK^T and PV on v_mfma_f32_16x16x32_bf16, probabilities rounded to bf16 for PV; f32: f32 FMAs (the arithmetic class of decode_attn_kernel<float>).
struct PromptAttnArgs {
  const void* q = nullptr; int ld_q = 0, q_col0 = 0;
  const void* kv_new = nullptr; int ld_new = 0, k_col0 = 0, v_col0 = 0;      // self: the n new rows per sequence; null for cross
  void* k_base = nullptr; void* v_base = nullptr;                            // self: the cache to fill; cross: the slabs
  int64_t stride_b = 0, stride_h = 0;
  const int32_t* page_table = nullptr; int pages_per_seq = 0; int64_t page_stride = 0;
  const UttPlan* plan = nullptr;                                             // cross
  const int32_t* key_start = nullptr;                                        // [batch] pad slots per sequence (null: 0)
  int n = 0, n_heads = 0;
  void* out = nullptr; int ld_out = 0;
};
template <typename T>
void launch_prompt_attention(const PromptAttnArgs& a, int batch, hipStream_t s);
// FP8 (OCP e4m3, power-of-two scales) quantisers of precision mode ASR_PRECISION_FP8W
void launch_quantize_rows_fp8(const bf16_t* W, int ld, int N, int K, unsigned char* W8, float* scale, bf16_t* Wdq, hipStream_t s);
// MXFP4 (e2m1 + one e8m0 scale per 32 k): W4 [N][K / 2] bytes, S [N][K / 32] bytes, Wdq (nullable) the exact bf16 dequantisation
void launch_quantize_rows_mxfp4(const bf16_t* W, int ld, int N, int K, unsigned char* W4, unsigned char* S, bf16_t* Wdq, hipStream_t s);
void launch_quantize_crosskv_fp8(bf16_t* slabs, size_t slab_elems, int n_slabs, const UttPlan* plan, int batch, unsigned char* out8, float* scale,
                                 int dq_in_place, hipStream_t s);
template <typename T>
void launch_decode_attention(const DecAttnArgs& a, int batch, hipStream_t s);
const char* decode_attn_last_kernel();   // form of this thread's last launch_decode_attention ("self_wave", "self_beam", "cross_1pass[_fp8]", "general_n1[_fp8]", "general_n8[_fp8]", each self form + "_ks" with key_start): test hook

// The hotword context graph as the device sees it: node 0 is the root; children of node n are child_tok / child_node [child_off[n], child_off[n + 1]), sorted
// by token. n_nodes <= 1: no hotwords (no pointer is read).
struct HotTrie {
  const int32_t *depth = nullptr, *is_end = nullptr, *child_off = nullptr, *child_tok = nullptr, *child_node = nullptr;
  int n_nodes = 0;
  float boost = 0.0f;
};

// ---- n-gram LM fusion of the autoregressive decoders (decoder_lm.hip; the float64 statement is tests/decoder_lm_ref.py). Every row carries a
// state of the NgramLm image. The LM term of token c from state s: c one of `ends` and the image lists </s> -> alpha * lm_step(s, </s>), the state stays;
// else (lp, s') = lm_step(s, c) and the term is __fadd_rn(__fmul_rn(alpha, lp), beta).
// (ngram_lm.h: lm_token_term, LmEnds)
constexpr int LM_TOPK_MAX = 32;
//   launch_lm_topk: per row the M <= LM_TOPK_MAX best (value, id) pairs of v[n] = logits[r][n] + (bias ? bias[n] : 0) over n < n_valid, value descending
//     then id ascending, and the row's log-sum-exp as launch_beam_topk forms it. cand_v / cand_i [rows][M]: raw values (not log-probabilities); a -inf
//     column is no candidate, ranks past the last candidate are (-inf, 0); lse [rows] (-inf for a row without a finite column). Exact for every layout
//     of the row: one pass in launch_beam_topk's geometry with per-thread best-8 lists, and a row where some thread dropped a value that is not
//     strictly below the M-th winner is redone by M strict-order passes. slow_rows (nullable, device): incremented once per row that took those.
//   launch_lm_pick: the greedy pick among a row's candidates by (value + LM term, then id ascending): next[r], and the pick's state into state[r]. The
//     row's state reads as lm.start_node while *n_saved == 0. logprob (nullable) [rows][ld_save]: value - lse of the pick at column *n_saved (dropped at
//     or past ld_save); a row without a candidate picks id 0, keeps its state and scores -inf. One wave per row, one candidate per lane.
//   launch_lm_rerank: the beam ranker's merge with the LM on. The K best of topM u S by ((value - lse) + delta) + LM term, then id ascending, go to
//     topv / topi [rows][K]; S and delta are launch_hotword_rerank's (a trie with n_nodes <= 1: S is empty, delta 0, node is not read). Row r's state is
//     state[r * stride], or lm.start_node when state is null (the first ranking). Ranks past the last candidate are (-inf, 0).
void launch_lm_topk(const float* logits, int ld, int rows, int n_valid, const float* bias, int M, float* cand_v, int32_t* cand_i, float* lse, hipStream_t s,
                    int32_t* slow_rows = nullptr);
void launch_lm_pick(const float* cand_v, const int32_t* cand_i, const float* lse, int rows, int M, const NgramLm& lm, const LmEnds& ends, int32_t* state,
                    const int32_t* n_saved, int32_t* next, float* logprob, int ld_save, hipStream_t s);
void launch_lm_rerank(const float* logits, int ld, int rows, int n_valid, const float* bias, const float* cand_v, const int32_t* cand_i, const float* lse, int M,
                      const HotTrie& trie, const int32_t* node, const NgramLm& lm, const LmEnds& ends, const int32_t* state, int stride, int K, float* topv,
                      int32_t* topi, hipStream_t s);

// ---- beam search ranking (Qwen3-ASR and Whisper; semantics of oracle/qwen_asr_oracle.py:beam_search_core). Hypotheses of utterance b are rows b * beam + r.
constexpr int BEAM_MAX = 8;
// per row: log-soft-max over the first n_valid columns of logits (+ bias[col] when bias is set: Whisper's BEGIN_SUPPRESS on the first ranking) and the
// K best (log-prob, id) pairs, ties -> lower id: topv / topi [rows][K]
// lse_out (nullable) [rows]: the log-sum-exp each row's topv was formed with (the hotword re-rank scores further columns against the very same value)
void launch_beam_topk(const float* logits, int ld, int rows, int n_valid, const float* bias, int K, float* topv, int32_t* topi, hipStream_t s,
                      float* lse_out = nullptr);
struct BeamArgs {
  int beam, K, ld, first, n_slots;       // ld: row stride of the ancestry / token tables; n_slots: generated cache slots after this pass
  const float* topv; const int32_t* topi;
  float* cum; int32_t* fin; int32_t* len; int32_t* next; int32_t* done;
  const int32_t* stop; int n_stop;
  const int32_t *src_in, *tok_in; int32_t *src_out, *tok_out;
  const int32_t* slots_dev = nullptr;    // when set, n_slots = *slots_dev + slots_off (a device counter: the pass replays from a captured graph)
  int slots_off = 0;
  // hotwords (null: none): node_in / node_out [rows] the rows' trie nodes before / after the pass -- a kept row inherits its parent's node advanced by its
  // token (trie_step); a finished hypothesis and the rows of a finished utterance keep theirs. first: every parent is at the root, node_in is not read.
  const int32_t* node_in = nullptr; int32_t* node_out = nullptr;
  HotTrie trie;
  // language model (state_out null: none): state_in / state_out [rows] the rows' LM states before / after the pass, handed over as the nodes are -- a kept
  // row inherits its parent's state advanced by its token (lm_token_term), a finished hypothesis and the rows of a finished utterance keep theirs.
  // first: every parent is at lm.start_node, state_in is not read.
  NgramLm lm;
  const int32_t* state_in = nullptr; int32_t* state_out = nullptr;
  LmEnds ends;
};
// one wave per utterance: rank the <= beam * K extensions (finished hypotheses stand as themselves), keep the best `beam` in order (score
// descending, then hypothesis, then rank inside the hypothesis), rebuild the rows' ancestry / token tables from their parents'; done[b] = best has ended
void launch_beam_select(const BeamArgs& a, int n_utt, hipStream_t s);

// ids[r] = first arg-max over n < n_valid of logits[r][n] + (extra ? extra[n] : 0)
void launch_argmax_rows(const float* logits, int ld, int rows, int n_valid, const float* extra, int32_t* ids, hipStream_t s);
// ---- token scores (the build's own mode, after OpenAI Whisper's `logprobs`; the reference reports none). The score of a pick is the natural-log soft-max at
// the picked id of v[n] = logits[r][n] + (extra ? extra[n] : 0) over n < n_valid -- the f32 row as the selection sees it, temperature / top-k / top-p not
// part of it. Rows hold finite values and -inf (a mask); +inf or NaN in a row is outside the contract (exp(inf - inf)), as it is for every soft-max here.
// A -inf column has zero weight; a row without a column above -inf, or a pick whose own column is -inf, scores -inf (never NaN); the pad columns
// [n_valid, ld) are not read into the sum. One pass over the row in launch_argmax_rows' geometry, (max, sum of exp(v - max)) carried online. The score is
// written to logprob[r * ld_save + *n_saved] (the counter lives on the device: a captured step replays for every position); columns at or past ld_save are
// dropped, as launch_append_ids drops them.
//   launch_argmax_logprob_rows: the greedy pick and its score in one kernel; ids equal launch_argmax_rows' bit for bit, score = -log S.
//   launch_logprob_at_rows: the score of ids[r], picked elsewhere (the sampler); an id outside [0, n_valid) scores -inf.
void launch_argmax_logprob_rows(const float* logits, int ld, int rows, int n_valid, const float* extra, int32_t* ids, float* logprob, int ld_save,
                                const int32_t* n_saved, hipStream_t s);
void launch_logprob_at_rows(const float* logits, int ld, int rows, int n_valid, const float* extra, const int32_t* ids, float* logprob, int ld_save,
                            const int32_t* n_saved, hipStream_t s);
// NO_SPEECH_DETECTION (Export_Whisper.py:334-348): prob[r] = softmax(logits[r] - penalty)[no_speech_id] over the first n_valid columns, where
// `penalty` is the permanent suppress bias the logits carry (-128 on the suppressed ids: subtracting it re-adds the +128 the reference adds back)
void launch_no_speech_prob(const float* logits, int ld, int rows, int n_valid, const float* penalty, int no_speech_id, float* prob, hipStream_t s);

// ---- penalty-greedy head (Export_Whisper.py:312-325 APPLY_PENALTY + :243-251 GREEDY_SEARCH): logits of the last `range` saved
// ids are multiplied by `value` once `range` ids are saved (the host's rule, Inference_Whisper_ONNX.py:630-632); gather first,
// scatter second, so a repeated id is scaled once. In place on the f32 logits. n_saved lives on the device (graph replay).
// partial = 1 (Qwen3-ASR, Export_Qwen_ASR.py:1403-1415): the window is save_id[:, -range:] of whatever exists -- fewer ids are penalised too.
void launch_apply_penalty(float* logits, int ld, int rows, const int32_t* save_ids, int ld_save, const int32_t* n_saved,
                          int range, float value, hipStream_t s, int partial = 0);
// save_ids[r][*n_saved] = next[r] (the counter itself is advanced by launch_add_scalar afterwards)
void launch_append_ids(const int32_t* next, int rows, int32_t* save_ids, int ld_save, const int32_t* n_saved, hipStream_t s);

// ---- hotword boosting of the autoregressive decoders (hotword.hip; the build's own mode, the float64 statement is tests/hotword_heads_ref.py).
// Every row carries a node of the HotTrie; delta(c) is what trie_step would add to the bonus for token c from that node: + boost for a child of the node,
// boost - depth * boost for a root child that is no child of the node, - depth * boost for everything else.
//   launch_hotword_bias: delta + the row constant depth * boost, in place on the f32 logits [rows][ld], before the selection: children of the node get
//     (float)(depth + 1) * boost, root children that are not children of the node get boost, nothing else is touched (a column in both lists is written once;
//     -inf stays -inf). Arg-max, soft-max and log-soft-max do not see a row constant, so the sparse form selects and scores as the dense one would. The node
//     is node[r], or the root while *n_saved == 0 (the step after a restart). root_save (nullable) [rows][child_off[1]]: while *n_saved == 0 the root
//     children's values before the update, in child order (launch_hotword_restore puts them back: the beam ranker's first pass needs the model's own row).
//   launch_hotword_advance: node[r] = trie_step(node[r] or the root while *n_saved == 0, next[r]); the pick need not be a valid column. Run it before the
//     counter moves. O(1) per row: one thread per row. save_ids (nullable) [rows][ld_save]: the pick is also appended to the id history, by
//     launch_append_ids' rule (the head's two per-row writes of a step in one launch; a full table drops the id and the node still moves).
//   launch_hotword_rerank: the beam ranker's merge. topv / topi [rows][K] hold launch_beam_topk's pairs of the UNBIASED row and lse [rows] its lse_out;
//     the K best of topK u S by (log-prob + delta, then id ascending) are written back, S = children of the row's node + children of the root scored as
//     (logits + bias) - lse. A column at -inf is no candidate, a top-K entry that is also in S counts once, ranks past the last candidate are (-inf, 0).
//     Among columns outside S delta is one constant, so nothing outside topK u S can enter. Row r's node is node[r * node_stride].
// All take one wave per row and walk child lists longer than 64 in lane strides. Tokens of the trie must lie in [0, n_valid) (set_hotwords checks; the
// kernels skip the others).
void launch_hotword_bias(float* logits, int ld, int rows, int n_valid, const HotTrie& trie, const int32_t* node, const int32_t* n_saved, float* root_save,
                         hipStream_t s);
void launch_hotword_restore(float* logits, int ld, int rows, int n_valid, const HotTrie& trie, const float* root_save, hipStream_t s);
void launch_hotword_advance(const int32_t* next, int rows, const HotTrie& trie, int32_t* node, const int32_t* n_saved, hipStream_t s,
                            int32_t* save_ids = nullptr, int ld_save = 0);
void launch_hotword_rerank(const float* logits, int ld, int rows, int n_valid, const float* bias, const float* lse, const HotTrie& trie, const int32_t* node,
                           int node_stride, int K, float* topv, int32_t* topi, hipStream_t s);

// ---- Whisper timestamp rules (OpenAI Whisper's ApplyTimestampRules; the reference has no timestamp mode, this one is the build's own). In place on the f32
// logits [rows][ld], before the selection. Columns: [0, eot) text, eot, (eot, ts_begin) specials, [ts_begin, n_valid) timestamps. Row r's history is
// ids[r * ld_ids .. + h), h = n_ids[r * n_ids_stride] (stride 0: one shared counter), both on the device (graph replay). In order:
//   1. no_timestamps_id is masked;
//   2. last_ts = h >= 1 and id[h-1] >= ts_begin, penult_ts = h < 2 or id[h-2] >= ts_begin: after a pair the timestamps are masked, after a lone
//      timestamp [0, eot) is;
//   3. m = the largest id >= ts_begin of the history: [ts_begin, m + 1) is masked -- [ts_begin, m) after a lone timestamp (the next segment may open where the last one closed; every other timestamp is strictly later);
//   4. h == 0: [0, ts_begin) is masked and, with max_initial >= 0, (ts_begin + max_initial, n_valid);
//   5. over what is left, L = log-sum-exp of the timestamp columns, T = max of [0, ts_begin): L > T masks [0, ts_begin) (an empty side is -inf).
// Masked = -inf. The pad columns [n_valid, ld) are not touched.
void launch_timestamp_rules(float* logits, int ld, int rows, int n_valid, const int32_t* ids, int ld_ids, const int32_t* n_ids, int n_ids_stride, int ts_begin,
                            int no_timestamps_id, int eot_id, int max_initial, hipStream_t s);

// ---- Whisper token / word timestamps (csrc/whisper_align.hip): OpenAI Whisper's cross-attention DTW (openai-whisper timing.py; the reference has no
// alignment, like the timestamp rules this is the build's own). Capture: the raw scores q . k (f32 accumulate, no extra scale: the folded projections carry
// it) of the selected heads of ONE decoder layer for one query row per sequence -- row b * n + n - 1 of `q` -- against all n_lfr keys of the sequence's slab,
// written to out[((b * n_pairs + slot) * max_rows + r) * ld + key], r = *pos_dev + row_bias (device-resident position: one captured graph serves every step).
// Rows outside [0, max_rows) are not written. sel [n_sel][2] (device) = (head, slot) of this layer's selected heads. Grid (64-key tile, selected head, sequence).
struct AlignScoresArgs {
  const void* q; int ld_q; int n;                              // the step's cross-q rows [B n][ld_q], head h at column h * 64
  const void* k_base; int64_t stride_h;                        // this layer's K slabs [H][rows][64]
  const UttPlan* plan;                                         // row_off / n_lfr per sequence
  const int32_t* sel; int n_sel;
  const int32_t* pos_dev; int row_bias;
  float* out; int n_pairs, max_rows, ld;
  int max_keys;                                                // upper bound of n_lfr (sizes the grid)
};
template <typename T> void launch_align_scores(const AlignScoresArgs& a, int B, hipStream_t s);
// The four launches of the alignment proper, on the captured scores [B][n_pairs][max_rows][ld]; n_rows / n_frames [B] live on the device, a sequence with
// n_rows = 0 is skipped by every kernel. rows_max / frames_max bound them (grid sizes).
//   1. soft-max, in place, over the first n_frames[b] scores of rows < n_rows[b];
//   2. per (b, pair, frame) mean and 1 / sqrt(population variance) over the n_rows[b] rows (two passes; variance 0 -> 0: the column standardises to 0)
//      -> stats [B][n_pairs][2][ld];
//   3. cost[b][r][j] = -mean over pairs of median over the `width` (odd, <= 9) reflect-padded neighbours of j of the standardised weights
//      (no filter when n_frames <= width / 2) -> cost [B][max_rows][ld];
//   4. DTW, one workgroup per sequence, anti-diagonal wavefront, OpenAI's recurrence and tie rule (diagonal if c0 < c1 && c0 < c2, else vertical if
//      c1 < c0 && c1 < c2, else horizontal), f32 costs; trace [B][trace_stride] bytes ((n_rows + 1) x (n_frames + 1) used); frames_out[b * out_stride + r] =
//      the smallest frame of row r on the path. path_out (nullable, tests) [B][path_stride][2]: the path's (row, frame) cells from the end backwards,
//      path_len [B] their count. rows_max bounds n_rows and sizes the three diagonals (dynamic LDS, 12 (rows_max + 1) bytes).
void launch_align_softmax(float* scores, int B, int n_pairs, int max_rows, int ld, const int32_t* n_rows, const int32_t* n_frames, int rows_max, hipStream_t s);
void launch_align_colstats(const float* scores, int B, int n_pairs, int max_rows, int ld, const int32_t* n_rows, const int32_t* n_frames, int frames_max,
                           float* stats, hipStream_t s);
void launch_align_cost(const float* scores, const float* stats, int B, int n_pairs, int max_rows, int ld, const int32_t* n_rows, const int32_t* n_frames,
                       int rows_max, int frames_max, int width, float* cost, hipStream_t s);
void launch_align_dtw(const float* cost, int B, int max_rows, int ld, const int32_t* n_rows, const int32_t* n_frames, int rows_max, unsigned char* trace, size_t trace_stride,
                      int32_t* frames_out, int out_stride, int32_t* path_out, int path_stride, int32_t* path_len, hipStream_t s);

// ---- TOPK_TOPP_SAMPLING head (Export_Whisper.py:263-308), one workgroup per sequence: repetition penalty on every saved id
// (negative logits multiplied, others divided; gather before scatter), + `extra` bias (BEGIN_SUPPRESS), x 1/temperature, top-k
// (k <= 64, ties to the lower index), soft-max + exclusive-cumsum top-p cut, Gumbel-max with clamped uniforms. The uniforms come
// from `noise` ([rows][top_k], caller-supplied: parity tests) or, when null, from a counter-based generator keyed by
// (seed, step = *n_saved, row, rank). Writes next[r]; the caller appends it to the history.
struct SampleArgs {
  float* logits; int ld; int rows; int n_valid;
  const float* extra;
  const int32_t* save_ids; int ld_save; const int32_t* n_saved;
  float temperature, top_p, repetition_penalty; int top_k;
  const float* noise; uint64_t seed;
  int32_t* next;
};
void launch_sample_topk_topp(const SampleArgs& a, hipStream_t s);

// ---- LFR stacking + CMVN + positions + prompt rows (Export_SenseVoice.py:280-287)
struct LfrArgs {
  const float* mel;            // [frames][n_mels]
  const UttPlan* plan;
  const int32_t* row_utt;      // per packed row: utterance (or -1)
  const float* cmvn_means;     // [feat]
  const float* cmvn_vars;      // [feat]
  const float* speech_pos;     // [max_lfr][feat]
  const float* language_embed; // [n_lang][feat]   (position-folded)
  const float* system_embed;   // [n_prompt-1][feat]
  float* out;                  // [rows][ld_out]
  int ld_out, feat, n_mels, lfr_m, lfr_n, n_prompt, n_rows;
  // affine_mode 1 (Paraformer, Export_Paraformer.py:483): x * cmvn_vars + bias_table[j] (bias_table = speech_pos), no prompts
  int affine_mode = 0;
  bf16_t* out_lo = nullptr;    // optional bf16 copy of `out` (same leading dimension): the operand of the LayerNorm-fused projection
};
void launch_lfr_cmvn(const LfrArgs& a, hipStream_t s);

// ---- LayerNorm over the last dim, one wave per row. gamma/beta may be null (affine folded away).
// Output in operand dtype with zero fill of columns [D, ld_fill).
template <typename OutT>
void launch_layernorm(const float* x, int ld_x, int rows, int D, const float* gamma, const float* beta, float eps,
                      OutT* out, int ld_out, int fill_to, hipStream_t s, const int32_t* rows_dev = nullptr);   // rows_dev: device-side row count
// f32 output (may be `x` itself) plus the bf16 rounding of the same values, from one pass over the rows (the stand-alone LayerNorm between two runs of
// LayerNorm-fused blocks: normed stream + its operand copy). Columns [0, D) only.
void launch_layernorm_with_bf16_copy(const float* x, int ld_x, int rows, int D, const float* gamma, const float* beta, float eps,
                                     float* out, int ld_out, bf16_t* out_lo, int ld_lo, hipStream_t s);


// ---- multi-head self-attention over packed ragged utterances (no mask inside an utterance).
// q, k: [rows][ld] row-major; vt: [H*HD][ld_vt] (time-contiguous); ctx out: [rows][ld_ctx].
// Scale is pre-folded into q and k (d^-1/4 each, Export_SenseVoice.py:210-216).
// Pad rows: the bf16 kernel stages keys in 32-key sub-tiles, so it READS the K rows and V^T columns from an utterance's T up to the next multiple of 32 (the
// rows up to its 16-row boundary, then whatever follows: the next utterance, or slack; reads past the allocation are clamped to its last row / last 8
// columns -- n_rows_alloc = ld_vt). Their scores are masked to -inf and their probabilities are exactly 0, but the zeros still enter the P.V product:
// every such row and column must hold FINITE values (0 x NaN and 0 x Inf are NaN). Any finite value gives the same bits. NaN / Inf there is outside the
// contract. The f32 kernel reads keys [0, T) only; it keeps a row's scores in LDS and takes max_T <= 2048 (launch_attention_f32 refuses more).
struct AttnArgs {
  const void* q; const void* k; int ld_qk;   // ld_qk: row stride of k (and of q unless ld_q is set)
  int ld_q = 0;
  const void* vt; int ld_vt;
  void* ctx; int ld_ctx;
  const UttPlan* plan;
  const int32_t* qb_utt;       // per query block: utterance
  const int32_t* qb_q0;        // per query block: first query row inside the utterance
  int n_qblocks, n_heads;
  // bf16 kernel geometry (attention_geometry): a query block = n_waves * qt tiles of 16 rows; max_T picks the chunk size.
  // The f32 kernel uses fixed 64-row blocks (qt = 0).
  int qt = 0, n_waves = 4, max_T = 0;
  // cross-attention: queries follow q_plan (row_off / T of the query rows), keys / values follow plan; null => self-attention
  const UttPlan* q_plan = nullptr;
  // bf16 kernels: causal = 1 masks keys > the query's own index (decoder prefill); kv_group > 1 = grouped-query attention,
  // q head h reads K / V head h / kv_group
  int causal = 0, kv_group = 1;
};
// query-block geometry for the longest utterance of a batch: rows per block = 16 * qt * n_waves
void attention_geometry(int max_T, int head_dim, int* qt, int* n_waves);
void launch_attention_bf16_hd128(const AttnArgs& a, hipStream_t s);
void launch_attention_bf16_hd64(const AttnArgs& a, hipStream_t s);
void launch_attention_f32(const AttnArgs& a, int head_dim, hipStream_t s);
// what this thread's last launch_attention_* ran: the bf16 instance <hd, chunk, qt> and its waves per workgroup (grid_z = 0), or the f32 kernel
// (chunk = qt = 0, waves = 4) and its gridDim.z: test hook
struct AttnLaunchInfo { int hd = 0, chunk = 0, qt = 0, waves = 0, grid_z = 0; };
const AttnLaunchInfo& attention_last_launch();

// ---- fused SANM attention half for windows of <= 144 rows (sanm_fused.hip): per (utterance, head) workgroup
// q|k|v projection -> attention -> FSMN, intermediates in LDS. h: [rows][ld_h] operand-dtype LayerNorm output;
// wqkv: [3 d][ldw] (q rows, k rows, v rows); ctx: bf16 [rows][ld_ctx]; mem: f32 [rows][ld_mem] (rows < T16 written).
struct SanmFusedArgs {
  const void* h; int ld_h; int K;
  const void* wqkv; int ldw;
  const float* bqkv;
  const float* wfsmn; const float* bfsmn;
  const UttPlan* plan; int n_utts, n_heads, d;
  void* ctx; int ld_ctx;
  float* mem; int ld_mem;
  int n_rows_alloc;            // rows of h that may be read (rows past an utterance's end are read but never used)
  // LayerNorm evaluated inside the projection: h holds the RAW rows x (bf16), row statistics over the first ln_dim columns
  // are accumulated from the LDS tiles while the MFMA loop runs and q|k|v = rstd (x W^T - mean colsum) + b. Needs the
  // LayerNorm affine folded into wqkv / bqkv; ln_colsum[n] = sum_k wqkv[n][k]. Null => h is already normalised.
  const float* ln_colsum = nullptr; int ln_dim = 0; float ln_eps = 1e-5f;
  const float2* ln_stats_in = nullptr; int ln_slots = 0;   // producer-side row statistics (GemmArgs::st_out layout); null => computed here
  int dbg = 0;
};
bool sanm_fused_supported(int max_T, int d_head, int n_heads, int d, int fsmn_taps, int K);

// ---- one whole SANM block per launch (csrc/sanm_block.hip): clusters of four workgroups per <= 144-row window, d = 512, 4 heads of 128,
// FFN 2048, LayerNorms folded into the projections (bf16 mode). Buffers are the packed row-major activations of the session.
// per-block constants of the 8-wave kernel (a launch walks `n_layers` consecutive entries of a device-side table)
struct SanmBlockLayer {
  const float *bqkv, *cqkv, *wfsmn, *bfsmn, *b1, *c1, *b2;
  const void* wpack;                                               // fragment-major copy of the block's four matrices (launch_sanm_block8_pack)
};
struct SanmBlockArgs {
  const bf16_t* wqkv; const float* bqkv; const float* cqkv;      // [1536][512] (LayerNorm affine folded), bias, column sums
  const float* wfsmn; const float* bfsmn;                          // [512][11], [512] (linear_out.bias rides here)
  const bf16_t* wout;                                              // [512][512]
  const bf16_t* w1; const float* b1; const float* c1;              // [2048][512] (LayerNorm affine folded), bias, column sums
  const bf16_t* w2; const float* b2;                               // [512][2048]
  const SanmBlockLayer* layers = nullptr; int n_layers = 1;        // 8-wave kernel: the launch's blocks (device table), first entry = the first block of the launch
  int flag_stride = 0;                                             // ... words between the exchange counters of consecutive blocks (flags points at the first block's)
  unsigned* place = nullptr;                                       // ... [n_utts] placement words of this launch (zeroed beforehand): byte h = XCD + 1 of workgroup (w, h)
  int times_layer = 0;                                             // ... which block of the launch `times` stamps
  int st_in_n = 16;                                                // partials per row in st_in: 16 (a GEMM epilogue's 32-column groups) or 4 (the 8-wave kernel's own records, one per workgroup, slots 0..3)
  int opt = 0;                                                     // tuning switches of the 8-wave kernel (ASR_SANM_BLOCK8_OPT): 1 = no L2 warm-up loads, 2 = deeper W fragment queues, 4 = always acquire-fence at an exchange (default: clusters that share an XCD read the payload with sc1 loads instead)
  int ffnk = 0;                                                    // round 6: FFN-2 K-split over the workgroup's own hidden columns, f16 partials exchanged instead of hid (needs the matching wpack order; `hid` then holds the partial images)
  const void* wpack = nullptr;                                     // round-4 kernel (sanm_block8.hip): fragment-major copy of the four matrices (launch_sanm_block8_pack)
  const bf16_t* x_lo; const float2* st_in;                         // block input rows (bf16) + their row statistics [rows][16] (null: derived in the kernel)
  float* x;                                                        // residual stream f32 [rows][512]: read (phase B) and overwritten (phase D) in place
  bf16_t* x_lo_out; float2* st_out;                                // bf16 copy + row statistics of the block output (may alias x_lo / st_in)
  bf16_t* ctx; bf16_t* x1_lo; float2* st1; bf16_t* hid;            // exchange buffers: [rows][512], [rows][512], [rows][16], [rows][2048]
  const UttPlan* plan; int utt0, n_utts;                           // windows utt0 .. utt0 + n_utts - 1 (all <= 144 rows)
  unsigned* flags;                                                 // [n_utts][4] exchange counters of THIS launch, zeroed beforehand
  unsigned* err;                                                   // err[0] != 0 after the run: a workgroup gave up waiting for its cluster
  int n_rows_alloc; float ln_eps; int scatter;                     // scatter != 0: test placement (a cluster spread over four XCDs)
  unsigned long long* times;                                       // tuning: [workgroups][16] wall-clock stamps (100 MHz) at the phase boundaries, or null
  int fault = 0;                                                   // tests: workgroup 5 withholds its first exchange count (its cluster then gives up after the bounded spin)
};
bool sanm_block_supported(int max_T, int d_head, int n_heads, int d, int d_ffn, int fsmn_taps);
int sanm_block_max_utts();                                         // windows one launch can take (all workgroups co-resident)
void launch_sanm_block8(const SanmBlockArgs& a, hipStream_t s);       // round-4 form: 8 waves, chunked A operand, register-streamed packed weights (needs a.wpack)
size_t sanm_block8_pack_bytes();                                      // bytes of one block's packed weights
void launch_sanm_block8_pack(const bf16_t* wqkv, const bf16_t* wout, const bf16_t* w1, const bf16_t* w2, void* dst, bool ffnk, hipStream_t s);
void launch_rows_to_bf16(const float* x, bf16_t* y, size_t n, hipStream_t s);     // f32 -> bf16 (RNE) copy, n a multiple of 8
void launch_sanm_qkv_attn(const SanmFusedArgs& a, hipStream_t s);

// ---- FSMN memory: depth-wise conv (k taps, zero padded inside each utterance) over V + bias.
// vt: [C][ld] time-contiguous (all rows of the padded packed layout); out: f32 row-major [n_rows_pad][ld_out]
// (Export_SenseVoice.py:217-220,240-244). n_rows_pad is a multiple of 64 (pad rows are written as zeros).
template <typename InT>
void launch_fsmn(const InT* vt, int ld, const float* w, const float* b, int C, int ktaps, const UttPlan* plan,
                 const int32_t* row_utt, int n_rows_pad, float* out, int ld_out, hipStream_t s);

// ---- CTC greedy collapse, circular next-neighbour rule (Export_SenseVoice.py:290-296)
void launch_ctc_collapse(const int32_t* frame_ids, const UttPlan* plan, int n_utts, int blank_id, int32_t* token_ids,
                         int max_tokens, int32_t* num_id, hipStream_t s);
// ... with each token's frame span and score: the token is emitted at last_frame = the last frame of its run, first_frame = the start of the maximal linear
// run of equal ids ending there (frames are rows of the utterance's sequence), token_logprob = mean of frame_logprob over first..last (f32 sum in ascending
// frame order / f32 count). Same ids, counts and max_tokens rule as launch_ctc_collapse.
void launch_ctc_collapse_timed(const int32_t* frame_ids, const float* frame_logprob, const UttPlan* plan, int n_utts, int blank_id, int32_t* token_ids,
                               int32_t* first_frame, int32_t* last_frame, float* token_logprob, int max_tokens, int32_t* num_id, hipStream_t s);

// ---- CTC prefix beam search (ctc_beam.hip)
// phrases (flattened ids, offsets [n_phrases + 1]) -> one int32 image [depth n][is_end n][child_off n + 1][child_tok n - 1][child_node n - 1]; hot_trie_view
// points a HotTrie into a device copy of it
std::vector<int32_t> build_hot_trie(const int32_t* ids, const int32_t* offsets, int n_phrases, int* n_nodes_out);
HotTrie hot_trie_view(const int32_t* dev_words, int n_nodes, float boost);
// Per row the `topk` (1..16) best columns n < n_valid of h W^T + bias and their log soft-max, from the per-slab partials of the timed CTC head (amax_val /
// amax_sum [M][n_slabs], 64-column slabs): only the topk slabs with the largest maxima are recomputed (f32 accumulation from the operand type T).
// cand_id / cand_lp [M][topk], higher value first, lower id on ties. m_dev (Paraformer's token rows; null: every row < M): a device-side row count -- rows at
// or past *m_dev are neither read nor written (their partials hold nothing defined).
template <typename T>
void launch_ctc_topk(const T* h, int ldh, const T* W, int ldw, const float* bias, int K, const float* amax_val, const float* amax_sum, int n_slabs, int M,
                     int n_valid, int topk, int32_t* cand_id, float* cand_lp, hipStream_t s, const int32_t* m_dev = nullptr);
// The search, one workgroup per utterance over rows plan[u].row_off .. + T of the candidate arrays. pool: [n_utts][pool_stride] (parent, token) nodes,
// pool_stride >= max T * beam. Outputs [n_utts][nbest] (token_ids [n_utts][nbest][max_tokens], best first; num_id keeps the full length); hypotheses beyond the
// number found have num_id 0 and score -inf. lm (ngram_lm.h; null or without nodes: none): a back-off n-gram model fused into the ranking; score
// then holds ctc + bonus + lm, ctc_score stays the CTC figure, and candidate ids must lie in the image's vocabulary.
struct NgramLm;
void launch_ctc_prefix_beam(const int32_t* cand_id, const float* cand_lp, int topk, const UttPlan* plan, int n_utts, int blank_id, int beam, int nbest,
                            const HotTrie& trie, int2* pool, int pool_stride, int32_t* token_ids, int max_tokens, int32_t* num_id, float* score, float* ctc_score,
                            hipStream_t s, const NgramLm* lm = nullptr);

// ---- beam search over the token rows of a non-autoregressive decoder (nar_beam.hip)
// One workgroup per utterance over rows token_plan[u].row_off .. + token_plan[u].n_lfr of the candidate arrays (the compact token plan of the CIF scan; the
// count is read on the device and cut at *m_dev when m_dev is given). Every hypothesis picks one candidate per row. pool: [n_utts][pool_stride] (parent rank,
// candidate column) nodes, pool_stride >= max n_lfr * beam. Outputs [n_utts][nbest], best first: token_ids / token_logprob (nullable) [n_utts][nbest][max_tokens],
// num_id the token count, score = acoustic + hotword bonus + lm, am_score = the sum of the picked candidates' log-probabilities; hypotheses beyond the number
// found have num_id 0 and both scores -inf. trie / lm as launch_ctc_prefix_beam takes them.
void launch_nar_beam(const int32_t* cand_id, const float* cand_lp, int topk, const UttPlan* token_plan, const int32_t* m_dev, int n_utts, int beam, int nbest,
                     const HotTrie& trie, int2* pool, int pool_stride, int32_t* token_ids, int max_tokens, int32_t* num_id, float* score, float* am_score,
                     float* token_logprob, hipStream_t s, const NgramLm* lm = nullptr);

// ---- the same search for a stream that arrives in chunks (nar_stream_beam.hip): carried state, fixed-lag commits
// One workgroup per stream of the call; token_plan[u].lang is the stream id (its state is state + id * state_stride, nar_stream_beam_state_words words; zeroed
// memory is a cleared stream), token_plan[u].row_off .. + n_lfr its rows of this call (0 is legal; cut at *m_dev when given). Streams not in the call are not
// touched, and a stream id may appear once per call. Before the row at position L is extended, L - C == pend_cap commits position C with the token of the best
// live hypothesis. Outputs per slot u of the call: the tokens committed by it (commit_* [n][commit_cap], commit_cap >= pend_cap + the call's longest row
// count), the pending tails of the best nbest live hypotheses (pend_ids / pend_lp [n][nbest][pend_cap], pend_num / pend_score / pend_am [n][nbest]; score and
// am without the end terms; num 0 and -inf beyond the live ones) and total = L. final_flags (nullable) [n]: a set flag ends the stream behind its rows -- the
// end terms of launch_nar_beam, the tails ranked again with their final scores, the best one's tail committed, the state cleared.
constexpr int NAR_STREAM_PEND_MAX = 64;
struct NarStreamOut {
  int32_t* commit_ids = nullptr; float* commit_lp = nullptr; int commit_cap = 0; int32_t* commit_num = nullptr;
  int32_t* pend_ids = nullptr; float* pend_lp = nullptr; int32_t* pend_num = nullptr; float* pend_score = nullptr; float* pend_am = nullptr;
  int32_t* total = nullptr;
};
int nar_stream_beam_state_words(int beam, int pend_cap);
void launch_nar_stream_beam(const int32_t* cand_id, const float* cand_lp, int topk, const UttPlan* token_plan, const int32_t* m_dev, const int32_t* final_flags,
                            int n_streams, int beam, int nbest, int pend_cap, const HotTrie& trie, int32_t* state, int state_stride, const NarStreamOut& out,
                            hipStream_t s, const NgramLm* lm = nullptr);

// ---- CTC forced alignment of a given transcript (ctc_align.hip)
// Emissions: for every row m < M with u = row_utt[m] >= 0, em[m][j] = log soft-max of h W^T + bias at slot j's column -- slot 0 the blank, slot j = 1 .. L_u
// target_ids[target_offsets[u] + j - 1] -- and -inf for L_u < j < ld_em. The logit is recomputed as launch_ctc_topk recomputes it and the row's log-sum-exp comes
// from the same per-slab partials, so a target that is also a candidate has that candidate's bits. Rows with row_utt < 0 are left alone.
template <typename T>
void launch_ctc_target_logprob(const T* h, int ldh, const T* W, int ldw, const float* bias, int K, const float* amax_val, const float* amax_sum, int n_slabs, int M,
                               const int32_t* row_utt, const int32_t* target_ids, const int32_t* target_offsets, int blank_id, float* em, int ld_em, hipStream_t s);
// Viterbi + forward trellis and the walk back, one workgroup per utterance over rows plan[u].row_off + row0 .. plan[u].row_off + plan[u].T - 1 of em
// [rows][ld_em] (slots as above). max_rows >= every plan[u].T, max_L >= every L_u (at most 1023). Per target j of utterance u, at [u][max_tokens]:
// first_frame / last_frame (rows of the utterance's sequence, row0 included) and token_logprob (mean emission over the span); per utterance path_score, loglik
// and status (0 aligned; 1 no alignment exists: the spans keep what they held and both scores are -inf). bp_ws: ctc_align_ws_bytes(...) bytes of workspace
// for the backpointers, may be null when that is 0 (they then live in LDS).
size_t ctc_align_ws_bytes(int n_utts, int max_rows, int row0, int max_L);
void launch_ctc_align(const float* em, int ld_em, const UttPlan* plan, int n_utts, int row0, int max_rows, const int32_t* target_ids, const int32_t* target_offsets,
                      int max_L, uint32_t* bp_ws, int32_t* first_frame, int32_t* last_frame, float* token_logprob, int max_tokens, float* path_score, float* loglik,
                      int32_t* status, hipStream_t s);

// ---- Paraformer CIF predictor + decoder helpers (Paraformer/Non-Streaming/Export_Paraformer.py:499-563)
// [x[t-1] | x[t] | x[t+1]] rows with zero padding at utterance edges: the k=3 conv as one GEMM (K = 3 d)
template <typename T>
void launch_shift3(const T* x, int d, const UttPlan* plan, const int32_t* row_utt, int n_rows, T* out, hipStream_t s);
// alpha[m] = sigmoid(dot(h[m], w) + b)
template <typename T>
void launch_alpha(const T* h, int d, const float* w, const float* b, int rows, float* alpha, hipStream_t s);
// continuous integrate-and-fire: float64 prefix sum of alpha (+ tail threshold), fire where floor() increments, acoustic
// embedding = difference of completed prefix integrals. Writes the token rows in the utterance's own row range and a
// DEVICE-side token plan (row_off, T = max(N,1), n_lfr = N) so the decoder needs no host round trip.
void launch_cif_scan(const float* alpha, const float* enc_out, int d, const UttPlan* plan, int n_utts, float tail_threshold,
                     float* acoustic, UttPlan* token_plan, int32_t* num_id, hipStream_t s);
// ... the same scan (every output above bit-identical) that also records where each token fired: fire_frame[u * max_tokens + k] = the row t in [0, T] at
// which floor((float)prefix sum) rose for token k (t == T: the tail threshold fired it behind the last row). Tokens at or past max_tokens are dropped;
// num_id keeps the full count.
void launch_cif_scan_timed(const float* alpha, const float* enc_out, int d, const UttPlan* plan, int n_utts, float tail_threshold,
                           float* acoustic, UttPlan* token_plan, int32_t* num_id, int32_t* fire_frame, int max_tokens, hipStream_t s);
// out[t] = res[t] + depth-wise conv (k taps, zero padded inside the token sequence) of x, all row-major f32
void launch_fsmn_rows(const float* x, const float* res, const float* w, int d, int ktaps, const UttPlan* token_plan,
                      const int32_t* row_utt, int n_rows, float* out, hipStream_t s, const int32_t* rows_dev = nullptr);
// compact token layout: utterance b's max(N_b, 1) token rows move from its own row range to offset sum_{j<b} roundup16(max(N_j, 1));
// writes the compact plan, the row -> utterance map of the compact rows (-1 past the end, n_rows_max entries) and the total row
// count (device side: the decoder's GEMM / LayerNorm launches are sized for the worst case and stop at this count)
void launch_token_compact(const UttPlan* own_plan, int n_utts, int n_rows_max, UttPlan* compact_plan, int32_t* row_utt, int32_t* total_rows,
                          hipStream_t s);
void launch_compact_rows(const float* src, const UttPlan* own_plan, const UttPlan* compact_plan, int n_utts, int d, float* dst, hipStream_t s);
// token_ids[b][i] = ids[row_off_b + i], i < N_b
void launch_gather_tokens(const int32_t* ids, const UttPlan* token_plan, int n_utts, int32_t* token_ids, int max_tokens, hipStream_t s);
// token_logprob[b][i] = row_logprob[row_off_b + i], i < N_b (the dummy row of a zero-token utterance is never read)
void launch_gather_token_logprob(const float* row_logprob, const UttPlan* token_plan, int n_utts, float* token_logprob, int max_tokens, hipStream_t s);


// ---- streaming Paraformer (Paraformer/Streaming/Export_Paraformer_Streaming.py:386-553). Every active stream owns a 16-row slot
// (13 rows used: 4 carried + 9 new); UttPlan.lang carries the stream id that indexes the per-stream state.
struct StreamLfrArgs {
  const float* mel; const UttPlan* plan; const float* cmvn_vars; const float* pos_bias;   // pos_bias[p] = means * vars + position p + 1
  const float* prev; const int32_t* start;      // state: carried rows [stream][n_prev][ld], absolute LFR position per stream
  float* out; int ld; int feat, n_mels, lfr_m, lfr_n, n_prev, n_new, n_rows, n_frames, pos_rows;
};
void launch_stream_lfr(const StreamLfrArgs& a, hipStream_t s);
// prev[stream] = rows [n_new .. n_new + n_prev) of the slot (the last n_prev of the n_prev + n_new rows); start[stream] += n_new
void launch_stream_carry(const float* x, int ld, const UttPlan* plan, int n_active, int n_prev, int n_new, float* prev, int32_t* start,
                         hipStream_t s);
// soft-max attention of the slot's query rows over [cached keys of the stream | the slot's current rows], head_dim 128
struct StreamAttnArgs {
  const void* q; int ld_q, q_col0;
  const void* k; int ld_k, k_col0; const void* v; int ld_v, v_col0; int n_cur;      // current rows (row-major, operand dtype)
  const void* cache_k; const void* cache_v; const int32_t* cache_len; int cap;        // [stream][head][cap][128]
  const UttPlan* q_plan;        // T = number of query rows (0 => nothing to do), row_off, lang = stream id
  int n_heads;
  void* ctx; int ld_ctx;
  // encoder layers: the same workgroup also (a) rolls its (stream, head) K / V history -- keep the last `cap` of (history ++ the first
  // roll_rows current rows) -- and (b) computes the FSMN memory term of the chunk rows (depth-wise conv over the CURRENT rows of V, taps
  // outside them are zero) for its 128 channels; both null / 0 for the decoder's cross-attention
  int roll_rows = 0;
  const float* fsmn_w = nullptr; const float* fsmn_b = nullptr; int ktaps = 0; float* mem = nullptr; int d = 0;
};
template <typename T> void launch_stream_attn(const StreamAttnArgs& a, int n_active, hipStream_t s);
// cache = last `cap` of (cache ++ current rows [0, n_app)); skipped for streams whose cond_plan[i].T == 0 (when cond_plan is given)
template <typename T>
void launch_stream_cache_roll(void* cache_k, void* cache_v, const int32_t* cache_len, int cap, const void* k, int ld_k, int k_col0,
                              const void* v, int ld_v, int v_col0, int n_app, const UttPlan* plan, const UttPlan* cond_plan, int n_active,
                              int n_heads, hipStream_t s);
// encoder FSMN over the slot's n_cur rows (zero padded at both ends), identity folded into the centre tap: mem = b + conv(v)
template <typename T>
void launch_stream_fsmn(const T* v, int ld_v, int v_col0, const float* w, const float* b, int d, int ktaps, int n_cur, int n_rows, float* mem,
                        hipStream_t s);
// unrolled integrate-and-fire over rows [0, n_int) of every slot with the carried (hidden, alphas) (:438-462)
void launch_stream_cif(const float* alpha, const float* enc, int d, const UttPlan* plan, int n_active, int n_int, float* cif_hidden,
                       float* cif_alphas, float* frames_out, UttPlan* token_plan, int32_t* num, hipStream_t s);
// ... that also records the integration step of every fire: fire_step[i * max_tokens + k] = t in [0, n_int), or -1 for the entry fire in front of the loop
// (the carried weight had already reached 1). Every other output is bit-identical.
void launch_stream_cif_timed(const float* alpha, const float* enc, int d, const UttPlan* plan, int n_active, int n_int, float* cif_hidden,
                             float* cif_alphas, float* frames_out, UttPlan* token_plan, int32_t* num, int32_t* fire_step, int max_tokens,
                             hipStream_t s);
// decoder FSMN over [hist | tokens] (valid conv, identity folded into the LAST tap) + residual; history advances when tokens exist
void launch_stream_dec_fsmn(const float* x, const float* res, const float* w, int d, int ktaps, const UttPlan* token_plan, int n_active,
                            float* hist, float* out, hipStream_t s);
void launch_stream_advance(const UttPlan* plan, const UttPlan* token_plan, int n_active, int en_add, int en_cap, int de_add, int de_cap,
                           int32_t* en_len, int32_t* de_len, hipStream_t s);
// Snapshot / restore of the recurrent state of the ACTIVE streams of a chunk step (K/V histories of every layer, decoder FSMN histories, carried rows, CIF
// state, history lengths): a fused chunk step whose cluster launch gave up has rolled the histories of the layers in front of the one that stalled, so the step
// can only be redone (on the per-launch path) from a copy taken in front of it. A segment = one state buffer laid out [outer][stream][per_stream bytes];
// the shadow has the same layout. restore = false: live -> shadow, true: shadow -> live.
struct StreamStateSeg { unsigned char* live; unsigned char* shadow; unsigned long long per_stream, outer_stride; int n_outer, first_item; };
void launch_stream_state_copy(const StreamStateSeg* segs, int n_segs, int n_items, const UttPlan* plan, int n_active, bool restore, hipStream_t s);

// ---- Paraformer online encoder layers of one chunk step as ONE launch (stream_layers.hip): clusters of four workgroups per stream, weights streamed
// from a fragment-major copy of every layer. bf16 sessions, d = 512 / 4 heads / d_ffn = 2048 / history + 16 <= 64 keys.
struct StreamLayer {
  const unsigned char* wpack;                               // launch_stream_layers_pack of this layer's q|k|v, out, w1, w2
  const float *bqkv, *wfsmn, *bfsmn, *b1, *b2;
  bf16_t* cache_k; bf16_t* cache_v;                        // this layer's histories [stream][head][cap][128]
};
struct StreamLayersArgs {
  const UttPlan* plan;                                      // per active stream: row_off (its 16-row slot), lang = stream id
  int n_streams, n_layers, n_cur, cap, roll_rows, ktaps;
  float ln_eps;
  const int32_t* cache_len;                                 // [stream] history rows (the same for every layer)
  const StreamLayer* layers;                                // device table
  float* x;                                                 // [rows][512] residual stream: in = rows entering the first layer of the table, out = rows leaving the last
  float* xb; bf16_t* ctx; bf16_t* hid;                      // the clusters' exchange buffers [rows][512] f32, [rows][512], [rows][2048]
  unsigned* flags;                                          // [n_layers][n_streams][4] counters, zero at launch
  int opt = 0;                                              // tuning: 1 = no L2 warm-up of the next phase's weights, 2 = FFN weights warmed while waiting for exchanges 1 / 2 instead of under the attention, 8 = a stream's four heads on one XCD instead of placement by head; bits 4..6 = phases (A, C, D) whose second weight batch is requested right behind the exchanged rows
  unsigned* err;                                            // raised by a cluster that gave up waiting (the launch's results are void)
  unsigned long long* times = nullptr; int times_layer = 0; // tuning: thread 0 of every workgroup stamps wall_clock64() at 13 points of layer `times_layer` ([wg][16])
  int fault = 0;                                            // tests: workgroup 5 withholds its count on the first exchange of the first layer (its cluster gives up)
};
size_t stream_layers_pack_bytes();
void launch_stream_layers_pack(const bf16_t* wqkv, const bf16_t* wout, const bf16_t* w1, const bf16_t* w2, void* dst, hipStream_t s);
bool stream_layers_supported(int d, int d_ffn, int n_heads, int cap, int n_cur, int ktaps);
void launch_stream_layers(const StreamLayersArgs& a, hipStream_t s);

// ---- SANM blocks of a SMALL batch of <= 144-row windows, a run of blocks as one launch (sanm_tiles.hip): a workgroup per (16-row tile, head), the streaming
// encoder's weight images (launch_stream_layers_pack) and layer table entries (cache pointers unused)
struct SanmTilesArgs {
  const UttPlan* plan;                                      // per window: T, row_off
  const int32_t* tile_win; const int32_t* tile_idx;         // per tile cluster: its window, its tile inside the window
  int n_tiles, n_windows, n_layers;
  float ln_eps;
  const StreamLayer* layers;                                // device table
  float* x;                                                 // [rows][512] residual stream, in place
  float* xb; bf16_t* ctx; bf16_t* hid;                      // exchange buffers of a tile's four heads: [rows][512] f32, [rows][512], [rows][2048]
  bf16_t* kv; size_t kv_parity_stride;                      // exchange buffer of a head's tiles: [block parity][rows][k | v][512], elements between the two
  unsigned* flags; int flag_stride;                         // per layer: [n_tiles][4] + [n_windows][4] counters, zero at launch; flag_stride = words per layer
  unsigned* err;
  int opt = 0;                                              // tuning: 1 = no L2 warm-up, 2 = a tile's four heads on one XCD instead of placement by head
  unsigned long long* times = nullptr; int times_layer = 0;
};
bool sanm_tiles_supported(int max_T, int d, int d_ffn, int n_heads, int d_head, int ktaps);
int sanm_tiles_max_tiles();
void launch_sanm_tiles(const SanmTilesArgs& a, hipStream_t s);

// ---- Paraformer online decoder layers of one chunk step as ONE launch (stream_dec.hip): the same clusters; a stream without a fired token leaves at once
struct StreamDecLayer {
  const unsigned char* wpack;                               // launch_stream_dec_pack of this layer's w1, w2, wq, wkv, wo
  const float *b1, *b2, *n2_g, *n2_b, *wfsmn, *bq, *bkv, *bo;
  float* fsmn_hist;                                         // [stream][10][512] f32
  bf16_t* cache_k; bf16_t* cache_v;                        // [stream][head][cap][128]
  int full;                                                 // 0: FFN-only block (the last one)
};
struct StreamDecArgs {
  const UttPlan* token_plan;                                // per active stream: T = fired tokens, row_off (its 16-row slot), lang = stream id
  int n_streams, n_layers, n_cur, cap;
  float ln_eps;
  const int32_t* cache_len;                                 // [stream] K/V history rows
  const StreamDecLayer* layers;                             // device table
  const bf16_t* enc;                                        // [rows][512] the chunk's encoder rows (after_norm, bf16)
  float* dec;                                               // [rows][512] fired frames in, decoder output rows out
  float* x1; float* x2; float* hid; bf16_t* ctx;            // exchange buffers [rows][512] f32 x 2, [rows][2048] f32, [rows][512] bf16
  unsigned* flags;                                          // [n_layers][n_streams][8] counters, zero at launch
  unsigned* err;
  int opt = 0;                                              // tuning: 1 = no L2 warm-up, 8 = placement by head (the encoder launch's default; slower here)
  unsigned long long* times = nullptr; int times_layer = 0;
};
size_t stream_dec_pack_bytes();
void launch_stream_dec_pack(const bf16_t* w1, const bf16_t* w2, const bf16_t* wq, const bf16_t* wkv, const bf16_t* wo, bool full, void* dst, hipStream_t s);
bool stream_dec_supported(int d, int d_ffn, int n_heads, int cap, int n_cur, int ktaps);
void launch_stream_dec(const StreamDecArgs& a, hipStream_t s);

