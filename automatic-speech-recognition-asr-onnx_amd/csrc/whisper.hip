// Whisper hot path on one MI355X.
//   encode : packed ragged batch -> STFT power / log-mel -> conv stem (two strided-view GEMMs, no im2col) ->
//            N encoder layers -> fused cross-KV projection written straight into per-(layer, head) slabs.
//            Follows WHISPER_ENCODER.forward (Whisper/Export_Whisper.py:422-447) + STFT_Process (:224-246).
//   prefill / decode : token+position embedding -> M decoder layers (self-attention with an in-place KV cache,
//            cross-attention over the slabs, FFN) -> tied proj_out + (-128) suppress penalty -> arg-max.
//            Follows WHISPER_DECODER_EMBED / WHISPER_PREFILL / WHISPER_DECODE / WHISPER_DECODER.forward
//            (:450-497,614-667) and the BEGIN_SUPPRESS / ARGMAX heads (:228-260).
// The reference grows the self-KV by torch.cat every token (O(L^2) copies, :640-641) and shuttles 128 KV tensors
// through Python per step; here the cache is appended in place and token ids stay on the device between steps.
#include <cstdlib>
#include <cstring>

#include "../../include/asr_mi355x.h"
#include "decode_head.h"
#include "engine.h"
#include "gemm.h"
#include "kernels.h"

namespace {

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Beam search: the prompt's self-K/V rows (slots < p0 of every layer: the prefill's, pad slots of a left-padded prompt included -- key_start keeps those out of the attention) from the session's cache -- the paged pool or the contiguous extents --
// into every hypothesis row's extent, once per search. Grid (rows, layers x 2 x heads); extents [layer][row][K | V][head][S][64].
template <typename T>
__global__ __launch_bounds__(256) void wh_beam_prompt_kernel(const T* __restrict__ pool, const int32_t* __restrict__ ptable, int pages_per_seq,
                                                             const T* __restrict__ kc, const T* __restrict__ vc, int max_pos, int B, int H, int p0, int beam,
                                                             int S, T* __restrict__ ext) {
  const int row = blockIdx.x, N = gridDim.x, lkh = blockIdx.y;   // lkh = (layer * 2 + K | V) * H + head
  const int h = lkh % H, kv = (lkh / H) & 1, l = lkh / (2 * H), b = row / beam;
  T* dst = ext + ((size_t)l * N + row) * 2 * H * S * 64 + ((size_t)kv * H + h) * S * 64;
  for (int i = threadIdx.x; i < p0 * 64; i += blockDim.x) {
    const int s = i >> 6, e = i & 63;
    const T* src = pool ? pool + (size_t)ptable[(size_t)b * pages_per_seq + (s >> 4)] * gridDim.y * 1024 + (size_t)lkh * 1024 + (size_t)(s & 15) * 64
                        : (kv ? vc : kc) + (((size_t)l * B + b) * H + h) * max_pos * 64 + (size_t)s * 64;
    dst[(size_t)s * 64 + e] = src[e];
  }
}

// one decoder pass of a beam search over its hypothesis rows (WhSession::beam_search)
struct BeamStep {
  int beam = 1, p0 = 0, S = 0;         // width, prompt positions, slots per row extent
  const int32_t* src = nullptr; int ld_src = 0;
  int32_t* hist = nullptr;             // the rows' position (all rows stand at the same one), advanced by the pass
  float* logits = nullptr;             // [rows][vpad]
};

struct EncLayer { const void *wqkv, *wo, *w1, *w2; const float *bqkv, *bo, *b1, *b2; };
struct DecLayer { const void *wqkv, *wo, *wcq, *wco, *w1, *w2; const float *bqkv, *bo, *bcq, *bco, *b1, *b2; };
struct Enc8Layer { const unsigned char *w1, *w2; const float *s1, *s2; };     // FP8MM mode: the encoder FFN pair as e4m3 bytes + per-row scales

struct WhSession : asr_session {
  asr_whisper_config cfg;
  int vpad = 0, act = ACT_GELU_ERF;
  FrontEnd fe;
  std::vector<EncLayer> enc;
  std::vector<DecLayer> dec;
  const float *conv1_b = nullptr, *conv2_b = nullptr, *enc_pos = nullptr, *enc_ln_g = nullptr,
              *enc_ln_b = nullptr, *ckv_b = nullptr, *dec_pos = nullptr, *suppress = nullptr, *begin = nullptr, *dec_ln_g = nullptr,
              *dec_ln_b = nullptr;
  const void *conv1_w = nullptr, *conv2_w = nullptr, *ckv_w = nullptr, *embed = nullptr;
  int k_conv1 = 0;

  // encoder state of the current batch
  int batch = 0, rows = 0, Mpad = 0, hist = 0, max_T_enc = 0;
  std::vector<UttPlan> plan;
  DeviceBuffer d_plan, d_audio, d_mel, d_blkmax, d_x0, d_h1, d_xa, d_xb, d_xc, d_h, d_qk, d_vt, d_ctx, d_ffn, d_cross;
  // decoder state
  DeviceBuffer d_kc, d_vc, d_ids, d_next, d_logits, d_dx, d_dqkv, d_dtok, d_hist;
  // Text prompts (asr_whisper_prefill_prompts): a batch of ragged prompt lengths is prefilled as n = max(len) slots per sequence, sequence b LEFT-padded by
  // pad[b] = n - len[b] slots, so the session keeps ONE history counter and every later single-token step stays uniform (one position per sequence, one
  // captured graph). Slot s of sequence b is position s - pad[b]; the keys in slots below pad[b] do not exist for it. d_kstart [B] holds pad[b] while
  // kstart_on (from such a prefill until the next prefill / encode): the embedding subtracts it, the single-token self-attention forms skip the keys below it.
  DeviceBuffer d_kstart;
  bool kstart_on = false;
  const int32_t* kstart() const { return kstart_on ? d_kstart.as<int32_t>() : nullptr; }
  // Paged self-KV cache (the default; ASR_KV_PAGED=0 keeps one contiguous max_target_positions extent per sequence and head in d_kc / d_vc).
  // Pool d_kvpool: pages of KV_PAGE positions, page-major [page][layer][K | V][head][KV_PAGE][64], so a page carries one 16-position slice of a
  // sequence for every layer and the pool grows by appending pages (the old pool is a prefix of the new one: one copy). Block table d_ptable
  // [batch][pages_per_seq] (int32 page ids, -1 = not allocated), shared by all layers. Pages are handed out a generation at a time (generation j = the
  // j-th page of every sequence of the batch: all sequences of a batch stand at the same position), first for the prompt + 48 positions, then doubling,
  // so a 32-token batch of 64 holds 4 x 64 pages (0.67 GB at large-v3) instead of 64 x 448 positions (9.4 GB).
  static constexpr int KV_PAGE = 16;
  DeviceBuffer d_kvpool, d_ptable;
  bool kv_paged = true;
  int kv_gens = 0, kv_batch = 0, kv_shuffle = 0;      // generations allocated, the batch they were cut for; kv_shuffle (tests): permute the page ids inside every generation
  void ensure_kv_pages(int B, int positions, size_t elem_bytes);
  TokenHead head;                      // arg-max / penalty-greedy / sampling (Inference_Whisper_ONNX.py:71-78) + the history of generated ids [B][max_target_positions]
  DeviceBuffer d_nsp;                  // no-speech probabilities of the last prefill
  bool use_graph = true;
  bool use_decode_gemm = true;         // ASR_DECODE_GEMM=0: decode steps through the generic weight-streaming GEMM + LayerNorm prologues
  DeviceBuffer d_colsum, d_dlo;        // column sums of the LayerNorm-folded decoder projections; bf16 copies of the decoder's residual rows
  // precision mode ASR_PRECISION_FP8W (opt-in; everything else as in bf16 mode): the six projections of every decoder layer as e4m3 bytes with a
  // power-of-two scale per output column, read by the decode GEMM (<= 64 rows); their exact bf16 dequantisation serves every other path
  // (prefill, > 64 rows), so all steps of a session see the same effective weights. The cross-K/V slabs are quantised once per batch with a
  // scale per (sequence, head) and streamed as bytes by the decode attention. ASR_FP8_FAKE=1: same quantisation, bf16 kernels throughout.
  // precision mode ASR_PRECISION_FP8MM (opt-in): FP8W plus the encoder's FFN pair on the FP8 matrix pipe (csrc/gemm_fp8.hip): fc1 / fc2 weights as e4m3 bytes with
  // per-row power-of-two scales, their activation operands (the second LayerNorm's output, the GELU output) as e4m3 bytes at unit scale
  // (saturating at 448: the LayerNorm output cannot get there -- its affine pair is folded into fc1, |row| <= sqrt(d_model) --; the GELU output can on a real
  // checkpoint: it is stored as value * 2^-act_shift (ASR_FP8MM_ACT_SHIFT / asr_whisper_set_fp8_act_shift, default 0), fc2 multiplies the shift back, and every
  // element that still meets the clamp is counted -- asr_whisper_fp8_stats; the Python session warns when the count moves)
  bool fp8_mm = false;
  int fp8_act_shift = 0;
  std::vector<Enc8Layer> enc8;
  DeviceBuffer d_ew8, d_ewscale, d_h8, d_ffn8, d_sat;
  bool fp4 = false;                    // precision mode ASR_PRECISION_MXFP4W (opt-in): FP8W with the decoder projections as MXFP4 (e2m1 + e8m0 per 32 k) instead of e4m3
  bool fp8 = false, fp8_fake = false, fp8_weights = true, fp8_kv = true;     // ASR_FP8_WEIGHTS=0 / ASR_FP8_KV=0: leave that half in bf16 (to price the halves separately)
  LowBitWeights dec8;                  // wqkv, wo, wcq, wco, w1, w2 of every decoder layer
  DeviceBuffer d_cross8, d_cscale;
  StepGraph dec_graph;                 // the whole single-token step
  StepGraph beam_graph[2];             // the beam-search step, one per ancestry-table parity
  // Beam search (asr_whisper_beam_search): hypothesis rows b * beam + r, each with its own self-K/V extent of S = prompt + max_new - 1 slots in d_bext
  // [layer][row][K | V][head][S][64] (large-v3, 160 rows x 447 slots: 11.7 GB; kept for the next search), a position counter and logits of its own, ranking
  // state and ancestry / token tables in `ranker`: the session's pages, block table, history, ids and logits are left as the prefill left them.
  DeviceBuffer d_bext, d_bhist, d_blogits;
  BeamRanker ranker;
  bool after_prefill = false;          // the last call on the session was a prefill (or a beam search, which leaves its state as it was)
  // Word timestamps (asr_whisper_set_word_timestamps; csrc/whisper_align.hip): while on, the last position of a prefill and every single-token step write the
  // raw cross-attention scores of the selected (layer, head) pairs into row position - wts_p0 of d_wscores, f32 [B][n_pairs][wts_max_rows][wts_ld]. The
  // scores are taken against the bf16 (f32) slabs of d_cross in every precision mode: alignment should not inherit e4m3 K. asr_whisper_align turns the
  // captured rows into frames: soft-max in place, column statistics (d_wstats), cost matrix (d_wcost [B][rows][ld]), DTW (d_wtrace, a byte per cell).
  bool wts_on = false, wts_consumed = false;
  int wts_max_rows = 0, wts_p0 = -1, wts_ld = 0, wts_rows = 0;      // wts_p0: prompt length - 1 of the last prefill under the mode; wts_rows: rows captured since
  uint64_t wts_epoch = 0;                                           // moves with the pair list
  std::vector<int32_t> wts_pairs;                                   // [n_pairs][2] as given
  std::vector<int> wts_first, wts_count;                            // per decoder layer: its run in d_wsel
  std::vector<int32_t> wts_n_rows, wts_n_frames;                    // of the last align
  DeviceBuffer d_wsel, d_wscores, d_wstats, d_wcost, d_wtrace, d_wn, d_wframes;
  PinnedBuffer h_walign;
  int n_pairs() const { return (int)wts_pairs.size() / 2; }
  void set_word_timestamps(int enable, const int32_t* pairs, int n, int max_rows);
  void align(const int32_t* n_rows, const int32_t* n_frames, int width, int32_t* frames_out, int out_stride);
  void align_read(int what, int b, void* host_out, size_t bytes, int32_t* shape_out);
  uint64_t ws_epoch = 1;
  PinnedBuffer h_plan, h_io;

  void init();
  SplitKGemm sk;
  void gemm(const GemmArgs& g) { sk.run(g, precision, stream); }
  template <typename T> void encode(const void* audio, int audio_mem, const int64_t* offs, int B, int32_t* n_pos_out);
  template <typename T> void enqueue_step(const int32_t* ids_dev, int n, bool is_prefill, bool use_hist_dev, const BeamStep* bs = nullptr, bool prompt = false);
  template <typename T> void step(const int32_t* ids_host, int n, bool is_prefill, int32_t* next_out, float* logits_out, const int32_t* pad_host = nullptr);
  void prefill_prompts(const int32_t* ids, const int32_t* offsets, int32_t* next_out, float* logits_out);
  template <typename T> void beam_search(int beam, int max_new, int eos_id, int32_t* tokens_out, int32_t* n_out, float* scores_out);
};

void WhSession::init() {
  const auto& c = cfg;
  ASR_REQUIRE(c.d_model == c.n_heads * c.d_head && c.d_head == 64, "whisper: head_dim must be 64 and d_model = heads * 64");
  ASR_REQUIRE(c.d_model % 128 == 0 && c.d_ffn % 128 == 0, "whisper: d_model and d_ffn must be multiples of 128");
  ASR_REQUIRE(c.nfft == 400 && c.hop_length == 160, "whisper: front-end is built for n_fft 400 / hop 160");
  ASR_REQUIRE(c.n_mels % 16 == 0, "whisper: n_mels must be a multiple of 16");
  ASR_REQUIRE(c.max_target_positions <= 1536, "whisper: decoder context too long for the attention kernel");
  vpad = round_up(c.vocab, 128);
  head.init(c.max_target_positions, 0, 20, 512);
  head.prof = &prof; ranker.prof = &prof;
  fe.init(c.nfft, c.nfft, c.hop_length, c.n_mels, 1, 1e-10f);
  model_rate = c.sample_rate;
  act = c.gelu_tanh ? ACT_GELU_TANH : ACT_GELU_ERF;
  const int wt = precision == ASR_PRECISION_BF16 ? ARENA_BF16 : ARENA_F32;
  const int d = c.d_model, dff = c.d_ffn, Ld = c.n_dec_layers;
  auto F = [&](const std::string& n, std::initializer_list<int64_t> sh) { return (const float*)arena.get(n, ARENA_F32, sh).ptr; };
  auto W = [&](const std::string& n, std::initializer_list<int64_t> sh) { return arena.get(n, wt, sh).ptr; };
  fe.dft = F("fe.dft", {(int64_t)fe.n_bin_tiles * 2 * fe.n_kchunks * 64 * 4});
  fe.melp = F("fe.mel", {(int64_t)(c.n_mels / 16) * fe.n_bin_tiles * 64 * 4});
  k_conv1 = round_up(3 * c.n_mels, 64);                 // whole GEMM K steps: the arena pads the three taps with zero columns (80 mels: 240 -> 256)
  conv1_w = W("enc.conv1_w", {d, k_conv1});
  conv1_b = F("enc.conv1_b", {d});
  conv2_w = W("enc.conv2_w", {d, 3 * d});
  conv2_b = F("enc.conv2_b", {d});
  enc_pos = F("enc.pos", {c.max_source_positions, d});
  enc_ln_g = F("enc.ln_g", {d});
  enc_ln_b = F("enc.ln_b", {d});
  ckv_w = W("ckv.w", {2 * Ld * d, d});
  ckv_b = F("ckv.b", {2 * Ld * d});
  embed = W("dec.embed", {vpad, d});
  dec_pos = F("dec.pos", {c.max_target_positions, d});
  suppress = F("dec.suppress", {vpad});
  begin = F("dec.begin", {vpad});
  dec_ln_g = F("dec.ln_g", {d});
  dec_ln_b = F("dec.ln_b", {d});
  enc.resize(c.n_enc_layers);
  for (int i = 0; i < c.n_enc_layers; ++i) {
    const std::string p = "enc" + std::to_string(i) + ".";
    enc[i] = EncLayer{W(p + "wqkv", {3 * d, d}), W(p + "wo", {d, d}), W(p + "w1", {dff, d}), W(p + "w2", {d, dff}),
                      F(p + "bqkv", {3 * d}), F(p + "bo", {d}), F(p + "b1", {dff}), F(p + "b2", {d})};
  }
  dec.resize(Ld);
  for (int i = 0; i < Ld; ++i) {
    const std::string p = "dec" + std::to_string(i) + ".";
    dec[i] = DecLayer{W(p + "wqkv", {3 * d, d}), W(p + "wo", {d, d}), W(p + "wcq", {d, d}), W(p + "wco", {d, d}),
                      W(p + "w1", {dff, d}), W(p + "w2", {d, dff}),
                      F(p + "bqkv", {3 * d}), F(p + "bo", {d}), F(p + "bcq", {d}), F(p + "bco", {d}), F(p + "b1", {dff}), F(p + "b2", {d})};
  }
  if (fp8_mm) {
    ASR_REQUIRE(d % 256 == 0 && dff % 256 == 0, "whisper: FP8MM mode needs d_model and d_ffn to be multiples of 256");
    const size_t per = (size_t)2 * d * dff;
    d_ew8.reserve((size_t)c.n_enc_layers * per, stream); d_ewscale.reserve((size_t)c.n_enc_layers * (d + dff) * 4, stream);
    d_sat.reserve(8, stream); HIP_CHECK(hipMemsetAsync(d_sat.ptr, 0, 8, stream));
    enc8.resize(c.n_enc_layers);
    for (int i = 0; i < c.n_enc_layers; ++i) {
      unsigned char* w8 = d_ew8.as<unsigned char>() + i * per;
      float* sc = d_ewscale.as<float>() + (size_t)i * (d + dff);
      launch_quantize_rows_fp8((const bf16_t*)enc[i].w1, d, dff, d, w8, sc, nullptr, stream);
      launch_quantize_rows_fp8((const bf16_t*)enc[i].w2, dff, d, dff, w8 + (size_t)dff * d, sc + dff, nullptr, stream);
      enc8[i] = Enc8Layer{w8, w8 + (size_t)dff * d, sc, sc + dff};
    }
  }
  if (fp8 && fp8_weights) {
    ASR_REQUIRE(d % 256 == 0 && dff % 256 == 0, "whisper: FP8 / MXFP4 mode needs d_model and d_ffn to be multiples of 256");
    dec8.build(Ld, fp4, [&](int i) {
      DecLayer& L = dec[i];
      return std::vector<LowBitWeights::Slot>{{&L.wqkv, 3 * d, d}, {&L.wo, d, d}, {&L.wcq, d, d}, {&L.wco, d, d}, {&L.w1, dff, d}, {&L.w2, d, dff}};
    }, stream);
  }
  if (precision == ASR_PRECISION_BF16 && use_decode_gemm) {      // column sums of the three LayerNorm-folded projections of every decoder layer: [3d | d | dff]
    const size_t per = (size_t)3 * d + d + dff;
    d_colsum.reserve((size_t)Ld * per * 4, stream);
    for (int i = 0; i < Ld; ++i) {
      float* c0 = d_colsum.as<float>() + i * per;
      launch_colsum_bf16((const bf16_t*)dec[i].wqkv, d, 3 * d, d, c0, stream);
      launch_colsum_bf16((const bf16_t*)dec[i].wcq, d, d, d, c0 + 3 * d, stream);
      launch_colsum_bf16((const bf16_t*)dec[i].w1, d, dff, d, c0 + 4 * d, stream);
    }
    HIP_CHECK(hipStreamSynchronize(stream));
  }
}

// ======================================================================================== encoder
template <typename T>
void WhSession::encode(const void* audio, int audio_mem, const int64_t* audio_offs, int B, int32_t* n_pos_out) {
  const auto& c = cfg;
  ASR_REQUIRE(B > 0 && audio && audio_offs, "whisper_encode: bad argument");
  HIP_CHECK(hipSetDevice(device));
  const AudioIn in = stage_input(*this, true, audio, audio_mem, audio_offs, B);     // default input format: the caller's own; else model-rate f32 and its offsets
  const int64_t* const offs = in.offs;
  const int d = c.d_model, dff = c.d_ffn, Ld = c.n_dec_layers, H = c.n_heads;
  plan.assign(B, UttPlan{});
  std::vector<UttPlan> splan(B);                          // the conv stem's view: same utterances, row_off in the gapped layout's row space
  int r = 0, rg = 0, frames = 0, n_fb = 0, n_qb = 0, max_T = 0;
  const int64_t base0 = offs[0];
  for (int b = 0; b < B; ++b) {
    UttPlan& p = plan[b];
    fe.plan_utt("whisper", b, offs, c.max_audio_len, p, frames, n_fb);      // n_frames = samples / hop (:96-103)
    p.T = (p.n_frames + 1) / 2;                          // conv2 stride 2, pad 1
    p.n_lfr = p.T;
    ASR_REQUIRE(p.T <= c.max_source_positions, "whisper: %d encoder positions exceed max_source_positions", p.T);
    p.row_off = r;
    splan[b] = p;
    splan[b].row_off = rg;
    r += round_up(p.T, 16);                              // encoder stream: compact, 16-row aligned (8 s: 400 rows per utterance)
    rg += round_up(p.T + 1, 16);                         // conv stem: +1 = room for the right zero-pad frame
    max_T = std::max(max_T, p.T);
    if (n_pos_out) n_pos_out[b] = p.T;
  }
  batch = B; rows = r; Mpad = round_up(r, 128); hist = 0; max_T_enc = max_T;
  const int rows_g = rg, Mg = round_up(rg, 128);
  int att_qt = 0, att_nw = 4, q_rows = 64;
  if (precision == ASR_PRECISION_BF16) { attention_geometry(max_T, c.d_head, &att_qt, &att_nw); q_rows = 16 * att_qt * att_nw; }
  for (int b = 0; b < B; ++b) n_qb += (plan[b].T + q_rows - 1) / q_rows;
  const int R = 2 * Mg;                                  // gapped (frame-rate) rows

  // plan blob: [UttPlan B (encoder rows)][UttPlan B (stem rows)][blk_utt][blk_f0][qb_utt][qb_q0][row_utt Mpad][pos_rows Mg][grow_utt R]
  PlanBlob pb(h_plan, d_plan);
  const auto s_plan = pb.add<UttPlan>(B), s_stem = pb.add<UttPlan>(B);
  const auto s_blk_utt = pb.add<int32_t>(n_fb), s_blk_f0 = pb.add<int32_t>(n_fb), s_qb_utt = pb.add<int32_t>(n_qb), s_qb_q0 = pb.add<int32_t>(n_qb);
  const auto s_row_utt = pb.add<int32_t>(Mpad), s_pos_rows = pb.add<int32_t>(Mg), s_grow_utt = pb.add<int32_t>(R);
  pb.commit(stream);
  if (pb.dev_moved) ++ws_epoch;
  memcpy(pb.host(s_plan), plan.data(), sizeof(UttPlan) * B);
  memcpy(pb.host(s_stem), splan.data(), sizeof(UttPlan) * B);
  fill_fbank_blocks(plan.data(), B, pb.host(s_blk_utt), pb.host(s_blk_f0));
  fill_query_blocks(plan.data(), B, q_rows, pb.host(s_qb_utt), pb.host(s_qb_q0));
  int32_t *row_utt = pb.host(s_row_utt), *pos_rows = pb.host(s_pos_rows), *grow_utt = pb.host(s_grow_utt);
  for (int i = 0; i < Mpad; ++i) row_utt[i] = -1;
  for (int i = 0; i < Mg; ++i) pos_rows[i] = 0;
  for (int i = 0; i < R; ++i) grow_utt[i] = -1;
  for (int b = 0; b < B; ++b) {
    const int rb = round_up(plan[b].T + 1, 16), rc = round_up(plan[b].T, 16);
    for (int t = 0; t < rc; ++t) row_utt[plan[b].row_off + t] = b;
    for (int t = 0; t < rb; ++t) {
      pos_rows[splan[b].row_off + t] = t < plan[b].T ? t : 0;
      grow_utt[2 * (splan[b].row_off + t)] = b;
      grow_utt[2 * (splan[b].row_off + t) + 1] = b;
    }
  }
  pb.upload(stream);
  const UttPlan *dp = pb.dev(s_plan), *dps = pb.dev(s_stem);
  const int32_t *d_blk_utt = pb.dev(s_blk_utt), *d_blk_f0 = pb.dev(s_blk_f0), *d_qb_utt = pb.dev(s_qb_utt), *d_qb_q0 = pb.dev(s_qb_q0);
  const int32_t *d_row_utt = pb.dev(s_row_utt), *d_pos_rows = pb.dev(s_pos_rows), *d_grow_utt = pb.dev(s_grow_utt);

  const size_t eT = sizeof(T);
  const void* d_aud = stage_audio(*this, d_audio, in, base0, offs[B] - base0);
  const int Rpad = R + 256;                                        // tile-edge + halo rows of the strided conv views
  d_mel.reserve((size_t)frames * c.n_mels * 4, stream);
  d_blkmax.reserve((size_t)n_fb * 4, stream);
  d_x0.reserve((size_t)(Rpad + 1) * c.n_mels * eT, stream);
  d_h1.reserve((size_t)Rpad * d * eT, stream);
  d_xa.reserve((size_t)Mpad * d * 4, stream);
  d_xb.reserve((size_t)Mpad * d * 4, stream);
  d_h.reserve((size_t)Mpad * d * eT, stream);
  d_qk.reserve((size_t)Mpad * 2 * d * eT, stream);
  d_vt.reserve((size_t)Mpad * d * eT, stream);
  d_ctx.reserve((size_t)Mpad * d * eT, stream);
  d_ffn.reserve(std::max((size_t)Mpad * dff * eT, (size_t)Mg * d * 4), stream);
  if (fp8_mm) { d_h8.reserve((size_t)Mpad * d, stream); d_ffn8.reserve((size_t)Mpad * dff, stream); }
  { void* before = d_cross.ptr; d_cross.reserve((size_t)2 * Ld * H * Mpad * 64 * eT, stream); if (d_cross.ptr != before) ++ws_epoch; }

  // ---- STFT power -> mel -> log10 (STFT_Process.py:224-246, Export_Whisper.py:424-425)
  {
    ProfScope ps(prof, "logmel", stream);
    const FbankArgs fa = fe.args(d_aud, in.dtype, dp, d_blk_utt, d_blk_f0, d_mel.as<float>(), d_blkmax.as<float>());
    launch_fbank(fa, n_fb, stream);
    // per-utterance max clamp + (x+4)/4, written behind one leading zero row (the conv view of row j starts at j-1)
    T* x0 = d_x0.as<T>();
    HIP_CHECK(hipMemsetAsync(x0, 0, (size_t)c.n_mels * eT, stream));
    // a padded K reads up to 63 elements behind a view's three rows; behind the last written row (R) they meet zero weights but must be finite
    if (k_conv1 > 3 * c.n_mels) HIP_CHECK(hipMemsetAsync(x0 + (size_t)(R + 1) * c.n_mels, 0, (size_t)4 * c.n_mels * eT, stream));
    launch_whisper_mel_finish<T>(d_mel.as<float>(), d_blkmax.as<float>(), dps, d_grow_utt, R, c.n_mels, x0 + c.n_mels, stream);
  }
  if (taps_enabled) save_tap("mel_gapped", d_x0.as<T>() + c.n_mels, R, c.n_mels, c.n_mels, (int)eT);
  // ---- conv stem as two GEMMs over strided views (no im2col): conv1 row j = frames j-1..j+1, conv2 row m = rows 2m..2m+2
  {
    ProfScope ps(prof, "conv_stem", stream);
    GemmArgs g1;
    g1.A = d_x0.ptr; g1.lda = c.n_mels; g1.W = conv1_w; g1.ldw = k_conv1; g1.M = R; g1.N = d; g1.K = k_conv1;
    g1.bias = conv1_b; g1.act = act; g1.out_lo = d_h1.ptr; g1.ld_out_lo = d;
    gemm(g1);
    launch_zero_gap_rows<T>(d_h1.as<T>(), d, d, dps, d_grow_utt, R, stream);     // conv2's zero padding
    // conv2's output rows live in the stem's row space (row m = gapped rows 2m .. 2m + 2); they land in the (still unused) FFN buffer and are
    // moved to the encoder's compact rows: every encoder GEMM then sees 16-row-aligned utterances without the pad row (8 s: 400, not 416)
    float* stem_out = d_ffn.as<float>();
    GemmArgs g2;
    g2.A = d_h1.ptr; g2.lda = 2 * d; g2.W = conv2_w; g2.ldw = 3 * d; g2.M = rows_g; g2.N = d; g2.K = 3 * d; g2.bias = conv2_b;
    g2.act = act; g2.add2 = enc_pos; g2.ld_add2 = d; g2.add2_rows = d_pos_rows; g2.out_f32 = stem_out; g2.ld_out_f32 = d;
    gemm(g2);
    launch_compact_rows(stem_out, dps, dp, d_row_utt, rows, d, d_xa.as<float>(), stream);
  }
  if (taps_enabled) save_tap("stem", d_xa.ptr, rows, d, d, 4);
  // ---- encoder layers (:430-437)
  float* xa = d_xa.as<float>();
  float* xb = d_xb.as<float>();
  T* h = d_h.as<T>();
  T* qk = d_qk.as<T>();
  T* vt = d_vt.as<T>();
  T* ctx = d_ctx.as<T>();
  T* ffn = d_ffn.as<T>();
  for (int i = 0; i < c.n_enc_layers; ++i) {
    const EncLayer& L = enc[i];
    { ProfScope ps(prof, "layernorm", stream); launch_layernorm<T>(xa, d, rows, d, nullptr, nullptr, 1e-5f, h, d, d, stream); }
    {
      ProfScope ps(prof, "gemm_qkv", stream);
      GemmArgs g;
      g.A = h; g.lda = d; g.W = L.wqkv; g.ldw = d; g.M = rows; g.N = 2 * d; g.K = d; g.bias = L.bqkv; g.out_lo = qk; g.ld_out_lo = 2 * d;
      gemm(g);
      GemmArgs gv;
      gv.A = h; gv.lda = d; gv.W = (const T*)L.wqkv + (size_t)2 * d * d; gv.ldw = d; gv.M = rows; gv.N = d; gv.K = d;
      gv.bias = L.bqkv + 2 * d; gv.out_t = vt; gv.ld_out_t = Mpad;
      gemm(gv);
    }
    {
      ProfScope ps(prof, "attention", stream);
      AttnArgs aa;
      aa.q = qk; aa.k = qk + d; aa.ld_qk = 2 * d; aa.vt = vt; aa.ld_vt = Mpad; aa.ctx = ctx; aa.ld_ctx = d; aa.plan = dp;
      aa.qb_utt = d_qb_utt; aa.qb_q0 = d_qb_q0; aa.n_qblocks = n_qb; aa.n_heads = H; aa.qt = att_qt; aa.n_waves = att_nw; aa.max_T = max_T;
      if (precision == ASR_PRECISION_BF16) launch_attention_bf16_hd64(aa, stream);
      else launch_attention_f32(aa, c.d_head, stream);
    }
    {
      ProfScope ps(prof, "gemm_out", stream);
      GemmArgs g;
      g.A = ctx; g.lda = d; g.W = L.wo; g.ldw = d; g.M = rows; g.N = d; g.K = d; g.bias = L.bo; g.add = xa; g.ld_add = d;
      g.out_f32 = xb; g.ld_out_f32 = d;
      gemm(g);
    }
    if (fp8_mm && sizeof(T) == 2) {                       // FFN pair on the FP8 matrix pipe: e4m3 operand rows, twice the bf16 MFMA rate
      { ProfScope ps(prof, "layernorm", stream); launch_layernorm_fp8(xb, d, rows, d, 1e-5f, 1.0f, d_h8.as<unsigned char>(), d, stream); }
      {
        ProfScope ps(prof, "gemm_ffn1", stream);
        Fp8GemmArgs g;
        g.A = d_h8.as<unsigned char>(); g.lda = d; g.W = enc8[i].w1; g.ldw = d; g.M = rows; g.N = dff; g.K = d; g.w_scale = enc8[i].s1; g.bias = L.b1;
        g.act = act; g.out8 = d_ffn8.as<unsigned char>(); g.ld_out8 = dff;
        g.out_inv_scale = ldexpf(1.0f, -fp8_act_shift); g.sat_count = d_sat.as<unsigned long long>();
        launch_gemm_fp8(g, stream);
      }
      {
        ProfScope ps(prof, "gemm_ffn2", stream);
        Fp8GemmArgs g;
        g.A = d_ffn8.as<unsigned char>(); g.lda = dff; g.W = enc8[i].w2; g.ldw = dff; g.M = rows; g.N = d; g.K = dff; g.w_scale = enc8[i].s2; g.bias = L.b2;
        g.a_scale = ldexpf(1.0f, fp8_act_shift);
        g.add = xb; g.ld_add = d; g.out_f32 = xa; g.ld_out_f32 = d;
        launch_gemm_fp8(g, stream);
      }
      if (taps_enabled) save_tap(("enc" + std::to_string(i)).c_str(), xa, rows, d, d, 4);
      continue;
    }
    { ProfScope ps(prof, "layernorm", stream); launch_layernorm<T>(xb, d, rows, d, nullptr, nullptr, 1e-5f, h, d, d, stream); }
    {
      ProfScope ps(prof, "gemm_ffn1", stream);
      GemmArgs g;
      g.A = h; g.lda = d; g.W = L.w1; g.ldw = d; g.M = rows; g.N = dff; g.K = d; g.bias = L.b1; g.act = act; g.out_lo = ffn; g.ld_out_lo = dff;
      gemm(g);
    }
    {
      ProfScope ps(prof, "gemm_ffn2", stream);
      GemmArgs g;
      g.A = ffn; g.lda = dff; g.W = L.w2; g.ldw = dff; g.M = rows; g.N = d; g.K = dff; g.bias = L.b2; g.add = xb; g.ld_add = d;
      g.out_f32 = xa; g.ld_out_f32 = d;
      gemm(g);
    }
    if (taps_enabled) save_tap(("enc" + std::to_string(i)).c_str(), xa, rows, d, d, 4);    // the f32 residual stream behind layer i (tests/whisper_layers_ref.py)
  }
  // ---- final LayerNorm + fused cross-KV projection into [kv][layer][head] slabs of [row][64] (:438-447)
  if (taps_enabled) {
    launch_layernorm<float>(xa, d, rows, d, enc_ln_g, enc_ln_b, 1e-5f, xb, d, d, stream);
    save_tap("enc_out", xb, rows, d, d, 4);
  }
  { ProfScope ps(prof, "layernorm", stream); launch_layernorm<T>(xa, d, rows, d, enc_ln_g, enc_ln_b, 1e-5f, h, d, d, stream); }
  {
    ProfScope ps(prof, "gemm_crosskv", stream);
    GemmArgs g;
    g.A = h; g.lda = d; g.W = ckv_w; g.ldw = d; g.M = rows; g.N = 2 * Ld * d; g.K = d; g.bias = ckv_b;
    g.out_lo = d_cross.ptr; g.lo_group = 64; g.ld_out_lo = Mpad * 64;
    gemm(g);
  }
  if constexpr (sizeof(T) == 2) {
    if (fp8 && fp8_kv) {
      ProfScope ps(prof, "quant_crosskv", stream);
      { void* before = d_cross8.ptr; void* before_s = d_cscale.ptr;      // either buffer moving invalidates the captured decode graph (the scales grow with B, the bytes with the rows)
        d_cross8.reserve((size_t)2 * Ld * H * Mpad * 64, stream); d_cscale.reserve((size_t)2 * Ld * H * B * 4, stream);
        if (d_cross8.ptr != before || d_cscale.ptr != before_s) ++ws_epoch; }
      launch_quantize_crosskv_fp8(d_cross.as<bf16_t>(), (size_t)Mpad * 64, 2 * Ld * H, dp, B, d_cross8.as<unsigned char>(), d_cscale.as<float>(),
                                  fp8_fake ? 1 : 0, stream);
    }
  }
  if (taps_enabled) save_tap("cross", d_cross.ptr, (int64_t)2 * Ld * H * Mpad, 64, 64, (int)eT);
  HIP_CHECK(hipStreamSynchronize(stream));
  if (prof.enabled) prof.collect();
}

// ======================================================================================== decoder step
// All launches of one step. `hist_dev` (device-resident history length) is what the kernels read, so the single-token
// step is position independent and ONE captured hipGraph replays for every decode position.
// Beam search (bs set, n = beam): the R = B * beam rows are hypotheses, one new position each (bs->hist); the self-attention follows every row's
// ancestry through the row extents, the cross-attention reads each utterance's slab once for its n = beam rows (the prefill's form), and the head
// ranks the rows' extensions instead of taking an arg-max.
// prompt: a prefill of left-padded prompts (pad_host of step()): n may exceed 8 and both attentions run on the prompt-attention kernel (csrc/prompt_attn.hip).
template <typename T>
void WhSession::enqueue_step(const int32_t* ids_dev, int n, bool is_prefill, bool use_hist_dev, const BeamStep* bs, bool prompt) {
  const auto& c = cfg;
  const int B = batch, d = c.d_model, dff = c.d_ffn, Ld = c.n_dec_layers, H = c.n_heads;
  const int R = B * n, Rp = round_up(R, 128);
  const int32_t* hd = bs ? bs->hist : use_hist_dev ? d_hist.as<int32_t>() : nullptr;
  float* xa = d_dx.as<float>();
  float* xb = xa + (size_t)Rp * d;
  float* xc = xb + (size_t)Rp * d;
  T* qkv = d_dqkv.as<T>();
  T* hh = qkv + (size_t)Rp * 3 * d;
  T* ctx = hh + (size_t)Rp * d;
  T* ffn = ctx + (size_t)Rp * d;
  T* cq = ffn + (size_t)Rp * dff;
  T* hl = cq + (size_t)Rp * d;
  const UttPlan* dp = d_plan.as<UttPlan>();              // (the first section of the blob encode() uploaded: the encoder-row plans)
  const size_t cache_l = (size_t)B * H * c.max_target_positions * 64;
  // bf16 mode, M <= 64 rows: the (affine-less) LayerNorm runs inside the skinny GEMM's prologue
  const bool fuse_ln = precision == ASR_PRECISION_BF16 && R <= 32 && d % 256 == 0;   // above 32 rows a separate LayerNorm launch is cheaper
  auto ln_gemm = [&](const float* x, GemmArgs& g) {
    // the prologue's registers / LDS hold one workgroup per CU: outputs wider than the chip (N / 16 > 256 workgroups, fc1) are faster
    // behind a separate LayerNorm launch, with two plain workgroups sharing a CU
    if (fuse_ln && (R <= 16 || g.N / 16 <= 256)) { g.A = nullptr; g.ln_x = x; g.ld_ln_x = d; }
    else { ProfScope ps(prof, "dec_layernorm", stream); launch_layernorm<T>(x, d, R, d, nullptr, nullptr, 1e-5f, hh, d, d, stream); g.A = hh; g.lda = d; }
    ProfScope ps(prof, "dec_gemm", stream);
    gemm(g);
  };
  // bf16 decode steps of <= 64 rows: the decode GEMM (csrc/decode_gemm.hip) with the three LayerNorms folded into q|k|v, cross-q and fc1
  bool dgm = false;
  bf16_t *xa_lo = nullptr, *xb_lo = nullptr, *xc_lo = nullptr;
  const float* csum = d_colsum.as<float>();
  const size_t cs_l = (size_t)3 * d + d + dff;
  if constexpr (sizeof(T) == 2) {
    dgm = use_decode_gemm && R <= 64 && d_colsum.ptr != nullptr && d % 256 == 0 && dff % 256 == 0;
    xa_lo = d_dlo.as<bf16_t>(); xb_lo = xa_lo + (size_t)Rp * d; xc_lo = xb_lo + (size_t)Rp * d;
  }
  const bool w8 = fp8 && fp8_weights && !fp8_fake;
  // (Round 5 also cut the batch into sub-batches whose layer loops ran on one stream each ("decode chains"): 3.29 vs 3.31 ms per token at 64 sequences,
  //  slower at 32 -- profiles/r05_whisper_decode_chains.txt; removed in round 6.)
  sk.ensure(stream);
  const int plan_rows = 0, NC = 1;
  auto dg = [&](hipStream_t st, int ci, int r0, int Rc, int layer, const void* A, int lda, const void* Wt, int wi, int N, int K, const float* bias, const float* colsum,
                const float* add, int act_, float* of32, void* olo, int ld_lo) {
    ProfScope ps(prof, "dec_gemm", st);
    DecGemmArgs g;
    g.A = (const bf16_t*)A + (size_t)r0 * lda; g.lda = lda; g.W = (const bf16_t*)Wt; g.ldw = K; g.M = Rc; g.plan_M = plan_rows; g.N = N; g.K = K; g.bias = bias; g.colsum = colsum;
    if (w8) { g.W = nullptr; dec8.select(g, layer, wi); }
    g.add = add ? add + (size_t)r0 * d : nullptr; g.ld_add = d; g.act = act_; g.out_f32 = of32 ? of32 + (size_t)r0 * d : nullptr; g.ld_out_f32 = d;
    g.out_lo = olo ? (bf16_t*)olo + (size_t)r0 * ld_lo : nullptr; g.ld_out_lo = ld_lo;
    g.ws = reinterpret_cast<float*>(static_cast<unsigned char*>(sk.ws.ptr) + (size_t)ci * SplitKGemm::WS_BYTES); g.ws_bytes = SplitKGemm::WS_BYTES;
    g.cnt = sk.cnt.as<int32_t>() + (size_t)ci * SplitKGemm::TICKETS;
    launch_decode_gemm(g, st);
  };
  // embedding + layer loop of sequences [b0, b0 + nb) on stream `st` (chain ci)
  auto run_chain = [&](hipStream_t st, int ci, int b0, int nb) {
    const int r0 = b0 * n, Rc = nb * n;
    { ProfScope ps(prof, "dec_embed", st);
      launch_embed_pos<T>(ids_dev + r0, Rc, bs ? 1 : n, hist, hd, (const T*)embed, dec_pos, d, xa + (size_t)r0 * d, st, kstart(), bs ? bs->beam : n);
      if (dgm) launch_rows_to_bf16(xa + (size_t)r0 * d, xa_lo + (size_t)r0 * d, (size_t)(NC == 1 ? Rp : Rc) * d, st); }
    if (taps_enabled) save_tap("dec_in", xa, R, d, d, 4);     // (a tapped step is never captured: `graphable` in step())
    for (int l = 0; l < Ld; ++l) {
      const DecLayer& L = dec[l];
      if (dgm) dg(st, ci, r0, Rc, l, xa_lo, d, L.wqkv, 0, 3 * d, d, L.bqkv, csum + l * cs_l, nullptr, ACT_NONE, nullptr, qkv, 3 * d);
      else {
        GemmArgs g;
        g.W = L.wqkv; g.ldw = d; g.M = R; g.N = 3 * d; g.K = d; g.bias = L.bqkv; g.out_lo = qkv; g.ld_out_lo = 3 * d;
        ln_gemm(xa, g);
      }
      {
        ProfScope ps(prof, "dec_self_attn", st);
        DecAttnArgs a{};                                   // (zeroed: the paged form sets no strides, and the prompt-attention launcher checks their alignment)
        a.q = qkv; a.ld_q = 3 * d; a.q_col0 = 0; a.kv_new = qkv; a.ld_new = 3 * d; a.k_col0 = d; a.v_col0 = 2 * d;
        if (bs) {
          T* ext = d_bext.as<T>() + (size_t)l * R * 2 * H * bs->S * 64;
          a.k_base = ext; a.v_base = ext + (size_t)H * bs->S * 64;
          a.stride_b = (int64_t)2 * H * bs->S * 64; a.stride_h = (int64_t)bs->S * 64;
          a.beam_src = bs->src; a.ld_src = bs->ld_src; a.beam_p0 = bs->p0; a.beam = bs->beam; a.key_start = kstart();
          a.plan = nullptr; a.hist = 0; a.hist_dev = hd; a.n = 1; a.n_heads = H; a.causal = 1; a.out = ctx; a.ld_out = d;
          a.max_keys = c.max_target_positions;
          launch_decode_attention<T>(a, R, st);
        } else {
        if (kv_paged) {
          a.k_base = d_kvpool.as<T>() + (size_t)(l * 2) * H * KV_PAGE * 64; a.v_base = d_kvpool.as<T>() + (size_t)(l * 2 + 1) * H * KV_PAGE * 64;
          a.page_table = d_ptable.as<int32_t>(); a.pages_per_seq = (c.max_target_positions + KV_PAGE - 1) / KV_PAGE;
          a.page_stride = (int64_t)Ld * 2 * H * KV_PAGE * 64;
        } else {
          a.k_base = d_kc.as<T>() + l * cache_l; a.v_base = d_vc.as<T>() + l * cache_l;
          a.stride_b = (int64_t)H * c.max_target_positions * 64; a.stride_h = (int64_t)c.max_target_positions * 64;
        }
        a.plan = nullptr; a.hist = hist; a.hist_dev = hd; a.n = n; a.n_heads = H; a.causal = 1; a.out = ctx; a.ld_out = d;
        a.max_keys = c.max_target_positions;
        a.b0 = b0;
        if (prompt) {                                      // left-padded prompt rows (history 0): all n K / V rows go to the cache, row i sees slots pad[b] .. i
          PromptAttnArgs pa;
          pa.q = qkv; pa.ld_q = 3 * d; pa.kv_new = qkv; pa.ld_new = 3 * d; pa.k_col0 = d; pa.v_col0 = 2 * d;
          pa.k_base = a.k_base; pa.v_base = a.v_base; pa.stride_b = a.stride_b; pa.stride_h = a.stride_h;
          pa.page_table = a.page_table; pa.pages_per_seq = a.pages_per_seq; pa.page_stride = a.page_stride;
          pa.key_start = kstart(); pa.n = n; pa.n_heads = H; pa.out = ctx; pa.ld_out = d;
          launch_prompt_attention<T>(pa, nb, st);
        } else {
          a.key_start = kstart();
          launch_decode_attention<T>(a, nb, st);
        }
        }
      }
      if (dgm) {
        dg(st, ci, r0, Rc, l, ctx, d, L.wo, 1, d, d, L.bo, nullptr, xa, ACT_NONE, xb, xb_lo, d);
        dg(st, ci, r0, Rc, l, xb_lo, d, L.wcq, 2, d, d, L.bcq, csum + l * cs_l + 3 * d, nullptr, ACT_NONE, nullptr, cq, d);
      } else {
        {
          ProfScope ps(prof, "dec_gemm", stream);
          GemmArgs g;
          g.A = ctx; g.lda = d; g.W = L.wo; g.ldw = d; g.M = R; g.N = d; g.K = d; g.bias = L.bo; g.add = xa; g.ld_add = d; g.out_f32 = xb; g.ld_out_f32 = d;
          gemm(g);
        }
        GemmArgs g;
        g.W = L.wcq; g.ldw = d; g.M = R; g.N = d; g.K = d; g.bias = L.bcq; g.out_lo = cq; g.ld_out_lo = d;
        ln_gemm(xb, g);
      }
      if (wts_on && !bs && wts_count[l]) {                 // word timestamps: this layer's selected heads, the step's last query row against the bf16 (f32) K slab
        ProfScope ps(prof, "align_scores", st);
        AlignScoresArgs a;
        a.q = cq; a.ld_q = d; a.n = n; a.k_base = d_cross.as<T>() + (size_t)(0 * Ld + l) * H * Mpad * 64; a.stride_h = (int64_t)Mpad * 64; a.plan = dp;
        a.sel = d_wsel.as<int32_t>() + 2 * wts_first[l]; a.n_sel = wts_count[l]; a.pos_dev = d_hist.as<int32_t>(); a.row_bias = n - 1 - wts_p0;
        a.out = d_wscores.as<float>(); a.n_pairs = n_pairs(); a.max_rows = wts_max_rows; a.ld = wts_ld; a.max_keys = max_T_enc;
        launch_align_scores<T>(a, B, st);
      }
      {
        ProfScope ps(prof, "dec_cross_attn", st);
        DecAttnArgs a;
        a.q = cq; a.ld_q = d; a.q_col0 = 0; a.kv_new = nullptr; a.ld_new = 0; a.k_col0 = a.v_col0 = 0;
        a.k_base = d_cross.as<T>() + (size_t)(0 * Ld + l) * H * Mpad * 64;
        a.v_base = d_cross.as<T>() + (size_t)(1 * Ld + l) * H * Mpad * 64;
        a.stride_b = 0; a.stride_h = (int64_t)Mpad * 64; a.plan = dp; a.hist = 0; a.hist_dev = nullptr; a.n = n; a.n_heads = H; a.causal = 0;
        a.max_keys = max_T_enc;
        a.out = ctx; a.ld_out = d;
        if (fp8 && fp8_kv && !fp8_fake) {
          a.k_base = d_cross8.as<unsigned char>() + (size_t)(0 * Ld + l) * H * Mpad * 64;
          a.v_base = d_cross8.as<unsigned char>() + (size_t)(1 * Ld + l) * H * Mpad * 64;
          a.k_scale = d_cscale.as<float>() + (size_t)(0 * Ld + l) * H * B; a.v_scale = d_cscale.as<float>() + (size_t)(1 * Ld + l) * H * B;
        }
        a.b0 = b0; a.scale_ld = B;
        if (prompt) {
          PromptAttnArgs pa;
          pa.q = cq; pa.ld_q = d; pa.k_base = a.k_base; pa.v_base = a.v_base; pa.stride_h = a.stride_h; pa.plan = dp;
          pa.key_start = kstart(); pa.n = n; pa.n_heads = H; pa.out = ctx; pa.ld_out = d;
          launch_prompt_attention<T>(pa, nb, st);
        } else {
          launch_decode_attention<T>(a, nb, st);
        }
      }
      if (dgm) {
        dg(st, ci, r0, Rc, l, ctx, d, L.wco, 3, d, d, L.bco, nullptr, xb, ACT_NONE, xc, xc_lo, d);
        dg(st, ci, r0, Rc, l, xc_lo, d, L.w1, 4, dff, d, L.b1, csum + l * cs_l + 4 * d, nullptr, act, nullptr, ffn, dff);
        if (Rc <= 32 || w8) dg(st, ci, r0, Rc, l, ffn, dff, L.w2, 5, d, dff, L.b2, nullptr, xc, ACT_NONE, xa, xa_lo, d);
        else {               // 33..64 rows: the tiled split-K pass shares the activation rows across 64 columns (13.8 vs 17.9 us); it writes the bf16 copy too (one chain only: Rc = R)
          ProfScope ps(prof, "dec_gemm", stream);
          GemmArgs g2;
          g2.A = ffn; g2.lda = dff; g2.W = L.w2; g2.ldw = dff; g2.M = R; g2.N = d; g2.K = dff; g2.bias = L.b2; g2.add = xc; g2.ld_add = d;
          g2.out_f32 = xa; g2.ld_out_f32 = d; g2.out_lo = xa_lo; g2.ld_out_lo = d;
          gemm(g2);
        }
      } else {
        {
          ProfScope ps(prof, "dec_gemm", stream);
          GemmArgs g;
          g.A = ctx; g.lda = d; g.W = L.wco; g.ldw = d; g.M = R; g.N = d; g.K = d; g.bias = L.bco; g.add = xb; g.ld_add = d; g.out_f32 = xc; g.ld_out_f32 = d;
          gemm(g);
        }
        GemmArgs g;
        g.W = L.w1; g.ldw = d; g.M = R; g.N = dff; g.K = d; g.bias = L.b1; g.act = act; g.out_lo = ffn; g.ld_out_lo = dff;
        ln_gemm(xc, g);
        ProfScope ps(prof, "dec_gemm", stream);
        GemmArgs g2;
        g2.A = ffn; g2.lda = dff; g2.W = L.w2; g2.ldw = dff; g2.M = R; g2.N = d; g2.K = dff; g2.bias = L.b2; g2.add = xc; g2.ld_add = d;
        g2.out_f32 = xa; g2.ld_out_f32 = d;
        gemm(g2);
      }
      if (taps_enabled) save_tap(("dec" + std::to_string(l)).c_str(), xa, R, d, d, 4);     // the f32 residual stream behind layer l, all R rows
    }
  };
  run_chain(stream, 0, 0, B);
  // final LayerNorm of the LAST position of every sequence, tied proj_out, -128 suppress penalty (:663-666)
  {
    ProfScope ps(prof, "dec_logits", stream);
    const int Ml = bs ? R : B, nl = bs ? 1 : n;           // beam search: every hypothesis row is a last position
    float* lg = bs ? bs->logits : d_logits.as<float>();
    GemmArgs g;
    g.W = embed; g.ldw = d; g.M = Ml; g.N = vpad; g.K = d; g.bias = suppress; g.out_f32 = lg; g.ld_out_f32 = vpad;
    // up to 16 sequences: LayerNorm inside the weight-streaming GEMM; above, a separate LayerNorm feeds the 128 x 128 tiles (every 16-column
    // granule of the streaming kernel would re-read all B activation rows: 170 us for 32 x 51 866 x 1280 against ~45)
    if (precision == ASR_PRECISION_BF16 && Ml <= 16 && d % 256 == 0) {
      g.ln_x = xa + (size_t)(nl - 1) * d; g.ld_ln_x = nl * d; g.ln_gamma = dec_ln_g; g.ln_beta = dec_ln_b;
    } else {
      launch_layernorm<T>(xa + (size_t)(nl - 1) * d, nl * d, Ml, d, dec_ln_g, dec_ln_b, 1e-5f, hl, d, d, stream);
      g.A = hl; g.lda = d;
    }
    gemm(g);
    if (bs) {                              // rank the rows' extensions; the select pass writes the ids of the next step and the ancestry of this one
      ProfScope pr(prof, "beam_rank", stream);
      ranker.enqueue_rank(lg, vpad, c.vocab, 0, stream);
      launch_add_scalar(bs->hist, 1, stream);
      return;
    }
    // BEGIN_SUPPRESS (-inf on begin_suppress_tokens) applies to the head after a prefill only (:228-240); the history is empty there (:312-325)
    head.enqueue(d_logits.as<float>(), vpad, B, c.vocab, is_prefill ? begin : nullptr, !is_prefill, d_next.as<int32_t>(), stream);
    launch_add_scalar(d_hist.as<int32_t>(), n, stream);
  }
}

// Block table + pool of the paged self-KV cache: make sure every sequence of the batch owns pages for `positions` positions. Growth appends whole
// generations (page ids j * B + slot, slot = b or -- tests -- a permutation of the batch), copies the old pool (a prefix of the new one), rewrites the table and
// invalidates the captured decode graph; with the first cut at prompt + 48 positions and doubling, a 448-position generation regrows at most three times.
void WhSession::ensure_kv_pages(int B, int positions, size_t elem_bytes) {
  const auto& c = cfg;
  const int P = (c.max_target_positions + KV_PAGE - 1) / KV_PAGE;
  const int need = std::min(P, (positions + KV_PAGE - 1) / KV_PAGE);
  if (B != kv_batch) { kv_gens = 0; kv_batch = B; }                       // another batch: the cache restarts with its prefill
  if (need <= kv_gens && d_kvpool.ptr && d_ptable.ptr) return;
  const int gens = std::min(P, std::max(need, kv_gens ? 2 * kv_gens : (positions + 48 + KV_PAGE - 1) / KV_PAGE));
  const size_t page_bytes = (size_t)c.n_dec_layers * 2 * c.n_heads * KV_PAGE * 64 * elem_bytes;
  const size_t bytes = (size_t)gens * B * page_bytes, old_bytes = std::min(d_kvpool.cap, (size_t)kv_gens * B * page_bytes);
  if (bytes > d_kvpool.cap) {
    DeviceBuffer fresh;
    fresh.reserve(bytes, stream);
    if (hist > 0 && old_bytes) HIP_CHECK(hipMemcpyAsync(fresh.ptr, d_kvpool.ptr, old_bytes, hipMemcpyDeviceToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    d_kvpool = std::move(fresh);
  }
  d_ptable.reserve((size_t)B * P * 4, stream);
  h_io.reserve((size_t)B * P * 4 + 64);
  int32_t* tab = h_io.as<int32_t>();
  for (int b = 0; b < B; ++b)
    for (int j = 0; j < P; ++j) tab[(size_t)b * P + j] = j < gens ? j * B + (kv_shuffle ? (B - 1 - b + j) % B : b) : -1;
  HIP_CHECK(hipMemcpyAsync(d_ptable.ptr, tab, (size_t)B * P * 4, hipMemcpyHostToDevice, stream));
  HIP_CHECK(hipStreamSynchronize(stream));                                 // (the pinned staging buffer is reused by the step that follows)
  kv_gens = gens;
  ++ws_epoch;
}

template <typename T>
void WhSession::step(const int32_t* ids_host, int n, bool is_prefill, int32_t* next_out, float* logits_out, const int32_t* pad_host) {
  const auto& c = cfg;
  ASR_REQUIRE(batch > 0, "whisper: encode a batch before prefill / decode");
  const bool prompt = pad_host != nullptr;       // left-padded prompts: [B][n] ids with pad_host[b] pad slots in front (prefill_prompts)
  ASR_REQUIRE(!prompt || (is_prefill && ids_host), "whisper: left-padded prompts belong to a prefill");
  ASR_REQUIRE(n >= 1 && n <= (prompt ? c.max_target_positions : 8), "whisper: %d tokens per step (1..%d)", n, prompt ? c.max_target_positions : 8);
  if (is_prefill) { hist = 0; kstart_on = false; }   // the reference always prefills with an empty self-KV (:476-480)
  ASR_REQUIRE(hist + n <= c.max_target_positions, "whisper: %d positions exceed max_target_positions %d", hist + n, c.max_target_positions);
  HIP_CHECK(hipSetDevice(device));
  const int B = batch, d = c.d_model, dff = c.d_ffn, Ld = c.n_dec_layers, H = c.n_heads;
  const int R = B * n, Rp = round_up(R, 128), Bp = round_up(B, 128);
  const size_t eT = sizeof(T);
  const size_t cache_elems = (size_t)Ld * B * H * c.max_target_positions * 64;
  auto grow = [&](DeviceBuffer& buf, size_t bytes) { void* before = buf.ptr; buf.reserve(bytes, stream); if (buf.ptr != before) ++ws_epoch; };
  if (kv_paged) ensure_kv_pages(B, hist + n, eT);
  else { grow(d_kc, cache_elems * eT); grow(d_vc, cache_elems * eT); }
  grow(d_ids, (size_t)B * std::max(n, 8) * 4);
  grow(d_next, (size_t)B * 4);
  grow(d_hist, 256);
  head.reserve(B, stream);
  grow(d_logits, (size_t)Bp * vpad * 4);
  grow(d_dx, (size_t)3 * Rp * d * 4);                  // three f32 residual-stream buffers
  if (precision == ASR_PRECISION_BF16) grow(d_dlo, (size_t)3 * Rp * d * 2);     // ... and their bf16 copies (operands of the LayerNorm-folded projections)
  grow(d_dqkv, (size_t)Rp * (3 * d + d + d + dff + d) * eT + (size_t)Bp * d * eT);
  if (wts_on) {
    ASR_REQUIRE(is_prefill || n == 1, "whisper: word-timestamp capture takes one position per decode step (%d given)", n);
    ASR_REQUIRE(is_prefill || wts_p0 >= 0, "whisper: word-timestamp capture starts at a prefill (none since the mode was switched on or the batch was encoded)");
    if (is_prefill) { wts_p0 = n - 1; wts_rows = 0; wts_consumed = false; wts_ld = round_up(max_T_enc, 16); }
    grow(d_wscores, (size_t)B * n_pairs() * wts_max_rows * wts_ld * 4);
  }
  const int32_t* ids_dev;
  if (ids_host) {
    h_io.reserve((size_t)(R + B) * 4 + 64);
    int32_t* stage = h_io.as<int32_t>();
    for (int i = 0; i < R; ++i) {
      ASR_REQUIRE(ids_host[i] >= 0 && ids_host[i] < c.vocab, "whisper: token id %d out of range", ids_host[i]);
      stage[i] = ids_host[i];
    }
    HIP_CHECK(hipMemcpyAsync(d_ids.ptr, stage, (size_t)R * 4, hipMemcpyHostToDevice, stream));
    ids_dev = d_ids.as<int32_t>();
  } else {
    ASR_REQUIRE(n == 1, "whisper: device-resident ids feed single-token decode steps only");
    ids_dev = d_next.as<int32_t>();
  }
  if (is_prefill) {
    HIP_CHECK(hipMemsetAsync(d_hist.ptr, 0, 4, stream));
    head.restart(stream);
  }
  if (prompt) {                                    // pad[b] behind the ids in the staging buffer (the copies above and here are ordered on the stream)
    grow(d_kstart, (size_t)std::max(B, 64) * 4);
    int32_t* stage = h_io.as<int32_t>() + R;
    for (int b = 0; b < B; ++b) stage[b] = pad_host[b];
    HIP_CHECK(hipMemcpyAsync(d_kstart.ptr, stage, (size_t)B * 4, hipMemcpyHostToDevice, stream));
    kstart_on = true;
  }
  // single-token steps fed from the device are position independent => one graph for all of them
  const bool graphable = use_graph && !ids_host && n == 1 && !taps_enabled && !prof.enabled && !head.noise_armed;
  GraphKey gk;
  gk.mix((uint64_t)B).mix((uint64_t)Mpad).mix(ws_epoch).mix(head.epoch).mix(stream);
  if (kstart_on) gk.mix((uint64_t)2).mix(d_kstart.ptr);                              // the single-token forms with key_start, and the pointer they read
  if (wts_on) gk.mix((uint64_t)1).mix(wts_epoch).mix((uint64_t)wts_p0).mix((uint64_t)wts_max_rows).mix((uint64_t)wts_ld).mix(d_wscores.ptr);      // what the capture bakes in
  const uint64_t key = gk.h;
  dec_graph.run(stream, graphable, key, [&] { enqueue_step<T>(ids_dev, n, is_prefill, true, nullptr, prompt); });
  if (wts_on) wts_rows = std::min(wts_rows + 1, wts_max_rows);
  hist += n;
  head.consumed();
  if (taps_enabled) save_tap("logits", d_logits.ptr, B, c.vocab, vpad, 4);
  if (next_out || logits_out) {
    download_step(h_io, d_next.ptr, d_logits.ptr, vpad, B, c.vocab, next_out, logits_out, stream);
    if (prof.enabled) prof.collect();
  }
}

// Prefill with one prompt per sequence (asr_whisper_prefill_prompts): equal lengths of at most 8 ids are the plain prefill; anything else is prefilled as
// max(len) left-padded slots per sequence. A pad slot is staged with id 0 at position 0: it only has to read inside the tables, no real row attends it.
void WhSession::prefill_prompts(const int32_t* ids, const int32_t* offsets, int32_t* next_out, float* logits_out) {
  const auto& c = cfg;
  ASR_REQUIRE(batch > 0, "whisper: encode a batch before prefill / decode");
  const int B = batch;
  ASR_REQUIRE(offsets[0] >= 0, "whisper_prefill_prompts: offsets[0] = %d is negative", offsets[0]);
  int n = 0, n_min = c.max_target_positions + 1;
  for (int b = 0; b < B; ++b) {
    ASR_REQUIRE(offsets[b + 1] > offsets[b], "whisper_prefill_prompts: offsets must ascend and every prompt needs at least one id (offsets[%d] = %d, offsets[%d] = %d)",
                b, offsets[b], b + 1, offsets[b + 1]);
    const int len = offsets[b + 1] - offsets[b];
    ASR_REQUIRE(len <= c.max_target_positions, "whisper_prefill_prompts: prompt %d has %d ids, max_target_positions is %d", b, len, c.max_target_positions);
    n = std::max(n, len); n_min = std::min(n_min, len);
  }
  const bool bf = precision == ASR_PRECISION_BF16;
  if (n == n_min && n <= 8) {                                      // uniform and short: the existing prefill, bit for bit
    if (bf) step<bf16_t>(ids + offsets[0], n, true, next_out, logits_out);
    else step<float>(ids + offsets[0], n, true, next_out, logits_out);
    return;
  }
  ASR_REQUIRE(!fp8, "whisper_prefill_prompts: FP8W / FP8MM / MXFP4W sessions take equal prompt lengths of at most 8 ids (their cross-K/V slabs are e4m3; "
                    "prompts of %d..%d ids need an F32 or BF16 session)", n_min, n);
  std::vector<int32_t> padded((size_t)B * n, 0), pad(B);
  for (int b = 0; b < B; ++b) {
    const int len = offsets[b + 1] - offsets[b];
    pad[b] = n - len;
    memcpy(padded.data() + (size_t)b * n + pad[b], ids + offsets[b], (size_t)len * 4);
  }
  if (bf) step<bf16_t>(padded.data(), n, true, next_out, logits_out, pad.data());
  else step<float>(padded.data(), n, true, next_out, logits_out, pad.data());
}

// Beam search after a prefill (semantics of oracle/qwen_asr_oracle.py:beam_search_core, stop set {eos_id}): the first ranking reads the prefill's logits + BEGIN_SUPPRESS,
// then every step is one decoder pass over the B * beam hypothesis rows at the same position. The prompt's K / V rows are copied once into every row's
// extent; generated positions stay in the extent of the row that computed them and the self-attention follows each row's ancestry table, so nothing is
// copied or re-ordered between steps. The cross-attention reads an utterance's slab once per step for all its rows. Ids, scores and tables stay on the
// device; the host reads back the per-utterance "best hypothesis has ended" flags once per step. The step replays from a captured graph (one per table parity).
// Output: per utterance its `beam` hypotheses best-first -- tokens_out [B][beam][max_new], n_out [B][beam], scores_out [B][beam] (nullable).
template <typename T>
void WhSession::beam_search(int beam, int max_new, int eos_id, int32_t* tokens_out, int32_t* n_out, float* scores_out) {
  const auto& c = cfg;
  ASR_REQUIRE(after_prefill && batch > 0 && hist > 0 && d_logits.ptr, "whisper_beam_search: prefill first");
  ASR_REQUIRE(beam >= 1 && beam <= BEAM_MAX, "whisper_beam_search: beam width %d outside 1..%d", beam, BEAM_MAX);
  ASR_REQUIRE(head.plain(), "whisper_beam_search: the penalty / sampling heads do not combine with beam search");     // (the timestamp rules do: they run before every ranking)
  ASR_REQUIRE(!wts_on, "whisper_beam_search: word-timestamp capture is on; align a beam's hypothesis with a forced pass over its ids after the search");
  ASR_REQUIRE(hist + max_new <= c.max_target_positions, "whisper_beam_search: %d prompt + %d new positions exceed max_target_positions %d", hist, max_new,
              c.max_target_positions);
  HIP_CHECK(hipSetDevice(device));
  const int B = batch, N = B * beam, p0 = hist, d = c.d_model, dff = c.d_ffn, Ld = c.n_dec_layers, H = c.n_heads;
  const int S = p0 + max_new - 1, ld = max_new;           // extent slots (positions ever written), stride of the ancestry / token tables
  const int Rp = round_up(N, 128);
  const size_t eT = sizeof(T);
  auto grow = [&](DeviceBuffer& buf, size_t bytes) { if (reserve_moved(buf, bytes, stream)) ++ws_epoch; };
  grow(d_bhist, 256);
  grow(d_bext, (size_t)Ld * N * 2 * H * S * 64 * eT);
  grow(d_blogits, (size_t)Rp * vpad * 4);
  grow(d_dx, (size_t)3 * Rp * d * 4);
  if (precision == ASR_PRECISION_BF16) grow(d_dlo, (size_t)3 * Rp * d * 2);
  grow(d_dqkv, (size_t)Rp * (3 * d + d + d + dff + d) * eT + (size_t)Rp * d * eT);
  const int n_stop = eos_id >= 0 ? 1 : 0;
  ranker.begin(B, beam, ld, &eos_id, n_stop, head.ts, head.hot_view("whisper_beam_search"), stream, head.lm, "whisper_beam_search");
  HIP_CHECK(hipMemcpyAsync(d_bhist.ptr, d_hist.ptr, 4, hipMemcpyDeviceToDevice, stream));      // the rows' position: the prompt length p0 the prefill left
  // ---- first ranking: the prefill's logits (B rows, left in place) + BEGIN_SUPPRESS, as the arg-max head after a prefill. In timestamp mode the head has
  // already masked them by the initial rule; the ranker applies it again, which changes nothing.
  ranker.rank_first(d_logits.as<float>(), vpad, c.vocab, begin, stream);
  ranker.slots_dev = d_bhist.as<int32_t>(); ranker.slots_off = 1 - p0;   // the pass at position p fills generated slot p - p0
  // ---- the prompt into every row's extent
  if (max_new > 1) {
    const int P = (c.max_target_positions + KV_PAGE - 1) / KV_PAGE;
    const T* pool = kv_paged ? d_kvpool.as<T>() : nullptr;
    hipLaunchKernelGGL(wh_beam_prompt_kernel<T>, dim3(N, Ld * 2 * H), dim3(256), 0, stream, pool, kv_paged ? d_ptable.as<int32_t>() : nullptr, P,
                       kv_paged ? nullptr : d_kc.as<T>(), kv_paged ? nullptr : d_vc.as<T>(), c.max_target_positions, B, H, p0, beam, S, d_bext.as<T>());
    HIP_CHECK(hipGetLastError());
  }
  BeamStep bs;
  bs.beam = beam; bs.p0 = p0; bs.S = S; bs.ld_src = ld; bs.hist = d_bhist.as<int32_t>(); bs.logits = d_blogits.as<float>();
  const bool graphable = use_graph && !taps_enabled && !prof.enabled;
  GraphKey key;                                             // everything the captured step bakes in
  for (uint64_t v : {(uint64_t)B, (uint64_t)beam, (uint64_t)S, (uint64_t)p0, (uint64_t)ld, (uint64_t)n_stop, (uint64_t)Mpad, ws_epoch, ranker.epoch,
                     (uint64_t)(uintptr_t)stream, head.epoch, (uint64_t)(kstart_on ? (uintptr_t)d_kstart.ptr : 0)})
    key.mix(v);
  for (int t = 0; t + 1 < max_new && !ranker.all_done(stream); ++t) {
    bs.src = ranker.ancestry();
    beam_graph[ranker.cur].run(stream, graphable, key.h, [&] { enqueue_step<T>(ranker.next_ids(), beam, false, true, &bs); });
    ranker.flip();
  }
  HIP_CHECK(hipGetLastError());
  ranker.download(tokens_out, max_new, n_out, scores_out, stream);
  if (prof.enabled) prof.collect();
}

// ---- word timestamps: the mode, the alignment after generation and its read-back (include/asr_mi355x.h)
void WhSession::set_word_timestamps(int enable, const int32_t* pairs, int n, int max_rows) {
  const auto& c = cfg;
  if (!enable) { wts_on = false; wts_p0 = -1; wts_rows = 0; wts_consumed = false; return; }
  ASR_REQUIRE(pairs && n >= 1 && n <= c.n_dec_layers * c.n_heads, "whisper_set_word_timestamps: %d (layer, head) pairs outside 1..%d", n, c.n_dec_layers * c.n_heads);
  ASR_REQUIRE(max_rows >= 1 && max_rows <= c.max_target_positions, "whisper_set_word_timestamps: max_rows %d outside 1..%d", max_rows, c.max_target_positions);
  std::vector<char> seen((size_t)c.n_dec_layers * c.n_heads, 0);
  for (int i = 0; i < n; ++i) {
    const int l = pairs[2 * i], h = pairs[2 * i + 1];
    ASR_REQUIRE(l >= 0 && l < c.n_dec_layers && h >= 0 && h < c.n_heads, "whisper_set_word_timestamps: pair %d = (layer %d, head %d) outside %d layers x %d heads", i, l, h,
                c.n_dec_layers, c.n_heads);
    ASR_REQUIRE(!seen[(size_t)l * c.n_heads + h], "whisper_set_word_timestamps: pair (layer %d, head %d) given twice", l, h);
    seen[(size_t)l * c.n_heads + h] = 1;
  }
  HIP_CHECK(hipSetDevice(device));
  HIP_CHECK(hipStreamSynchronize(stream));                  // a step in flight may still read the old list
  wts_p0 = -1; wts_rows = 0; wts_consumed = false;        // the arguments hold: the old capture ends here, the new one starts at the next prefill
  wts_pairs.assign(pairs, pairs + 2 * n);
  wts_max_rows = max_rows;
  wts_first.assign(c.n_dec_layers, 0); wts_count.assign(c.n_dec_layers, 0);
  std::vector<int32_t> sel;                                 // (head, slot) runs, layer by layer; slot = the pair's index as given
  for (int l = 0; l < c.n_dec_layers; ++l) {
    wts_first[l] = (int)sel.size() / 2;
    for (int i = 0; i < n; ++i)
      if (pairs[2 * i] == l) { sel.push_back(pairs[2 * i + 1]); sel.push_back(i); ++wts_count[l]; }
  }
  d_wsel.reserve(sel.size() * 4, stream);
  HIP_CHECK(hipMemcpy(d_wsel.ptr, sel.data(), sel.size() * 4, hipMemcpyHostToDevice));
  ++wts_epoch;
  wts_on = true;
}

void WhSession::align(const int32_t* n_rows, const int32_t* n_frames, int width, int32_t* frames_out, int out_stride) {
  ASR_REQUIRE(n_rows && n_frames && frames_out, "whisper_align: null argument");
  ASR_REQUIRE(wts_on && wts_p0 >= 0 && wts_rows > 0 && batch > 0 && d_wscores.ptr, "whisper_align: nothing captured (switch word timestamps on, then prefill and decode)");
  ASR_REQUIRE(!wts_consumed, "whisper_align: the captured rows were aligned already (the soft-max runs in place); prefill and decode again");
  ASR_REQUIRE(width >= 1 && width <= 9 && (width & 1), "whisper_align: medfilt_width %d (odd, 1..9)", width);
  const int B = batch, P = n_pairs();
  int rows_max = 0, frames_max = 0;
  for (int b = 0; b < B; ++b) {
    ASR_REQUIRE(n_rows[b] == 0 || (n_rows[b] >= 2 && n_rows[b] <= wts_rows), "whisper_align: n_rows[%d] = %d (0, or 2..%d rows captured since the prefill)", b, n_rows[b], wts_rows);
    ASR_REQUIRE(n_frames[b] >= 1 && n_frames[b] <= plan[b].n_lfr, "whisper_align: n_frames[%d] = %d outside 1..%d", b, n_frames[b], plan[b].n_lfr);
    ASR_REQUIRE(n_rows[b] <= out_stride, "whisper_align: out_stride %d below n_rows[%d] = %d", out_stride, b, n_rows[b]);
    rows_max = std::max(rows_max, n_rows[b]);
    if (n_rows[b]) frames_max = std::max(frames_max, n_frames[b]);
  }
  wts_n_rows.assign(n_rows, n_rows + B); wts_n_frames.assign(n_frames, n_frames + B);
  if (rows_max == 0) return;
  HIP_CHECK(hipSetDevice(device));
  const size_t trace_stride = (size_t)(wts_max_rows + 1) * (wts_ld + 1);
  d_wn.reserve((size_t)2 * B * 4, stream);
  d_wstats.reserve((size_t)B * P * 2 * wts_ld * 4, stream);
  d_wcost.reserve((size_t)B * wts_max_rows * wts_ld * 4, stream);
  d_wtrace.reserve((size_t)B * trace_stride, stream);
  d_wframes.reserve((size_t)B * wts_max_rows * 4, stream);
  h_walign.reserve((size_t)B * std::max(2, wts_max_rows) * 4);
  int32_t* stage = h_walign.as<int32_t>();
  memcpy(stage, n_rows, (size_t)B * 4); memcpy(stage + B, n_frames, (size_t)B * 4);
  HIP_CHECK(hipMemcpyAsync(d_wn.ptr, stage, (size_t)2 * B * 4, hipMemcpyHostToDevice, stream));
  HIP_CHECK(hipStreamSynchronize(stream));                  // (the staging buffer receives the frames below)
  const int32_t* dn = d_wn.as<int32_t>();
  const int32_t* df = dn + B;
  {
    ProfScope ps(prof, "align", stream);
    launch_align_softmax(d_wscores.as<float>(), B, P, wts_max_rows, wts_ld, dn, df, rows_max, stream);
    launch_align_colstats(d_wscores.as<float>(), B, P, wts_max_rows, wts_ld, dn, df, frames_max, d_wstats.as<float>(), stream);
    launch_align_cost(d_wscores.as<float>(), d_wstats.as<float>(), B, P, wts_max_rows, wts_ld, dn, df, rows_max, frames_max, width, d_wcost.as<float>(), stream);
    launch_align_dtw(d_wcost.as<float>(), B, wts_max_rows, wts_ld, dn, df, rows_max, d_wtrace.as<unsigned char>(), trace_stride, d_wframes.as<int32_t>(),
                     wts_max_rows, nullptr, 0, nullptr, stream);
  }
  wts_consumed = true;
  HIP_CHECK(hipMemcpyAsync(stage, d_wframes.ptr, (size_t)B * wts_max_rows * 4, hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  for (int b = 0; b < B; ++b)
    for (int r = 0; r < n_rows[b]; ++r) frames_out[(size_t)b * out_stride + r] = stage[(size_t)b * wts_max_rows + r];
  if (prof.enabled) prof.collect();
}

// what 0: the captured scores of utterance b, f32 [n_pairs][rows captured][n_lfr] (after an align the aligned part holds the soft-max: it runs in place);
// what 1: its cost matrix of the last align, f32 [1][n_rows][n_frames]. shape_out [3] (nullable) receives the three extents; host_out null: only that.
void WhSession::align_read(int what, int b, void* host_out, size_t bytes, int32_t* shape_out) {
  ASR_REQUIRE(what == 0 || what == 1, "whisper_align_read: what = %d (0 captured scores, 1 cost matrix)", what);
  ASR_REQUIRE(wts_on && wts_p0 >= 0 && wts_rows > 0 && d_wscores.ptr, "whisper_align_read: nothing captured");
  ASR_REQUIRE(b >= 0 && b < batch, "whisper_align_read: utterance %d outside the batch of %d", b, batch);
  ASR_REQUIRE(what == 0 || ((int)wts_n_rows.size() == batch && wts_consumed), "whisper_align_read: no cost matrix (align first)");
  const int P = what == 0 ? n_pairs() : 1, rows = what == 0 ? wts_rows : wts_n_rows[b], cols = what == 0 ? plan[b].n_lfr : wts_n_frames[b];
  if (shape_out) { shape_out[0] = P; shape_out[1] = rows; shape_out[2] = cols; }
  if (!host_out) return;
  ASR_REQUIRE(bytes == (size_t)P * rows * cols * 4, "whisper_align_read: %zu bytes given, %zu expected", bytes, (size_t)P * rows * cols * 4);
  if (bytes == 0) return;
  HIP_CHECK(hipSetDevice(device));
  HIP_CHECK(hipStreamSynchronize(stream));
  const float* src = what == 0 ? d_wscores.as<float>() + (size_t)b * n_pairs() * wts_max_rows * wts_ld : d_wcost.as<float>() + (size_t)b * wts_max_rows * wts_ld;
  for (int p = 0; p < P; ++p)
    HIP_CHECK(hipMemcpy2D((float*)host_out + (size_t)p * rows * cols, (size_t)cols * 4, src + (size_t)p * wts_max_rows * wts_ld, (size_t)wts_ld * 4, (size_t)cols * 4, rows,
                          hipMemcpyDeviceToHost));
}

}  // namespace

extern "C" int asr_whisper_create(const asr_whisper_config* cfg, const void* arena, size_t arena_bytes, int arena_mem,
                                  int device_id, int precision, asr_session** out) {
  return asr_guard([&] {
    ASR_REQUIRE(cfg && arena && out, "whisper_create: null argument");
    ASR_REQUIRE(precision == ASR_PRECISION_BF16 || precision == ASR_PRECISION_F32 || precision == ASR_PRECISION_FP8W || precision == ASR_PRECISION_FP8MM ||
                precision == ASR_PRECISION_MXFP4W, "whisper_create: bad precision %d", precision);
    asr_require_device(device_id);
    WhSession* s = new WhSession();
    try {
      s->kind = 2;
      s->device = device_id;
      asr_tenant_attach(s);
      s->fp4 = precision == ASR_PRECISION_MXFP4W;
      s->fp8 = precision == ASR_PRECISION_FP8W || precision == ASR_PRECISION_FP8MM || s->fp4;
      s->fp8_mm = precision == ASR_PRECISION_FP8MM;
      s->precision = s->fp8 ? ASR_PRECISION_BF16 : precision;        // FP8 mode = bf16 mode with byte-wide decoder weights and cross-K/V
      s->cfg = *cfg;
      gemm_reload_env();
      s->fp8_fake = env_on("ASR_FP8_FAKE", s->fp8_fake);
      s->fp8_act_shift = std::min(std::max(env_int("ASR_FP8MM_ACT_SHIFT", s->fp8_act_shift), 0), 16);
      s->fp8_weights = env_flag("ASR_FP8_WEIGHTS", s->fp8_weights);
      s->fp8_kv = env_flag("ASR_FP8_KV", s->fp8_kv);
      s->use_graph = !env_on("ASR_NO_GRAPH", !s->use_graph);
      s->kv_paged = env_flag("ASR_KV_PAGED", s->kv_paged);
      s->kv_shuffle = env_on("ASR_KV_PAGE_SHUFFLE", s->kv_shuffle);
      s->use_decode_gemm = env_flag("ASR_DECODE_GEMM", s->use_decode_gemm);
      HIP_CHECK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
      s->own_stream = true;
      s->arena.load(arena, arena_bytes, arena_mem, s->stream);
      s->init();
    } catch (...) {
      delete s;
      throw;
    }
    *out = s;
  });
}

extern "C" int asr_whisper_encode(asr_session* s, const void* audio, int audio_mem, const int64_t* audio_offsets, int batch,
                                  int32_t* n_positions_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 2, "whisper_encode: not a Whisper session");
    TenantScope tenant(s);
    WhSession* w = static_cast<WhSession*>(s);
    w->after_prefill = false;
    w->wts_p0 = -1; w->wts_rows = 0;                      // captured rows belong to the slabs they were scored against
    w->kstart_on = false;
    if (w->precision == ASR_PRECISION_BF16) w->encode<bf16_t>(audio, audio_mem, audio_offsets, batch, n_positions_out);
    else w->encode<float>(audio, audio_mem, audio_offsets, batch, n_positions_out);
  });
}

extern "C" int asr_whisper_prefill(asr_session* s, const int32_t* ids, int n, int32_t* next_ids_out, float* logits_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 2 && ids, "whisper_prefill: bad argument");
    TenantScope tenant(s);
    WhSession* w = static_cast<WhSession*>(s);
    w->after_prefill = false;
    if (w->precision == ASR_PRECISION_BF16) w->step<bf16_t>(ids, n, true, next_ids_out, logits_out);
    else w->step<float>(ids, n, true, next_ids_out, logits_out);
    w->after_prefill = true;
  });
}

extern "C" int asr_whisper_prefill_prompts(asr_session* s, const int32_t* ids, const int32_t* offsets, int32_t* next_ids_out, float* logits_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 2 && ids && offsets, "whisper_prefill_prompts: bad argument");
    TenantScope tenant(s);
    WhSession* w = static_cast<WhSession*>(s);
    w->after_prefill = false;
    w->prefill_prompts(ids, offsets, next_ids_out, logits_out);
    w->after_prefill = true;
  });
}

extern "C" int asr_whisper_decode(asr_session* s, const int32_t* ids, int32_t* next_ids_out, float* logits_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 2, "whisper_decode: not a Whisper session");
    TenantScope tenant(s);
    WhSession* w = static_cast<WhSession*>(s);
    w->after_prefill = false;
    if (w->precision == ASR_PRECISION_BF16) w->step<bf16_t>(ids, 1, false, next_ids_out, logits_out);
    else w->step<float>(ids, 1, false, next_ids_out, logits_out);
  });
}

// the decode-head entries: the checks and the state are TokenHead's (decode_head.h)
static WhSession* whisper_session(asr_session* s, const char* who) {
  ASR_REQUIRE(s && s->kind == 2, "%s: not a Whisper session", who);
  return static_cast<WhSession*>(s);
}

extern "C" int asr_whisper_set_penalty(asr_session* s, float repeat_penalty, int penalty_range) {
  return asr_guard([&] { whisper_session(s, "whisper_set_penalty")->head.set_penalty(repeat_penalty, penalty_range, "whisper_set_penalty"); });
}

extern "C" int asr_whisper_no_speech_prob(asr_session* s, int no_speech_id, float* prob_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 2 && prob_out, "whisper_no_speech_prob: bad argument");
    WhSession* w = static_cast<WhSession*>(s);
    ASR_REQUIRE(w->batch > 0 && w->hist > 0 && w->d_logits.ptr, "whisper_no_speech_prob: run a prefill first (the probe's logits are the input)");
    HIP_CHECK(hipSetDevice(w->device));
    const int B = w->batch;
    w->d_nsp.reserve((size_t)std::max(B, 64) * 4, w->stream);
    launch_no_speech_prob(w->d_logits.as<float>(), w->vpad, B, w->cfg.vocab, w->suppress, no_speech_id, w->d_nsp.as<float>(), w->stream);
    HIP_CHECK(hipMemcpyAsync(prob_out, w->d_nsp.ptr, (size_t)B * 4, hipMemcpyDeviceToHost, w->stream));
    HIP_CHECK(hipStreamSynchronize(w->stream));
  });
}

extern "C" int asr_whisper_set_fp8_act_shift(asr_session* s, int shift) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 2, "whisper_set_fp8_act_shift: not a Whisper session");
    ASR_REQUIRE(shift >= 0 && shift <= 16, "whisper_set_fp8_act_shift: shift %d outside 0 .. 16", shift);
    static_cast<WhSession*>(s)->fp8_act_shift = shift;          // (the encoder is not graph-captured: the next encode uses it)
  });
}

extern "C" int asr_whisper_fp8_stats(asr_session* s, uint64_t stats[2]) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 2 && stats, "whisper_fp8_stats: not a Whisper session");
    WhSession* w = static_cast<WhSession*>(s);
    HIP_CHECK(hipSetDevice(w->device));
    stats[0] = 0; stats[1] = (uint64_t)w->fp8_act_shift;
    if (w->fp8_mm && w->d_sat.ptr) {
      unsigned long long n = 0;
      HIP_CHECK(hipStreamSynchronize(w->stream));
      HIP_CHECK(hipMemcpy(&n, w->d_sat.ptr, 8, hipMemcpyDeviceToHost));
      stats[0] = n;
    }
  });
}

extern "C" int asr_whisper_track_history(asr_session* s, int enable) {
  return asr_guard([&] { whisper_session(s, "whisper_track_history")->head.set_track_history(enable != 0); });
}

extern "C" int asr_whisper_set_sampling(asr_session* s, int enable, float temperature, int top_k, float top_p,
                                        float repetition_penalty, uint64_t seed) {
  return asr_guard([&] {
    whisper_session(s, "whisper_set_sampling")->head.set_sampling(enable != 0, temperature, top_k, top_p, repetition_penalty, seed, "whisper_set_sampling");
  });
}

extern "C" int asr_whisper_set_timestamps(asr_session* s, int enable, int timestamp_begin_id, int no_timestamps_id, int eot_id, int max_initial_index) {
  return asr_guard([&] {
    WhSession* w = whisper_session(s, "whisper_set_timestamps");
    w->head.set_timestamps(enable != 0, timestamp_begin_id, no_timestamps_id, eot_id, max_initial_index, w->cfg.vocab, "whisper_set_timestamps");
  });
}

extern "C" int asr_whisper_set_hotwords(asr_session* s, const int32_t* ids, const int32_t* offsets, int n_phrases, float boost) {
  return asr_guard([&] {
    WhSession* w = whisper_session(s, "whisper_set_hotwords");
    HIP_CHECK(hipSetDevice(w->device));
    w->head.set_hotwords(ids, offsets, n_phrases, boost, w->cfg.vocab, w->stream, "whisper_set_hotwords");
  });
}

extern "C" int asr_whisper_set_lm(asr_session* s, const int32_t* image_words, int64_t n_words, float alpha, float beta, float oov_logprob, int topk,
                                  const int32_t* end_ids, int n_end_ids) {
  return asr_guard([&] {
    WhSession* w = whisper_session(s, "whisper_set_lm");
    HIP_CHECK(hipSetDevice(w->device));
    w->head.set_lm(image_words, n_words, alpha, beta, oov_logprob, topk, end_ids, n_end_ids, w->cfg.vocab, w->stream, "whisper_set_lm");
  });
}

extern "C" int asr_whisper_set_token_scores(asr_session* s, int enable) {
  return asr_guard([&] { whisper_session(s, "whisper_set_token_scores")->head.set_scores(enable != 0); });
}

extern "C" int asr_whisper_token_scores(asr_session* s, float* logprob_out, int out_stride, int32_t* n_out) {
  return asr_guard([&] {
    WhSession* w = whisper_session(s, "whisper_token_scores");
    HIP_CHECK(hipSetDevice(w->device));
    w->head.download_scores(w->batch, logprob_out, out_stride, n_out, w->stream, "whisper_token_scores");
  });
}

extern "C" int asr_whisper_set_sampling_noise(asr_session* s, const float* uniforms, int count) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 2 && uniforms, "whisper_set_sampling_noise: bad argument");
    WhSession* w = static_cast<WhSession*>(s);
    ASR_REQUIRE(w->head.sampling && w->batch > 0 && count == w->batch * w->head.top_k, "whisper_set_sampling_noise: expects batch x top_k = %d uniforms for the next step",
                w->batch * w->head.top_k);
    HIP_CHECK(hipSetDevice(w->device));
    w->head.arm_noise(uniforms, count, w->stream);
  });
}

extern "C" int asr_whisper_generate(asr_session* s, int max_new, int eos_id, int32_t* tokens_out, int32_t* n_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 2 && tokens_out && n_out && max_new >= 1, "whisper_generate: bad argument");
    TenantScope tenant(s);
    WhSession* w = static_cast<WhSession*>(s);
    ASR_REQUIRE(w->hist > 0, "whisper_generate: prefill first");
    w->after_prefill = false;
    const int B = w->batch;
    std::vector<int32_t> cur(B);
    HIP_CHECK(hipSetDevice(w->device));
    HIP_CHECK(hipMemcpyAsync(cur.data(), w->d_next.ptr, (size_t)B * 4, hipMemcpyDeviceToHost, w->stream));
    HIP_CHECK(hipStreamSynchronize(w->stream));
    std::vector<char> done(B, 0);
    for (int b = 0; b < B; ++b) n_out[b] = 0;
    for (int t = 0; t < max_new; ++t) {
      bool all_done = true;
      for (int b = 0; b < B; ++b) {
        if (!done[b]) {
          if (cur[b] == eos_id) done[b] = 1;                         // the stop token itself is not emitted (:648)
          else tokens_out[(size_t)b * max_new + n_out[b]++] = cur[b];
        }
        all_done = all_done && done[b];
      }
      if (all_done || t + 1 == max_new || w->hist + 1 > w->cfg.max_target_positions) break;
      // token ids stay on the device between steps; one small D2H per step for the stop test
      if (w->precision == ASR_PRECISION_BF16) w->step<bf16_t>(nullptr, 1, false, cur.data(), nullptr);
      else w->step<float>(nullptr, 1, false, cur.data(), nullptr);
    }
  });
}

extern "C" int asr_whisper_beam_search(asr_session* s, int beam, int max_new, int eos_id, int32_t* tokens_out, int32_t* n_out, float* scores_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 2 && tokens_out && n_out && max_new >= 1, "whisper_beam_search: bad argument");
    TenantScope tenant(s);
    WhSession* w = static_cast<WhSession*>(s);
    if (w->precision == ASR_PRECISION_BF16) w->beam_search<bf16_t>(beam, max_new, eos_id, tokens_out, n_out, scores_out);
    else w->beam_search<float>(beam, max_new, eos_id, tokens_out, n_out, scores_out);
  });
}

extern "C" int asr_whisper_set_word_timestamps(asr_session* s, int enable, const int32_t* layer_head_pairs, int n_pairs, int max_rows) {
  return asr_guard([&] { whisper_session(s, "whisper_set_word_timestamps")->set_word_timestamps(enable, layer_head_pairs, n_pairs, max_rows); });
}

extern "C" int asr_whisper_align(asr_session* s, const int32_t* n_rows, const int32_t* n_frames, int medfilt_width, int32_t* token_frames_out, int out_stride) {
  return asr_guard([&] {
    WhSession* w = whisper_session(s, "whisper_align");
    TenantScope tenant(s);
    w->align(n_rows, n_frames, medfilt_width, token_frames_out, out_stride);
  });
}

extern "C" int asr_whisper_align_read(asr_session* s, int what, int b, void* host_out, size_t bytes, int32_t* shape_out) {
  return asr_guard([&] { whisper_session(s, "whisper_align_read")->align_read(what, b, host_out, bytes, shape_out); });
}
