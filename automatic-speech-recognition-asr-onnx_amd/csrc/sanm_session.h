// The session behind three products that share the SANM encoder: SenseVoice (encoder + CTC head, greedy / timed / prefix beam), offline Paraformer (encoder +
// CIF predictor + non-autoregressive decoder) and streaming Paraformer (the same model chunk by chunk with per-stream state). sensevoice.hip holds the offline
// forms, paraformer_stream.hip the streaming one. What a call brings home -- tokens, counts, the status word, spans / fire rows and scores, the beam's
// hypotheses -- is laid out by result_layout.h: the copies a step enqueues and the host reads behind the sync use the same section handles (ResultBlob).
#pragma once
#include "../../include/asr_mi355x.h"
#include "engine.h"
#include "gemm.h"
#include "kernels.h"
#include "ngram_lm.h"

struct SvBlock {
  const float *ln1_g, *ln1_b, *bqkv, *wfsmn, *bfsmn, *ln2_g, *ln2_b, *b1, *b2;
  const float *cqkv, *c1;       // column sums of wqkv / w1 (bf16 arenas with folded LayerNorm affines): LayerNorm inside the GEMM
  const void *wqkv, *wout, *w1, *w2;
  int in_size, kpad;
};

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Paraformer decoder block (Export_Paraformer.py:536-552): FFN (norm folded) -> LayerNorm -> FSMN + residual -> cross-attention
struct PfDecLayer {
  const void *w1, *w2, *wq, *wkv, *wo;
  const float *b1, *b2, *n2_g, *n2_b, *wfsmn, *bq, *bkv, *bo;
  bool full;     // false: FFN-only block (decoders3)
};

// What a call asks for. PLAIN: ids and counts; TIMED: also per-token times and log-probabilities; BEAM: n-best hypotheses with scores (SenseVoice: CTC prefix
// beam search; Paraformer: beam search over the decoder's token rows, with the fire rows and per-token log-probabilities); ALIGN (SenseVoice): the spans and
// scores of a transcript the caller supplies. STREAM_BEAM (streaming Paraformer): the timed step followed by the candidates of its token rows and the streaming
// search (nar_stream_beam.hip) -- the caller keeps the timed step's outputs and gets the committed tokens and the pending tails on top.
enum class SvForm { PLAIN, TIMED, BEAM, ALIGN, STREAM_BEAM };
struct SvRunReq {               // offline: asr_sensevoice_run / _run_timed / _run_beam / _align, asr_paraformer_run / _run_timed / _run_beam
  SvForm form = SvForm::PLAIN;
  const void* audio = nullptr; int audio_mem = 0; const int64_t* offs = nullptr; int batch = 0;
  const int32_t* lang = nullptr;                        // SenseVoice only
  int max_tokens = 0;
  int32_t *tok_out = nullptr, *num_out = nullptr;       // BEAM: [batch][nbest][max_tokens] / [batch][nbest]
  int32_t *first_out = nullptr, *last_out = nullptr;    // TIMED: SenseVoice frame spans; Paraformer: first_out = the CIF fire rows, no last_out
  float* logprob_out = nullptr;                         // TIMED
  int beam = 0, topk = 0, nbest = 0;                    // BEAM
  float *score_out = nullptr, *ctc_out = nullptr;       // BEAM (Paraformer: ctc_out = the acoustic score)
  float* hyp_logprob_out = nullptr;                     // Paraformer BEAM, nullable: [batch][nbest][max_tokens]; first_out (nullable) = the CIF fire rows [batch][max_tokens]
  // ALIGN: the transcripts (ragged: ids [sum L], offsets [batch + 1]); first_out / last_out / logprob_out are ragged in the same layout, no tok_out / num_out
  const int32_t *tgt_ids = nullptr, *tgt_off = nullptr;
  float *path_out = nullptr, *loglik_out = nullptr; int32_t* astatus_out = nullptr;      // [batch]
};
struct SvStreamBeamOut {        // host arrays of the streaming search (asr_paraformer_stream_step_beam / _finish_beam), per stream of the call
  int32_t* commit_ids = nullptr; float* commit_logprob = nullptr; int32_t* commit_num = nullptr;      // [n][pend_cap + max_tokens], [n]
  int32_t* pend_ids = nullptr; float* pend_logprob = nullptr;                                         // [n][nbest][pend_cap]
  int32_t* pend_num = nullptr; float *pend_score = nullptr, *pend_am = nullptr;                       // [n][nbest]
  int32_t* total = nullptr;                                                                            // [n]
  bool complete() const { return commit_ids && commit_logprob && commit_num && pend_ids && pend_logprob && pend_num && pend_score && pend_am && total; }
};
struct SvStepReq {              // streaming: asr_paraformer_stream_step / _step_timed / _step_beam
  SvForm form = SvForm::PLAIN;
  const void* audio = nullptr; int audio_mem = 0; const int32_t* stream_ids = nullptr; int n = 0, max_tokens = 0;
  int32_t *tok_out = nullptr, *num_out = nullptr, *fire_out = nullptr;      // fire_out / logprob_out: TIMED, STREAM_BEAM
  float* logprob_out = nullptr;
  SvStreamBeamOut beam_out;                                                 // STREAM_BEAM
};

// Everything a forward pass needs once the host plan is uploaded; captured into a hipGraph for replay.
struct SvRunCtx {
  int batch, rows, Mpad, frames, n_fb, n_qb, max_T, max_tokens, att_qt, att_nw;
  const void* d_aud;          // packed samples of audio_dtype: the session's, or f32 behind the resampler
  int audio_dtype;
  const UttPlan* dp;
  const int32_t *d_blk_utt, *d_blk_f0, *d_qb_utt, *d_qb_q0, *d_row_utt;
  const int32_t *d_tile_win = nullptr, *d_tile_idx = nullptr;    // small batches (sanm_tiles.hip): per 16-row tile its window / its index inside the window
  int n_tiles = 0;
  bool tiles = false;
  bool timed = false;         // CTC head with frame log-probabilities, collapse with spans
  int beam = 0, topk = 0, nbest = 0, pool_stride = 0;     // beam > 0: CTC head with the sum-of-exponentials partial, candidates, prefix beam search
  bool align = false;         // CTC head with the sum-of-exponentials partial, gathered emissions, forced alignment (max_tokens = the longest transcript)
  int max_L = 0, ld_em = 0;
  const int32_t *d_tgt_ids = nullptr, *d_tgt_off = nullptr;
  const ResultBlob* out = nullptr;                        // where the step's D2H copies land
};

struct ASR_LOCAL SvSession : asr_session {
  // ---- shared SANM encoder: front end, blocks, workspace (grow-only), staging, graphs ----------------------------------------------
  asr_sensevoice_config cfg;
  int feat = 0, kpad0 = 0, vpad = 0, max_lfr = 0;
  FrontEnd fe;
  std::vector<SvBlock> blocks;
  const float *cmvn_means = nullptr, *cmvn_vars = nullptr, *speech_pos = nullptr;
  const float *language_embed = nullptr, *system_embed = nullptr;
  const float *after_g = nullptr, *after_b = nullptr;
  DeviceBuffer d_x0lo, d_xalo, d_xblo;     // bf16 copies of the residual stream (operands of the LayerNorm-fused projections)
  DeviceBuffer d_sta, d_stb;               // per-row (sum, sum of squares) partials of those copies, 32-column groups
  DeviceBuffer d_plan, d_audio, d_mel, d_x0, d_xa, d_xb, d_h, d_qk, d_vt, d_ctx, d_mem, d_ffn, d_amax_v, d_amax_i, d_ids, d_tok, d_num, d_logits;
  DeviceBuffer d_amax_s, d_flp, d_first, d_last, d_tlp;   // timed runs only: sum-of-exponentials partials, frame log-probabilities, token spans and scores
                                                          // (Paraformer: row log-probabilities in d_flp, fire rows / steps in d_first, token log-probabilities in d_tlp)
  PinnedBuffer h_plan, h_out;   // pinned staging: the plan blob (PlanBlob) and the result blob (ResultBlob, result_layout.h)
  DeviceBuffer d_dft_split;
  DeviceBuffer d_layer_tab;     // SanmBlockLayer[n_blocks]: the per-block constants a launch of the 8-wave kernel walks
  DeviceBuffer d_wpack;         // 8-wave form: fragment-major copy of every 512 -> 512 block's weights, made once per session (ensure_block_pack)
  DeviceBuffer d_tpack, d_tlayer_tab, d_tkv;      // small batches: a workgroup per (16-row tile, head), csrc/sanm_tiles.hip
  DeviceBuffer d_times;         // phase clocks of a debugged launch (block_dbg, tiles_dbg)
  DeviceBuffer d_flags;         // exchange counters of the block kernel: [n_blocks][batch][4] + the error word at the end
  bool wpack_ready = false, tpack_ready = false;
  int block_giveups = 0;        // forward passes redone on the four-launch path because a cluster gave up (see run())
  bool foreign_now = false;     // a foreign section (RCCL collective, engine.h: ClusterScope) is open on this GPU: this pass launches no cluster kernel
  int foreign_diverted = 0;     // passes that took the cluster-free path for that reason
  int block_cooldown = 0;       // batches left on the four-launch path after a give-up (other sessions are holding CUs: do not walk into the same wait again)
  StepGraph graph;              // hipGraph replay of the forward pass (one graph per batch geometry)
  StepGraph graph_timed;        // ... of the timed forms, so that a caller who alternates the two forms replays both
  uint64_t ws_epoch = 1;
  SplitKGemm sk;
  // debug / ablation switches, re-read at every session creation (load_env)
  bool use_graph = true;
  bool use_ln_alg = true;       // LayerNorm evaluated inside the projections from row statistics (ASR_LN_FUSED=0 disables)
  bool use_fused = true;        // fused q|k|v + attention + FSMN kernel for windows of <= 144 rows (ASR_SANM_FUSED=0 disables)
  bool use_block = true;        // one launch per SANM block (clusters of four workgroups per window; ASR_SANM_BLOCK=0 disables)
  bool use_fbank_split = true;  // ASR_FBANK_SPLIT=0: exact-f32 MFMA DFT in bf16 sessions too
  int block8_opt = 0;           // ASR_SANM_BLOCK8_OPT: tuning switches of the 8-wave kernel (SanmBlockArgs::opt)
  bool block_persist = true;    // ASR_SANM_BLOCK_PERSIST=0: the 8-wave kernel is launched once per block instead of once per run of blocks
  bool use_tiles = true;        // ASR_SANM_TILES=0: four launches per block for small batches, as before the tile kernel
  int tiles_opt = 0, tiles_dbg = -1;       // ASR_SANM_TILES_OPT (SanmTilesArgs::opt), ASR_SANM_TILES_DBG=<block>: phase clock of that block on stderr
  int block_fault = 0;          // ASR_SANM_BLOCK_FAULT=1 (tests): one workgroup of the first block launch withholds an exchange count
  bool block_ffnk = true;       // ASR_SANM_BLOCK_FFNK=0: the round-4 form of the block kernel's FFN pair (hid exchanged); default: FFN-2 split over K, f16 partials exchanged (round 6)
  int block_scatter = 0;        // ASR_SANM_BLOCK_SCATTER=1: test placement, every cluster spread over four XCDs
  int block_min_utts = 12;      // ASR_SANM_BLOCK_MIN=<windows>: smallest batch that takes the block kernel (8-wave form: faster from ~10 windows on; tools/probes/block_min_sweep.sh)
  int block_dbg = -1;           // ASR_SANM_BLOCK_DBG=<block index>: phase clock of that block's launch on stderr
  void load_env() {
    gemm_reload_env();
    use_graph = !env_on("ASR_NO_GRAPH", !use_graph);
    use_fused = env_flag("ASR_SANM_FUSED", use_fused);
    use_block = env_flag("ASR_SANM_BLOCK", use_block);
    use_fbank_split = env_flag("ASR_FBANK_SPLIT", use_fbank_split);
    block8_opt = env_int("ASR_SANM_BLOCK8_OPT", block8_opt);
    block_ffnk = env_flag("ASR_SANM_BLOCK_FFNK", block_ffnk);
    if ((block8_opt >> 4) & 15) block_ffnk = false;          // the timing-only ablations exist for the round-4 loops
    use_tiles = env_flag("ASR_SANM_TILES", use_tiles);
    tiles_opt = env_int("ASR_SANM_TILES_OPT", tiles_opt);
    tiles_dbg = env_int("ASR_SANM_TILES_DBG", tiles_dbg);
    block_persist = env_flag("ASR_SANM_BLOCK_PERSIST", block_persist);
    block_scatter = env_on("ASR_SANM_BLOCK_SCATTER", block_scatter);
    block_fault = env_on("ASR_SANM_BLOCK_FAULT", block_fault);
    block_dbg = env_int("ASR_SANM_BLOCK_DBG", block_dbg);
    block_min_utts = env_int("ASR_SANM_BLOCK_MIN", block_min_utts);
    use_ln_alg = env_flag("ASR_LN_FUSED", use_ln_alg);
  }
  void init();
  void ensure_tiles_pack();
  void ensure_block_pack();
  void copy_block_status(const SvRunCtx& r);             // the block kernel's error word rides home in the result blob's status section
  void validate(const SvRunReq& q) const;                // every form's argument checks
  template <typename T> void enqueue(const SvRunCtx& r);
  template <typename T> void run(const SvRunReq& q);
  void gemm(const GemmArgs& g0) {
    const GemmArgs g = sk.attach(g0, stream);          // in f32 sessions too: the workspace lets single windows split K
    if (precision != ASR_PRECISION_BF16) launch_gemm_f32(g, stream);
    else launch_gemm_bf16(g, stream);
  }

  // ---- SenseVoice: CTC head, prefix beam search (asr_sensevoice_run_beam, ctc_beam.hip); the beam buffers, hotwords and language model also serve
  // Paraformer's beam search over token rows (asr_paraformer_run_beam, nar_beam.hip) ----------------------------------------------------
  const float *tp_g = nullptr, *tp_b = nullptr, *ctc_b = nullptr;
  const void* ctc_w = nullptr;
  // beam runs only: candidates [rows][topk], the (parent, token) node pool, the outputs as one block (result_layout.h: the beam block), the hotword trie image
  DeviceBuffer d_cand_i, d_cand_l, d_pool, d_bout, d_hot;
  int hot_nodes = 0; float hot_boost = 0.0f;
  uint64_t beam_epoch = 1;      // bumped when a beam-only buffer moves or the hotword list or language model changes: part of the beam graph's key, not of the others'
  StepGraph graph_beam;         // hipGraph replay of the beam form
  void set_hotwords(const int32_t* ids, const int32_t* offsets, int n_phrases, float boost);
  // the n-gram language model of the beam form (asr_sensevoice_set_lm, ngram_lm.h): the image in HBM, its checked header, the weights
  DeviceBuffer d_lm;
  int32_t lm_header[6] = {0, 0, 0, 0, 0, -1};            // n_nodes (word 1) == 0: no model
  float lm_alpha = 0.0f, lm_beta = 0.0f, lm_oov = 0.0f;
  void set_lm(const int32_t* image_words, int64_t n_words, float alpha, float beta, float oov_logprob);
  NgramLm lm_view() const {     // what the three searches take; without a model it has no nodes, and the search without one is launched
    return lm_header[1] > 0 ? ngram_lm_view(d_lm.as<int32_t>(), lm_header, lm_alpha, lm_beta, lm_oov) : NgramLm{};
  }
  // align runs only (asr_sensevoice_align, ctc_align.hip): emissions [rows][ld_em], the backpointer workspace of transcripts too long for LDS, per-utterance
  // scores and status; the spans land in d_first / d_last / d_tlp
  DeviceBuffer d_em, d_abp, d_apath, d_alik, d_astat;
  StepGraph graph_align;        // hipGraph replay of the align form

  // ---- offline Paraformer: CIF predictor + decoder ------------------------------------------------------------------------------------
  bool paraformer = false;
  asr_paraformer_config pcfg{};
  std::vector<PfDecLayer> pdec;
  const void *cif_conv_w = nullptr, *pf_out_w = nullptr;
  const float *cif_conv_b = nullptr, *cif_out_w = nullptr, *cif_out_b = nullptr, *pf_out_b = nullptr;
  DeviceBuffer d_enc_lo, d_ck, d_cifa, d_alpha, d_dec, d_x2, d_sa, d_ffn32, d_tplan;
  DeviceBuffer d_ctplan, d_mdev, d_trow;   // compact token plan, device-side token-row count, row -> utterance map of the token rows
  // the cross-attention K / V projections of ALL decoder layers as two GEMMs over the encoder output (they depend on nothing the decoder computes): the layers' wkv halves
  // gathered once into [n_full d][d] images (ASR_PF_KV_BATCH=0: one pair of launches per layer, the round-2..5 form)
  DeviceBuffer d_wk_all, d_wv_all, d_bk_all, d_bv_all; int pf_n_full = 0; bool pf_kv_batch = true;
  template <typename T> void enqueue_paraformer_tail(const SvRunCtx& r);

  // ---- streaming Paraformer (kind 4, paraformer_stream.hip): per-stream recurrent state in HBM, every step advances n streams by one chunk ----
  int st_chunk = 0, st_B = 0, st_C = 0, st_en_cap = 0, st_de_cap = 0, st_max = 0, st_frames = 0;
  DeviceBuffer st_enk, st_env, st_dek, st_dev, st_defsmn, st_prev, st_cifh, st_cifa, st_enlen, st_delen, st_start, d_sqkv, d_skv;
  // streaming encoder layers 1 .. as one launch (stream_layers.hip): fragment-major weight copies, the device layer table, exchange counters (+ err)
  DeviceBuffer st_wpack, st_layer_tab, st_flags, st_times, st_dpack, st_dlayer_tab;     // (st_d*: the decoder launch, stream_dec.hip)
  DeviceBuffer st_zero;                 // a device counter that stays 0: the timed step's head saves each row's score at column 0 (launch_argmax_logprob_rows)
  bool st_fused = false, st_dec_fused = false;
  int st_times_layer = -1;              // ASR_STREAM_TIMES=<layer>: phase clocks of that fused layer, printed to stderr after every step (tuning)
  int st_opt = 0;                       // ASR_STREAM_OPT: tuning switches of the fused launch (kernels.h: StreamLayersArgs::opt)
  int st_fused_env = 2;                 // ASR_STREAM_FUSED: 0 = every layer on the per-launch path, 1 = encoder launch only, 2 = encoder and decoder launches
  // Which steps take the cluster launches (round 5). (i) Above st_fused_max active streams the per-launch GEMMs amortise a layer's weights over all the rows
  // while a cluster launch streams them once per CU-load of clusters: 256 streams ran 10.4 ms fused against 9.0 per launch -- default from the
  // CU count, ASR_STREAM_FUSED_MAX overrides. (ii) While ANOTHER session of this process is computing on this GPU (asr_tenant_busy_others) the step takes the
  // per-launch path: (streams x 4) 150-KB workgroups hold every CU for a whole launch and starved a co-tenant's chain of small kernels 10x, and a cluster that is
  // split across dispatch waves by someone else's kernels can give up. ASR_STREAM_SHARE=0 disables the rule. (iii) A fused step is RECOVERABLE when a snapshot of
  // the active streams' recurrent state was taken in front of it (launch_stream_state_copy): on a give-up the state is restored, the step is redone on the per-launch
  // path and the session stays there for st_cooldown_steps steps. Snapshots are taken when other sessions exist on this GPU (they may start computing at any time)
  // or always with ASR_STREAM_SNAPSHOT=1 (=0: never; a give-up then fails the step and the caller has to reset its streams, as in round 4).
  int st_fused_max = 0, st_share_rule = 1, st_snapshot_env = -1, st_fault = 0, st_cooldown = 0;
  int st_giveups = 0, st_shared_steps = 0, st_snapshots = 0;      // counters (asr_paraformer_stream_stats)
  static constexpr int st_cooldown_steps = 64;
  DeviceBuffer st_segs, st_shadow;      // StreamStateSeg table + the shadow copies
  int st_n_segs = 0, st_n_items = 0;
  StepGraph st_graph[3];                // streaming chunk step: per-launch / fused / fused + snapshot
  StepGraph st_graph_timed[3];          // ... of the timed step
  // the streaming beam search (asr_paraformer_stream_set_beam, nar_stream_beam.hip; the build's own mode): per-stream search state for st_max streams, made by
  // the setter; the hotword trie and the language model are the offline search's members above (d_hot, d_lm). sb_len is what the host knows of every stream's
  // L from the totals that came back: the setters refuse to change anything the carried trie nodes and model states refer to while a stream holds history.
  int sb_beam = 0, sb_topk = 0, sb_nbest = 0, sb_cap = 0, sb_words = 0;
  DeviceBuffer st_bstate, st_bfinal;    // [st_max][sb_words] search state; [st_max] ones: the finish's flags
  std::vector<int32_t> sb_len;
  bool stream_search_history() const { for (int32_t v : sb_len) if (v > 0) return true; return false; }
  void stream_set_beam(int beam, int topk, int nbest, int pend_cap);
  void stream_search(const ResultBlob& out, const UttPlan* token_plan, const int32_t* stream_ids, int n, int rows, bool final, const SvStreamBeamOut& o);
  void stream_finish_beam(const int32_t* stream_ids, int n, const SvStreamBeamOut& o);
  void ensure_stream_shadow();
  void stream_init(int chunk, int look_back_encoder, int look_back_decoder, int max_streams);
  void stream_reset(int sid);
  template <typename T> void stream_step(const SvStepReq& q);
  // the streaming input format (launch_resample_stream in front of the chunk step). Per stream in HBM: its step count since the reset and the last
  // 2 W input frames as mono f32, in two halves by step parity. On the host: the same counts (what asr_paraformer_stream_input_frames answers from) and what
  // each stream holds -- 0 nothing (reset), 1 stepped at the default format (no frames), 2 stepped with a format (frames that belong to its filter).
  DeviceBuffer st_rs_count, st_rs_hist, st_rs_out;        // [st_max] int32; [2][st_max][2 W] f32; [n][chunk] f32: what the front end of a formatted step reads
  int st_rs_rate = 0;                                     // the rate st_rs_hist is laid out for (0: not yet)
  std::vector<int64_t> st_rs_steps;
  std::vector<char> st_rs_state;
  void check_input_format_change(int sample_rate, int channels) override;
  void stream_input_frames(const int32_t* stream_ids, int n, int32_t* frames_out, int32_t* pitch_out);
};

// f(T{}) with T the operand type of the session's precision: `by_precision(sv, [&](auto t) { sv->run<decltype(t)>(q); })`
template <typename F> void by_precision(const asr_session* s, F&& f) {
  if (s->precision == ASR_PRECISION_BF16) f(bf16_t{});
  else f(float{});
}
