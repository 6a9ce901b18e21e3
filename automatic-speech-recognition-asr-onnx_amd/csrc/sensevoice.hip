// SenseVoiceSmall hot path on one MI355X: packed ragged batch -> fbank -> LFR/CMVN -> SANM blocks ->
// CTC arg-max + collapse. Follows SENSE_VOICE.forward (SenseVoice/Export_SenseVoice.py:271-296). Offline Paraformer shares the encoder (sanm_session.h).
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "sanm_session.h"

void SvSession::init() {
  const auto& c = cfg;
  ASR_REQUIRE(c.d_model == c.n_heads * c.d_head, "sensevoice: d_model != n_heads * d_head");
  ASR_REQUIRE(c.d_model % 128 == 0 && c.d_ffn % 128 == 0, "sensevoice: d_model and d_ffn must be multiples of 128");
  ASR_REQUIRE(c.d_head == 128 || (precision == ASR_PRECISION_F32 && c.d_head <= 128), "sensevoice: head_dim %d unsupported", c.d_head);
  ASR_REQUIRE(c.win_length == 400 && c.hop_length == 160, "sensevoice: front-end is built for 25 ms / 10 ms frames");
  ASR_REQUIRE(c.n_mels % 16 == 0, "sensevoice: n_mels must be a multiple of 16");
  ASR_REQUIRE(c.n_blocks >= 1 && c.n_main >= 1 && c.n_main <= c.n_blocks, "sensevoice: bad block counts");
  auto opt = [&](const std::string& n, std::initializer_list<int64_t> sh) -> const float* {
    return arena.has(n) ? (const float*)arena.get(n, ARENA_F32, sh).ptr : nullptr;
  };
  feat = c.n_mels * c.lfr_m;
  kpad0 = round_up(feat, 64);
  vpad = round_up(c.vocab, 128);
  fe.init(c.nfft, c.win_length, c.hop_length, c.n_mels, 0, 1.1920928955078125e-07f);
  model_rate = c.sample_rate;
  const int n_frames_max = (c.max_audio_len - c.win_length) / c.hop_length + 1;
  max_lfr = (n_frames_max + c.lfr_n - 1) / c.lfr_n;
  const int wt = precision == ASR_PRECISION_BF16 ? ARENA_BF16 : ARENA_F32;
  const int d = c.d_model, dff = c.d_ffn;

  fe.dft = (const float*)arena.get("fe.dft", ARENA_F32, {(int64_t)fe.n_bin_tiles * 2 * fe.n_kchunks * 64 * 4}).ptr;
  if (precision == ASR_PRECISION_BF16 && use_fbank_split) {       // bf16 sessions: the DFT on the bf16 pipe with split operands (kernels.hip: fbank_split_kernel)
    d_dft_split.reserve(fbank_split_table_bytes(fe.n_bin_tiles, cfg.win_length), stream);
    launch_fbank_split_table(fe.dft, fe.n_bin_tiles, fe.n_kchunks, d_dft_split.ptr, stream);
    HIP_CHECK(hipStreamSynchronize(stream));
    fe.dft_split = d_dft_split.ptr;
  }
  fe.melp = (const float*)arena.get("fe.mel", ARENA_F32, {(int64_t)(c.n_mels / 16) * fe.n_bin_tiles * 64 * 4}).ptr;
  cmvn_means = opt("fe.cmvn_means", {feat});
  cmvn_vars = (const float*)arena.get("fe.cmvn_vars", ARENA_F32, {feat}).ptr;
  speech_pos = (const float*)arena.get("fe.speech_pos", ARENA_F32, {max_lfr, feat}).ptr;
  language_embed = c.n_prompt > 0 ? (const float*)arena.get("fe.language_embed", ARENA_F32, {c.n_languages, feat}).ptr : nullptr;
  system_embed = c.n_prompt > 1 ? (const float*)arena.get("fe.system_embed", ARENA_F32, {c.n_prompt - 1, feat}).ptr : nullptr;
  after_g = (const float*)arena.get("after_norm_g", ARENA_F32, {d}).ptr;
  after_b = (const float*)arena.get("after_norm_b", ARENA_F32, {d}).ptr;
  if (!paraformer) {
    tp_g = (const float*)arena.get("tp_norm_g", ARENA_F32, {d}).ptr;
    tp_b = (const float*)arena.get("tp_norm_b", ARENA_F32, {d}).ptr;
    ctc_w = arena.get("ctc.w", wt, {vpad, d}).ptr;
    ctc_b = (const float*)arena.get("ctc.b", ARENA_F32, {vpad}).ptr;
  } else {
    const int dd = pcfg.d_dec_ffn;
    ASR_REQUIRE(dd % 128 == 0 && dd <= 2048 && (3 * d) % 64 == 0 && pcfg.cif_kernel == 3, "paraformer: unsupported decoder geometry");
    cif_conv_w = arena.get("cif.conv_w", wt, {d, 3 * d}).ptr;
    cif_conv_b = (const float*)arena.get("cif.conv_b", ARENA_F32, {d}).ptr;
    cif_out_w = (const float*)arena.get("cif.out_w", ARENA_F32, {d}).ptr;
    cif_out_b = (const float*)arena.get("cif.out_b", ARENA_F32, {1}).ptr;
    pf_out_w = arena.get("out.w", wt, {vpad, d}).ptr;
    pf_out_b = (const float*)arena.get("out.b", ARENA_F32, {vpad}).ptr;
    pdec.resize(pcfg.n_dec + pcfg.n_dec3);
    for (int j = 0; j < (int)pdec.size(); ++j) {
      PfDecLayer& L = pdec[j];
      const std::string q = "dec" + std::to_string(j) + ".";
      L.full = j < pcfg.n_dec;
      L.w1 = arena.get(q + "w1", wt, {dd, d}).ptr;
      L.b1 = (const float*)arena.get(q + "b1", ARENA_F32, {dd}).ptr;
      L.w2 = arena.get(q + "w2", wt, {d, dd}).ptr;
      L.b2 = (const float*)arena.get(q + "b2", ARENA_F32, {d}).ptr;
      if (L.full) {
        L.n2_g = (const float*)arena.get(q + "n2_g", ARENA_F32, {d}).ptr;
        L.n2_b = (const float*)arena.get(q + "n2_b", ARENA_F32, {d}).ptr;
        L.wfsmn = (const float*)arena.get(q + "wfsmn", ARENA_F32, {d, c.fsmn_kernel}).ptr;
        L.wq = arena.get(q + "wq", wt, {d, d}).ptr;
        L.bq = (const float*)arena.get(q + "bq", ARENA_F32, {d}).ptr;
        L.wkv = arena.get(q + "wkv", wt, {2 * d, d}).ptr;
        L.bkv = (const float*)arena.get(q + "bkv", ARENA_F32, {2 * d}).ptr;
        L.wo = arena.get(q + "wo", wt, {d, d}).ptr;
        L.bo = (const float*)arena.get(q + "bo", ARENA_F32, {d}).ptr;
      }
    }
    pf_kv_batch = env_flag("ASR_PF_KV_BATCH", pf_kv_batch);
    pf_n_full = 0;
    for (const PfDecLayer& L : pdec) pf_n_full += L.full ? 1 : 0;
    if (pf_kv_batch && pf_n_full > 0) {
      const size_t ew = wt == ARENA_BF16 ? 2 : 4, wbytes = (size_t)d * d * ew;
      d_wk_all.reserve(pf_n_full * wbytes, stream); d_wv_all.reserve(pf_n_full * wbytes, stream);
      d_bk_all.reserve((size_t)pf_n_full * d * 4, stream); d_bv_all.reserve((size_t)pf_n_full * d * 4, stream);
      int li = 0;
      for (const PfDecLayer& L : pdec) {
        if (!L.full) continue;
        HIP_CHECK(hipMemcpyAsync((unsigned char*)d_wk_all.ptr + li * wbytes, L.wkv, wbytes, hipMemcpyDeviceToDevice, stream));
        HIP_CHECK(hipMemcpyAsync((unsigned char*)d_wv_all.ptr + li * wbytes, (const unsigned char*)L.wkv + wbytes, wbytes, hipMemcpyDeviceToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_bk_all.as<float>() + (size_t)li * d, L.bkv, (size_t)d * 4, hipMemcpyDeviceToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_bv_all.as<float>() + (size_t)li * d, L.bkv + d, (size_t)d * 4, hipMemcpyDeviceToDevice, stream));
        ++li;
      }
    }
  }
  blocks.resize(c.n_blocks);
  for (int i = 0; i < c.n_blocks; ++i) {
    SvBlock& b = blocks[i];
    const std::string p = "blk" + std::to_string(i) + ".";
    b.kpad = (int)arena.get(p + "wqkv").shape[1];
    b.in_size = b.kpad == d ? d : feat;
    ASR_REQUIRE(b.kpad == round_up(b.in_size, 64), "sensevoice: block %d has K = %d", i, b.kpad);
    b.ln1_g = opt(p + "ln1_g", {b.in_size});             // absent when the affine is folded into the Linear (Paraformer)
    b.ln1_b = opt(p + "ln1_b", {b.in_size});
    b.wqkv = arena.get(p + "wqkv", wt, {3 * d, b.kpad}).ptr;
    b.bqkv = (const float*)arena.get(p + "bqkv", ARENA_F32, {3 * d}).ptr;
    b.wfsmn = (const float*)arena.get(p + "wfsmn", ARENA_F32, {d, c.fsmn_kernel}).ptr;
    b.bfsmn = (const float*)arena.get(p + "bfsmn", ARENA_F32, {d}).ptr;
    b.wout = arena.get(p + "wout", wt, {d, d}).ptr;
    b.cqkv = opt(p + "cqkv", {3 * d});
    b.c1 = opt(p + "c1", {dff});
    b.ln2_g = opt(p + "ln2_g", {d});
    b.ln2_b = opt(p + "ln2_b", {d});
    b.w1 = arena.get(p + "w1", wt, {dff, d}).ptr;
    b.b1 = (const float*)arena.get(p + "b1", ARENA_F32, {dff}).ptr;
    b.w2 = arena.get(p + "w2", wt, {d, dff}).ptr;
    b.b2 = (const float*)arena.get(p + "b2", ARENA_F32, {d}).ptr;
  }
}

// fragment-major weight copies for the 8-wave block kernel: one pass over the arena's bf16 matrices per session, outside any graph capture
void SvSession::ensure_block_pack() {
  if (wpack_ready) return;
  const size_t per = sanm_block8_pack_bytes();
  d_wpack.reserve(per * cfg.n_blocks, stream);
  for (int i = 0; i < cfg.n_blocks; ++i) {
    const SvBlock& b = blocks[i];
    if (b.in_size != cfg.d_model) continue;              // (block 0 maps 560 -> 512: it keeps the separate launches)
    launch_sanm_block8_pack((const bf16_t*)b.wqkv, (const bf16_t*)b.wout, (const bf16_t*)b.w1, (const bf16_t*)b.w2, (unsigned char*)d_wpack.ptr + per * i, block_ffnk, stream);
  }
  std::vector<SanmBlockLayer> tab(cfg.n_blocks);
  for (int i = 0; i < cfg.n_blocks; ++i) {
    const SvBlock& b = blocks[i];
    tab[i] = SanmBlockLayer{b.bqkv, b.cqkv, b.wfsmn, b.bfsmn, b.b1, b.c1, b.b2, (const unsigned char*)d_wpack.ptr + per * i};
  }
  d_layer_tab.reserve(tab.size() * sizeof(SanmBlockLayer), stream);
  HIP_CHECK(hipMemcpyAsync(d_layer_tab.ptr, tab.data(), tab.size() * sizeof(SanmBlockLayer), hipMemcpyHostToDevice, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  wpack_ready = true;
}

void SvSession::copy_block_status(const SvRunCtx& r) {
  r.out->enqueue_copy(r.out->lay.status, d_flags.as<unsigned>() + (size_t)cfg.n_blocks * r.batch * 4, stream);
}

// the same for the tile kernel of small batches: the streaming encoder's image format and table entries
void SvSession::ensure_tiles_pack() {
  if (tpack_ready) return;
  const size_t per = stream_layers_pack_bytes();
  d_tpack.reserve(per * cfg.n_blocks, stream);
  std::vector<StreamLayer> tab(cfg.n_blocks);
  for (int i = 0; i < cfg.n_blocks; ++i) {
    const SvBlock& b = blocks[i];
    tab[i] = StreamLayer{};
    if (b.in_size != cfg.d_model) continue;
    unsigned char* dst = (unsigned char*)d_tpack.ptr + per * i;
    launch_stream_layers_pack((const bf16_t*)b.wqkv, (const bf16_t*)b.wout, (const bf16_t*)b.w1, (const bf16_t*)b.w2, dst, stream);
    tab[i].wpack = dst; tab[i].bqkv = b.bqkv; tab[i].wfsmn = b.wfsmn; tab[i].bfsmn = b.bfsmn; tab[i].b1 = b.b1; tab[i].b2 = b.b2;
  }
  d_tlayer_tab.reserve(tab.size() * sizeof(StreamLayer), stream);
  HIP_CHECK(hipMemcpyAsync(d_tlayer_tab.ptr, tab.data(), tab.size() * sizeof(StreamLayer), hipMemcpyHostToDevice, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  tpack_ready = true;
}

template <typename T>
void SvSession::enqueue(const SvRunCtx& r) {
  const auto& c = cfg;
  const int d = c.d_model, dff = c.d_ffn, rows = r.rows, Mpad = r.Mpad;
  const int n_slabs = vpad / 64;
  // ---- 1. Kaldi fbank (Export_SenseVoice.py:275-278) ---------------------------------------
  {
    ProfScope ps(prof, "fbank", stream);
    const FbankArgs fa = fe.args(r.d_aud, r.audio_dtype, r.dp, r.d_blk_utt, r.d_blk_f0, d_mel.as<float>(), nullptr);
    launch_fbank(fa, r.n_fb, stream);
  }
  save_tap("mel", d_mel.ptr, r.frames, c.n_mels, c.n_mels, 4);
  // LayerNorm inside the projections (bf16 mode, 8 s windows): the residual stream is kept in f32 AND as its bf16 rounding;
  // the fused attention kernel and the FFN-1 GEMM read the raw bf16 rows, accumulate the row statistics from their LDS tiles
  // and apply rstd (x W^T - mean colsum(W)) + b in the epilogue -- no LayerNorm launches, no normalised copy in memory.
  bool alg = false;
  if constexpr (sizeof(T) == 2) {
    const SvBlock& b1 = blocks[c.n_blocks - 1];
    GemmArgs probe;
    probe.M = rows; probe.N = dff; probe.K = d; probe.ln_dim = d; probe.ln_colsum = b1.c1; probe.act = ACT_RELU; probe.bias = b1.b1;
    probe.out_lo = d_ffn.ptr; probe.A = d_xblo.ptr; probe.W = b1.w1;
    // a single window is weight-streaming bound: its GEMMs take the skinny split-K kernel, which wants separately normalised rows
    const bool skinny144 = gemm_skinny144_enabled();
    alg = (rows > 144 || !skinny144) && use_ln_alg && use_fused && b1.cqkv && b1.c1 && blocks[0].cqkv &&
          sanm_fused_supported(r.max_T, c.d_head, c.n_heads, d, c.fsmn_kernel, blocks[0].kpad) && gemm_ln_fusable(probe);
  }
  bf16_t* x0lo = d_x0lo.as<bf16_t>();
  bf16_t* xalo = d_xalo.as<bf16_t>();
  bf16_t* xblo = d_xblo.as<bf16_t>();
  // ---- 2./3. LFR + CMVN + positions + prompts (Export_SenseVoice.py:280-287) ---------------
  {
    ProfScope ps(prof, "lfr_cmvn", stream);
    LfrArgs la;
    if (alg) la.out_lo = x0lo;
    la.mel = d_mel.as<float>(); la.plan = r.dp; la.row_utt = r.d_row_utt; la.cmvn_means = cmvn_means; la.cmvn_vars = cmvn_vars;
    la.speech_pos = speech_pos; la.language_embed = language_embed; la.system_embed = system_embed;
    la.out = d_x0.as<float>(); la.ld_out = kpad0; la.feat = feat; la.n_mels = c.n_mels; la.lfr_m = c.lfr_m; la.lfr_n = c.lfr_n;
    la.n_prompt = c.n_prompt; la.n_rows = Mpad; la.affine_mode = paraformer ? 1 : 0;
    launch_lfr_cmvn(la, stream);
  }
  save_tap("enc_in", d_x0.ptr, rows, feat, kpad0, 4);

  // ---- 4. SANM blocks (Export_SenseVoice.py:227-269) ---------------------------------------
  // one launch per block (csrc/sanm_block.hip) when every window fits a 144-row tile and the LayerNorms are folded into the projections
  // (it has its own tiling, so unlike `alg` it does not need batches of near-full windows: ragged batches qualify too)
  bool blk = false;
  if constexpr (sizeof(T) == 2)
    blk = use_block && block_cooldown == 0 && !foreign_now && use_ln_alg && use_fused && blocks[c.n_blocks - 1].cqkv && blocks[c.n_blocks - 1].c1 && c.n_blocks > 1 &&
          r.batch >= block_min_utts &&          // four workgroups per window: a small batch leaves most CUs idle (one window: 4 of 256), the tiled GEMMs do not
          sanm_block_supported(r.max_T, c.d_head, c.n_heads, d, dff, c.fsmn_kernel);
  const size_t flag_words = (size_t)c.n_blocks * r.batch * 4;
  const size_t tile_flag0 = flag_words + 4 + (size_t)c.n_blocks * r.batch, tile_flag_stride = ((size_t)r.n_tiles + r.batch) * 4;       // the tile kernel's counters: per block [tile][4] + [window][4]
  const bool tiles = r.tiles && block_cooldown == 0 && !foreign_now;
  HIP_CHECK(hipMemsetAsync(d_flags.ptr, 0, (tile_flag0 + (tiles ? (size_t)c.n_blocks * tile_flag_stride : 0)) * 4, stream));      // per (block, window, exchange) counters + the error word + per (launch, window) placement words
  const float* x_in = d_x0.as<float>();
  const bf16_t* x_in_lo = x0lo;
  const float2* st_in = nullptr;            // statistics of x_in_lo's rows when its producer wrote them
  bool st_in_block8 = false;                // ... by the 8-wave block kernel: one record per row and workgroup instead of one per 32 columns
  float2* sta = d_sta.as<float2>();
  float2* stb = d_stb.as<float2>();
  int ld_in = kpad0;
  float* xa = d_xa.as<float>();
  float* xb = d_xb.as<float>();
  T* h = d_h.as<T>();
  T* qk = d_qk.as<T>();
  T* vt = d_vt.as<T>();
  T* ctx = d_ctx.as<T>();
  float* mem = d_mem.as<float>();
  T* ffn = d_ffn.as<T>();
  for (int i = 0; i < c.n_blocks; ++i) {
    const SvBlock& b = blocks[i];
    if constexpr (sizeof(T) == 2) {
      if (blk && b.in_size == d && x_in == xa) {             // (block 0 maps 560 -> 512 without a residual: it keeps the separate launches)
        if (!alg && i == 1) {                                // block 0 ran without the bf16 copy / statistics outputs: make the copy, derive the statistics in the kernel
          ProfScope ps0(prof, "layernorm", stream);
          launch_rows_to_bf16(xa, xalo, (size_t)Mpad * d, stream);
          st_in = nullptr;
        }
        const int per = sanm_block_max_utts();
        // 8-wave kernel: one launch walks every block up to the next stand-alone LayerNorm (blocks 1 .. n_main - 1, then n_main .. n_blocks - 1): a window's
        // blocks depend on its own cluster only (ASR_SANM_BLOCK_PERSIST=0: one launch per block)
        const int run_end = (!paraformer && i < c.n_main) ? c.n_main : c.n_blocks;
        const int n_run = block_persist ? run_end - i : 1;
        for (int u0 = 0; u0 < r.batch; u0 += per) {
          ProfScope ps(prof, "sanm_block", stream);
          SanmBlockArgs ba{};
          ba.wqkv = (const bf16_t*)b.wqkv; ba.bqkv = b.bqkv; ba.cqkv = b.cqkv; ba.wfsmn = b.wfsmn; ba.bfsmn = b.bfsmn;
          ba.wout = (const bf16_t*)b.wout; ba.w1 = (const bf16_t*)b.w1; ba.b1 = b.b1; ba.c1 = b.c1; ba.w2 = (const bf16_t*)b.w2; ba.b2 = b.b2;
          ba.x_lo = xalo; ba.st_in = st_in; ba.x = xa; ba.x_lo_out = xalo; ba.st_out = sta;
          ba.ctx = (bf16_t*)ctx; ba.x1_lo = xblo; ba.st1 = stb; ba.hid = (bf16_t*)ffn;
          ba.plan = r.dp; ba.utt0 = u0; ba.n_utts = std::min(per, r.batch - u0);
          ba.flags = d_flags.as<unsigned>() + ((size_t)i * r.batch + u0) * 4; ba.err = d_flags.as<unsigned>() + flag_words;
          ba.flag_stride = r.batch * 4; ba.place = d_flags.as<unsigned>() + flag_words + 4 + (size_t)i * r.batch + u0;
          ba.n_rows_alloc = Mpad; ba.ln_eps = 1e-5f; ba.scatter = block_scatter; ba.fault = (block_fault && i == 1) ? 1 : 0;
          if (block_dbg >= i && block_dbg < i + n_run && u0 == 0) {
            d_times.reserve(256 * 16 * 8, stream); HIP_CHECK(hipMemsetAsync(d_times.ptr, 0, 256 * 16 * 8, stream)); ba.times = d_times.as<unsigned long long>();
            ba.times_layer = block_dbg - i;
          }
          ba.layers = d_layer_tab.as<SanmBlockLayer>() + i; ba.n_layers = n_run; ba.opt = block8_opt; ba.ffnk = block_ffnk ? 1 : 0;
          ba.st_in_n = st_in_block8 ? 4 : 16;
          launch_sanm_block8(ba, stream);
        }
        i += n_run - 1;                                        // (the loop header steps over the last block of the run)
        st_in = sta;
        st_in_block8 = true;
        if (i == c.n_main - 1 && !paraformer) {
          ProfScope ps2(prof, "layernorm", stream);
          launch_layernorm_with_bf16_copy(xa, d, rows, d, after_g, after_b, 1e-5f, xa, d, xalo, d, stream); st_in = nullptr;
        }
        continue;
      }
    }
    if constexpr (sizeof(T) == 2) {
      if (tiles && !blk && b.in_size == d && x_in == xa) {   // small batch: every block up to the next stand-alone LayerNorm in one launch of (tile, head) workgroups
        const int run_end = (!paraformer && i < c.n_main) ? c.n_main : c.n_blocks;
        {
          ProfScope ps(prof, "sanm_tiles", stream);
          SanmTilesArgs ta;
          ta.plan = r.dp; ta.tile_win = r.d_tile_win; ta.tile_idx = r.d_tile_idx; ta.n_tiles = r.n_tiles; ta.n_windows = r.batch; ta.n_layers = run_end - i;
          ta.ln_eps = 1e-5f; ta.layers = d_tlayer_tab.as<StreamLayer>() + i;
          ta.x = xa; ta.xb = xb; ta.ctx = (bf16_t*)ctx; ta.hid = (bf16_t*)ffn; ta.kv = d_tkv.as<bf16_t>(); ta.kv_parity_stride = (size_t)Mpad * 2 * d;
          ta.flags = d_flags.as<unsigned>() + tile_flag0 + (size_t)i * tile_flag_stride; ta.flag_stride = (int)tile_flag_stride;
          ta.err = d_flags.as<unsigned>() + flag_words; ta.opt = tiles_opt;
          if (tiles_dbg >= i && tiles_dbg < run_end) {
            d_times.reserve(256 * 16 * 8, stream); HIP_CHECK(hipMemsetAsync(d_times.ptr, 0, 256 * 16 * 8, stream)); ta.times = d_times.as<unsigned long long>();
            ta.times_layer = tiles_dbg - i;
          }
          launch_sanm_tiles(ta, stream);
        }
        i = run_end - 1;
        st_in = nullptr;
        if (i == c.n_main - 1 && !paraformer) {
          ProfScope ps2(prof, "layernorm", stream);
          launch_layernorm<float>(xa, d, rows, d, after_g, after_b, 1e-5f, xa, d, d, stream);
        }
        continue;
      }
    }
    if (!alg) {
      ProfScope ps(prof, "layernorm", stream);
      launch_layernorm<T>(x_in, ld_in, rows, b.in_size, b.ln1_g, b.ln1_b, 1e-5f, h, b.kpad, b.kpad, stream);
    }
    const bool fused = use_fused && precision == ASR_PRECISION_BF16 &&
                       sanm_fused_supported(r.max_T, c.d_head, c.n_heads, d, c.fsmn_kernel, b.kpad);
    if (fused) {
      ProfScope ps(prof, "sanm_fused", stream);
      SanmFusedArgs fa;
      fa.h = h; fa.ld_h = b.kpad; fa.K = b.kpad;
      if (alg) { fa.h = x_in_lo; fa.ln_colsum = b.cqkv; fa.ln_dim = b.in_size; fa.ln_stats_in = st_in; fa.ln_slots = d / 32; } fa.wqkv = b.wqkv; fa.ldw = b.kpad; fa.bqkv = b.bqkv;
      fa.wfsmn = b.wfsmn; fa.bfsmn = b.bfsmn; fa.plan = r.dp; fa.n_utts = r.batch; fa.n_heads = c.n_heads; fa.d = d;
      fa.ctx = ctx; fa.ld_ctx = d; fa.mem = mem; fa.ld_mem = d; fa.n_rows_alloc = Mpad;
      launch_sanm_qkv_attn(fa, stream);
    } else {
      {
        ProfScope ps(prof, "gemm_qkv", stream);
        GemmArgs g;                               // q | k, row-major
        g.A = h; g.lda = b.kpad; g.W = b.wqkv; g.ldw = b.kpad; g.M = rows; g.N = 2 * d; g.K = b.kpad; g.bias = b.bqkv;
        g.out_lo = qk; g.ld_out_lo = 2 * d;
        gemm(g);
        GemmArgs gv;                              // v, stored transposed (time-contiguous) for the P.V operand and the FSMN
        gv.A = h; gv.lda = b.kpad; gv.W = (const T*)b.wqkv + (size_t)2 * d * b.kpad; gv.ldw = b.kpad; gv.M = rows; gv.N = d;
        gv.K = b.kpad; gv.bias = b.bqkv + 2 * d; gv.out_t = vt; gv.ld_out_t = Mpad;
        gemm(gv);
      }
      {
        ProfScope ps(prof, "fsmn", stream);
        launch_fsmn<T>(vt, Mpad, b.wfsmn, b.bfsmn, d, c.fsmn_kernel, r.dp, r.d_row_utt, Mpad, mem, d, stream);
      }
      {
        ProfScope ps(prof, "attention", stream);
        AttnArgs aa;
        aa.q = qk; aa.k = qk + d; aa.ld_qk = 2 * d; aa.vt = vt; aa.ld_vt = Mpad; aa.ctx = ctx; aa.ld_ctx = d;
        aa.plan = r.dp; aa.qb_utt = r.d_qb_utt; aa.qb_q0 = r.d_qb_q0; aa.n_qblocks = r.n_qb; aa.n_heads = c.n_heads;
        aa.qt = r.att_qt; aa.n_waves = r.att_nw; aa.max_T = r.max_T;
        if (precision == ASR_PRECISION_BF16) launch_attention_bf16_hd128(aa, stream);
        else launch_attention_f32(aa, c.d_head, stream);
      }
    }
    {
      ProfScope ps(prof, "gemm_out", stream);
      GemmArgs g;
      g.A = ctx; g.lda = d; g.W = b.wout; g.ldw = d; g.M = rows; g.N = d; g.K = d;
      g.add = mem; g.ld_add = d;                                  // FSMN memory rides in as the GEMM's additive term (:244)
      if (b.in_size == d) { g.add2 = x_in; g.ld_add2 = ld_in; }    // residual only when in/out sizes match (:246-256)
      g.out_f32 = xb; g.ld_out_f32 = d;
      if (alg) { g.out_lo = xblo; g.ld_out_lo = d; g.st_out = stb; }
      gemm(g);
    }
    if (!alg) {
      ProfScope ps(prof, "layernorm", stream);
      launch_layernorm<T>(xb, d, rows, d, b.ln2_g, b.ln2_b, 1e-5f, h, d, d, stream);
    }
    {
      ProfScope ps(prof, "gemm_ffn1", stream);
      GemmArgs g;
      g.A = h; g.lda = d; g.W = b.w1; g.ldw = d; g.M = rows; g.N = dff; g.K = d; g.bias = b.b1; g.act = ACT_RELU;
      g.out_lo = ffn; g.ld_out_lo = dff;
      if (alg) { g.A = xblo; g.ln_colsum = b.c1; g.ln_dim = d; g.ln_stats_in = stb; g.ln_slots = d / 32; }
      gemm(g);
    }
    {
      ProfScope ps(prof, "gemm_ffn2", stream);
      GemmArgs g;
      g.A = ffn; g.lda = dff; g.W = b.w2; g.ldw = dff; g.M = rows; g.N = d; g.K = dff; g.bias = b.b2;
      g.add = xb; g.ld_add = d; g.out_f32 = xa; g.ld_out_f32 = d;
      if (alg) { g.out_lo = xalo; g.ld_out_lo = d; g.st_out = sta; }
      gemm(g);
    }
    x_in = xa;
    x_in_lo = xalo;
    st_in = sta;
    ld_in = d;
    if (i == 0) save_tap("block0", xa, rows, d, d, 4);
    if (i == c.n_main - 1 && !paraformer) {
      ProfScope ps(prof, "layernorm", stream);
      if (alg) { launch_layernorm_with_bf16_copy(xa, d, rows, d, after_g, after_b, 1e-5f, xa, d, xalo, d, stream); st_in = nullptr; }   // normed stream + its operand copy
      else launch_layernorm<float>(xa, d, rows, d, after_g, after_b, 1e-5f, xa, d, d, stream);
    }
  }
  if (paraformer) { copy_block_status(r); enqueue_paraformer_tail<T>(r); return; }
  // tp_norm -> operand dtype for the CTC GEMM (f32 copy kept only for the tap)
  if (taps_enabled) {
    launch_layernorm<float>(xa, d, rows, d, tp_g, tp_b, 1e-5f, xb, d, d, stream);
    save_tap("enc_out", xb, rows, d, d, 4);
  }
  {
    ProfScope ps(prof, "layernorm", stream);
    launch_layernorm<T>(xa, d, rows, d, tp_g, tp_b, 1e-5f, h, d, d, stream);
  }
  // ---- 5. CTC head: GEMM with fused row arg-max, then circular collapse (:290-296) ----------
  {
    ProfScope ps(prof, "gemm_ctc", stream);
    GemmArgs g;
    g.A = h; g.lda = d; g.W = ctc_w; g.ldw = d; g.M = rows; g.N = vpad; g.K = d; g.bias = ctc_b;
    g.amax_val = d_amax_v.as<float>(); g.amax_idx = d_amax_i.as<int32_t>(); g.n_valid = c.vocab;
    if (r.timed || r.beam || r.align) g.amax_sum = d_amax_s.as<float>();
    if (taps_enabled) { g.out_f32 = d_logits.as<float>(); g.ld_out_f32 = vpad; }
    gemm(g);
  }
  if (r.beam) {                                           // ---- 5b. prefix beam search over the top-k tokens of every row
    const ResultBlob& o = *r.out;
    {
      ProfScope ps(prof, "ctc_topk", stream);
      launch_ctc_topk<T>(h, d, (const T*)ctc_w, d, ctc_b, d, d_amax_v.as<float>(), d_amax_s.as<float>(), n_slabs, rows, c.vocab, r.topk, d_cand_i.as<int32_t>(),
                         d_cand_l.as<float>(), stream);
    }
    {
      ProfScope ps(prof, "ctc_beam", stream);
      const NgramLm lm = lm_view();
      launch_ctc_prefix_beam(d_cand_i.as<int32_t>(), d_cand_l.as<float>(), r.topk, r.dp, r.batch, c.blank_id, r.beam, r.nbest,
                             hot_trie_view(d_hot.as<int32_t>(), hot_nodes, hot_boost), (int2*)d_pool.ptr, r.pool_stride, o.dev(o.lay.hyp_tokens, d_bout), r.max_tokens,
                             o.dev(o.lay.hyp_counts, d_bout), o.dev(o.lay.hyp_scores, d_bout), o.dev(o.lay.hyp_ctc, d_bout), stream, &lm);
    }
    if (taps_enabled) {
      save_tap("logits", d_logits.ptr, rows, c.vocab, vpad, 4);
      save_tap("cand_ids", d_cand_i.ptr, rows, r.topk, r.topk, 4);
      save_tap("cand_logprob", d_cand_l.ptr, rows, r.topk, r.topk, 4);
    }
    copy_block_status(r);                                 // the plain outputs' sections stay unused; the beam block comes home in one copy
    o.enqueue_copy(o.lay.beam, d_bout.ptr, stream);
    return;
  }
  if (r.align) {                                          // ---- 5c. forced alignment of the caller's transcripts
    const ResultBlob& o = *r.out;
    {
      ProfScope ps(prof, "ctc_align_em", stream);
      launch_ctc_target_logprob<T>(h, d, (const T*)ctc_w, d, ctc_b, d, d_amax_v.as<float>(), d_amax_s.as<float>(), n_slabs, rows, r.d_row_utt, r.d_tgt_ids, r.d_tgt_off,
                                   c.blank_id, d_em.as<float>(), r.ld_em, stream);
    }
    {
      ProfScope ps(prof, "ctc_align", stream);
      launch_ctc_align(d_em.as<float>(), r.ld_em, r.dp, r.batch, c.n_prompt, r.max_T, r.d_tgt_ids, r.d_tgt_off, r.max_L, d_abp.as<uint32_t>(), d_first.as<int32_t>(),
                       d_last.as<int32_t>(), d_tlp.as<float>(), r.max_tokens, d_apath.as<float>(), d_alik.as<float>(), d_astat.as<int32_t>(), stream);
    }
    if (taps_enabled) {
      save_tap("logits", d_logits.ptr, rows, c.vocab, vpad, 4);
      save_tap("align_logprob", d_em.ptr, rows, r.ld_em, r.ld_em, 4);
    }
    copy_block_status(r);                                 // the token sections stay unused
    o.enqueue_copy(o.lay.first, d_first.ptr, stream); o.enqueue_copy(o.lay.last, d_last.ptr, stream); o.enqueue_copy(o.lay.logprob, d_tlp.ptr, stream);
    o.enqueue_copy(o.lay.path_score, d_apath.ptr, stream); o.enqueue_copy(o.lay.loglik, d_alik.ptr, stream); o.enqueue_copy(o.lay.align_status, d_astat.ptr, stream);
    return;
  }
  {
    ProfScope ps(prof, "ctc_tail", stream);
    if (r.timed) {
      launch_argmax_lse_reduce(d_amax_v.as<float>(), d_amax_i.as<int32_t>(), d_amax_s.as<float>(), rows, n_slabs, d_ids.as<int32_t>(), d_flp.as<float>(), stream);
      launch_ctc_collapse_timed(d_ids.as<int32_t>(), d_flp.as<float>(), r.dp, r.batch, c.blank_id, d_tok.as<int32_t>(), d_first.as<int32_t>(), d_last.as<int32_t>(),
                                d_tlp.as<float>(), r.max_tokens, d_num.as<int32_t>(), stream);
    } else {
      launch_argmax_reduce(d_amax_v.as<float>(), d_amax_i.as<int32_t>(), rows, n_slabs, d_ids.as<int32_t>(), stream);
      launch_ctc_collapse(d_ids.as<int32_t>(), r.dp, r.batch, c.blank_id, d_tok.as<int32_t>(), r.max_tokens, d_num.as<int32_t>(), stream);
    }
  }
  if (taps_enabled) {
    save_tap("logits", d_logits.ptr, rows, c.vocab, vpad, 4);
    save_tap("frame_ids", d_ids.ptr, rows, 1, 1, 4);
    if (r.timed) save_tap("frame_logprob", d_flp.ptr, rows, 1, 1, 4);
  }
  // ---- outputs (pinned host staging) ---------------------------------------------------------
  const ResultBlob& o = *r.out;
  o.enqueue_copy(o.lay.tokens, d_tok.ptr, stream);
  o.enqueue_copy(o.lay.counts, d_num.ptr, stream);
  copy_block_status(r);
  if (r.timed) { o.enqueue_copy(o.lay.first, d_first.ptr, stream); o.enqueue_copy(o.lay.last, d_last.ptr, stream); o.enqueue_copy(o.lay.logprob, d_tlp.ptr, stream); }
}

// ---- Paraformer: CIF predictor + non-autoregressive decoder (Export_Paraformer.py:497-563) ----------------------
template <typename T>
void SvSession::enqueue_paraformer_tail(const SvRunCtx& r) {
  const auto& c = cfg;
  const int d = c.d_model, dd = pcfg.d_dec_ffn, rows = r.rows, Mpad = r.Mpad, n_slabs = vpad / 64;
  float* xa = d_xa.as<float>();
  float* enc32 = d_xb.as<float>();                 // after_norm output, f32: CIF integrals
  T* enc_lo = d_enc_lo.as<T>();                    // same in the operand dtype: GEMM input (predictor conv, cross-KV)
  T* h = d_h.as<T>();
  T* q = d_qk.as<T>();
  T* ck = d_ck.as<T>();
  T* cvt = d_vt.as<T>();
  T* ctx = d_ctx.as<T>();
  T* ffn = d_ffn.as<T>();
  float* ffn32 = d_ffn32.as<float>();
  float* x1 = d_mem.as<float>();
  float* dec = d_dec.as<float>();
  float* x2 = d_x2.as<float>();
  float* x2_own = d_sa.as<float>();                    // scratch for the un-packed CIF output (sa is not live yet)
  float* sa = d_sa.as<float>();
  UttPlan* own_plan = d_tplan.as<UttPlan>();            // token rows inside each utterance's own row range (CIF scan output)
  UttPlan* tplan = d_ctplan.as<UttPlan>();              // compact token rows: the decoder works on these
  const int32_t* m_dev = d_mdev.as<int32_t>();          // their total count, device side
  const int32_t* trow_utt = d_trow.as<int32_t>();
  {
    ProfScope ps(prof, "layernorm", stream);
    launch_layernorm<float>(xa, d, rows, d, after_g, after_b, 1e-5f, enc32, d, d, stream);
    launch_layernorm<T>(xa, d, rows, d, after_g, after_b, 1e-5f, enc_lo, d, d, stream);
  }
  save_tap("enc_out", enc32, rows, d, d, 4);
  {
    ProfScope ps(prof, "cif", stream);
    launch_shift3<T>(enc_lo, d, r.dp, r.d_row_utt, Mpad, d_cifa.as<T>(), stream);     // conv k=3 (pad folded) as one GEMM
    GemmArgs g;
    g.A = d_cifa.ptr; g.lda = 3 * d; g.W = cif_conv_w; g.ldw = 3 * d; g.M = rows; g.N = d; g.K = 3 * d; g.bias = cif_conv_b; g.act = ACT_RELU;
    g.out_lo = ctx; g.ld_out_lo = d;
    gemm(g);
    launch_alpha<T>(ctx, d, cif_out_w, cif_out_b, rows, d_alpha.as<float>(), stream);
    // fired frames land in the utterance's own rows first; then they are packed (16-row aligned per utterance) so that the decoder
    // touches ~ the token count of the batch instead of every encoder row -- the count stays on the device (GemmArgs::m_dev)
    if (r.timed || r.beam)                                   // (the beam form reports the fire rows too: every hypothesis of an utterance shares them)
      launch_cif_scan_timed(d_alpha.as<float>(), enc32, d, r.dp, r.batch, pcfg.tail_threshold, x2_own, own_plan, d_num.as<int32_t>(), d_first.as<int32_t>(),
                            r.max_tokens, stream);
    else
      launch_cif_scan(d_alpha.as<float>(), enc32, d, r.dp, r.batch, pcfg.tail_threshold, x2_own, own_plan, d_num.as<int32_t>(), stream);
    launch_token_compact(own_plan, r.batch, Mpad, tplan, d_trow.as<int32_t>(), d_mdev.as<int32_t>(), stream);
    launch_compact_rows(x2_own, own_plan, tplan, r.batch, d, dec, stream);
  }
  save_tap("alphas", d_alpha.ptr, rows, 1, 1, 4);
  if (taps_enabled) save_tap("acoustic", dec, rows, d, d, 4);          // the packed token rows; like `logits`, rows at or past *m_dev hold nothing defined
  int tap_i = 0;
  auto tap_layer = [&] { if (taps_enabled) save_tap(("dec" + std::to_string(tap_i++)).c_str(), dec, rows, d, d, 4); };
  auto ffn_block = [&](const PfDecLayer& L, float* out, const float* res) {
    { ProfScope ps(prof, "layernorm", stream); launch_layernorm<T>(dec, d, rows, d, nullptr, nullptr, 1e-5f, h, d, d, stream, m_dev); }
    ProfScope ps(prof, "gemm_dec", stream);
    GemmArgs g;
    g.A = h; g.lda = d; g.W = L.w1; g.ldw = d; g.M = rows; g.N = dd; g.K = d; g.bias = L.b1; g.act = ACT_RELU; g.out_f32 = ffn32; g.ld_out_f32 = dd; g.m_dev = m_dev;
    gemm(g);
    launch_layernorm<T>(ffn32, dd, rows, dd, nullptr, nullptr, 1e-5f, ffn, dd, dd, stream, m_dev);   // ff.norm, affine folded into w_2
    GemmArgs g2;
    g2.A = ffn; g2.lda = dd; g2.W = L.w2; g2.ldw = dd; g2.M = rows; g2.N = d; g2.K = dd; g2.bias = L.b2; g2.out_f32 = out; g2.ld_out_f32 = d; g2.m_dev = m_dev;
    if (res) { g2.add = res; g2.ld_add = d; }
    gemm(g2);
  };
  const bool kv_all = pf_kv_batch && pf_n_full > 0;
  const int ld_k = kv_all ? pf_n_full * d : d;
  if (kv_all) {                                                       // every layer's cross K (row-major, layer l at columns l d ..) and V (transposed, layer l at rows l d ..) from the memory
    ProfScope ps(prof, "gemm_dec", stream);
    GemmArgs gk;
    gk.A = enc_lo; gk.lda = d; gk.W = d_wk_all.ptr; gk.ldw = d; gk.M = rows; gk.N = pf_n_full * d; gk.K = d; gk.bias = d_bk_all.as<float>(); gk.out_lo = ck; gk.ld_out_lo = ld_k;
    gemm(gk);
    GemmArgs gv;
    gv.A = enc_lo; gv.lda = d; gv.W = d_wv_all.ptr; gv.ldw = d; gv.M = rows; gv.N = pf_n_full * d; gv.K = d; gv.bias = d_bv_all.as<float>();
    gv.out_t = cvt; gv.ld_out_t = Mpad;
    gemm(gv);
  }
  int full_i = 0;
  for (const PfDecLayer& L : pdec) {
    if (!L.full) { ffn_block(L, dec, nullptr); tap_layer(); continue; }           // decoders3: dec = FFN(dec), no residual (:553-555)
    T* ck_l = kv_all ? ck + (size_t)full_i * d : ck;
    T* cvt_l = kv_all ? cvt + (size_t)full_i * d * Mpad : cvt;
    ++full_i;
    if (!kv_all) {
      ProfScope ps(prof, "gemm_dec", stream);                        // this layer's cross K (row-major) and V (transposed) from the memory
      GemmArgs gk;
      gk.A = enc_lo; gk.lda = d; gk.W = L.wkv; gk.ldw = d; gk.M = rows; gk.N = d; gk.K = d; gk.bias = L.bkv; gk.out_lo = ck; gk.ld_out_lo = d;
      gemm(gk);
      GemmArgs gv;
      gv.A = enc_lo; gv.lda = d; gv.W = (const T*)L.wkv + (size_t)d * d; gv.ldw = d; gv.M = rows; gv.N = d; gv.K = d; gv.bias = L.bkv + d;
      gv.out_t = cvt; gv.ld_out_t = Mpad;
      gemm(gv);
    }
    ffn_block(L, x1, nullptr);                                       // x = w_2(norm(relu(w_1(norm1(dec)))))
    {
      ProfScope ps(prof, "fsmn", stream);
      launch_layernorm<float>(x1, d, rows, d, L.n2_g, L.n2_b, 1e-5f, sa, d, d, stream, m_dev);
      launch_fsmn_rows(sa, dec, L.wfsmn, d, c.fsmn_kernel, tplan, trow_utt, Mpad, x2, stream, m_dev);   // x = dec + fsmn(norm2(x))
    }
    { ProfScope ps(prof, "layernorm", stream); launch_layernorm<T>(x2, d, rows, d, nullptr, nullptr, 1e-5f, h, d, d, stream, m_dev); }
    {
      ProfScope ps(prof, "gemm_dec", stream);
      GemmArgs g;
      g.A = h; g.lda = d; g.W = L.wq; g.ldw = d; g.M = rows; g.N = d; g.K = d; g.bias = L.bq; g.out_lo = q; g.ld_out_lo = d; g.m_dev = m_dev;
      gemm(g);
    }
    {
      ProfScope ps(prof, "attention", stream);
      AttnArgs aa;
      aa.q = q; aa.ld_q = d; aa.k = ck_l; aa.ld_qk = ld_k; aa.vt = cvt_l; aa.ld_vt = Mpad; aa.ctx = ctx; aa.ld_ctx = d;
      aa.plan = r.dp; aa.q_plan = tplan; aa.qb_utt = r.d_qb_utt; aa.qb_q0 = r.d_qb_q0; aa.n_qblocks = r.n_qb; aa.n_heads = c.n_heads;
      aa.qt = r.att_qt; aa.n_waves = r.att_nw; aa.max_T = r.max_T;
      if (precision == ASR_PRECISION_BF16) launch_attention_bf16_hd128(aa, stream);
      else launch_attention_f32(aa, c.d_head, stream);
    }
    {
      ProfScope ps(prof, "gemm_dec", stream);
      GemmArgs g;
      g.A = ctx; g.lda = d; g.W = L.wo; g.ldw = d; g.M = rows; g.N = d; g.K = d; g.bias = L.bo; g.add = x2; g.ld_add = d; g.out_f32 = dec; g.ld_out_f32 = d; g.m_dev = m_dev;
      gemm(g);
    }
    tap_layer();
  }
  { ProfScope ps(prof, "layernorm", stream); launch_layernorm<T>(dec, d, rows, d, nullptr, nullptr, 1e-5f, h, d, d, stream, m_dev); }
  {
    ProfScope ps(prof, "gemm_out", stream);
    GemmArgs g;
    g.A = h; g.lda = d; g.W = pf_out_w; g.ldw = d; g.M = rows; g.N = vpad; g.K = d; g.bias = pf_out_b;
    g.amax_val = d_amax_v.as<float>(); g.amax_idx = d_amax_i.as<int32_t>(); g.n_valid = c.vocab; g.m_dev = m_dev;
    if (r.timed || r.beam) g.amax_sum = d_amax_s.as<float>();         // (rows at or past *m_dev are neither computed nor stored: the epilogue's row guard uses the device-side count)
    if (taps_enabled) { g.out_f32 = d_logits.as<float>(); g.ld_out_f32 = vpad; }
    gemm(g);
    if (r.timed) {
      // reduce rows at or past the device-side token-row count merge partials nobody wrote: they hold nothing defined and the gathers below, which walk
      // the token plan, never read them
      launch_argmax_lse_reduce(d_amax_v.as<float>(), d_amax_i.as<int32_t>(), d_amax_s.as<float>(), rows, n_slabs, d_ids.as<int32_t>(), d_flp.as<float>(), stream);
      launch_gather_tokens(d_ids.as<int32_t>(), tplan, r.batch, d_tok.as<int32_t>(), r.max_tokens, stream);
      launch_gather_token_logprob(d_flp.as<float>(), tplan, r.batch, d_tlp.as<float>(), r.max_tokens, stream);
    } else if (!r.beam) {                                    // (the beam form has no row arg-max: its candidates come from the partials, below)
      launch_argmax_reduce(d_amax_v.as<float>(), d_amax_i.as<int32_t>(), rows, n_slabs, d_ids.as<int32_t>(), stream);
      launch_gather_tokens(d_ids.as<int32_t>(), tplan, r.batch, d_tok.as<int32_t>(), r.max_tokens, stream);
    }
  }
  if (r.beam) {                                          // ---- beam search over the token rows
    const ResultBlob& o = *r.out;
    {
      ProfScope ps(prof, "ctc_topk", stream);
      launch_ctc_topk<T>(h, d, (const T*)pf_out_w, d, pf_out_b, d, d_amax_v.as<float>(), d_amax_s.as<float>(), n_slabs, rows, c.vocab, r.topk, d_cand_i.as<int32_t>(),
                         d_cand_l.as<float>(), stream, m_dev);
    }
    {
      ProfScope ps(prof, "nar_beam", stream);
      const NgramLm lm = lm_view();
      launch_nar_beam(d_cand_i.as<int32_t>(), d_cand_l.as<float>(), r.topk, tplan, m_dev, r.batch, r.beam, r.nbest, hot_trie_view(d_hot.as<int32_t>(), hot_nodes, hot_boost),
                      (int2*)d_pool.ptr, r.pool_stride, o.dev(o.lay.hyp_tokens, d_bout), r.max_tokens, o.dev(o.lay.hyp_counts, d_bout), o.dev(o.lay.hyp_scores, d_bout),
                      o.dev(o.lay.hyp_ctc, d_bout), o.dev(o.lay.hyp_logprob, d_bout), stream, &lm);
    }
    if (taps_enabled) {                                   // (rows at or past *m_dev hold nothing defined, in all three)
      save_tap("logits", d_logits.ptr, rows, c.vocab, vpad, 4);
      save_tap("cand_ids", d_cand_i.ptr, rows, r.topk, r.topk, 4);
      save_tap("cand_logprob", d_cand_l.ptr, rows, r.topk, r.topk, 4);
      save_tap("fire_frames", d_first.ptr, r.batch, r.max_tokens, r.max_tokens, 4);
    }
    o.enqueue_copy(o.lay.counts, d_num.ptr, stream);      // the fire counts: how much of each fire row is valid; the token section stays unused
    o.enqueue_copy(o.lay.first, d_first.ptr, stream);
    o.enqueue_copy(o.lay.beam, d_bout.ptr, stream);
    return;
  }
  if (taps_enabled) {
    save_tap("logits", d_logits.ptr, rows, c.vocab, vpad, 4);
    if (r.timed) {
      save_tap("fire_frames", d_first.ptr, r.batch, r.max_tokens, r.max_tokens, 4);
      save_tap("token_logprob", d_tlp.ptr, r.batch, r.max_tokens, r.max_tokens, 4);
    }
  }
  const ResultBlob& o = *r.out;
  o.enqueue_copy(o.lay.tokens, d_tok.ptr, stream);
  o.enqueue_copy(o.lay.counts, d_num.ptr, stream);
  if (r.timed) { o.enqueue_copy(o.lay.first, d_first.ptr, stream); o.enqueue_copy(o.lay.logprob, d_tlp.ptr, stream); }      // fire rows and scores: result_layout.h, the Paraformer-timed form
}

void SvSession::validate(const SvRunReq& q) const {
  if (q.form == SvForm::BEAM) {
    const char* who = paraformer ? "paraformer_run_beam" : "sensevoice_run_beam";
    ASR_REQUIRE(q.beam >= 1 && q.beam <= 16 && q.topk >= 1 && q.topk <= 16 && q.nbest >= 1 && q.nbest <= q.beam && q.topk <= cfg.vocab,
                "%s: beam %d, topk %d, nbest %d (beam and topk 1..16, nbest 1..beam)", who, q.beam, q.topk, q.nbest);
    ASR_REQUIRE(q.tok_out && q.num_out && q.score_out && q.ctc_out, "%s: null output", who);
    ASR_REQUIRE(cfg.d_model <= 2048, "%s: d_model %d (the candidate kernel holds a row of 2048 at most)", who, cfg.d_model);
  }
  if (q.form == SvForm::ALIGN) {
    ASR_REQUIRE(!paraformer, "sensevoice_align: not a SenseVoice session");
    ASR_REQUIRE(q.batch > 0 && q.tgt_ids && q.tgt_off && q.first_out && q.last_out && q.logprob_out && q.path_out && q.loglik_out && q.astatus_out, "sensevoice_align: null argument");
    ASR_REQUIRE(cfg.d_model <= 2048, "sensevoice_align: d_model %d (the emission kernel holds a row of 2048 at most)", cfg.d_model);
    ASR_REQUIRE(q.tgt_off[0] == 0, "sensevoice_align: target_offsets[0] = %d", q.tgt_off[0]);
    for (int b = 0; b < q.batch; ++b) {
      ASR_REQUIRE(q.tgt_off[b + 1] >= q.tgt_off[b], "sensevoice_align: target_offsets decrease at utterance %d", b);
      ASR_REQUIRE(q.tgt_off[b + 1] - q.tgt_off[b] <= 1023, "sensevoice_align: utterance %d has %d targets (at most 1023)", b, q.tgt_off[b + 1] - q.tgt_off[b]);
      for (int32_t i = q.tgt_off[b]; i < q.tgt_off[b + 1]; ++i) {
        ASR_REQUIRE(q.tgt_ids[i] >= 0 && q.tgt_ids[i] < cfg.vocab, "sensevoice_align: utterance %d holds token %d (vocabulary %d)", b, q.tgt_ids[i], cfg.vocab);
        ASR_REQUIRE(q.tgt_ids[i] != cfg.blank_id, "sensevoice_align: utterance %d holds the blank id", b);
      }
    }
  }
  ASR_REQUIRE(q.form != SvForm::TIMED || (q.first_out && q.logprob_out && (paraformer ? !q.last_out : q.last_out != nullptr)),
              "sensevoice: the timed form needs all of its outputs");
  ASR_REQUIRE(q.batch > 0, "sensevoice: empty batch");
  ASR_REQUIRE(q.audio && q.offs && (q.lang || paraformer) && (q.form == SvForm::ALIGN || (q.tok_out && q.num_out)), "sensevoice: null argument");
}

template <typename T>
void SvSession::run(const SvRunReq& q) {
  const auto& c = cfg;
  validate(q);
  const bool timed = q.form == SvForm::TIMED, bq = q.form == SvForm::BEAM, al = q.form == SvForm::ALIGN;
  const int32_t* const lang = q.lang;
  const int batch = q.batch;
  HIP_CHECK(hipSetDevice(device));
  // a non-default input format is resampled here, in front of everything the step graphs capture: the plan below sees model-rate lengths, and a captured step
  // reads the resampler's buffer (its address and the f32 type are in the key), so it is the same step whatever format filled that buffer
  const AudioIn in = stage_input(*this, false, q.audio, q.audio_mem, q.offs, batch);
  const int64_t* const offs = in.offs;
  int max_L = 0;
  if (al) for (int b = 0; b < batch; ++b) max_L = std::max(max_L, q.tgt_off[b + 1] - q.tgt_off[b]);
  const int max_tokens = al ? std::max(max_L, 1) : q.max_tokens;          // the align form's token sections are as wide as its longest transcript
  const int n_tgt = al ? q.tgt_off[batch] : 0, ld_em = round_up(max_L + 1, 4);
  // no cluster kernel beside a foreign (RCCL) section: this whole call -- it returns with the stream drained -- is one cluster pass, or takes the four-launch path
  ClusterScope cluster(device);
  foreign_now = !cluster.ok;
  if (foreign_now) ++foreign_diverted;
  const int d = c.d_model, dff = c.d_ffn;

  // ---- host plan -------------------------------------------------------------------------
  std::vector<UttPlan> plan(batch);
  SvRunCtx r{};
  int rows = 0, frames = 0, n_fb = 0, n_qb = 0, max_T = 0;
  const int64_t base0 = offs[0];
  GraphKey key;                                          // everything that shapes the launch sequence
  for (int b = 0; b < batch; ++b) {
    UttPlan& p = plan[b];
    fe.plan_utt("sensevoice", b, offs, c.max_audio_len, p, frames, n_fb);
    ASR_REQUIRE(paraformer || (lang[b] >= 0 && lang[b] < c.n_languages), "sensevoice: language_idx %d out of range", lang[b]);
    p.n_lfr = (p.n_frames + c.lfr_n - 1) / c.lfr_n;
    p.T = p.n_lfr + c.n_prompt;
    p.row_off = rows;
    p.lang = lang ? lang[b] : 0;
    rows += round_up(p.T, 16);
    max_T = std::max(max_T, p.T);
    key.mix((uint64_t)p.n_samples);
  }
  ASR_REQUIRE(max_tokens >= 1, "sensevoice: max_tokens must be positive");
  int att_qt = 0, att_nw = 4, q_rows = 64;             // f32 kernel: fixed 64-row query blocks
  if (precision == ASR_PRECISION_BF16) { attention_geometry(max_T, c.d_head, &att_qt, &att_nw); q_rows = 16 * att_qt * att_nw; }
  for (int b = 0; b < batch; ++b) n_qb += (plan[b].T + q_rows - 1) / q_rows;
  const int Mpad = round_up(rows, 128);

  // plan blob: [UttPlan x B][blk_utt n_fb][blk_f0 n_fb][qb_utt n_qb][qb_q0 n_qb][row_utt Mpad][tile_win n_tiles][tile_idx n_tiles]
  const int n_tiles = rows / 16;
  PlanBlob pb(h_plan, d_plan);
  const auto s_plan = pb.add<UttPlan>(batch);
  const auto s_blk_utt = pb.add<int32_t>(n_fb), s_blk_f0 = pb.add<int32_t>(n_fb), s_qb_utt = pb.add<int32_t>(n_qb), s_qb_q0 = pb.add<int32_t>(n_qb);
  const auto s_row_utt = pb.add<int32_t>(Mpad), s_tile_win = pb.add<int32_t>(n_tiles), s_tile_idx = pb.add<int32_t>(n_tiles);
  PlanSection<int32_t> s_tgt_ids{}, s_tgt_off{};         // the align form's transcripts ride behind the sections every form has
  if (al) { s_tgt_ids = pb.add<int32_t>(std::max(n_tgt, 1)); s_tgt_off = pb.add<int32_t>(batch + 1); }
  pb.commit(stream);
  if (pb.host_moved) ++ws_epoch;                        // (any re-allocation invalidates the captured graph)
  if (pb.dev_moved) ++ws_epoch;
  memcpy(pb.host(s_plan), plan.data(), sizeof(UttPlan) * batch);
  if (al) {
    pb.host(s_tgt_ids)[0] = 0;
    memcpy(pb.host(s_tgt_ids), q.tgt_ids, (size_t)n_tgt * 4);
    memcpy(pb.host(s_tgt_off), q.tgt_off, (size_t)(batch + 1) * 4);
  }
  fill_fbank_blocks(plan.data(), batch, pb.host(s_blk_utt), pb.host(s_blk_f0));
  fill_query_blocks(plan.data(), batch, q_rows, pb.host(s_qb_utt), pb.host(s_qb_q0));
  {
    int32_t *row_utt = pb.host(s_row_utt), *tile_win = pb.host(s_tile_win), *tile_idx = pb.host(s_tile_idx);
    int ti = 0;
    for (int b = 0; b < batch; ++b) {
      const int r16 = round_up(plan[b].T, 16);
      for (int t = 0; t < r16; ++t) row_utt[plan[b].row_off + t] = b;
      for (int t = 0; t < r16 / 16; ++t) { tile_win[ti] = b; tile_idx[ti++] = t; }
    }
    for (int t = rows; t < Mpad; ++t) row_utt[t] = -1;
  }
  // small batches take the tile kernel (bf16, LayerNorm-folded arenas of the standard geometry, every workgroup resident at once)
  const bool tiles = sizeof(T) == 2 && use_tiles && c.n_blocks > 1 && blocks[c.n_blocks - 1].cqkv && blocks[c.n_blocks - 1].c1 &&
                     !(use_block && batch >= block_min_utts) && n_tiles <= sanm_tiles_max_tiles() &&
                     sanm_tiles_supported(max_T, d, dff, c.n_heads, c.d_head, c.fsmn_kernel);
  key.mix((uint64_t)tiles);
  // ---- workspace (grow-only; any re-allocation invalidates the captured graph) -----------------
  const size_t eT = sizeof(T);
  auto grow = [&](DeviceBuffer& buf, size_t bytes) { if (reserve_moved(buf, bytes, stream)) ++ws_epoch; };
  ResultBlob out(h_out, ResultLayout(batch, max_tokens, bq ? (paraformer ? ResultForm::PF_BEAM : ResultForm::SV_BEAM) : al ? ResultForm::SV_ALIGN : !timed ? ResultForm::PLAIN : paraformer ? ResultForm::PF_TIMED : ResultForm::SV_TIMED, bq ? q.nbest : 1));
  if (out.commit()) ++ws_epoch;
  r.out = &out;
  bool audio_moved = false;
  r.d_aud = stage_audio(*this, d_audio, in, base0, offs[batch] - base0, &audio_moved);
  r.audio_dtype = in.dtype;
  if (audio_moved) ++ws_epoch;
  grow(d_mel, (size_t)frames * c.n_mels * 4);
  grow(d_x0, (size_t)Mpad * kpad0 * 4);
  for (DeviceBuffer* b : {&d_xa, &d_xb, &d_mem}) grow(*b, (size_t)Mpad * d * 4);
  grow(d_h, (size_t)Mpad * std::max(kpad0, d) * eT);
  if (precision == ASR_PRECISION_BF16) {
    grow(d_x0lo, (size_t)Mpad * kpad0 * 2);
    for (DeviceBuffer* b : {&d_xalo, &d_xblo}) grow(*b, (size_t)Mpad * d * 2);
    for (DeviceBuffer* b : {&d_sta, &d_stb}) grow(*b, (size_t)Mpad * (d / 32) * 8);
  }
  grow(d_qk, (size_t)Mpad * 2 * d * eT);
  for (DeviceBuffer* b : {&d_vt, &d_ctx}) grow(*b, (size_t)Mpad * d * eT);
  grow(d_ffn, (size_t)Mpad * dff * eT);
  const int n_slabs = vpad / 64;
  for (DeviceBuffer* b : {&d_amax_v, &d_amax_i}) grow(*b, (size_t)Mpad * n_slabs * 4);
  grow(d_ids, (size_t)Mpad * 4);
  grow(d_flags, ((size_t)c.n_blocks * batch * 5 + 4 + (tiles ? (size_t)c.n_blocks * (n_tiles + batch) * 4 : 0)) * 4);
  if (tiles) grow(d_tkv, (size_t)Mpad * 2 * d * 2 * 2);          // [block][window][4] exchange counters + error word (4) + [block][window] placement words
  grow(d_tok, (size_t)batch * max_tokens * 4);
  grow(d_num, (size_t)batch * 4);
  if (taps_enabled) grow(d_logits, (size_t)Mpad * vpad * 4);
  if (timed) {
    grow(d_amax_s, (size_t)Mpad * n_slabs * 4);
    grow(d_flp, (size_t)Mpad * 4);
    for (DeviceBuffer* b : {&d_first, &d_last, &d_tlp}) grow(*b, (size_t)batch * max_tokens * 4);
  }
  if (al) {
    grow(d_amax_s, (size_t)Mpad * n_slabs * 4);
    grow(d_em, (size_t)Mpad * ld_em * 4);
    for (DeviceBuffer* b : {&d_first, &d_last, &d_tlp}) grow(*b, (size_t)batch * max_tokens * 4);
    for (DeviceBuffer* b : {&d_apath, &d_alik, &d_astat}) grow(*b, (size_t)batch * 4);
    grow(d_abp, ctc_align_ws_bytes(batch, max_T, c.n_prompt, max_L));     // 0 when the backpointers fit in LDS
  }
  if (bq) {
    auto grow_beam = [&](DeviceBuffer& buf, size_t bytes) { if (reserve_moved(buf, bytes, stream)) ++beam_epoch; };
    grow(d_amax_s, (size_t)Mpad * n_slabs * 4);
    for (DeviceBuffer* b : {&d_cand_i, &d_cand_l}) grow_beam(*b, (size_t)Mpad * q.topk * 4);
    grow_beam(d_pool, (size_t)batch * (max_T + (paraformer ? 1 : 0)) * q.beam * sizeof(int2));      // (the CIF scan fires at most T + 1 tokens: the tail threshold is row T)
    grow_beam(d_bout, out.lay.bytes(out.lay.beam));
    if (paraformer) grow(d_first, (size_t)batch * max_tokens * 4);
  }
  if (paraformer) {
    const int dd = pcfg.d_dec_ffn;
    grow(d_enc_lo, (size_t)Mpad * d * eT);
    grow(d_ck, (size_t)Mpad * d * eT * (pf_kv_batch ? std::max(pf_n_full, 1) : 1));
    if (pf_kv_batch) grow(d_vt, (size_t)Mpad * d * eT * std::max(pf_n_full, 1));
    grow(d_cifa, (size_t)Mpad * 3 * d * eT);
    for (DeviceBuffer* b : {&d_alpha, &d_trow}) grow(*b, (size_t)Mpad * 4);
    for (DeviceBuffer* b : {&d_dec, &d_x2, &d_sa}) grow(*b, (size_t)Mpad * d * 4);
    grow(d_ffn32, (size_t)Mpad * dd * 4);
    grow(d_ffn, (size_t)Mpad * std::max(dd, dff) * eT);
    for (DeviceBuffer* b : {&d_tplan, &d_ctplan}) grow(*b, sizeof(UttPlan) * batch);
    grow(d_mdev, 256);
  }
  pb.upload(stream);
  r.batch = batch; r.rows = rows; r.Mpad = Mpad; r.frames = frames; r.n_fb = n_fb; r.n_qb = n_qb; r.max_T = max_T;
  r.max_tokens = max_tokens; r.att_qt = att_qt; r.att_nw = att_nw;
  r.dp = pb.dev(s_plan);
  r.n_tiles = n_tiles; r.tiles = tiles; r.timed = timed;
  if (bq) { r.beam = q.beam; r.topk = q.topk; r.nbest = q.nbest; r.pool_stride = (max_T + (paraformer ? 1 : 0)) * q.beam; }
  if (al) { r.align = true; r.max_L = max_L; r.ld_em = ld_em; r.d_tgt_ids = pb.dev(s_tgt_ids); r.d_tgt_off = pb.dev(s_tgt_off); }
  r.d_blk_utt = pb.dev(s_blk_utt); r.d_blk_f0 = pb.dev(s_blk_f0); r.d_qb_utt = pb.dev(s_qb_utt); r.d_qb_q0 = pb.dev(s_qb_q0);
  r.d_row_utt = pb.dev(s_row_utt); r.d_tile_win = pb.dev(s_tile_win); r.d_tile_idx = pb.dev(s_tile_idx);
  // (the result blob adds nothing to the key: its offsets are functions of batch, max_tokens, timed and nbest, all mixed in here; a moved h_out bumps ws_epoch)
  key.mix((uint64_t)batch); key.mix((uint64_t)max_tokens); key.mix((uint64_t)(uintptr_t)r.d_aud); key.mix((uint64_t)in.dtype); key.mix((uint64_t)in.resampled); key.mix(ws_epoch); key.mix((uint64_t)(uintptr_t)stream);
  key.mix((uint64_t)(block_cooldown > 0 || foreign_now));        // a session cooling down after a cluster give-up replays the four-launch capture, not the block one
  key.mix((uint64_t)timed);                                      // the timed CTC tail is another launch sequence
  if (al) {                                                      // the align tail, per transcript length: ld_em, the trellis launch, where the plan blob's sections lie
    key.mix((uint64_t)q.form);
    for (int b = 0; b < batch; ++b) key.mix((uint64_t)(q.tgt_off[b + 1] - q.tgt_off[b]));
  }
  if (bq) {                                                      // ... and so is the beam tail, per (beam, topk, nbest), hotword list and boost, language model and weights
    uint32_t boost_bits; memcpy(&boost_bits, &hot_boost, 4);
    key.mix((uint64_t)q.beam); key.mix((uint64_t)q.topk); key.mix((uint64_t)q.nbest); key.mix(beam_epoch); key.mix((uint64_t)hot_nodes); key.mix((uint64_t)boost_bits);
    uint32_t lm_bits[3]; memcpy(lm_bits, &lm_alpha, 4); memcpy(lm_bits + 1, &lm_beta, 4); memcpy(lm_bits + 2, &lm_oov, 4);
    key.mix((uint64_t)lm_header[1]); key.mix((uint64_t)lm_header[2]); key.mix((uint64_t)lm_bits[0]); key.mix((uint64_t)lm_bits[1]); key.mix((uint64_t)lm_bits[2]);
  }

  if (sizeof(T) == 2 && use_block && cfg.n_blocks > 1 && blocks[cfg.n_blocks - 1].cqkv && blocks[cfg.n_blocks - 1].c1 && batch >= block_min_utts &&
      sanm_block_supported(max_T, cfg.d_head, cfg.n_heads, cfg.d_model, cfg.d_ffn, cfg.fsmn_kernel))
    ensure_block_pack();
  if (tiles) ensure_tiles_pack();
  // ---- launch: eager the first time a geometry is seen (allocations settle), then capture once and replay ----
  // 570 launches per forward are host-launch-bound when issued eagerly (~13 us each); replay costs ~1 us per node.
  (bq ? graph_beam : al ? graph_align : timed ? graph_timed : graph).run(stream, use_graph && !taps_enabled && !prof.enabled, key.h, [&] { enqueue<T>(r); });
  HIP_CHECK(hipStreamSynchronize(stream));
  if (prof.enabled) prof.collect();
  char title[48];
  if (tiles_dbg >= 0 && tiles && d_times.ptr) {          // tuning: mean phase intervals of one block of the tile kernel over its workgroups
    snprintf(title, sizeof title, "sanm_tiles block %d", tiles_dbg);
    dump_phase_clocks(d_times, 256, 1, 13, nullptr, title);
  }
  if (block_dbg >= 0 && d_times.ptr) {                   // ... and the 8-wave kernel's, per named phase
    static const char* const names8[14] = {"A loop (4 chunks)", "stats+images+attention", "ctx store+publish", "fsmn", "B prologue+wait 0", "B loop", "B epilogue+publish", "C wait 1+stats",
                                           "C loop", "C epilogue (hid)", "publish 2", "D own chunk+wait 2", "D loop (rest)", "D epilogue"};
    snprintf(title, sizeof title, "sanm_block %d", block_dbg);
    dump_phase_clocks(d_times, 256, 1, 14, names8, title, (block8_opt & 2048) != 0);
  }
  {
    // The four workgroups of a cluster must be resident together. That holds when the launch has the chip to itself; when another stream's
    // kernels hold CUs (several sessions in flight) a cluster can be split across dispatch waves and, in the worst case, wait in a circle
    // with another session's clusters until the bounded spin gives up. Such a forward pass is void: it is redone here on the four-launch
    // path (no cross-workgroup waits), still on the GPU; the error is raised only if that fails too.
    const uint32_t* blk_err = out.host(out.lay.status);
    if (*blk_err != 0 && (use_block || use_tiles)) {
      if (block_giveups++ == 0)
        fprintf(stderr, "[asr_mi355x] sanm_block: a workgroup gave up waiting for its cluster; the batch is redone on the four-launch path\n");
      block_cooldown = 16;                       // this batch and the next ones stay on the four-launch path
      enqueue<T>(r);
      HIP_CHECK(hipStreamSynchronize(stream));
    }
    else if (block_cooldown > 0) --block_cooldown;
    ASR_REQUIRE(*blk_err == 0, "sensevoice: a SANM block workgroup gave up waiting for its cluster (results are invalid)");
  }
  const ResultLayout& L = out.lay;
  if (bq) {
    memcpy(q.num_out, out.host(L.hyp_counts), L.bytes(L.hyp_counts));
    memcpy(q.score_out, out.host(L.hyp_scores), L.bytes(L.hyp_scores));
    memcpy(q.ctc_out, out.host(L.hyp_ctc), L.bytes(L.hyp_ctc));
    out.scatter_rows(L.hyp_tokens, q.tok_out, q.num_out, max_tokens);
    if (paraformer) {                                    // the hypotheses' token log-probabilities, and the fire rows every hypothesis of an utterance shares
      if (q.hyp_logprob_out) out.scatter_rows(L.hyp_logprob, q.hyp_logprob_out, q.num_out, max_tokens);
      if (q.first_out) out.scatter_rows(L.first, q.first_out, out.host(L.counts), max_tokens);
    }
    return;
  }
  if (al) {                                              // ragged, in the layout of the targets; an utterance without an alignment keeps the caller's fill
    memcpy(q.path_out, out.host(L.path_score), L.bytes(L.path_score));
    memcpy(q.loglik_out, out.host(L.loglik), L.bytes(L.loglik));
    memcpy(q.astatus_out, out.host(L.align_status), L.bytes(L.align_status));
    for (int b = 0; b < batch; ++b) {
      if (q.astatus_out[b] != 0) continue;
      const size_t n = (size_t)(q.tgt_off[b + 1] - q.tgt_off[b]) * 4, src = (size_t)b * max_tokens, dst = q.tgt_off[b];
      memcpy(q.first_out + dst, out.host(L.first) + src, n);
      memcpy(q.last_out + dst, out.host(L.last) + src, n);
      memcpy(q.logprob_out + dst, out.host(L.logprob) + src, n);
    }
    return;
  }
  memcpy(q.num_out, out.host(L.counts), L.bytes(L.counts));
  out.scatter_rows(L.tokens, q.tok_out, q.num_out, max_tokens);
  if (timed) {
    out.scatter_rows(L.first, q.first_out, q.num_out, max_tokens);
    if (L.has(L.last)) out.scatter_rows(L.last, q.last_out, q.num_out, max_tokens);
    out.scatter_rows(L.logprob, q.logprob_out, q.num_out, max_tokens);
  }
}

void SvSession::set_hotwords(const int32_t* ids, const int32_t* offsets, int n_phrases, float boost) {
  const char* who = kind == 4 ? "paraformer_stream_set_hotwords" : paraformer ? "paraformer_set_hotwords" : "sensevoice_set_hotwords";      // (Paraformer has no blank: cfg.blank_id is -1 and no id is refused for it)
  ASR_REQUIRE(n_phrases >= 0 && (n_phrases == 0 || (ids && offsets)) && std::isfinite(boost), "%s: bad argument", who);
  HIP_CHECK(hipSetDevice(device));
  if (n_phrases == 0) { hot_nodes = 0; hot_boost = 0.0f; ++beam_epoch; return; }
  ASR_REQUIRE(offsets[0] >= 0, "%s: offsets[0] = %d", who, offsets[0]);
  for (int p = 0; p < n_phrases; ++p) {
    ASR_REQUIRE(offsets[p + 1] > offsets[p], "%s: phrase %d is empty", who, p);
    for (int32_t i = offsets[p]; i < offsets[p + 1]; ++i) {
      ASR_REQUIRE(ids[i] >= 0 && ids[i] < cfg.vocab, "%s: phrase %d holds token %d (vocabulary %d)", who, p, ids[i], cfg.vocab);
      ASR_REQUIRE(ids[i] != cfg.blank_id, "%s: phrase %d holds the blank id", who, p);
    }
  }
  int n_nodes = 0;
  const std::vector<int32_t> img = build_hot_trie(ids, offsets, n_phrases, &n_nodes);
  HIP_CHECK(hipStreamSynchronize(stream));
  d_hot.reserve(img.size() * 4, stream);
  HIP_CHECK(hipMemcpyAsync(d_hot.ptr, img.data(), img.size() * 4, hipMemcpyHostToDevice, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  hot_nodes = n_nodes; hot_boost = boost;
  ++beam_epoch;                                          // the trie's words are graph-kernel operands: a captured beam step is stale
}

// The image is checked in full before it replaces the one in force (a rejected image changes nothing); its words are graph-kernel operands like the trie's.
void SvSession::set_lm(const int32_t* image_words, int64_t n_words, float alpha, float beta, float oov_logprob) {
  const char* who = kind == 4 ? "paraformer_stream_set_lm" : paraformer ? "paraformer_set_lm" : "sensevoice_set_lm";                  // (Paraformer: the image check is told "no blank", cfg.blank_id = -1)
  ASR_REQUIRE(n_words >= 0 && (n_words == 0 || image_words), "%s: bad argument", who);
  HIP_CHECK(hipSetDevice(device));
  if (n_words == 0) { lm_header[1] = 0; lm_alpha = lm_beta = lm_oov = 0.0f; ++beam_epoch; return; }
  ngram_lm_validate(image_words, n_words, cfg.vocab, cfg.blank_id, alpha, beta, oov_logprob, who);
  HIP_CHECK(hipStreamSynchronize(stream));
  d_lm.reserve((size_t)n_words * 4, stream);
  HIP_CHECK(hipMemcpyAsync(d_lm.ptr, image_words, (size_t)n_words * 4, hipMemcpyHostToDevice, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  memcpy(lm_header, image_words, sizeof lm_header);
  lm_alpha = alpha; lm_beta = beta; lm_oov = oov_logprob;
  ++beam_epoch;                                          // a captured beam step is stale
}

namespace {
// a session of `kind` on `device_id`: `configure` fills in the model's geometry, then the switches, the stream, the arena and the weights' pointers
template <typename F>
SvSession* create_session(int kind, const void* arena, size_t arena_bytes, int arena_mem, int device_id, int precision, F&& configure) {
  asr_require_device(device_id);
  SvSession* s = new SvSession();
  try {
    s->kind = kind;
    s->device = device_id;
    asr_tenant_attach(s);
    s->precision = precision;
    configure(*s);
    s->load_env();
    HIP_CHECK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    s->own_stream = true;
    s->arena.load(arena, arena_bytes, arena_mem, s->stream);
    s->init();
  } catch (...) {
    delete s;
    throw;
  }
  return s;
}
}  // namespace

extern "C" int asr_sensevoice_create(const asr_sensevoice_config* cfg, const void* arena, size_t arena_bytes, int arena_mem,
                                     int device_id, int precision, asr_session** out) {
  return asr_guard([&] {
    ASR_REQUIRE(cfg && arena && out, "sensevoice_create: null argument");
    ASR_REQUIRE(precision == ASR_PRECISION_BF16 || precision == ASR_PRECISION_F32, "sensevoice_create: bad precision %d", precision);
    *out = create_session(1, arena, arena_bytes, arena_mem, device_id, precision, [&](SvSession& s) { s.cfg = *cfg; });
  });
}

namespace {
// what every offline form asks for; the timed and the beam entries add their outputs
SvRunReq run_req(SvForm form, const void* audio, int audio_mem, const int64_t* offs, int batch, const int32_t* lang, int32_t* tok_out, int max_tokens, int32_t* num_out) {
  SvRunReq q;
  q.form = form; q.audio = audio; q.audio_mem = audio_mem; q.offs = offs; q.batch = batch; q.lang = lang; q.tok_out = tok_out; q.max_tokens = max_tokens; q.num_out = num_out;
  return q;
}
void run_entry(asr_session* s, const SvRunReq& q) {
  TenantScope tenant(s);
  SvSession* sv = static_cast<SvSession*>(s);
  by_precision(sv, [&](auto t) { sv->run<decltype(t)>(q); });
}
}  // namespace

extern "C" int asr_sensevoice_run(asr_session* s, const void* audio, int audio_mem, const int64_t* audio_offsets, int batch,
                                  const int32_t* language_idx, int32_t* token_ids_out, int max_tokens, int32_t* num_id_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 1, "sensevoice_run: not a SenseVoice session");
    run_entry(s, run_req(SvForm::PLAIN, audio, audio_mem, audio_offsets, batch, language_idx, token_ids_out, max_tokens, num_id_out));
  });
}

extern "C" int asr_sensevoice_run_timed(asr_session* s, const void* audio, int audio_mem, const int64_t* audio_offsets, int batch,
                                        const int32_t* language_idx, int32_t* token_ids_out, int max_tokens, int32_t* num_id_out,
                                        int32_t* first_frame_out, int32_t* last_frame_out, float* logprob_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 1, "sensevoice_run_timed: not a SenseVoice session");
    ASR_REQUIRE(first_frame_out && last_frame_out && logprob_out, "sensevoice_run_timed: null span output");
    SvRunReq q = run_req(SvForm::TIMED, audio, audio_mem, audio_offsets, batch, language_idx, token_ids_out, max_tokens, num_id_out);
    q.first_out = first_frame_out; q.last_out = last_frame_out; q.logprob_out = logprob_out;
    run_entry(s, q);
  });
}

extern "C" int asr_sensevoice_seq_len(const asr_sensevoice_config* cfg, int n_samples, int* seq_len) {
  return asr_guard([&] {
    ASR_REQUIRE(cfg && seq_len, "seq_len: null argument");
    ASR_REQUIRE(n_samples >= cfg->win_length, "seq_len: fewer samples than one frame");
    const int frames = (n_samples - cfg->win_length) / cfg->hop_length + 1;
    *seq_len = (frames + cfg->lfr_n - 1) / cfg->lfr_n + cfg->n_prompt;
  });
}

extern "C" int asr_paraformer_create(const asr_paraformer_config* cfg, const void* arena, size_t arena_bytes, int arena_mem,
                                     int device_id, int precision, asr_session** out) {
  return asr_guard([&] {
    ASR_REQUIRE(cfg && arena && out, "paraformer_create: null argument");
    ASR_REQUIRE(precision == ASR_PRECISION_BF16 || precision == ASR_PRECISION_F32, "paraformer_create: bad precision %d", precision);
    *out = create_session(3, arena, arena_bytes, arena_mem, device_id, precision, [&](SvSession& s) {
      s.paraformer = true;
      s.pcfg = *cfg;
      asr_sensevoice_config& c = s.cfg;
      memset(&c, 0, sizeof(c));
      c.sample_rate = cfg->sample_rate; c.n_mels = cfg->n_mels; c.nfft = cfg->nfft; c.win_length = cfg->win_length; c.hop_length = cfg->hop_length;
      c.lfr_m = cfg->lfr_m; c.lfr_n = cfg->lfr_n; c.d_model = cfg->d_model; c.n_heads = cfg->n_heads; c.d_head = cfg->d_head; c.d_ffn = cfg->d_ffn;
      c.n_blocks = cfg->n_blocks; c.n_main = cfg->n_blocks; c.fsmn_kernel = cfg->fsmn_kernel; c.vocab = cfg->vocab; c.blank_id = -1;
      c.n_prompt = 0; c.n_languages = 0; c.max_audio_len = cfg->max_audio_len;
    });
  });
}

extern "C" int asr_sensevoice_run_beam(asr_session* s, const void* audio, int audio_mem, const int64_t* audio_offsets, int batch,
                                       const int32_t* language_idx, int beam, int topk, int nbest, int32_t* token_ids_out, int max_tokens,
                                       int32_t* num_id_out, float* score_out, float* ctc_score_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 1, "sensevoice_run_beam: not a SenseVoice session");
    SvRunReq q = run_req(SvForm::BEAM, audio, audio_mem, audio_offsets, batch, language_idx, token_ids_out, max_tokens, num_id_out);
    q.beam = beam; q.topk = topk; q.nbest = nbest; q.score_out = score_out; q.ctc_out = ctc_score_out;
    run_entry(s, q);
  });
}

extern "C" int asr_sensevoice_align(asr_session* s, const void* audio, int audio_mem, const int64_t* audio_offsets, int batch, const int32_t* language_idx,
                                    const int32_t* target_ids, const int32_t* target_offsets, int32_t* first_frame_out, int32_t* last_frame_out,
                                    float* token_logprob_out, float* path_score_out, float* loglik_out, int32_t* status_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && (s->kind == 1 || s->kind == 3), "sensevoice_align: not a SenseVoice session");
    SvRunReq q = run_req(SvForm::ALIGN, audio, audio_mem, audio_offsets, batch, language_idx, nullptr, 0, nullptr);
    q.tgt_ids = target_ids; q.tgt_off = target_offsets; q.first_out = first_frame_out; q.last_out = last_frame_out; q.logprob_out = token_logprob_out;
    q.path_out = path_score_out; q.loglik_out = loglik_out; q.astatus_out = status_out;
    run_entry(s, q);
  });
}

extern "C" int asr_sensevoice_set_lm(asr_session* s, const int32_t* image_words, int64_t n_words, float alpha, float beta, float oov_logprob) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 1, "sensevoice_set_lm: not a SenseVoice session");
    static_cast<SvSession*>(s)->set_lm(image_words, n_words, alpha, beta, oov_logprob);
  });
}

extern "C" int asr_sensevoice_set_hotwords(asr_session* s, const int32_t* ids, const int32_t* offsets, int n_phrases, float boost) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 1, "sensevoice_set_hotwords: not a SenseVoice session");
    static_cast<SvSession*>(s)->set_hotwords(ids, offsets, n_phrases, boost);
  });
}

extern "C" int asr_sanm_stats(asr_session* s, int32_t* out8) {
  return asr_guard([&] {
    ASR_REQUIRE(s && (s->kind == 1 || s->kind == 3 || s->kind == 4) && out8, "sanm_stats: not a SenseVoice / Paraformer session");
    SvSession* sv = static_cast<SvSession*>(s);
    out8[0] = sv->block_giveups; out8[1] = sv->block_cooldown; out8[2] = sv->foreign_diverted; out8[3] = sv->use_block ? 1 : 0;
    out8[4] = out8[5] = out8[6] = out8[7] = 0;
  });
}

extern "C" int asr_paraformer_run(asr_session* s, const void* audio, int audio_mem, const int64_t* audio_offsets, int batch,
                                  int32_t* token_ids_out, int max_tokens, int32_t* num_id_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 3, "paraformer_run: not a Paraformer session");
    run_entry(s, run_req(SvForm::PLAIN, audio, audio_mem, audio_offsets, batch, nullptr, token_ids_out, max_tokens, num_id_out));
  });
}

extern "C" int asr_paraformer_run_timed(asr_session* s, const void* audio, int audio_mem, const int64_t* audio_offsets, int batch,
                                        int32_t* token_ids_out, int max_tokens, int32_t* num_id_out, int32_t* fire_frame_out, float* logprob_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 3, "paraformer_run_timed: not a Paraformer session");
    ASR_REQUIRE(fire_frame_out && logprob_out, "paraformer_run_timed: null timed output");
    SvRunReq q = run_req(SvForm::TIMED, audio, audio_mem, audio_offsets, batch, nullptr, token_ids_out, max_tokens, num_id_out);
    q.first_out = fire_frame_out; q.logprob_out = logprob_out;
    run_entry(s, q);
  });
}

extern "C" int asr_paraformer_run_beam(asr_session* s, const void* audio, int audio_mem, const int64_t* audio_offsets, int batch, int beam, int topk, int nbest,
                                       int32_t* token_ids_out, int max_tokens, int32_t* num_id_out, float* score_out, float* am_score_out, int32_t* fire_frame_out,
                                       float* token_logprob_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 3, "paraformer_run_beam: not a Paraformer session");
    SvRunReq q = run_req(SvForm::BEAM, audio, audio_mem, audio_offsets, batch, nullptr, token_ids_out, max_tokens, num_id_out);
    q.beam = beam; q.topk = topk; q.nbest = nbest; q.score_out = score_out; q.ctc_out = am_score_out; q.first_out = fire_frame_out; q.hyp_logprob_out = token_logprob_out;
    run_entry(s, q);
  });
}

extern "C" int asr_paraformer_set_hotwords(asr_session* s, const int32_t* ids, const int32_t* offsets, int n_phrases, float boost) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 3, "paraformer_set_hotwords: not an offline Paraformer session");
    static_cast<SvSession*>(s)->set_hotwords(ids, offsets, n_phrases, boost);
  });
}

extern "C" int asr_paraformer_set_lm(asr_session* s, const int32_t* image_words, int64_t n_words, float alpha, float beta, float oov_logprob) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 3, "paraformer_set_lm: not an offline Paraformer session");
    static_cast<SvSession*>(s)->set_lm(image_words, n_words, alpha, beta, oov_logprob);
  });
}
