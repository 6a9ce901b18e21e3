// Streaming Paraformer on one MI355X: the SANM session (sanm_session.h) advanced chunk by chunk, per-stream recurrent state in HBM. Host code only: the
// kernels are in kernels.hip, stream_layers.hip and stream_dec.hip.
// Follows Paraformer/Streaming/Export_Paraformer_Streaming.py:386-553; host loop Inference_..._Streaming_ONNX.py:401-449.
#include <cstring>
#include <type_traits>

#include "sanm_session.h"

void SvSession::stream_init(int chunk, int look_back_encoder, int look_back_decoder, int max_streams) {
  const auto& c = cfg;
  ASR_REQUIRE(paraformer, "streaming: needs a Paraformer session");
  ASR_REQUIRE(chunk >= c.win_length && max_streams >= 1 && look_back_encoder >= 1 && look_back_decoder >= 1, "streaming: bad geometry");
  st_chunk = chunk;
  st_frames = (chunk - c.win_length) / c.hop_length + 1;
  st_B = ((c.lfr_m - 1) / 2 + st_frames) / c.lfr_n + 1;
  st_C = st_B / 2;
  st_en_cap = look_back_encoder * st_B;
  st_de_cap = look_back_decoder * st_B;
  st_max = max_streams;
  ASR_REQUIRE(st_B + st_C <= 16 && st_frames <= 64 && st_en_cap + st_B + st_C <= 64 && st_de_cap + st_B + st_C <= 64 && c.d_head == 128,
              "streaming: chunk of %d samples gives %d + %d rows per step (16-row slots, 64-key attention)", chunk, st_C, st_B);
  const size_t T = precision == ASR_PRECISION_BF16 ? 2 : 4;
  const size_t head_row = (size_t)c.n_heads * 128;
  st_enk.reserve((size_t)c.n_blocks * max_streams * st_en_cap * head_row * T, stream);
  st_env.reserve((size_t)c.n_blocks * max_streams * st_en_cap * head_row * T, stream);
  st_dek.reserve((size_t)pcfg.n_dec * max_streams * st_de_cap * head_row * T, stream);
  st_dev.reserve((size_t)pcfg.n_dec * max_streams * st_de_cap * head_row * T, stream);
  st_defsmn.reserve((size_t)pcfg.n_dec * max_streams * (c.fsmn_kernel - 1) * c.d_model * 4, stream);
  st_prev.reserve((size_t)max_streams * st_C * kpad0 * 4, stream);
  st_cifh.reserve((size_t)max_streams * c.d_model * 4, stream);
  st_cifa.reserve((size_t)max_streams * 4, stream);
  st_enlen.reserve((size_t)max_streams * 4, stream);
  st_delen.reserve((size_t)max_streams * 4, stream);
  st_start.reserve((size_t)max_streams * 4, stream);
  // bf16 sessions of the standard geometry: layers 1 .. n - 1 of a chunk step run as one launch (layer 0 has the 560-wide input and no residual)
  st_fused_env = env_int("ASR_STREAM_FUSED", st_fused_env);
  st_times_layer = env_int("ASR_STREAM_TIMES", st_times_layer);
  st_opt = env_int("ASR_STREAM_OPT", st_opt);
  st_fused_max = gemm_env_cus() * 3 / 4;               // 192 streams on 256 CUs: tools/probes/stream_fused_sweep.sh (profiles/r05_stream_fused_sweep.txt) -- the cluster launches step by CU-loads of 64 streams
                                                       // (2.5 / 5.2 / 7.8 / 10.4 ms), the per-launch path grows smoothly (5.3 ms at 64, 8.1 at 192, 8.9 at 256) and is ahead from 193 on
  st_fused_max = env_int("ASR_STREAM_FUSED_MAX", st_fused_max);
  st_share_rule = env_int("ASR_STREAM_SHARE", st_share_rule);
  st_snapshot_env = env_int("ASR_STREAM_SNAPSHOT", st_snapshot_env);
  st_fault = env_int("ASR_STREAM_FAULT", st_fault);
  st_fused = st_fused_env != 0 && precision == ASR_PRECISION_BF16 && c.n_blocks > 1 &&
             stream_layers_supported(c.d_model, c.d_ffn, c.n_heads, st_en_cap, st_B + st_C, c.fsmn_kernel) && blocks[1].kpad == c.d_model;
  if (st_fused) {
    const int nl = c.n_blocks - 1;
    const size_t pk = stream_layers_pack_bytes(), en_layer = (size_t)st_max * c.n_heads * st_en_cap * 128;
    st_wpack.reserve(pk * nl, stream);
    st_layer_tab.reserve(sizeof(StreamLayer) * nl, stream);
    st_flags.reserve(((size_t)nl * st_max * 4 + 4 + (size_t)pdec.size() * st_max * 8) * 4, stream);       // encoder counters, err, decoder counters
    std::vector<StreamLayer> tab(nl);
    for (int i = 0; i < nl; ++i) {
      const SvBlock& b = blocks[i + 1];
      unsigned char* dst = (unsigned char*)st_wpack.ptr + pk * i;
      launch_stream_layers_pack((const bf16_t*)b.wqkv, (const bf16_t*)b.wout, (const bf16_t*)b.w1, (const bf16_t*)b.w2, dst, stream);
      tab[i].wpack = dst; tab[i].bqkv = b.bqkv; tab[i].wfsmn = b.wfsmn; tab[i].bfsmn = b.bfsmn; tab[i].b1 = b.b1; tab[i].b2 = b.b2;
      tab[i].cache_k = st_enk.as<bf16_t>() + (size_t)(i + 1) * en_layer;
      tab[i].cache_v = st_env.as<bf16_t>() + (size_t)(i + 1) * en_layer;
    }
    HIP_CHECK(hipMemcpyAsync(st_layer_tab.ptr, tab.data(), sizeof(StreamLayer) * nl, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
  }
  // ... and so does the decoder (every block of it)
  st_dec_fused = st_fused && st_fused_env >= 2 && !pdec.empty() &&
                 stream_dec_supported(c.d_model, pcfg.d_dec_ffn, c.n_heads, st_de_cap, st_B + st_C, c.fsmn_kernel);
  if (st_dec_fused) {
    const int ndl = (int)pdec.size();
    const size_t pk = stream_dec_pack_bytes(), de_layer = (size_t)st_max * c.n_heads * st_de_cap * 128, fs_layer = (size_t)st_max * (c.fsmn_kernel - 1) * c.d_model;
    st_dpack.reserve(pk * ndl, stream);
    st_dlayer_tab.reserve(sizeof(StreamDecLayer) * ndl, stream);
    std::vector<StreamDecLayer> tab(ndl);
    int li = 0;
    for (int j = 0; j < ndl; ++j) {
      const PfDecLayer& L = pdec[j];
      unsigned char* dst = (unsigned char*)st_dpack.ptr + pk * j;
      launch_stream_dec_pack((const bf16_t*)L.w1, (const bf16_t*)L.w2, (const bf16_t*)L.wq, (const bf16_t*)L.wkv, (const bf16_t*)L.wo, L.full, dst, stream);
      StreamDecLayer& t = tab[j];
      t = StreamDecLayer{};
      t.wpack = dst; t.b1 = L.b1; t.b2 = L.b2; t.full = L.full ? 1 : 0;
      if (L.full) {
        t.n2_g = L.n2_g; t.n2_b = L.n2_b; t.wfsmn = L.wfsmn; t.bq = L.bq; t.bkv = L.bkv; t.bo = L.bo;
        t.fsmn_hist = st_defsmn.as<float>() + (size_t)li * fs_layer;
        t.cache_k = st_dek.as<bf16_t>() + (size_t)li * de_layer;
        t.cache_v = st_dev.as<bf16_t>() + (size_t)li * de_layer;
        ++li;
      }
    }
    HIP_CHECK(hipMemcpyAsync(st_dlayer_tab.ptr, tab.data(), sizeof(StreamDecLayer) * ndl, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
  }
  st_rs_count.reserve((size_t)max_streams * 4, stream);
  st_rs_steps.assign(max_streams, 0);
  st_rs_state.assign(max_streams, 0);
  stream_reset(-1);
}

void SvSession::ensure_stream_shadow() {
  if (st_n_segs) return;
  const auto& c = cfg;
  const size_t T = precision == ASR_PRECISION_BF16 ? 2 : 4, head_row = (size_t)c.n_heads * 128;
  struct Spec { DeviceBuffer* buf; size_t per_stream; int n_outer; };
  const Spec specs[] = {
      {&st_enk, st_en_cap * head_row * T, c.n_blocks}, {&st_env, st_en_cap * head_row * T, c.n_blocks},
      {&st_dek, st_de_cap * head_row * T, pcfg.n_dec}, {&st_dev, st_de_cap * head_row * T, pcfg.n_dec},
      {&st_defsmn, (size_t)(c.fsmn_kernel - 1) * c.d_model * 4, pcfg.n_dec}, {&st_prev, (size_t)st_C * kpad0 * 4, 1},
      {&st_cifh, (size_t)c.d_model * 4, 1}, {&st_cifa, 4, 1}, {&st_enlen, 4, 1}, {&st_delen, 4, 1}, {&st_start, 4, 1}};
  size_t total = 0;
  for (const Spec& sp : specs) total += (sp.per_stream * st_max * sp.n_outer + 255) / 256 * 256;
  st_shadow.reserve(total, stream);
  std::vector<StreamStateSeg> segs;
  size_t off = 0;
  int item = 0;
  for (const Spec& sp : specs) {
    if (sp.per_stream == 0 || sp.n_outer == 0) continue;
    StreamStateSeg g;
    g.live = (unsigned char*)sp.buf->ptr; g.shadow = (unsigned char*)st_shadow.ptr + off;
    g.per_stream = sp.per_stream; g.outer_stride = sp.per_stream * st_max; g.n_outer = sp.n_outer; g.first_item = item;
    segs.push_back(g);
    item += sp.n_outer;
    off += (sp.per_stream * st_max * sp.n_outer + 255) / 256 * 256;
  }
  st_segs.reserve(sizeof(StreamStateSeg) * segs.size(), stream);
  HIP_CHECK(hipMemcpyAsync(st_segs.ptr, segs.data(), sizeof(StreamStateSeg) * segs.size(), hipMemcpyHostToDevice, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  st_n_segs = (int)segs.size(); st_n_items = item;
}

void SvSession::stream_reset(int sid) {
  const auto& c = cfg;
  ASR_REQUIRE(st_max > 0 && sid >= -1 && sid < st_max, "streaming: stream id %d out of range", sid);
  HIP_CHECK(hipSetDevice(device));
  const int lo = sid < 0 ? 0 : sid, cnt = sid < 0 ? st_max : 1;
  // K/V histories are guarded by their length counters; the additive state must really be zero
  HIP_CHECK(hipMemsetAsync(st_enlen.as<int32_t>() + lo, 0, (size_t)cnt * 4, stream));
  HIP_CHECK(hipMemsetAsync(st_delen.as<int32_t>() + lo, 0, (size_t)cnt * 4, stream));
  HIP_CHECK(hipMemsetAsync(st_start.as<int32_t>() + lo, 0, (size_t)cnt * 4, stream));
  HIP_CHECK(hipMemsetAsync(st_cifa.as<float>() + lo, 0, (size_t)cnt * 4, stream));
  HIP_CHECK(hipMemsetAsync(st_cifh.as<float>() + (size_t)lo * c.d_model, 0, (size_t)cnt * c.d_model * 4, stream));
  HIP_CHECK(hipMemsetAsync(st_prev.as<float>() + (size_t)lo * st_C * kpad0, 0, (size_t)cnt * st_C * kpad0 * 4, stream));
  const size_t hist = (size_t)(c.fsmn_kernel - 1) * c.d_model;
  for (int l = 0; l < pcfg.n_dec; ++l)
    HIP_CHECK(hipMemsetAsync(st_defsmn.as<float>() + ((size_t)l * st_max + lo) * hist, 0, (size_t)cnt * hist * 4, stream));
  if (sb_beam > 0) {                                     // the stream's search too: zeroed words are a cleared stream (nar_stream_beam.hip)
    HIP_CHECK(hipMemsetAsync(st_bstate.as<int32_t>() + (size_t)lo * sb_words, 0, (size_t)cnt * sb_words * 4, stream));
    std::fill(sb_len.begin() + lo, sb_len.begin() + lo + cnt, 0);
  }
  // the streaming input format: step count 0, no carried frames (frames in front of a stream's first are zeros: both halves)
  HIP_CHECK(hipMemsetAsync(st_rs_count.as<int32_t>() + lo, 0, (size_t)cnt * 4, stream));
  if (st_rs_hist.ptr && st_rs_rate) {
    const int keep = resample_stream_keep(resampler.table(st_rs_rate, model_rate, stream).d);
    for (int half = 0; half < 2 && keep > 0; ++half)
      HIP_CHECK(hipMemsetAsync(st_rs_hist.as<float>() + ((size_t)half * st_max + lo) * keep, 0, (size_t)cnt * keep * 4, stream));
  }
  std::fill(st_rs_steps.begin() + lo, st_rs_steps.begin() + lo + cnt, 0);
  std::fill(st_rs_state.begin() + lo, st_rs_state.begin() + lo + cnt, 0);
  HIP_CHECK(hipStreamSynchronize(stream));
}

// ---- the streaming input format (asr_mi355x.h) ---------------------------------------------------------------------------------------
void SvSession::check_input_format_change(int, int) {
  if (st_max <= 0) return;
  for (int i = 0; i < st_max; ++i)
    ASR_REQUIRE(st_rs_state[i] != 2, "input format: stream %d holds audio history (it was stepped with the format in force and not reset since: its carried frames belong to "
                "that filter); reset it first", i);
}

void SvSession::stream_input_frames(const int32_t* stream_ids, int n, int32_t* frames_out, int32_t* pitch_out) {
  ASR_REQUIRE(st_max > 0, "paraformer_stream_input_frames: session was not created with asr_paraformer_stream_create");
  ASR_REQUIRE((stream_ids && frames_out) || n == 0, "paraformer_stream_input_frames: null argument");
  ASR_REQUIRE(n >= 0 && pitch_out, "paraformer_stream_input_frames: bad argument (n = %d)", n);
  ResampleDesign d{};
  if (in_rate) { HIP_CHECK(hipSetDevice(device)); d = resampler.table(in_rate, model_rate, stream).d; }
  *pitch_out = in_rate ? resample_stream_pitch(d, st_chunk) : st_chunk;
  for (int i = 0; i < n; ++i) {
    const int id = stream_ids[i];
    ASR_REQUIRE(id >= 0 && id < st_max, "paraformer_stream_input_frames: stream id %d out of range", id);
    ASR_REQUIRE(!in_rate || st_rs_state[id] != 1, "input format: stream %d was stepped at the default format and not reset since; until the reset of such a stream "
                "streaming sessions take model-rate mono for it", id);
    frames_out[i] = in_rate ? resample_stream_need(d, st_chunk, st_rs_steps[id]) : st_chunk;
  }
}

// ---- the streaming beam search (the build's own mode) -----------------------------------------------------------------------------
void SvSession::stream_set_beam(int beam, int topk, int nbest, int pend_cap) {
  ASR_REQUIRE(st_max > 0, "paraformer_stream_set_beam: session was not created with asr_paraformer_stream_create");
  ASR_REQUIRE(!stream_search_history(), "paraformer_stream_set_beam: a stream holds search history; finish or reset it first");
  HIP_CHECK(hipSetDevice(device));
  HIP_CHECK(hipStreamSynchronize(stream));
  if (beam == 0) {                                       // off: the state is freed
    sb_beam = sb_topk = sb_nbest = sb_cap = sb_words = 0;
    st_bstate.release(); st_bfinal.release();
    sb_len.clear();
    return;
  }
  ASR_REQUIRE(beam >= 1 && beam <= 16 && topk >= 1 && topk <= BEAM_MAX && topk <= cfg.vocab && nbest >= 1 && nbest <= beam && pend_cap >= 1 && pend_cap <= NAR_STREAM_PEND_MAX,
              "paraformer_stream_set_beam: beam %d (1..16), topk %d (1..%d), nbest %d (1..beam), pend_cap %d (1..%d)", beam, topk, BEAM_MAX, nbest, pend_cap, NAR_STREAM_PEND_MAX);
  const int words = nar_stream_beam_state_words(beam, pend_cap);
  st_bstate.reserve((size_t)st_max * words * 4, stream);
  HIP_CHECK(hipMemsetAsync(st_bstate.ptr, 0, (size_t)st_max * words * 4, stream));
  st_bfinal.reserve((size_t)st_max * 4, stream);
  const std::vector<int32_t> ones(st_max, 1);
  HIP_CHECK(hipMemcpyAsync(st_bfinal.ptr, ones.data(), (size_t)st_max * 4, hipMemcpyHostToDevice, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  sb_beam = beam; sb_topk = topk; sb_nbest = nbest; sb_cap = pend_cap; sb_words = words;
  sb_len.assign(st_max, 0);
}

// The candidates of the step's token rows and the search, or (rows == 0) the finish: enqueued once, behind a validated step and outside every captured graph,
// so a step that was redone on the per-launch path advances the search state exactly once. The second synchronisation of a beam step is here.
void SvSession::stream_search(const ResultBlob& out, const UttPlan* token_plan, const int32_t* stream_ids, int n, int rows, bool final, const SvStreamBeamOut& o) {
  const ResultLayout& lay = out.lay;
  d_bout.reserve(lay.bytes(lay.beam), stream);
  if (rows > 0) {                                        // the log soft-max pairs of every row of the step's slots, lower id on ties as the greedy pick
    d_cand_i.reserve((size_t)rows * sb_topk * 4, stream);
    d_cand_l.reserve((size_t)rows * sb_topk * 4, stream);
    ProfScope ps(prof, "beam_topk", stream);
    launch_beam_topk(d_logits.as<float>(), vpad, rows, cfg.vocab, nullptr, sb_topk, d_cand_l.as<float>(), d_cand_i.as<int32_t>(), stream);
  }
  {
    ProfScope ps(prof, "nar_stream_beam", stream);
    const NgramLm lm = lm_view();
    NarStreamOut so;
    so.commit_ids = out.dev(lay.commit_ids, d_bout); so.commit_lp = out.dev(lay.commit_logprob, d_bout); so.commit_cap = (int)lay.commit_cap;
    so.commit_num = out.dev(lay.commit_num, d_bout); so.pend_ids = out.dev(lay.pend_ids, d_bout); so.pend_lp = out.dev(lay.pend_logprob, d_bout);
    so.pend_num = out.dev(lay.pend_num, d_bout); so.pend_score = out.dev(lay.pend_score, d_bout); so.pend_am = out.dev(lay.pend_am, d_bout);
    so.total = out.dev(lay.total_rows, d_bout);
    launch_nar_stream_beam(d_cand_i.as<int32_t>(), d_cand_l.as<float>(), sb_topk, token_plan, nullptr, final ? st_bfinal.as<int32_t>() : nullptr, n, sb_beam, sb_nbest, sb_cap,
                           hot_trie_view(d_hot.as<int32_t>(), hot_nodes, hot_boost), st_bstate.as<int32_t>(), sb_words, so, stream, &lm);
  }
  if (taps_enabled && rows > 0) {                         // (only the token rows of a slot hold candidates of a decoder row)
    save_tap("cand_ids", d_cand_i.ptr, rows, sb_topk, sb_topk, 4);
    save_tap("cand_logprob", d_cand_l.ptr, rows, sb_topk, sb_topk, 4);
  }
  out.enqueue_copy(lay.beam, d_bout.ptr, stream);
  HIP_CHECK(hipStreamSynchronize(stream));
  if (prof.enabled) prof.collect();
  const size_t cc = lay.commit_cap, nb = sb_nbest, pc = sb_cap;
  memcpy(o.commit_num, out.host(lay.commit_num), lay.bytes(lay.commit_num));
  memcpy(o.total, out.host(lay.total_rows), lay.bytes(lay.total_rows));
  memcpy(o.pend_num, out.host(lay.pend_num), lay.bytes(lay.pend_num));
  memcpy(o.pend_score, out.host(lay.pend_score), lay.bytes(lay.pend_score));
  memcpy(o.pend_am, out.host(lay.pend_am), lay.bytes(lay.pend_am));
  for (int i = 0; i < n; ++i) {                          // rows hold their counts' worth of entries, the rest of the caller's arrays stays untouched
    const size_t nc = (size_t)std::min<int64_t>(std::max(o.commit_num[i], 0), (int64_t)cc);
    memcpy(o.commit_ids + i * cc, out.host(lay.commit_ids) + i * cc, nc * 4);
    memcpy(o.commit_logprob + i * cc, out.host(lay.commit_logprob) + i * cc, nc * 4);
    for (size_t m = 0; m < nb; ++m) {
      const size_t at = (i * nb + m) * pc, np = (size_t)std::min<int64_t>(std::max(o.pend_num[i * nb + m], 0), (int64_t)pc);
      memcpy(o.pend_ids + at, out.host(lay.pend_ids) + at, np * 4);
      memcpy(o.pend_logprob + at, out.host(lay.pend_logprob) + at, np * 4);
    }
    sb_len[stream_ids[i]] = final ? 0 : o.total[i];
  }
}

void SvSession::stream_finish_beam(const int32_t* stream_ids, int n, const SvStreamBeamOut& o) {
  ASR_REQUIRE(st_max > 0 && sb_beam > 0, "paraformer_stream_finish_beam: the beam mode is off (asr_paraformer_stream_set_beam)");
  ASR_REQUIRE(stream_ids && n >= 1 && n <= st_max && o.complete(), "paraformer_stream_finish_beam: bad argument (n = %d)", n);
  HIP_CHECK(hipSetDevice(device));
  std::vector<char> seen(st_max, 0);
  PlanBlob pb(h_plan, d_plan);
  const auto s_plan = pb.add<UttPlan>(n);
  pb.commit(stream);
  UttPlan* hp = pb.host(s_plan);
  for (int i = 0; i < n; ++i) {
    ASR_REQUIRE(stream_ids[i] >= 0 && stream_ids[i] < st_max && !seen[stream_ids[i]], "paraformer_stream_finish_beam: stream id %d invalid or repeated", stream_ids[i]);
    seen[stream_ids[i]] = 1;
    memset(&hp[i], 0, sizeof(UttPlan));
    hp[i].row_off = i * 16; hp[i].lang = stream_ids[i];  // no rows: n_lfr = 0
  }
  ResultBlob out(h_out, ResultLayout(n, 0, ResultForm::PF_STREAM_BEAM, sb_nbest, sb_cap));
  out.commit();
  pb.upload(stream);
  stream_search(out, pb.dev(s_plan), stream_ids, n, 0, true, o);
}

template <typename T>
void SvSession::stream_step(const SvStepReq& q) {
  const auto& c = cfg;
  const int32_t* const stream_ids = q.stream_ids;
  const int n = q.n, max_tokens = q.max_tokens;
  const bool beam = q.form == SvForm::STREAM_BEAM;      // the timed step, then (behind its validation, below) the candidates and the search
  const bool timed = q.form == SvForm::TIMED || beam;
  ASR_REQUIRE(st_max > 0, "streaming: session was not created with asr_paraformer_stream_create");
  ASR_REQUIRE(!beam || (sb_beam > 0 && q.beam_out.complete()), "streaming: the beam step needs the mode on (asr_paraformer_stream_set_beam) and all of its outputs");
  ASR_REQUIRE(q.audio && stream_ids && q.tok_out && q.num_out && n >= 1 && n <= st_max && max_tokens >= st_B + 1, "streaming: bad argument (n = %d)", n);
  ASR_REQUIRE(!timed || (q.fire_out && q.logprob_out), "streaming: the timed step needs both of its outputs");
  HIP_CHECK(hipSetDevice(device));
  ClusterScope cluster(device);                          // (as in run(): fused = cluster kernels; a foreign section open on this GPU sends the step down the per-launch path)
  foreign_now = !cluster.ok;
  if (foreign_now) ++foreign_diverted;
  const int d = c.d_model, dff = c.d_ffn, dd = pcfg.d_dec_ffn, H = c.n_heads, n_cur = st_B + st_C;
  const int rows = n * 16, Mpad = round_up(rows, 128), frames = n * st_frames, n_slabs = vpad / 64;
  std::vector<char> seen(st_max, 0);
  // ---- a non-default input format: the step's rows are frames at in_rate, resampled per stream in front of the fbank launch (inside the captured step: its geometry
  // is the streams' own step counts on the device). The first formatted step at a rate lays the carried frames out for its filter; no stream holds any then.
  const bool fmt = in_rate != 0;
  const Resampler::Table* rs = fmt ? &resampler.table(in_rate, model_rate, stream) : nullptr;
  const int rs_pitch = fmt ? resample_stream_pitch(rs->d, st_chunk) : 0, rs_keep = fmt ? resample_stream_keep(rs->d) : 0;
  if (fmt) {
    ASR_REQUIRE(in_channels >= 1 && in_channels <= 8, "input format: %d channels (1..8)", in_channels);
    if (st_rs_rate != in_rate) {
      st_rs_hist.reserve(std::max<size_t>((size_t)2 * st_max * rs_keep * 4, 16), stream);
      HIP_CHECK(hipMemsetAsync(st_rs_hist.ptr, 0, std::max<size_t>((size_t)2 * st_max * rs_keep * 4, 16), stream));
      st_rs_rate = in_rate;
    }
    st_rs_out.reserve((size_t)n * st_chunk * 4, stream);
  }
  // ---- plan: one 16-row slot / one fbank workgroup per active stream
  // plan blob: [UttPlan n][blk_utt n][blk_f0 n][row_utt Mpad]
  PlanBlob pb(h_plan, d_plan);
  const auto s_plan = pb.add<UttPlan>(n);
  const auto s_blk_utt = pb.add<int32_t>(n), s_blk_f0 = pb.add<int32_t>(n), s_row_utt = pb.add<int32_t>(Mpad);
  pb.commit(stream);                                     // (this step's graphs are keyed on the buffers themselves)
  UttPlan* hp = pb.host(s_plan);
  int32_t *blk_utt = pb.host(s_blk_utt), *blk_f0 = pb.host(s_blk_f0), *row_utt = pb.host(s_row_utt);
  for (int i = 0; i < n; ++i) {
    ASR_REQUIRE(stream_ids[i] >= 0 && stream_ids[i] < st_max && !seen[stream_ids[i]], "streaming: stream id %d invalid or repeated", stream_ids[i]);
    seen[stream_ids[i]] = 1;
    ASR_REQUIRE(!fmt || st_rs_state[stream_ids[i]] != 1, "input format: stream %d was stepped at the default format and not reset since; until the reset of such a stream "
                "streaming sessions take model-rate mono for it", stream_ids[i]);
    UttPlan& p = hp[i];
    p.audio_off = (int64_t)i * st_chunk; p.n_samples = st_chunk; p.n_frames = st_frames; p.frame_off = i * st_frames;
    p.n_lfr = st_B; p.T = n_cur; p.row_off = i * 16; p.lang = stream_ids[i]; p.blk0 = i;
    blk_utt[i] = i; blk_f0[i] = 0;
    for (int t = 0; t < 16; ++t) row_utt[i * 16 + t] = i;
  }
  for (int t = rows; t < Mpad; ++t) row_utt[t] = -1;
  const size_t eT = sizeof(T);
  auto grow = [&](DeviceBuffer& buf, size_t bytes) { buf.reserve(bytes, stream); };
  // (one fixed-size copy either way: n chunks, or n rows of rs_pitch frames)
  const void* d_raw = stage_audio(*this, d_audio, AudioIn{q.audio, q.audio_mem, nullptr, audio_dtype, false}, 0, fmt ? (int64_t)n * rs_pitch * in_channels : (int64_t)n * st_chunk);
  const void* d_aud = fmt ? st_rs_out.ptr : d_raw;       // what the front end reads
  const int fe_dtype = fmt ? AUDIO_F32 : audio_dtype;
  bool resample_now = fmt;                               // (a step that is redone behind a give-up keeps the samples and the advanced counts of its first pass)
  grow(d_mel, (size_t)frames * c.n_mels * 4);
  grow(d_x0, (size_t)Mpad * kpad0 * 4);
  grow(d_xa, (size_t)Mpad * d * 4);
  grow(d_xb, (size_t)Mpad * d * 4);
  grow(d_h, (size_t)Mpad * std::max(kpad0, d) * eT);
  grow(d_sqkv, (size_t)Mpad * 3 * d * eT);
  grow(d_skv, (size_t)Mpad * 2 * d * eT);
  grow(d_qk, (size_t)Mpad * 2 * d * eT);
  grow(d_ctx, (size_t)Mpad * d * eT);
  grow(d_mem, (size_t)Mpad * d * 4);
  grow(d_ffn, (size_t)Mpad * std::max(dd, dff) * eT);
  grow(d_amax_v, (size_t)Mpad * n_slabs * 4);
  grow(d_amax_i, (size_t)Mpad * n_slabs * 4);
  grow(d_ids, (size_t)Mpad * 4);
  grow(d_tok, (size_t)n * max_tokens * 4);
  grow(d_num, (size_t)n * 4);
  grow(d_logits, (size_t)Mpad * vpad * 4);
  grow(d_enc_lo, (size_t)Mpad * d * eT);
  grow(d_cifa, (size_t)Mpad * 3 * d * eT);
  grow(d_alpha, (size_t)Mpad * 4);
  grow(d_dec, (size_t)Mpad * d * 4);
  grow(d_x2, (size_t)Mpad * d * 4);
  grow(d_sa, (size_t)Mpad * d * 4);
  grow(d_ffn32, (size_t)Mpad * dd * 4);
  grow(d_tplan, sizeof(UttPlan) * n);
  if (timed) {
    if (!st_zero.ptr) {                                 // made by the first timed step: a session that never asks for times allocates what it always did
      st_zero.reserve(256, stream);
      HIP_CHECK(hipMemsetAsync(st_zero.ptr, 0, 256, stream));
    }
    grow(d_flp, (size_t)Mpad * 4);
    grow(d_first, (size_t)n * max_tokens * 4);
    grow(d_tlp, (size_t)n * max_tokens * 4);
  }
  if (precision == ASR_PRECISION_BF16) {                // LayerNorm inside the per-launch layers' projections (see the layer loop): bf16 copies of the residual stream + their row statistics
    grow(d_xblo, (size_t)Mpad * d * 2);
    grow(d_stb, (size_t)Mpad * (d / 32) * 8);
  }
  ResultBlob out(h_out, beam ? ResultLayout(n, max_tokens, ResultForm::PF_STREAM_BEAM, sb_nbest, sb_cap) : ResultLayout(n, max_tokens, timed ? ResultForm::PF_TIMED : ResultForm::PLAIN));
  const ResultLayout& lay = out.lay;
  out.commit();                                          // (the copies into it are issued behind the captured step, not inside it)
  pb.upload(stream);
  // ---- which path this step takes (see the comment at st_fused_max)
  bool step_fused = st_fused && std::is_same<T, bf16_t>::value && n <= st_fused_max && st_cooldown == 0 && !foreign_now;
  bool snapshot = false;
  if (st_cooldown > 0) --st_cooldown;
  if (step_fused && st_share_rule && asr_tenant_busy_others(this, 5.0) > 0) { step_fused = false; ++st_shared_steps; }
  if (step_fused) snapshot = st_snapshot_env == 1 || (st_snapshot_env < 0 && asr_tenant_live_others(this) > 0);
  if (snapshot) { ensure_stream_shadow(); ++st_snapshots; }
  const bool inject_fault = step_fused && st_fault == 1;
  if (inject_fault) st_fault = 2;                        // once per session
  const UttPlan* dp = pb.dev(s_plan);
  const int32_t *d_blk_utt = pb.dev(s_blk_utt), *d_blk_f0 = pb.dev(s_blk_f0), *d_row_utt = pb.dev(s_row_utt);

  // Everything below reads its geometry from the uploaded plan and the device-side state (history lengths, fired-token counts), so
  // the launch sequence depends on n only: one captured hipGraph replays every chunk step of a given set size.
  auto enqueue = [&]() {
  if (resample_now) {
    ProfScope ps(prof, "resample", stream);
    ResampleStreamArgs ra;
    ra.audio = d_raw; ra.sid = &dp[0].lang; ra.sid_stride = (int)(sizeof(UttPlan) / 4); ra.count = st_rs_count.as<int32_t>(); ra.hist = st_rs_hist.as<float>();
    ra.streams = st_max; ra.tab_t = rs->tab_t.as<float>(); ra.out = st_rs_out.as<float>(); ra.need_out = nullptr; ra.d = rs->d; ra.chunk = st_chunk;
    ra.pitch = rs_pitch; ra.channels = in_channels; ra.scale = 1.0f; ra.audio_dtype = audio_dtype;      // (int16 as the offline Paraformer session widens it)
    launch_resample_stream(ra, n, stream);
    save_tap("resampled", st_rs_out.ptr, n, st_chunk, st_chunk, 4);
  }
  if (snapshot && step_fused)
    launch_stream_state_copy(st_segs.as<StreamStateSeg>(), st_n_segs, st_n_items, dp, n, false, stream);
  // ---- front-end: fbank of the chunk, LFR rows, carried rows in front (:386-399)
  {
    ProfScope ps(prof, "fbank", stream);
    const FbankArgs fa = fe.args(d_aud, fe_dtype, dp, d_blk_utt, d_blk_f0, d_mel.as<float>(), nullptr);
    launch_fbank(fa, n, stream);
  }
  if (taps_enabled) save_tap("mel", d_mel.ptr, frames, c.n_mels, c.n_mels, 4);
  {
    ProfScope ps(prof, "lfr_cmvn", stream);
    StreamLfrArgs la;
    la.mel = d_mel.as<float>(); la.plan = dp; la.cmvn_vars = cmvn_vars; la.pos_bias = speech_pos; la.prev = st_prev.as<float>();
    la.start = st_start.as<int32_t>(); la.out = d_x0.as<float>(); la.ld = kpad0; la.feat = feat; la.n_mels = c.n_mels; la.lfr_m = c.lfr_m;
    la.lfr_n = c.lfr_n; la.n_prev = st_C; la.n_new = st_B; la.n_rows = rows; la.n_frames = st_frames; la.pos_rows = max_lfr;
    launch_stream_lfr(la, stream);
    launch_stream_carry(d_x0.as<float>(), kpad0, dp, n, st_C, st_B, st_prev.as<float>(), st_start.as<int32_t>(), stream);
  }
  save_tap("enc_in", d_x0.ptr, rows, feat, kpad0, 4);
  // ---- encoder layers with K/V history (:400-435)
  const float* x_in = d_x0.as<float>();
  int ld_in = kpad0;
  float* xa = d_xa.as<float>();
  float* xb = d_xb.as<float>();
  T* h = d_h.as<T>();
  T* qkv = d_sqkv.as<T>();
  T* ctx = d_ctx.as<T>();
  float* mem = d_mem.as<float>();
  T* ffn = d_ffn.as<T>();
  const size_t en_layer = (size_t)st_max * H * st_en_cap * 128;
  const bool fused = step_fused;
  // Round 5: the per-launch layers evaluate their SECOND LayerNorm inside FFN-1, as the offline four-launch path does (rstd (x W^T - mean colsum(W)) + b over the bf16 copy of
  // the out-projection's result, row statistics handed over by that GEMM's epilogue) -- at 256 streams the ~100 stand-alone LayerNorm launches of a chunk step were 10 % of it at
  // their 5.4 us launch floor; this removes half of them. The first LayerNorm stays a launch: the LayerNorm-folded GEMM has no instance for the q|k|v epilogue (the offline path
  // folds it inside sanm_qkv_attn_kernel). ASR_LN_FUSED=0 restores the launches.
  bool st_alg = false;
  bf16_t* xblo = nullptr;
  float2* stb = nullptr;
  if constexpr (sizeof(T) == 2) {
    const SvBlock& bl = blocks[c.n_blocks - 1];
    GemmArgs probe;
    probe.M = rows; probe.N = dff; probe.K = d; probe.ln_dim = d; probe.ln_colsum = bl.c1; probe.act = ACT_RELU; probe.bias = bl.b1;
    probe.out_lo = d_ffn.ptr; probe.A = d_xblo.ptr; probe.W = bl.w1;
    st_alg = use_ln_alg && bl.c1 && d_xblo.ptr && gemm_ln_fusable(probe);
    xblo = d_xblo.as<bf16_t>(); stb = d_stb.as<float2>();
  }
  for (int i = 0; i < c.n_blocks; ++i) {
    const SvBlock& b = blocks[i];
    if (fused && i == 1) {               // layers 1 .. n - 1: one launch, the stream's rows stay in xa
      ProfScope ps(prof, "stream_layers", stream);
      const int nl = c.n_blocks - 1;
      HIP_CHECK(hipMemsetAsync(st_flags.ptr, 0, ((size_t)nl * n * 4 + 4 + (size_t)pdec.size() * n * 8) * 4, stream));
      StreamLayersArgs la;
      la.plan = dp; la.n_streams = n; la.n_layers = nl; la.n_cur = n_cur; la.cap = st_en_cap; la.roll_rows = st_B; la.ktaps = c.fsmn_kernel;
      la.ln_eps = 1e-5f; la.cache_len = st_enlen.as<int32_t>(); la.layers = st_layer_tab.as<StreamLayer>();
      la.x = xa; la.xb = xb; la.ctx = (bf16_t*)ctx; la.hid = (bf16_t*)ffn;
      la.flags = st_flags.as<unsigned>(); la.err = st_flags.as<unsigned>() + (size_t)nl * n * 4;
      la.opt = st_opt; la.fault = inject_fault ? 1 : 0;
      if (st_times_layer >= 0) {
        st_times.reserve((size_t)((n + 7) / 8) * 32 * 16 * 8, stream);
        HIP_CHECK(hipMemsetAsync(st_times.ptr, 0, (size_t)((n + 7) / 8) * 32 * 16 * 8, stream));
        la.times = st_times.as<unsigned long long>(); la.times_layer = st_times_layer;
      }
      launch_stream_layers(la, stream);
      break;
    }
    { ProfScope ps(prof, "layernorm", stream); launch_layernorm<T>(x_in, ld_in, rows, b.in_size, b.ln1_g, b.ln1_b, 1e-5f, h, b.kpad, b.kpad, stream); }
    {
      ProfScope ps(prof, "gemm_qkv", stream);
      GemmArgs g;
      g.A = h; g.lda = b.kpad; g.W = b.wqkv; g.ldw = b.kpad; g.M = rows; g.N = 3 * d; g.K = b.kpad; g.bias = b.bqkv; g.out_lo = qkv; g.ld_out_lo = 3 * d;
      gemm(g);
    }
    {
      ProfScope ps(prof, "attention", stream);
      T* ck = st_enk.as<T>() + (size_t)i * en_layer;
      T* cv = st_env.as<T>() + (size_t)i * en_layer;
      StreamAttnArgs sa;
      sa.q = qkv; sa.ld_q = 3 * d; sa.q_col0 = 0; sa.k = qkv; sa.ld_k = 3 * d; sa.k_col0 = d; sa.v = qkv; sa.ld_v = 3 * d; sa.v_col0 = 2 * d;
      sa.n_cur = n_cur; sa.cache_k = ck; sa.cache_v = cv; sa.cache_len = st_enlen.as<int32_t>(); sa.cap = st_en_cap; sa.q_plan = dp; sa.n_heads = H;
      sa.ctx = ctx; sa.ld_ctx = d;
      // the same launch rolls the history -- [-(cap + C) : -C] of (history ++ chunk): append the first B rows, keep the last cap (:421-422) --
      // and computes the FSMN memory term of the chunk rows
      sa.roll_rows = st_B;
      sa.fsmn_w = b.wfsmn; sa.fsmn_b = b.bfsmn; sa.ktaps = c.fsmn_kernel; sa.mem = mem; sa.d = d;
      if (taps_enabled && i == 0) {                        // (bisect taps, tools/probes/stream_determinism.py: the layer's history as the attention launch finds it)
        save_tap("s0_ck", ck, (int64_t)st_max * H * st_en_cap, 128, 128, sizeof(T));
        save_tap("s0_cv", cv, (int64_t)st_max * H * st_en_cap, 128, 128, sizeof(T));
        save_tap("s0_len", st_enlen.ptr, st_max, 1, 1, 4);
      }
      launch_stream_attn<T>(sa, n, stream);
    }
    if (taps_enabled && (i == 0 || i == 3)) {             // (bisect taps of layers 0 and 3: what tools/probes/stream_determinism.py compares between a solo pass and a pass beside a co-tenant)
      const std::string pre = "s" + std::to_string(i) + "_";
      save_tap((pre + "h").c_str(), h, rows, b.kpad, b.kpad, sizeof(T));
      save_tap((pre + "qkv").c_str(), qkv, rows, 3 * d, 3 * d, sizeof(T));
      save_tap((pre + "ctx").c_str(), ctx, rows, d, d, sizeof(T));
      save_tap((pre + "mem").c_str(), mem, rows, d, d, 4);
    }
    {
      ProfScope ps(prof, "gemm_out", stream);
      GemmArgs g;
      g.A = ctx; g.lda = d; g.W = b.wout; g.ldw = d; g.M = rows; g.N = d; g.K = d; g.add = mem; g.ld_add = d;
      if (i > 0) { g.add2 = x_in; g.ld_add2 = ld_in; }             // residual from the second layer on (:402-403,431-432)
      g.out_f32 = xb; g.ld_out_f32 = d;
      if (st_alg) { g.out_lo = xblo; g.ld_out_lo = d; g.st_out = stb; }
      gemm(g);
    }
    if (!st_alg) { ProfScope ps(prof, "layernorm", stream); launch_layernorm<T>(xb, d, rows, d, b.ln2_g, b.ln2_b, 1e-5f, h, d, d, stream); }
    {
      ProfScope ps(prof, "gemm_ffn1", stream);
      GemmArgs g;
      g.A = h; g.lda = d; g.W = b.w1; g.ldw = d; g.M = rows; g.N = dff; g.K = d; g.bias = b.b1; g.act = ACT_RELU; g.out_lo = ffn; g.ld_out_lo = dff;
      if (st_alg) { g.A = xblo; g.ln_colsum = b.c1; g.ln_dim = d; g.ln_stats_in = stb; g.ln_slots = d / 32; }
      gemm(g);
    }
    {
      ProfScope ps(prof, "gemm_ffn2", stream);
      GemmArgs g;
      g.A = ffn; g.lda = dff; g.W = b.w2; g.ldw = dff; g.M = rows; g.N = d; g.K = dff; g.bias = b.b2; g.add = xb; g.ld_add = d; g.out_f32 = xa; g.ld_out_f32 = d;
      gemm(g);
    }
    if (taps_enabled && (i == 0 || i == 3)) {
      const std::string pre = "s" + std::to_string(i) + "_";
      save_tap((pre + "xb").c_str(), xb, rows, d, d, 4);
      save_tap((pre + "ffn").c_str(), ffn, rows, dff, dff, sizeof(T));
      save_tap((pre + "xa").c_str(), xa, rows, d, d, 4);
    }
    x_in = xa;
    ld_in = d;
  }
  // ---- after_norm, CIF conv + alphas, unrolled integrate-and-fire with the carried state (:436-462)
  float* enc32 = d_xb.as<float>();
  T* enc_lo = d_enc_lo.as<T>();
  float* dec = d_dec.as<float>();
  UttPlan* tplan = d_tplan.as<UttPlan>();
  {
    ProfScope ps(prof, "layernorm", stream);
    launch_layernorm<float>(xa, d, rows, d, after_g, after_b, 1e-5f, enc32, d, d, stream);
    launch_layernorm<T>(xa, d, rows, d, after_g, after_b, 1e-5f, enc_lo, d, d, stream);
  }
  save_tap("enc_out", enc32, rows, d, d, 4);
  {
    ProfScope ps(prof, "cif", stream);
    launch_shift3<T>(enc_lo, d, dp, d_row_utt, Mpad, d_cifa.as<T>(), stream);
    GemmArgs g;
    g.A = d_cifa.ptr; g.lda = 3 * d; g.W = cif_conv_w; g.ldw = 3 * d; g.M = rows; g.N = d; g.K = 3 * d; g.bias = cif_conv_b; g.act = ACT_RELU;
    g.out_lo = ctx; g.ld_out_lo = d;
    gemm(g);
    launch_alpha<T>(ctx, d, cif_out_w, cif_out_b, rows, d_alpha.as<float>(), stream);
    if (timed)
      launch_stream_cif_timed(d_alpha.as<float>(), enc32, d, dp, n, st_B, st_cifh.as<float>(), st_cifa.as<float>(), dec, tplan, d_num.as<int32_t>(),
                              d_first.as<int32_t>(), max_tokens, stream);
    else
      launch_stream_cif(d_alpha.as<float>(), enc32, d, dp, n, st_B, st_cifh.as<float>(), st_cifa.as<float>(), dec, tplan, d_num.as<int32_t>(), stream);
  }
  save_tap("alphas", d_alpha.ptr, rows, 1, 1, 4);
  save_tap("list_frame", dec, rows, d, d, 4);
  // ---- decoder over the fired frames (:508-553); streams without a fired frame leave their decoder state untouched
  T* q = d_qk.as<T>();
  T* kv = d_skv.as<T>();
  float* ffn32 = d_ffn32.as<float>();
  float* x1 = d_mem.as<float>();
  float* x2 = d_x2.as<float>();
  float* sa32 = d_sa.as<float>();
  const size_t de_layer = (size_t)st_max * H * st_de_cap * 128, fs_layer = (size_t)st_max * (c.fsmn_kernel - 1) * d;
  auto ffn_block = [&](const PfDecLayer& L, float* out) {
    { ProfScope ps(prof, "layernorm", stream); launch_layernorm<T>(dec, d, rows, d, nullptr, nullptr, 1e-5f, h, d, d, stream); }
    ProfScope ps(prof, "gemm_dec", stream);
    GemmArgs g;
    g.A = h; g.lda = d; g.W = L.w1; g.ldw = d; g.M = rows; g.N = dd; g.K = d; g.bias = L.b1; g.act = ACT_RELU; g.out_f32 = ffn32; g.ld_out_f32 = dd;
    gemm(g);
    launch_layernorm<T>(ffn32, dd, rows, dd, nullptr, nullptr, 1e-5f, ffn, dd, dd, stream);
    GemmArgs g2;
    g2.A = ffn; g2.lda = dd; g2.W = L.w2; g2.ldw = dd; g2.M = rows; g2.N = d; g2.K = dd; g2.bias = L.b2; g2.out_f32 = out; g2.ld_out_f32 = d;
    gemm(g2);
  };
  int li = 0;
  if (st_dec_fused && step_fused) {      // every decoder block in one launch (stream_dec.hip); streams without a fired frame skip it
    ProfScope ps(prof, "stream_dec", stream);
    StreamDecArgs da;
    da.token_plan = tplan; da.n_streams = n; da.n_layers = (int)pdec.size(); da.n_cur = n_cur; da.cap = st_de_cap; da.ln_eps = 1e-5f;
    da.cache_len = st_delen.as<int32_t>(); da.layers = st_dlayer_tab.as<StreamDecLayer>(); da.enc = (const bf16_t*)enc_lo;
    da.dec = dec; da.x1 = x1; da.x2 = x2; da.hid = ffn32; da.ctx = (bf16_t*)ctx;
    unsigned* fb = st_flags.as<unsigned>() + (size_t)(c.n_blocks - 1) * n * 4;
    da.err = fb; da.flags = fb + 4; da.opt = st_opt >> 8;
    if (st_times_layer <= -2) {
      st_times.reserve((size_t)((n + 7) / 8) * 32 * 16 * 8, stream);
      HIP_CHECK(hipMemsetAsync(st_times.ptr, 0, (size_t)((n + 7) / 8) * 32 * 16 * 8, stream));
      da.times = st_times.as<unsigned long long>(); da.times_layer = -2 - st_times_layer;
    }
    launch_stream_dec(da, stream);
  } else
  for (const PfDecLayer& L : pdec) {
    if (!L.full) { ffn_block(L, dec); continue; }
    ffn_block(L, x1);
    {
      ProfScope ps(prof, "fsmn", stream);
      launch_layernorm<float>(x1, d, rows, d, L.n2_g, L.n2_b, 1e-5f, sa32, d, d, stream);
      launch_stream_dec_fsmn(sa32, dec, L.wfsmn, d, c.fsmn_kernel, tplan, n, st_defsmn.as<float>() + (size_t)li * fs_layer, x2, stream);
    }
    { ProfScope ps(prof, "layernorm", stream); launch_layernorm<T>(x2, d, rows, d, nullptr, nullptr, 1e-5f, h, d, d, stream); }
    {
      ProfScope ps(prof, "gemm_dec", stream);
      GemmArgs g;
      g.A = h; g.lda = d; g.W = L.wq; g.ldw = d; g.M = rows; g.N = d; g.K = d; g.bias = L.bq; g.out_lo = q; g.ld_out_lo = d;
      gemm(g);
      GemmArgs gk;
      gk.A = enc_lo; gk.lda = d; gk.W = L.wkv; gk.ldw = d; gk.M = rows; gk.N = 2 * d; gk.K = d; gk.bias = L.bkv; gk.out_lo = kv; gk.ld_out_lo = 2 * d;
      gemm(gk);
    }
    {
      ProfScope ps(prof, "attention", stream);
      T* ck = st_dek.as<T>() + (size_t)li * de_layer;
      T* cv = st_dev.as<T>() + (size_t)li * de_layer;
      StreamAttnArgs sa;
      sa.q = q; sa.ld_q = d; sa.q_col0 = 0; sa.k = kv; sa.ld_k = 2 * d; sa.k_col0 = 0; sa.v = kv; sa.ld_v = 2 * d; sa.v_col0 = d; sa.n_cur = n_cur;
      sa.cache_k = ck; sa.cache_v = cv; sa.cache_len = st_delen.as<int32_t>(); sa.cap = st_de_cap; sa.q_plan = tplan; sa.n_heads = H;
      sa.ctx = ctx; sa.ld_ctx = d;
      launch_stream_attn<T>(sa, n, stream);
      launch_stream_cache_roll<T>(ck, cv, st_delen.as<int32_t>(), st_de_cap, kv, 2 * d, 0, kv, 2 * d, d, n_cur, dp, tplan, n, H, stream);
    }
    {
      ProfScope ps(prof, "gemm_dec", stream);
      GemmArgs g;
      g.A = ctx; g.lda = d; g.W = L.wo; g.ldw = d; g.M = rows; g.N = d; g.K = d; g.bias = L.bo; g.add = x2; g.ld_add = d; g.out_f32 = dec; g.ld_out_f32 = d;
      gemm(g);
    }
    ++li;
  }
  { ProfScope ps(prof, "layernorm", stream); launch_layernorm<T>(dec, d, rows, d, nullptr, nullptr, 1e-5f, h, d, d, stream); }
  {
    ProfScope ps(prof, "gemm_out", stream);
    GemmArgs g;
    g.A = h; g.lda = d; g.W = pf_out_w; g.ldw = d; g.M = rows; g.N = vpad; g.K = d; g.bias = pf_out_b; g.out_f32 = d_logits.as<float>(); g.ld_out_f32 = vpad;
    gemm(g);
    if (timed) {                                        // the pick and its score in one kernel (ids equal launch_argmax_rows' bit for bit); one score per row: column 0 of a 1-wide history
      launch_argmax_logprob_rows(d_logits.as<float>(), vpad, rows, c.vocab, nullptr, d_ids.as<int32_t>(), d_flp.as<float>(), 1, st_zero.as<int32_t>(), stream);
      launch_gather_tokens(d_ids.as<int32_t>(), tplan, n, d_tok.as<int32_t>(), max_tokens, stream);
      launch_gather_token_logprob(d_flp.as<float>(), tplan, n, d_tlp.as<float>(), max_tokens, stream);
    } else {
      launch_argmax_rows(d_logits.as<float>(), vpad, rows, c.vocab, nullptr, d_ids.as<int32_t>(), stream);
      launch_gather_tokens(d_ids.as<int32_t>(), tplan, n, d_tok.as<int32_t>(), max_tokens, stream);
    }
  }
  launch_stream_advance(dp, tplan, n, st_B, st_en_cap, n_cur, st_de_cap, st_enlen.as<int32_t>(), st_delen.as<int32_t>(), stream);
  };
  {
    GraphKey key;
    for (const void* q : {(const void*)d_aud, (const void*)d_plan.ptr, (const void*)d_mel.ptr, (const void*)d_x0.ptr, (const void*)d_xa.ptr, (const void*)d_xb.ptr,
                          (const void*)d_h.ptr, (const void*)d_sqkv.ptr, (const void*)d_skv.ptr, (const void*)d_qk.ptr, (const void*)d_ctx.ptr, (const void*)d_mem.ptr,
                          (const void*)d_ffn.ptr, (const void*)d_amax_v.ptr, (const void*)d_amax_i.ptr, (const void*)d_ids.ptr, (const void*)d_tok.ptr, (const void*)d_num.ptr,
                          (const void*)d_logits.ptr, (const void*)d_enc_lo.ptr, (const void*)d_cifa.ptr, (const void*)d_alpha.ptr, (const void*)d_dec.ptr, (const void*)d_x2.ptr,
                          (const void*)d_sa.ptr, (const void*)d_ffn32.ptr, (const void*)d_tplan.ptr, (const void*)stream, (const void*)(uintptr_t)n,
                          (const void*)(uintptr_t)max_tokens, (const void*)st_shadow.ptr, (const void*)d_xblo.ptr, (const void*)d_stb.ptr})
      key.mix(q);
    key.mix((uint64_t)audio_dtype);                                 // the front end is inside the captured step
    key.mix((uint64_t)in_rate); key.mix((uint64_t)in_channels);     // ... and so is the resampler of a non-default format, with its buffers
    if (fmt) for (const void* q : {d_raw, (const void*)st_rs_hist.ptr, (const void*)st_rs_count.ptr, (const void*)rs->tab_t.ptr}) key.mix(q);
    key.mix((uint64_t)timed);                                       // the timed step is another launch sequence ...
    if (timed) for (const void* q : {(const void*)d_flp.ptr, (const void*)d_first.ptr, (const void*)d_tlp.ptr}) key.mix(q);     // ... over three more buffers
    const int gi = step_fused ? (snapshot ? 2 : 1) : 0;            // one cached graph per path: a session that alternates (a co-tenant comes and goes) does not re-capture
    (timed ? st_graph_timed : st_graph)[gi].run(stream, use_graph && !taps_enabled && !prof.enabled && !inject_fault, key.h, enqueue);
  }
  for (int i = 0; i < n; ++i) {                          // what the streams hold from here on, and the counts the device moved
    st_rs_state[stream_ids[i]] = fmt ? 2 : 1;
    if (fmt) ++st_rs_steps[stream_ids[i]];
  }
  resample_now = false;
  if (taps_enabled) {
    save_tap("logits", d_logits.ptr, rows, c.vocab, vpad, 4);
    if (timed) {
      save_tap("fire_frames", d_first.ptr, n, max_tokens, max_tokens, 4);
      save_tap("token_logprob", d_tlp.ptr, n, max_tokens, max_tokens, 4);
    }
  }
  auto copy_out = [&]() {
    out.enqueue_copy(lay.tokens, d_tok.ptr, stream);
    out.enqueue_copy(lay.counts, d_num.ptr, stream);
    if (timed) { out.enqueue_copy(lay.first, d_first.ptr, stream); out.enqueue_copy(lay.logprob, d_tlp.ptr, stream); }
  };
  copy_out();
  const bool fused_ran = step_fused;
  uint32_t* h_err = out.host(lay.status);
  *h_err = 0;
  if (fused_ran) out.enqueue_copy(lay.status, st_flags.as<unsigned>() + (size_t)(c.n_blocks - 1) * n * 4, stream);
  HIP_CHECK(hipStreamSynchronize(stream));
  if (prof.enabled) prof.collect();
  // (a cluster that gave up has rolled the histories of the layers in front of it: with a snapshot the state is restored and the step redone on the per-launch path
  //  below; without one -- no other session existed when the step started -- the step fails loudly and the streams have to be reset)
  if (fused_ran && (st_times_layer >= 0 || st_times_layer <= -2)) {               // tuning: mean phase intervals over the workgroups
    char title[48];
    snprintf(title, sizeof title, "%s layer %d", st_times_layer >= 0 ? "stream_layers" : "stream_dec", st_times_layer >= 0 ? st_times_layer : -2 - st_times_layer);
    dump_phase_clocks(st_times, (n + 7) / 8 * 32, 1, st_times_layer >= 0 ? 12 : 13, nullptr, title);
  }
  if (fused_ran && *h_err != 0 && snapshot) {
    // A cluster gave up (its workgroups were not co-resident: somebody else's kernels hold CUs). The histories of the layers in front of the stall are rolled,
    // everything behind the launch ran on garbage: put the active streams' state back as it was in front of the step, redo the step on the per-launch path
    // (no cross-workgroup waits) and stay there for a while.
    ++st_giveups;
    st_cooldown = st_cooldown_steps;
    fprintf(stderr, "asr_mi355x: streaming step: a cluster of the fused launch gave up; state restored, step redone on the per-launch path (give-up %d of this session)\n", st_giveups);
    launch_stream_state_copy(st_segs.as<StreamStateSeg>(), st_n_segs, st_n_items, dp, n, true, stream);
    step_fused = false; snapshot = false;
    enqueue();
    copy_out();                                          // (the redone step's outputs, the timed ones included)
    HIP_CHECK(hipStreamSynchronize(stream));
    if (prof.enabled) prof.collect();
    *h_err = 0;
  }
  ASR_REQUIRE(*h_err == 0, "streaming: a workgroup of the fused encoder launch gave up waiting for its cluster and no snapshot was taken (ASR_STREAM_SNAPSHOT=0, or no other "
              "session existed on this GPU when the step started); the step's results are invalid, reset its streams");
  memcpy(q.num_out, out.host(lay.counts), lay.bytes(lay.counts));
  out.scatter_rows(lay.tokens, q.tok_out, q.num_out, max_tokens);
  if (timed) {
    out.scatter_rows(lay.first, q.fire_out, q.num_out, max_tokens);
    out.scatter_rows(lay.logprob, q.logprob_out, q.num_out, max_tokens);
  }
  if (beam) stream_search(out, d_tplan.as<UttPlan>(), stream_ids, n, rows, false, q.beam_out);
}

extern "C" int asr_paraformer_stream_create(const asr_paraformer_config* cfg, const void* arena, size_t arena_bytes, int arena_mem,
                                            int device_id, int precision, int chunk_samples, int look_back_encoder, int look_back_decoder,
                                            int max_streams, asr_session** out) {
  asr_session* base = nullptr;
  const int rc = asr_paraformer_create(cfg, arena, arena_bytes, arena_mem, device_id, precision, &base);
  if (rc != ASR_OK) return rc;
  const int rc2 = asr_guard([&] {
    SvSession* sv = static_cast<SvSession*>(base);
    sv->kind = 4;
    sv->stream_init(chunk_samples, look_back_encoder, look_back_decoder, max_streams);
    *out = base;
  });
  if (rc2 != ASR_OK) delete base;
  return rc2;
}

extern "C" int asr_paraformer_stream_input_frames(asr_session* s, const int32_t* stream_ids, int n_streams, int32_t* frames_out, int32_t* pitch_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 4, "paraformer_stream_input_frames: not a streaming Paraformer session");
    static_cast<SvSession*>(s)->stream_input_frames(stream_ids, n_streams, frames_out, pitch_out);
  });
}

extern "C" int asr_paraformer_stream_reset(asr_session* s, int stream_id) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 4, "paraformer_stream_reset: not a streaming Paraformer session");
    static_cast<SvSession*>(s)->stream_reset(stream_id);
  });
}

namespace {
void step_entry(asr_session* s, SvForm form, const void* audio, int audio_mem, const int32_t* stream_ids, int n_streams, int32_t* tok_out, int max_tokens, int32_t* num_out,
                int32_t* fire_out, float* logprob_out, const SvStreamBeamOut* beam_out = nullptr) {
  TenantScope tenant(s);
  SvSession* sv = static_cast<SvSession*>(s);
  SvStepReq q;
  q.form = form; q.audio = audio; q.audio_mem = audio_mem; q.stream_ids = stream_ids; q.n = n_streams; q.max_tokens = max_tokens;
  q.tok_out = tok_out; q.num_out = num_out; q.fire_out = fire_out; q.logprob_out = logprob_out;
  if (beam_out) q.beam_out = *beam_out;
  by_precision(sv, [&](auto t) { sv->stream_step<decltype(t)>(q); });
}
}  // namespace

extern "C" int asr_paraformer_stream_step(asr_session* s, const void* audio, int audio_mem, const int32_t* stream_ids, int n_streams,
                                          int32_t* token_ids_out, int max_tokens, int32_t* num_id_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 4, "paraformer_stream_step: not a streaming Paraformer session");
    step_entry(s, SvForm::PLAIN, audio, audio_mem, stream_ids, n_streams, token_ids_out, max_tokens, num_id_out, nullptr, nullptr);
  });
}

extern "C" int asr_paraformer_stream_step_timed(asr_session* s, const void* audio, int audio_mem, const int32_t* stream_ids, int n_streams,
                                                int32_t* token_ids_out, int max_tokens, int32_t* num_id_out, int32_t* fire_step_out, float* logprob_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 4, "paraformer_stream_step_timed: not a streaming Paraformer session");
    ASR_REQUIRE(fire_step_out && logprob_out, "paraformer_stream_step_timed: null timed output");
    step_entry(s, SvForm::TIMED, audio, audio_mem, stream_ids, n_streams, token_ids_out, max_tokens, num_id_out, fire_step_out, logprob_out);
  });
}

namespace {
SvStreamBeamOut beam_out_of(int32_t* commit_ids, float* commit_logprob, int32_t* commit_num, int32_t* pend_ids, float* pend_logprob, int32_t* pend_num, float* pend_score,
                            float* pend_am, int32_t* total) {
  SvStreamBeamOut o;
  o.commit_ids = commit_ids; o.commit_logprob = commit_logprob; o.commit_num = commit_num; o.pend_ids = pend_ids; o.pend_logprob = pend_logprob; o.pend_num = pend_num;
  o.pend_score = pend_score; o.pend_am = pend_am; o.total = total;
  return o;
}
}  // namespace

extern "C" int asr_paraformer_stream_set_beam(asr_session* s, int beam, int topk, int nbest, int pend_cap) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 4, "paraformer_stream_set_beam: not a streaming Paraformer session");
    static_cast<SvSession*>(s)->stream_set_beam(beam, topk, nbest, pend_cap);
  });
}

extern "C" int asr_paraformer_stream_set_hotwords(asr_session* s, const int32_t* ids, const int32_t* offsets, int n_phrases, float boost) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 4, "paraformer_stream_set_hotwords: not a streaming Paraformer session");
    SvSession* sv = static_cast<SvSession*>(s);
    ASR_REQUIRE(!sv->stream_search_history(), "paraformer_stream_set_hotwords: a stream holds search history (its trie nodes belong to the list in force); finish or reset it first");
    sv->set_hotwords(ids, offsets, n_phrases, boost);
  });
}

extern "C" int asr_paraformer_stream_set_lm(asr_session* s, const int32_t* image_words, int64_t n_words, float alpha, float beta, float oov_logprob) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 4, "paraformer_stream_set_lm: not a streaming Paraformer session");
    SvSession* sv = static_cast<SvSession*>(s);
    ASR_REQUIRE(!sv->stream_search_history(), "paraformer_stream_set_lm: a stream holds search history (its model states belong to the image in force); finish or reset it first");
    sv->set_lm(image_words, n_words, alpha, beta, oov_logprob);
  });
}

extern "C" int asr_paraformer_stream_step_beam(asr_session* s, const void* audio, int audio_mem, const int32_t* stream_ids, int n_streams, int32_t* token_ids_out,
                                               int max_tokens, int32_t* num_id_out, int32_t* fire_step_out, float* logprob_out, int32_t* commit_ids_out,
                                               float* commit_logprob_out, int32_t* commit_num_out, int32_t* pend_ids_out, float* pend_logprob_out, int32_t* pend_num_out,
                                               float* pend_score_out, float* pend_am_out, int32_t* total_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 4, "paraformer_stream_step_beam: not a streaming Paraformer session");
    ASR_REQUIRE(fire_step_out && logprob_out, "paraformer_stream_step_beam: null timed output");
    const SvStreamBeamOut o = beam_out_of(commit_ids_out, commit_logprob_out, commit_num_out, pend_ids_out, pend_logprob_out, pend_num_out, pend_score_out, pend_am_out, total_out);
    step_entry(s, SvForm::STREAM_BEAM, audio, audio_mem, stream_ids, n_streams, token_ids_out, max_tokens, num_id_out, fire_step_out, logprob_out, &o);
  });
}

extern "C" int asr_paraformer_stream_finish_beam(asr_session* s, const int32_t* stream_ids, int n_streams, int32_t* commit_ids_out, float* commit_logprob_out,
                                                 int32_t* commit_num_out, int32_t* pend_ids_out, float* pend_logprob_out, int32_t* pend_num_out, float* pend_score_out,
                                                 float* pend_am_out, int32_t* total_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 4, "paraformer_stream_finish_beam: not a streaming Paraformer session");
    TenantScope tenant(s);
    static_cast<SvSession*>(s)->stream_finish_beam(stream_ids, n_streams, beam_out_of(commit_ids_out, commit_logprob_out, commit_num_out, pend_ids_out, pend_logprob_out,
                                                                                       pend_num_out, pend_score_out, pend_am_out, total_out));
  });
}

extern "C" int asr_paraformer_stream_stats(asr_session* s, int32_t* out8) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 4 && out8, "paraformer_stream_stats: not a streaming Paraformer session");
    SvSession* sv = static_cast<SvSession*>(s);
    out8[0] = sv->st_giveups; out8[1] = sv->st_shared_steps; out8[2] = sv->st_snapshots; out8[3] = sv->st_fused_max; out8[4] = sv->st_cooldown;
    out8[5] = sv->st_fused ? 1 : 0; out8[6] = sv->foreign_diverted; out8[7] = 0;
  });
}
