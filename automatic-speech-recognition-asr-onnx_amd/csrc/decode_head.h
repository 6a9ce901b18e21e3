// What follows the logits GEMM of a decoder step, once for every decoder family: the token-selection head (arg-max, penalty-greedy,
// top-k / top-p sampling + the id history they share), the beam-search ranking state, and the read-back of a step's picks and logits.
// Header-only and hidden: the sessions and the probe library each compile their own copy, the product library exports nothing new.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>

#include "engine.h"
#include "kernels.h"

// ---- Whisper's timestamp rules (kernels.h: launch_timestamp_rules) as a head / ranker setting; off for every other family
struct ASR_LOCAL TimestampRule {
  bool on = false;
  int ts_begin = 0, no_timestamps_id = 0, eot_id = 0, max_initial = -1;
  bool operator==(const TimestampRule& o) const {
    return on == o.on && ts_begin == o.ts_begin && no_timestamps_id == o.no_timestamps_id && eot_id == o.eot_id && max_initial == o.max_initial;
  }
  void enqueue(Profiler* prof, float* logits, int ld, int rows, int n_valid, const int32_t* ids, int ld_ids, const int32_t* n_ids, int n_ids_stride,
               hipStream_t s) const {
    const bool timed = prof && prof->enabled;
    if (timed) prof->begin(prof->cls("timestamp_rules"), s);
    launch_timestamp_rules(logits, ld, rows, n_valid, ids, ld_ids, n_ids, n_ids_stride, ts_begin, no_timestamps_id, eot_id, max_initial, s);
    if (timed) prof->end(s);
  }
};

// ---- hotwords (kernels.h: launch_hotword_*) as the beam ranker takes them from the head: the trie view, and the root children's values the head
// saved when it biased the prefill's row in place (null: that row is the model's own)
struct ASR_LOCAL HotView {
  HotTrie trie;
  const float* root_save = nullptr;
  bool on() const { return trie.n_nodes > 1; }
};
struct ASR_LOCAL HotScope {            // the hotword launches of the head and the ranker are a profile class of their own, as the timestamp rules are
  Profiler* p; hipStream_t s;
  HotScope(Profiler* p_, hipStream_t s_) : p(p_ && p_->enabled ? p_ : nullptr), s(s_) { if (p) p->begin(p->cls("hotwords"), s); }
  ~HotScope() { if (p) p->end(s); }
};

// ---- n-gram LM fusion (kernels.h: launch_lm_*) as the beam ranker takes it from the head: the image's view, the candidate width and the end ids
struct ASR_LOCAL LmView {
  NgramLm lm;
  int topk = 0;
  LmEnds ends;
  bool on() const { return lm.n_nodes > 0; }
};
struct ASR_LOCAL LmScope {             // the LM launches of the head and the ranker are a profile class of their own, beside "hotwords"
  Profiler* p; hipStream_t s;
  LmScope(Profiler* p_, hipStream_t s_) : p(p_ && p_->enabled ? p_ : nullptr), s(s_) { if (p) p->begin(p->cls("lm"), s); }
  ~LmScope() { if (p) p->end(s); }
};

// ---- token-selection head (Export_Whisper.py:228-325, Inference_Qwen_ASR_ONNX.py:369-376): arg-max, penalty-greedy (APPLY_PENALTY + GREEDY_SEARCH) or
// TOPK_TOPP_SAMPLING, and the history of picked ids [rows][ld_save] the last two read. What differs between the families is data, set by init().
struct ASR_LOCAL TokenHead {
  int ld_save = 0;                     // history capacity per sequence: max_target_positions (Whisper), max_seq_len (Qwen3)
  int partial = 0;                     // launch_apply_penalty's window rule: 0 Whisper (nothing until `range` ids are saved), 1 Qwen3
  int sampling_ld_limit = 0;           // set_sampling refuses a history wider than this
  float penalty_value = 1.0f;          // 1.0 = plain greedy (REPEAT_PENALTY)
  int penalty_range = 0;
  bool track_history = false;          // GREEDY_SEARCH graphs append every pick to save_id even while the penalty value is 1.0
  bool sampling = false;               // TOPK_TOPP_SAMPLING head (USE_SAMPLING)
  float temperature = 0.8f, top_p = 0.95f, samp_rep_penalty = 1.0f;
  int top_k = 10;
  uint64_t samp_seed = 0;
  TimestampRule ts;                    // Whisper's timestamp mode: the rules run before every selection, every pick joins the history
  bool scores = false;                 // token scores (kernels.h: launch_argmax_logprob_rows): every pick's log-probability joins d_scores, every pick the history
  Profiler* prof = nullptr;            // the owning session's, when it has one: the rule kernel is a profile class of its own
  DeviceBuffer d_save, d_nsaved;       // generated ids per sequence + their count (on the device: a captured step replays for every position)
  int score_rows = 0;                  // rows d_scores was last reserved for
  bool scored = false;                 // a prefill has restarted the histories since scores were switched on: d_scores[.., 0 .. *d_nsaved) are this run's
  DeviceBuffer d_scores;               // scores mode: the picks' log-probabilities [rows][ld_save] f32, column for column beside d_save under the same counter
  DeviceBuffer d_noise;                // caller-supplied uniforms [rows][top_k] for the next step (parity tests); consumed once
  bool noise_armed = false;            // a step with armed noise is not graphable
  uint64_t epoch = 0;                  // moves with everything a captured step bakes in: a setter that changed a value, a history buffer that moved
  // hotwords: the trie image on the device (its words are kernel operands: a new list moves the epoch), every row's node, and the root children's values of
  // the row a prefill biased (the beam ranker's first pass restores them). Off (hot_nodes <= 1) nothing is allocated and no step launches anything new.
  DeviceBuffer d_trie, d_node, d_rootsave;
  int hot_nodes = 0, hot_root = 0, node_rows = 0;
  float hot_boost = 0.0f;
  uint64_t hot_gen = 0, biased_gen = 0;   // the list's generation, and the one the last prefill row was biased with
  bool row_biased = false;             // the logits row of the last prefill carries the bias (restart clears)
  // language model: the image on the device (once per session), every row's state, and the candidate list of a step (launch_lm_topk's outputs). Off
  // (lm.on() false) nothing is allocated and no step launches anything new.
  DeviceBuffer d_lm, d_lmstate, d_lmv, d_lmi, d_lmlse;
  LmView lm;
  int lm_rows = 0;

  void init(int ld_save_, int partial_, int default_range, int sampling_ld_limit_) {
    ld_save = ld_save_; partial = partial_; penalty_range = default_range; sampling_ld_limit = sampling_ld_limit_;
  }
  bool plain() const { return !sampling && penalty_value == 1.0f; }

  // `who`: the C entry's name, the prefix of its messages
  void set_penalty(float value, int range, const char* who) {
    ASR_REQUIRE(value > 0.0f && range >= 1 && range <= 64, "%s: value %g range %d", who, value, range);
    if (penalty_value != value || penalty_range != range) { penalty_value = value; penalty_range = range; ++epoch; }
  }
  void set_track_history(bool enable) {
    if (track_history != enable) { track_history = enable; ++epoch; }
  }
  void set_sampling(bool enable, float t, int k, float p, float rp, uint64_t seed, const char* who) {
    if (enable) {
      ASR_REQUIRE(t > 0.0f && k >= 1 && k <= 64 && p > 0.0f && rp > 0.0f && ld_save <= sampling_ld_limit, "%s: temperature %g top_k %d top_p %g penalty %g", who, t, k, p, rp);
      temperature = t; top_k = k; top_p = p; samp_rep_penalty = rp; samp_seed = seed;
    }
    sampling = enable;
    noise_armed = false;
    ++epoch;
  }
  void set_timestamps(bool enable, int ts_begin, int no_timestamps_id, int eot_id, int max_initial, int vocab, const char* who) {
    TimestampRule t;
    if (enable) {
      ASR_REQUIRE(0 <= eot_id && eot_id < no_timestamps_id && no_timestamps_id < ts_begin && ts_begin < vocab && max_initial >= -1,
                  "%s: eot %d < no_timestamps %d < timestamp_begin %d < vocab %d expected, max_initial_index %d >= -1", who, eot_id, no_timestamps_id, ts_begin, vocab,
                  max_initial);
      t.on = true; t.ts_begin = ts_begin; t.no_timestamps_id = no_timestamps_id; t.eot_id = eot_id; t.max_initial = max_initial;
    }
    if (!(t == ts)) { ts = t; ++epoch; }
  }
  void set_scores(bool enable) {
    if (scores != enable) { scores = enable; scored = false; ++epoch; }
  }
  bool hot() const { return hot_nodes > 1; }
  HotTrie hot_trie() const { return hot() ? hot_trie_view(d_trie.as<int32_t>(), hot_nodes, hot_boost) : HotTrie{}; }
  // what the beam ranker needs; `who` fails when the prefill's row was biased with another list than the current one (it cannot be restored)
  HotView hot_view(const char* who) const {
    ASR_REQUIRE(!row_biased || biased_gen == hot_gen, "%s: the hotword list changed since the prefill; prefill again", who);
    HotView v;
    v.trie = hot_trie();
    if (row_biased && hot()) v.root_save = d_rootsave.as<float>();
    return v;
  }
  // phrases as flattened ids + offsets [n_phrases + 1] (asr_sensevoice_set_hotwords' shape); an empty list switches the mode off. Checked before anything
  // changes: ids in [0, vocab), no empty phrase, a finite boost. Every row's node goes back to the root.
  void set_hotwords(const int32_t* ids, const int32_t* offsets, int n_phrases, float boost, int vocab, hipStream_t s, const char* who) {
    ASR_REQUIRE(n_phrases >= 0 && (n_phrases == 0 || (ids && offsets)) && std::isfinite(boost), "%s: bad argument", who);
    if (n_phrases > 0) {
      ASR_REQUIRE(offsets[0] >= 0, "%s: offsets[0] = %d", who, offsets[0]);
      for (int p = 0; p < n_phrases; ++p) {
        ASR_REQUIRE(offsets[p + 1] > offsets[p], "%s: phrase %d is empty", who, p);
        for (int32_t i = offsets[p]; i < offsets[p + 1]; ++i)
          ASR_REQUIRE(ids[i] >= 0 && ids[i] < vocab, "%s: phrase %d holds token %d (vocabulary %d)", who, p, ids[i], vocab);
      }
    }
    HIP_CHECK(hipStreamSynchronize(s));                  // (nothing in flight reads the image that is about to change)
    if (n_phrases == 0) { hot_nodes = 0; hot_root = 0; hot_boost = 0.0f; }
    else {
      int n = 0;
      const std::vector<int32_t> words = build_hot_trie(ids, offsets, n_phrases, &n);
      d_trie.reserve(words.size() * 4, s);
      HIP_CHECK(hipMemcpyAsync(d_trie.ptr, words.data(), words.size() * 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipStreamSynchronize(s));
      hot_nodes = n; hot_boost = boost;
      hot_root = words[(size_t)2 * n + 1];               // child_off[1]: the root's children
    }
    if (d_node.ptr && node_rows > 0) HIP_CHECK(hipMemsetAsync(d_node.ptr, 0, (size_t)node_rows * 4, s));
    ++hot_gen;
    ++epoch;
  }
  // The back-off n-gram model fused into the greedy heads and the beam ranker: image_words as asr_sensevoice_set_lm takes them, checked by
  // ngram_lm_validate against `vocab` (these families have no blank id); null or n_words == 0 clears the model. Everything is checked before anything
  // changes: a refused call leaves the model in force. Every row's state goes back to start_node.
  void set_lm(const int32_t* image_words, int64_t n_words, float alpha, float beta, float oov, int topk, const int32_t* end_ids, int n_end, int vocab, hipStream_t s,
              const char* who) {
    const bool clear = !image_words || n_words == 0;
    LmView v;
    if (!clear) {
      ASR_REQUIRE(topk >= 1 && topk <= LM_TOPK_MAX, "%s: topk %d outside 1..%d", who, topk, LM_TOPK_MAX);
      ASR_REQUIRE(n_end >= 0 && n_end <= LM_ENDS_MAX && (n_end == 0 || end_ids), "%s: %d end ids (at most %d)", who, n_end, LM_ENDS_MAX);
      for (int i = 0; i < n_end; ++i) ASR_REQUIRE(end_ids[i] >= 0 && end_ids[i] < vocab, "%s: end id %d outside the vocabulary of %d", who, end_ids[i], vocab);
      ngram_lm_validate(image_words, n_words, vocab, -1, alpha, beta, oov, who);
      v.topk = topk; v.ends.n = n_end;
      for (int i = 0; i < n_end; ++i) v.ends.id[i] = end_ids[i];
    }
    HIP_CHECK(hipStreamSynchronize(s));                  // (nothing in flight reads the image that is about to change)
    if (!clear) {
      d_lm.reserve((size_t)n_words * 4, s);
      HIP_CHECK(hipMemcpyAsync(d_lm.ptr, image_words, (size_t)n_words * 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipStreamSynchronize(s));
      v.lm = ngram_lm_view(d_lm.as<int32_t>(), image_words, alpha, beta, oov);
    }
    lm = v;
    if (lm.on() && d_lmstate.ptr && lm_rows > 0) fill_states(0, std::max(lm_rows, 64), s);
    ++epoch;
  }
  void arm_noise(const float* uniforms, int count, hipStream_t s) {
    d_noise.reserve((size_t)count * 4, s);
    HIP_CHECK(hipMemcpyAsync(d_noise.ptr, uniforms, (size_t)count * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    noise_armed = true;
  }

  void reserve(int rows, hipStream_t s) {
    bool moved = reserve_moved(d_nsaved, 256, s);
    moved |= reserve_moved(d_save, (size_t)rows * ld_save * 4, s);
    if (scores) { moved |= reserve_moved(d_scores, (size_t)rows * ld_save * 4, s); score_rows = rows; }
    if (hot()) {
      if (reserve_moved(d_node, (size_t)std::max(rows, 64) * 4, s) || rows > node_rows) {       // fresh rows start at the root
        moved = true;
        HIP_CHECK(hipMemsetAsync(d_node.ptr, 0, (size_t)std::max(rows, 64) * 4, s));
      }
      node_rows = std::max(node_rows, rows);
      moved |= reserve_moved(d_rootsave, (size_t)rows * std::max(hot_root, 1) * 4, s);
    }
    if (lm.on()) {
      const int cap = std::max(rows, 64);
      if (reserve_moved(d_lmstate, (size_t)cap * 4, s) || rows > lm_rows) {                     // fresh rows start at start_node
        moved = true;
        fill_states(0, cap, s);
      }
      lm_rows = std::max(lm_rows, rows);
      for (DeviceBuffer* q : {&d_lmv, &d_lmi}) moved |= reserve_moved(*q, (size_t)rows * LM_TOPK_MAX * 4, s);
      moved |= reserve_moved(d_lmlse, (size_t)cap * 4, s);
    }
    if (moved) ++epoch;
  }
  void restart(hipStream_t s) { HIP_CHECK(hipMemsetAsync(d_nsaved.ptr, 0, 4, s)); scored = scores; row_biased = false; }      // every prefill starts from an empty history (ids and scores: one counter)

  // The head's launches on logits [rows][ld]: picks go to next [rows]. bias: Whisper's BEGIN_SUPPRESS after a prefill, else null. penalise: false on a
  // prefill (the prefill graphs select from the raw logits with an empty history; the decode graphs apply the penalty first). Timestamp mode: the rules
  // run on both, after the penalty and before the selection (an empty history is their initial rule). Scores mode: the arg-max is the fused kernel, the
  // sampler is followed by the at-id kernel (it sees the sampler's in-place repetition penalty), the pick joins the history; off, nothing new is launched.
  // Hotwords: the sparse bias (launch_hotword_bias) after the penalty and before the timestamp rules, so the selection, rule 5 and the token score all read
  // the biased row ("the row the selection sees"), and logits_out of the step shows it; the node follows the pick in the launch that appends it. Every pick
  // joins the history. Off, nothing new is launched.
  void enqueue(float* logits, int ld, int rows, int n_valid, const float* bias, bool penalise, int32_t* next, hipStream_t s) {
    const bool penalised = penalty_value != 1.0f && !sampling;
    int32_t* save = d_save.as<int32_t>();
    int32_t* n_saved = d_nsaved.as<int32_t>();
    // the score kernels write row r of d_scores for every r < rows: reserve(rows) must have run with the mode on (the sessions call it before every step)
    ASR_REQUIRE(!scores || (d_scores.ptr && rows <= score_rows), "token scores: the score history holds %d rows, this step has %d (switch token scores on before the prefill)",
                d_scores.ptr ? score_rows : 0, rows);
    if (penalised && penalise) launch_apply_penalty(logits, ld, rows, save, ld_save, n_saved, penalty_range, penalty_value, s, partial);
    const HotTrie trie = hot_trie();
    if (hot()) {
      ASR_REQUIRE(d_node.ptr && rows <= node_rows, "hotwords: the node table holds %d rows, this step has %d", d_node.ptr ? node_rows : 0, rows);
      HotScope hs(prof, s);
      launch_hotword_bias(logits, ld, rows, n_valid, trie, d_node.as<int32_t>(), n_saved, penalise ? nullptr : d_rootsave.as<float>(), s);
      if (!penalise) { row_biased = true; biased_gen = hot_gen; }
    }
    if (ts.on) ts.enqueue(prof, logits, ld, rows, n_valid, save, ld_save, n_saved, 0, s);
    if (sampling) {                        // the bias first, history = every sampled id
      SampleArgs sa;
      sa.logits = logits; sa.ld = ld; sa.rows = rows; sa.n_valid = n_valid; sa.extra = bias;
      sa.save_ids = save; sa.ld_save = ld_save; sa.n_saved = n_saved;
      sa.temperature = temperature; sa.top_p = top_p; sa.repetition_penalty = samp_rep_penalty; sa.top_k = top_k;
      sa.noise = noise_armed ? d_noise.as<float>() : nullptr; sa.seed = samp_seed; sa.next = next;
      launch_sample_topk_topp(sa, s);
      if (scores) {
        ScoreScope sc(prof, s);
        launch_logprob_at_rows(logits, ld, rows, n_valid, bias, next, d_scores.as<float>(), ld_save, n_saved, s);
      }
    } else if (lm.on()) {                  // the fused greedy pick: the topk best columns of the row as it stands, value + LM term, the state follows the pick
      ASR_REQUIRE(d_lmstate.ptr && rows <= lm_rows, "language model: the state table holds %d rows, this step has %d", d_lmstate.ptr ? lm_rows : 0, rows);
      LmScope ls(prof, s);
      launch_lm_topk(logits, ld, rows, n_valid, bias, lm.topk, d_lmv.as<float>(), d_lmi.as<int32_t>(), d_lmlse.as<float>(), s);
      launch_lm_pick(d_lmv.as<float>(), d_lmi.as<int32_t>(), d_lmlse.as<float>(), rows, lm.topk, lm.lm, lm.ends, d_lmstate.as<int32_t>(), n_saved, next,
                     scores ? d_scores.as<float>() : nullptr, ld_save, s);
    } else if (scores) {
      ScoreScope sc(prof, s);
      launch_argmax_logprob_rows(logits, ld, rows, n_valid, bias, next, d_scores.as<float>(), ld_save, n_saved, s);
    } else {
      launch_argmax_rows(logits, ld, rows, n_valid, bias, next, s);
    }
    if (penalised || sampling || track_history || ts.on || scores || hot() || lm.on()) {   // GREEDY_SEARCH / the sampling head append their pick to the history
      if (hot()) {                         // the append and the node's step are one launch: the mode adds the bias kernel to a head that keeps a history
        HotScope hs(prof, s);
        launch_hotword_advance(next, rows, trie, d_node.as<int32_t>(), n_saved, s, save, ld_save);
      } else {
        launch_append_ids(next, rows, save, ld_save, n_saved, s);
      }
      launch_add_scalar(n_saved, 1, s);
    }
  }
  void consumed() { noise_armed = false; }        // after the step: caller-supplied uniforms serve exactly one

  // The scores of the picks since the last restart, oldest first: logprob_out [rows][out_stride] gets min(count, out_stride) per row (slots past the count keep
  // the caller's fill), *n_out the count. Returns with the stream drained. `who`: the C entry's name.
  void download_scores(int rows, float* logprob_out, int out_stride, int32_t* n_out, hipStream_t s, const char* who) {
    ASR_REQUIRE(logprob_out && n_out && out_stride >= 1, "%s: bad argument", who);
    ASR_REQUIRE(scores, "%s: token scores are off (switch them on before the prefill)", who);
    ASR_REQUIRE(rows > 0 && rows <= score_rows && scored && d_scores.ptr && d_nsaved.ptr, "%s: no prefill since token scores were switched on", who);
    int32_t n = 0;
    HIP_CHECK(hipMemcpyAsync(&n, d_nsaved.ptr, 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    n = std::min(std::max(n, 0), ld_save);
    *n_out = n;
    const int take = std::min(n, out_stride);
    if (take > 0) {
      HIP_CHECK(hipMemcpy2DAsync(logprob_out, (size_t)out_stride * 4, d_scores.ptr, (size_t)ld_save * 4, (size_t)take * 4, rows, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
    }
  }

 private:
  void fill_states(int first, int count, hipStream_t s) {      // rows [first, first + count) of d_lmstate = start_node (returns with the copy done)
    const std::vector<int32_t> h((size_t)count, lm.lm.start_node);
    HIP_CHECK(hipMemcpyAsync(d_lmstate.as<int32_t>() + first, h.data(), (size_t)count * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
  struct ScoreScope {                  // the score launches are a profile class of their own, as the timestamp rules are
    Profiler* p; hipStream_t s;
    ScoreScope(Profiler* p_, hipStream_t s_) : p(p_ && p_->enabled ? p_ : nullptr), s(s_) { if (p) p->begin(p->cls("token_scores"), s); }
    ~ScoreScope() { if (p) p->end(s); }
  };
};

// ---- beam-search ranking (semantics of oracle/qwen_asr_oracle.py:beam_search_core): hypothesis rows b * beam + r, their scores, lengths and ended flags, the
// double-buffered ancestry / token tables [rows][ld] and the ids of the next pass, all on the device. The family keeps its hypothesis caches and its decoder pass.
struct ASR_LOCAL BeamRanker {
  DeviceBuffer topv, topi, cum, fin, len, done, next, stop, src[2], tok[2];
  DeviceBuffer node[2], lse;           // hotwords: the rows' trie nodes, double-buffered with `cur` like src / tok, and beam_topk's log-sum-exp per row
  HotView hot;                         // set by begin (the head's); off, no pass launches anything new
  DeviceBuffer state[2], lmv, lmi;     // language model: the rows' states, double-buffered like node, and launch_lm_topk's candidate list per row (lse is shared)
  LmView lmod;                         // set by begin (the head's); off, no pass launches anything new
  PinnedBuffer stage;                  // its own: a prefill called with null outputs may still be copying from the session's. [0, done_off) stop ids, then done flags
  uint64_t epoch = 0;                  // moves when a buffer moved: a captured step that ranks is stale
  int B = 0, beam = 0, ld = 0, n_stop = 0, done_off = 0, cur = 0;
  TimestampRule ts;                    // Whisper's timestamp mode (set by begin): the rules run on every row before it is ranked
  Profiler* prof = nullptr;
  const int32_t* slots_dev = nullptr;  // when set, the generated cache slots after a pass are *slots_dev + slots_off (a device counter: the pass replays from a captured graph)
  int slots_off = 0;

  int rows() const { return B * beam; }
  const int32_t* ancestry() const { return src[cur].as<int32_t>(); }     // the table the next pass's self-attention follows
  int32_t* next_ids() const { return next.as<int32_t>(); }

  void begin(int B_, int beam_, int ld_, const int32_t* stop_ids, int n_stop_, const TimestampRule& ts_, const HotView& hot_, hipStream_t s,
             const LmView& lm_ = LmView{}, const char* who = "beam_search") {
    ASR_REQUIRE(!lm_.on() || lm_.topk >= beam_, "%s: the language model's topk %d is below the beam width %d", who, lm_.topk, beam_);
    B = B_; beam = beam_; ld = ld_; n_stop = n_stop_; cur = 0; slots_dev = nullptr; slots_off = 0; ts = ts_; hot = hot_; lmod = lm_;
    const size_t N = (size_t)rows(), Nn = std::max<size_t>(N, 64);
    bool moved = false;
    for (DeviceBuffer* q : {&topv, &topi}) moved |= reserve_moved(*q, Nn * BEAM_MAX * 4, s);
    for (DeviceBuffer* q : {&cum, &fin, &len, &done, &next}) moved |= reserve_moved(*q, Nn * 4, s);
    moved |= reserve_moved(stop, (size_t)std::max(n_stop, 16) * 4, s);
    for (DeviceBuffer* q : {&src[0], &src[1], &tok[0], &tok[1]}) moved |= reserve_moved(*q, N * ld * 4, s);
    if (hot.on()) for (DeviceBuffer* q : {&node[0], &node[1], &lse}) moved |= reserve_moved(*q, Nn * 4, s);
    if (lmod.on()) {
      for (DeviceBuffer* q : {&state[0], &state[1], &lse}) moved |= reserve_moved(*q, Nn * 4, s);
      for (DeviceBuffer* q : {&lmv, &lmi}) moved |= reserve_moved(*q, Nn * LM_TOPK_MAX * 4, s);
    }
    if (moved) ++epoch;
    HIP_CHECK(hipStreamSynchronize(s));
    done_off = std::max(n_stop, 16);
    stage.reserve((size_t)(done_off + std::max(B, 64)) * 4);
    if (n_stop) {
      memcpy(stage.ptr, stop_ids, (size_t)n_stop * 4);
      HIP_CHECK(hipMemcpyAsync(stop.ptr, stage.ptr, (size_t)n_stop * 4, hipMemcpyHostToDevice, s));
    }
    HIP_CHECK(hipMemsetAsync(done.ptr, 0, (size_t)B * 4, s));
    HIP_CHECK(hipMemsetAsync(len.ptr, 0, N * 4, s));
    if (hot.on()) HIP_CHECK(hipMemsetAsync(node[0].ptr, 0, Nn * 4, s));        // every hypothesis starts at the root
  }
  // the first ranking: the prefill's logits, one row per utterance (+ bias: Whisper's BEGIN_SUPPRESS, as the arg-max head after a prefill). Timestamp mode:
  // the rules with an empty history first (len is zero after begin; the token table is not read). Hotwords: a row the head biased in place gets the model's
  // own values back first -- a hypothesis score is log-soft-max(model) + delta, and a soft-max over the biased row would renormalise
  void rank_first(float* logits, int ld_logits, int n_valid, const float* bias, hipStream_t s) {
    if (hot.on() && hot.root_save) { HotScope hs(prof, s); launch_hotword_restore(logits, ld_logits, B, n_valid, hot.trie, hot.root_save, s); }
    if (ts.on) ts.enqueue(prof, logits, ld_logits, B, n_valid, tok[cur].as<int32_t>(), ld, len.as<int32_t>(), 0, s);
    if (lmod.on()) rerank_lm(logits, ld_logits, B, n_valid, bias, beam, true, s);     // every utterance starts at the model's start_node
    else {
      launch_beam_topk(logits, ld_logits, B, n_valid, bias, beam, topv.as<float>(), topi.as<int32_t>(), s, hot.on() ? lse.as<float>() : nullptr);
      if (hot.on()) rerank(logits, ld_logits, B, n_valid, bias, beam, s);      // utterance b's one row is at the root, as node[cur][b * beam] says
    }
    select(1, 0, s);
    flip();
  }
  // Rank the rows' extensions on the current tables: the select pass writes the ids of the next pass and the ancestry of this one. n_slots: generated cache
  // slots after the pass (ignored once slots_dev is set). The caller flips afterwards -- outside a captured step, whose replay runs no host code.
  // Timestamp mode: the rules first, row r's history being its len[r] ids of the current token table.
  void enqueue_rank(float* logits, int ld_logits, int n_valid, int n_slots, hipStream_t s) {
    if (ts.on) ts.enqueue(prof, logits, ld_logits, rows(), n_valid, tok[cur].as<int32_t>(), ld, len.as<int32_t>(), 1, s);
    if (lmod.on()) rerank_lm(logits, ld_logits, rows(), n_valid, nullptr, 1, false, s);
    else {
      launch_beam_topk(logits, ld_logits, rows(), n_valid, nullptr, beam, topv.as<float>(), topi.as<int32_t>(), s, hot.on() ? lse.as<float>() : nullptr);
      if (hot.on()) rerank(logits, ld_logits, rows(), n_valid, nullptr, 1, s);
    }
    select(0, n_slots, s);
  }
  void flip() { cur ^= 1; }
  // the per-utterance "best hypothesis has ended" flags, read back once per step
  bool all_done(hipStream_t s) {
    int32_t* h_done = stage.as<int32_t>() + done_off;
    HIP_CHECK(hipMemcpyAsync(h_done, done.ptr, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    bool all = true;
    for (int b = 0; b < B; ++b) all = all && h_done[b] != 0;
    return all;
  }
  // per utterance its hypotheses best-first: tokens_out [rows][out_stride], n_out [rows], scores_out [rows] (nullable)
  void download(int32_t* tokens_out, int out_stride, int32_t* n_out, float* scores_out, hipStream_t s) {
    const size_t N = (size_t)rows();
    std::vector<int32_t> h_tok(N * ld), h_len(N);
    std::vector<float> h_cum(N);
    HIP_CHECK(hipMemcpyAsync(h_tok.data(), tok[cur].ptr, N * ld * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(h_len.data(), len.ptr, N * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(h_cum.data(), cum.ptr, N * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    for (size_t r = 0; r < N; ++r) {
      n_out[r] = h_len[r];
      if (scores_out) scores_out[r] = h_cum[r];
      for (int j = 0; j < h_len[r] && j < out_stride; ++j) tokens_out[r * out_stride + j] = h_tok[r * ld + j];
    }
  }

 private:
  // hotwords: the K best of topK u S by log-prob + delta, back into topv / topi (launch_hotword_rerank)
  void rerank(const float* logits, int ld_logits, int n_rows, int n_valid, const float* bias, int node_stride, hipStream_t s) {
    HotScope hs(prof, s);
    launch_hotword_rerank(logits, ld_logits, n_rows, n_valid, bias, lse.as<float>(), hot.trie, node[cur].as<int32_t>(), node_stride, beam, topv.as<float>(),
                          topi.as<int32_t>(), s);
  }
  // language model: the topk best columns of every row, then the K best of topM u S by log-prob + delta + LM term (launch_lm_topk / launch_lm_rerank: they
  // replace beam_topk + the hotword re-rank; the trie is optional)
  void rerank_lm(const float* logits, int ld_logits, int n_rows, int n_valid, const float* bias, int stride, bool first, hipStream_t s) {
    LmScope ls(prof, s);
    launch_lm_topk(logits, ld_logits, n_rows, n_valid, bias, lmod.topk, lmv.as<float>(), lmi.as<int32_t>(), lse.as<float>(), s);
    launch_lm_rerank(logits, ld_logits, n_rows, n_valid, bias, lmv.as<float>(), lmi.as<int32_t>(), lse.as<float>(), lmod.topk, hot.trie,
                     hot.on() ? node[cur].as<int32_t>() : nullptr, lmod.lm, lmod.ends, first ? nullptr : state[cur].as<int32_t>(), stride, beam, topv.as<float>(),
                     topi.as<int32_t>(), s);
  }
  void select(int first, int n_slots, hipStream_t s) {
    BeamArgs a{};
    a.beam = beam; a.K = beam; a.ld = ld; a.first = first; a.n_slots = n_slots;
    a.topv = topv.as<float>(); a.topi = topi.as<int32_t>();
    a.cum = cum.as<float>(); a.fin = fin.as<int32_t>(); a.len = len.as<int32_t>(); a.done = done.as<int32_t>(); a.next = next.as<int32_t>();
    a.stop = stop.as<int32_t>(); a.n_stop = n_stop;
    a.src_in = src[cur].as<int32_t>(); a.tok_in = tok[cur].as<int32_t>();
    a.src_out = src[cur ^ 1].as<int32_t>(); a.tok_out = tok[cur ^ 1].as<int32_t>();
    if (!first) { a.slots_dev = slots_dev; a.slots_off = slots_off; }
    if (hot.on()) { a.node_in = node[cur].as<int32_t>(); a.node_out = node[cur ^ 1].as<int32_t>(); a.trie = hot.trie; }
    if (lmod.on()) { a.lm = lmod.lm; a.ends = lmod.ends; a.state_in = state[cur].as<int32_t>(); a.state_out = state[cur ^ 1].as<int32_t>(); }
    launch_beam_select(a, B, s);
  }
};

// A step's picks next [rows] and logits [rows][n_valid] (row stride ld on the device) to the caller through pinned staging; either output may be null.
// Returns with the stream drained.
ASR_LOCAL inline void download_step(PinnedBuffer& stage, const void* next, const void* logits, int ld, int rows, int n_valid, int32_t* next_out, float* logits_out,
                                    hipStream_t s) {
  const size_t nbytes = (size_t)rows * 4, lbytes = (size_t)rows * n_valid * 4;
  stage.reserve(nbytes + 64 + (logits_out ? lbytes : 0));
  unsigned char* st = stage.as<unsigned char>();
  if (next_out) HIP_CHECK(hipMemcpyAsync(st, next, nbytes, hipMemcpyDeviceToHost, s));
  if (logits_out)
    HIP_CHECK(hipMemcpy2DAsync(st + nbytes + 64, (size_t)n_valid * 4, logits, (size_t)ld * 4, (size_t)n_valid * 4, rows, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  if (next_out) memcpy(next_out, st, nbytes);
  if (logits_out) memcpy(logits_out, st + nbytes + 64, lbytes);
}
