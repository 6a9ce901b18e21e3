// Back-off n-gram language model: the image's layout, its host-side check and the device-side walk. Its users: the three token-synchronous
// beam searches through beam_dev.h (ctc_beam.hip, nar_beam.hip, nar_stream_beam.hip), the autoregressive decoders' selection head and beam ranker
// (decoder_lm.hip, kernels.hip; the end of this file), the sessions that hold an image (sanm_session.h, decode_head.h) and the host-array entry points
// (api.hip). The float64 statement is tests/ctc_lm_ref.py: build_image / lm_step.
//
// One blob of 32-bit words over token ids, order N in 1..5:
//   header  [order, n_nodes, n_edges, vocab, start_node, eos_edge_token]
//   depth   i32 [n_nodes]        nodes are the contexts: node 0 the empty one, every listed n-gram of order 1..N-1 a node of depth n
//   backoff f32 [n_nodes]        natural log
//   suffix  i32 [n_nodes]        the node of the context minus its first token(s): its longest proper suffix that is a node (the root for depth 1)
//   child_off i32 [n_nodes + 1]  edges of node n: [child_off[n], child_off[n + 1]), sorted strictly by token
//   tok     i32 [n_edges]        edges are the listed n-grams of order 1..N: context node + token
//   logp    f32 [n_edges]        natural log, <= 0
//   next    i32 [n_edges]        the node of the longest suffix of the full n-gram that is a node: the state after the token
//   uni     i32 [vocab + 2]      the root's edge for token c, or -1; </s> and <s> take the ids vocab and vocab + 1 and are never candidates
// start_node is `next` of the <s> unigram (0 without one); eos_edge_token is vocab when the model lists </s>, else -1.
#pragma once
#include <cmath>
#include <cstring>

#include "common.h"

constexpr int NGRAM_LM_HEADER = 6;
constexpr int NGRAM_LM_MAX_ORDER = 5;

struct NgramLm {                      // the image as the device sees it; n_nodes == 0: no language model (no pointer is read)
  const int32_t *suffix = nullptr, *child_off = nullptr, *tok = nullptr, *next = nullptr, *uni = nullptr;
  const float *backoff = nullptr, *logp = nullptr;
  int n_nodes = 0, start_node = 0, eos = -1;
  float alpha = 0.0f, beta = 0.0f, oov = 0.0f;
};

inline int64_t ngram_lm_words(int64_t n_nodes, int64_t n_edges, int64_t vocab) { return NGRAM_LM_HEADER + 4 * n_nodes + 1 + 3 * n_edges + vocab + 2; }

// Everything the walk relies on, checked on the host before an image is used: sizes, monotone offsets, sorted children, suffix links that lose depth (the
// walk ends at the root), states in range, finite non-positive log-probabilities, finite back-offs, a `uni` table that mirrors the root's edges.
inline void ngram_lm_validate(const int32_t* w, int64_t n_words, int vocab, int blank_id, float alpha, float beta, float oov, const char* who) {
  ASR_REQUIRE(std::isfinite(alpha) && alpha >= 0.0f && std::isfinite(beta) && std::isfinite(oov) && oov <= 0.0f,
              "%s: alpha %g (finite, >= 0), beta %g (finite), oov_logprob %g (finite, <= 0)", who, (double)alpha, (double)beta, (double)oov);
  ASR_REQUIRE(w && n_words >= NGRAM_LM_HEADER, "%s: a language model image has at least %d words", who, NGRAM_LM_HEADER);
  const int order = w[0], n_nodes = w[1], n_edges = w[2], v = w[3], start = w[4], eos = w[5];
  ASR_REQUIRE(order >= 1 && order <= NGRAM_LM_MAX_ORDER && n_nodes >= 1 && n_edges >= 0 && v >= 1, "%s: header (order %d, %d nodes, %d edges, vocabulary %d)", who, order,
              n_nodes, n_edges, v);
  ASR_REQUIRE(v == vocab, "%s: the image is over a vocabulary of %d, the search over %d", who, v, vocab);
  ASR_REQUIRE(ngram_lm_words(n_nodes, n_edges, v) == n_words, "%s: %lld words, the header asks for %lld", who, (long long)n_words, (long long)ngram_lm_words(n_nodes, n_edges, v));
  const int32_t* depth = w + NGRAM_LM_HEADER;
  const int32_t *backoff = depth + n_nodes, *suffix = backoff + n_nodes, *off = suffix + n_nodes, *tok = off + n_nodes + 1, *logp = tok + n_edges, *next = logp + n_edges,
                *uni = next + n_edges;
  auto f32 = [](int32_t bits) { float f; memcpy(&f, &bits, 4); return f; };
  ASR_REQUIRE(start >= 0 && start < n_nodes && (eos == -1 || eos == v), "%s: start_node %d, eos_edge_token %d", who, start, eos);
  ASR_REQUIRE(depth[0] == 0 && suffix[0] == 0 && off[0] == 0 && off[n_nodes] == n_edges, "%s: malformed root or child_off", who);
  for (int n = 0; n < n_nodes; ++n) {
    ASR_REQUIRE(std::isfinite(f32(backoff[n])), "%s: node %d has a back-off that is not finite", who, n);
    ASR_REQUIRE(off[n] <= off[n + 1] && off[n + 1] <= n_edges, "%s: child_off decreases at node %d", who, n);
    if (n > 0)
      ASR_REQUIRE(depth[n] >= 1 && depth[n] < order && suffix[n] >= 0 && suffix[n] < n_nodes && depth[suffix[n]] < depth[n], "%s: node %d (depth %d) has the suffix link %d", who, n,
                  depth[n], suffix[n]);
  }
  for (int n = 0; n < n_nodes; ++n)
    for (int e = off[n]; e < off[n + 1]; ++e) {
      ASR_REQUIRE(tok[e] >= 0 && tok[e] < v + 2 && tok[e] != blank_id && (e == off[n] || tok[e - 1] < tok[e]), "%s: node %d, edge %d: token %d (sorted, no blank)", who, n, e, tok[e]);
      const float lp = f32(logp[e]);
      ASR_REQUIRE(std::isfinite(lp) && lp <= 0.0f, "%s: edge %d has the log-probability %g", who, e, (double)lp);
      ASR_REQUIRE(next[e] >= 0 && next[e] < n_nodes && depth[next[e]] <= depth[n] + 1, "%s: edge %d leads to node %d", who, e, next[e]);
      if (n == 0) ASR_REQUIRE(uni[tok[e]] == e, "%s: uni[%d] = %d, the root's edge is %d", who, tok[e], uni[tok[e]], e);
    }
  for (int c = 0; c < v + 2; ++c)
    ASR_REQUIRE(uni[c] == -1 || (uni[c] >= 0 && uni[c] < off[1] && tok[uni[c]] == c), "%s: uni[%d] = %d", who, c, uni[c]);
  ASR_REQUIRE(eos < 0 || uni[eos] >= 0, "%s: eos_edge_token without a </s> unigram", who);
}

// points an NgramLm into a device copy of an image whose (checked) header is host_words
inline NgramLm ngram_lm_view(const int32_t* dev_words, const int32_t* host_words, float alpha, float beta, float oov) {
  NgramLm m;
  const int n_nodes = host_words[1], n_edges = host_words[2];
  const int32_t* depth = dev_words + NGRAM_LM_HEADER;
  m.backoff = reinterpret_cast<const float*>(depth + n_nodes);
  m.suffix = depth + 2 * n_nodes; m.child_off = m.suffix + n_nodes; m.tok = m.child_off + n_nodes + 1;
  m.logp = reinterpret_cast<const float*>(m.tok + n_edges);
  m.next = m.tok + 2 * n_edges; m.uni = m.next + n_edges;
  m.n_nodes = n_nodes; m.start_node = host_words[4]; m.eos = host_words[5];
  m.alpha = alpha; m.beta = beta; m.oov = oov;
  return m;
}

// log P(c | state) and the state after c. A token without a unigram is out of vocabulary: it costs oov and the state does not move (SenseVoice's prompt rows
// emit tags no text model knows). Otherwise back off from the state until a context lists c: at most `order` lookups, each a binary search of one child list
// (the root's through uni); the loop bound only restates what ngram_lm_validate guarantees.
__device__ __forceinline__ float lm_step(const NgramLm& lm, int& state, int c) {
  const int ue = lm.uni[c];
  if (ue < 0) return lm.oov;
  float acc = 0.0f;
  int n = state;
  for (int hop = 0; hop < NGRAM_LM_MAX_ORDER; ++hop) {
    int e = -1;
    if (n == 0) e = ue;
    else {
      int lo = lm.child_off[n], hi = lm.child_off[n + 1];
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int t = lm.tok[mid];
        if (t == c) { e = mid; break; }
        if (t < c) lo = mid + 1; else hi = mid;
      }
    }
    if (e >= 0) { state = lm.next[e]; return acc + lm.logp[e]; }
    acc += lm.backoff[n];
    n = lm.suffix[n];
  }
  return acc;                         // (not reached with a checked image)
}

// ---- the autoregressive decoders' use of the walk (decoder_lm.hip, beam_select_kernel). `ends`: the family's end-of-text ids, scored as </s>.
constexpr int LM_ENDS_MAX = 8;
struct LmEnds { int n = 0; int32_t id[LM_ENDS_MAX] = {}; };

// The LM term of token c from `state`, and the state after it: an end id, when the image lists </s>, costs alpha * log P(</s> | state) without the length
// bonus and leaves the state; every other token alpha * log P(c | state) + beta, each operation rounded on its own.
__device__ __forceinline__ float lm_token_term(const NgramLm& lm, const LmEnds& ends, int& state, int c) {
  bool is_end = false;
#pragma unroll
  for (int i = 0; i < LM_ENDS_MAX; ++i) is_end = is_end || (i < ends.n && ends.id[i] == c);     // (constant indices: the list stays in scalar registers)
  if (is_end && lm.eos >= 0) { int keep = state; return __fmul_rn(lm.alpha, lm_step(lm, keep, lm.eos)); }
  return __fadd_rn(__fmul_rn(lm.alpha, lm_step(lm, state, c)), lm.beta);
}
