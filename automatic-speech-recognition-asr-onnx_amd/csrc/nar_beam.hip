// Token-synchronous beam search over the token rows of a non-autoregressive decoder (offline Paraformer), with the hotword context graph
// (hot_trie.h) and, in the kLm instantiation, a back-off n-gram language model (ngram_lm.h) fused into the ranking. Not a CTC search: there is no blank, no
// collapse and no merging -- every hypothesis of an utterance picks exactly one candidate per token row, so all of them have the utterance's token count and
// two hypotheses with different picks differ in content. The candidates come from ctc_topk_kernel (ctc_beam.hip) behind the decoder's vocabulary GEMM. The
// float64 statement is tests/nar_beam_ref.py.
#include <type_traits>

#include "engine.h"
#include "hot_trie.h"
#include "kernels.h"
#include "ngram_lm.h"

namespace {

constexpr int NAR_BEAM_MAX = 16;
constexpr int NAR_BEAM_THREADS = NAR_BEAM_MAX * NAR_BEAM_MAX;        // one thread per extension of a row

template <bool kLm> struct NarLmState {};
template <> struct NarLmState<true> {                // a hypothesis' language-model total (alpha * logp + beta over its tokens) and state
  float lm[NAR_BEAM_MAX];
  int lmstate[NAR_BEAM_MAX];
};
template <bool kLm>
struct NarLive : NarLmState<kLm> {                   // the live hypotheses of one row, in rank order
  float am[NAR_BEAM_MAX], bonus[NAR_BEAM_MAX];
  int node[NAR_BEAM_MAX];
};
struct NarNoLm {};

// One workgroup per utterance, sequential over its N token rows plan[u].row_off .. + N of the compact token plan, N = plan[u].n_lfr read here (rows at or
// past *m_dev are never read: N is cut there). Entry e = p * topk + j of row k extends live hypothesis p (rank order) by candidate column j; a candidate
// with lp = -inf makes no entry. Every entry carries, all in f32 and in this order of operations:
//   am' = am[p] + lp[k][j]                                   (the running acoustic sum, in row order)
//   (node', bonus') = trie_step(node[p], bonus[p], token)
//   lm' = lm[p] + (alpha * log P(token | state[p]) + beta)   (kLm; product and sum rounded separately; an out-of-vocabulary token costs oov and keeps the state)
//   key = (am' + bonus') + lm'
// The best min(beam, entries) survive by key descending, ties to the lower e; their rank is their index at the next row. A kept entry appends
// (parent rank, candidate column) to the utterance's pool at [k * beam + rank]: the walk back reads the token and its log-probability from the candidate
// arrays at (row k, column). After the last row a hypothesis inside a phrase gives depth[node] * boost back, (kLm) adds alpha * log P(</s> | state) when
// the model lists </s>, the hypotheses are ranked again by (am + bonus) + lm (ties to the lower rank) and the best nbest are walked back. An utterance
// without tokens yields the one empty hypothesis. Candidate ids of a row must be distinct and, with a model, lie in [0, vocab) of the image.
template <bool kLm>
__global__ __launch_bounds__(NAR_BEAM_THREADS) void nar_beam_kernel(const int32_t* __restrict__ cand_id, const float* __restrict__ cand_lp, int topk,
                                                                    const UttPlan* __restrict__ plan, const int32_t* __restrict__ m_dev, int beam, int nbest,
                                                                    HotTrie tr, typename std::conditional<kLm, NgramLm, NarNoLm>::type lmod,
                                                                    int2* __restrict__ pool_all, int pool_stride, int32_t* __restrict__ tok_out,
                                                                    int max_tokens, int32_t* __restrict__ num_out, float* __restrict__ score_out,
                                                                    float* __restrict__ am_out, float* __restrict__ tlp_out) {
  __shared__ NarLive<kLm> live[2];
  __shared__ float e_score[NAR_BEAM_MAX * NAR_BEAM_MAX];
  __shared__ int c_id[NAR_BEAM_MAX], f_order[NAR_BEAM_MAX];
  __shared__ float c_lp[NAR_BEAM_MAX], f_score[NAR_BEAM_MAX], f_am[NAR_BEAM_MAX];
  const int u = blockIdx.x, e = threadIdx.x;
  const int row0 = plan[u].row_off;
  int N = plan[u].n_lfr;
  if (m_dev) N = min(N, max(*m_dev - row0, 0));
  N = max(min(N, pool_stride / beam), 0);
  int2* pool = pool_all + (size_t)u * pool_stride;
  if (e == 0) {
    live[0].am[0] = 0.0f; live[0].bonus[0] = 0.0f; live[0].node[0] = 0;
    if constexpr (kLm) { live[0].lm[0] = 0.0f; live[0].lmstate[0] = lmod.start_node; }
  }
  int n_live = 1;
  int nx_id = 0; float nx_lp = 0.0f;                    // the next row's candidate of this thread (threads < topk), fetched a row ahead
  if (e < topk && N > 0) { nx_id = cand_id[(size_t)row0 * topk + e]; nx_lp = cand_lp[(size_t)row0 * topk + e]; }
  for (int k = 0; k < N; ++k) {
    const NarLive<kLm>& cur = live[k & 1];
    NarLive<kLm>& nxt = live[(k + 1) & 1];
    if (e < topk) {
      c_id[e] = nx_id; c_lp[e] = nx_lp;
      if (k + 1 < N) { nx_id = cand_id[(size_t)(row0 + k + 1) * topk + e]; nx_lp = cand_lp[(size_t)(row0 + k + 1) * topk + e]; }
    }
    __syncthreads();
    // 1. every entry's state and key
    const int n_ent = n_live * topk;
    const int p = e / topk, j = e - p * topk;
    bool active = e < n_ent;
    float am = 0.0f, bonus = 0.0f, nlm = 0.0f, sc = -INFINITY;
    int node = 0, nstate = 0;
    if (active) {
      const float lp = c_lp[j];
      active = lp > -INFINITY;                           // (a NaN makes no entry either)
      if (active) {
        const int c = c_id[j];
        am = cur.am[p] + lp;
        node = cur.node[p]; bonus = cur.bonus[p];
        trie_step(tr, node, bonus, c);
        sc = am + bonus;
        if constexpr (kLm) {
          nstate = cur.lmstate[p];
          const float lmp = lm_step(lmod, nstate, c);
          nlm = cur.lm[p] + __fadd_rn(__fmul_rn(lmod.alpha, lmp), lmod.beta);
          sc += nlm;
        }
        active = sc > -INFINITY;
        if (!active) sc = -INFINITY;
      }
    }
    e_score[e] = sc;
    const int n_valid = __syncthreads_count(active ? 1 : 0);
    // 2. rank by (key descending, entry ascending); the best `beam` are the next row's live hypotheses
    if (active) {
      int rank = 0;
      for (int q = 0; q < n_ent; ++q) {
        const float o = e_score[q];
        rank += (o > sc || (o == sc && q < e)) ? 1 : 0;
      }
      if (rank < beam) {
        pool[k * beam + rank] = make_int2(p, j);
        nxt.am[rank] = am; nxt.bonus[rank] = bonus; nxt.node[rank] = node;
        if constexpr (kLm) { nxt.lm[rank] = nlm; nxt.lmstate[rank] = nstate; }
      }
    }
    __syncthreads();
    n_live = min(beam, n_valid);
  }
  // ---- the end of the utterance: an open partial phrase gives its bonus back; (kLm) the </s> term; rank again (stable over the rank order)
  const NarLive<kLm>& fin = live[N & 1];
  if (e < n_live) {
    float bonus = fin.bonus[e];
    if (tr.n_nodes > 1 && fin.node[e] != 0) bonus -= (float)tr.depth[fin.node[e]] * tr.boost;
    float sc = fin.am[e] + bonus;
    if constexpr (kLm) {
      float lm = fin.lm[e];
      if (lmod.eos >= 0) { int st = fin.lmstate[e]; lm += __fmul_rn(lmod.alpha, lm_step(lmod, st, lmod.eos)); }
      sc += lm;
    }
    f_am[e] = fin.am[e]; f_score[e] = sc;
  }
  __syncthreads();
  if (e < n_live) {
    const float sc = f_score[e];
    int rank = 0;
    for (int q = 0; q < n_live; ++q) rank += (f_score[q] > sc || (f_score[q] == sc && q < e)) ? 1 : 0;
    f_order[rank] = e;
  }
  __syncthreads();
  if (e < nbest) {
    const size_t o = (size_t)u * nbest + e;
    if (e < n_live) {
      int r = f_order[e];
      num_out[o] = N; score_out[o] = f_score[r]; am_out[o] = f_am[r];
      for (int k = N - 1; k >= 0; --k) {
        const int2 nd = pool[k * beam + r];
        if (k < max_tokens) {
          const size_t at = (size_t)(row0 + k) * topk + nd.y;
          tok_out[o * max_tokens + k] = cand_id[at];
          if (tlp_out) tlp_out[o * max_tokens + k] = cand_lp[at];
        }
        r = nd.x;
      }
    } else { num_out[o] = 0; score_out[o] = -INFINITY; am_out[o] = -INFINITY; }
  }
}

}  // namespace

void launch_nar_beam(const int32_t* cand_id, const float* cand_lp, int topk, const UttPlan* token_plan, const int32_t* m_dev, int n_utts, int beam, int nbest,
                     const HotTrie& trie, int2* pool, int pool_stride, int32_t* token_ids, int max_tokens, int32_t* num_id, float* score, float* am_score,
                     float* token_logprob, hipStream_t s, const NgramLm* lm) {
  ASR_REQUIRE(beam >= 1 && beam <= NAR_BEAM_MAX && topk >= 1 && topk <= NAR_BEAM_MAX && nbest >= 1 && nbest <= beam, "nar_beam: beam %d, topk %d, nbest %d (1..16, nbest <= beam)",
              beam, topk, nbest);
  ASR_REQUIRE(n_utts > 0 && max_tokens >= 1 && pool && pool_stride >= beam, "nar_beam: bad argument");
  if (lm && lm->n_nodes > 0)
    hipLaunchKernelGGL(nar_beam_kernel<true>, dim3(n_utts), dim3(NAR_BEAM_THREADS), 0, s, cand_id, cand_lp, topk, token_plan, m_dev, beam, nbest, trie, *lm, pool,
                       pool_stride, token_ids, max_tokens, num_id, score, am_score, token_logprob);
  else
    hipLaunchKernelGGL(nar_beam_kernel<false>, dim3(n_utts), dim3(NAR_BEAM_THREADS), 0, s, cand_id, cand_lp, topk, token_plan, m_dev, beam, nbest, trie, NarNoLm{}, pool,
                       pool_stride, token_ids, max_tokens, num_id, score, am_score, token_logprob);
  HIP_CHECK(hipGetLastError());
}
