// Device pieces shared by the three token-synchronous beam searches, one workgroup per utterance: ctc_prefix_beam_kernel (ctc_beam.hip),
// nar_beam_kernel (nar_beam.hip, 4.4b) and nar_stream_beam_kernel (nar_stream_beam.hip, 4.5b). The rule of one token row of the two NAR searches and the end
// of their utterances live here once, so that a stream within pend_cap has the offline search's bits by construction. Every helper is inlined; one that holds
// a barrier says so and is called by every thread of the workgroup, outside any divergent branch.
#pragma once
#include <type_traits>

#include "hot_trie.h"
#include "kernels.h"
#include "nar_stream_state.h"
#include "ngram_lm.h"

constexpr int TOKEN_BEAM_MAX = 16;    // widest beam, and most candidates per row, of the three searches (BEAM_MAX, kernels.h, is the autoregressive rankers')
static_assert(nar_stream_state::PLANE == TOKEN_BEAM_MAX, "a stream's carried state holds the widest beam per live plane");

template <bool kLm> struct LmLive {};
template <> struct LmLive<true> {     // a live hypothesis' language-model total (alpha * logp + beta over its tokens) and state: functions of its content
  float lm[TOKEN_BEAM_MAX];
  int lmstate[TOKEN_BEAM_MAX];
};
struct NoLm {};
template <bool kLm> using LmArg = typename std::conditional<kLm, NgramLm, NoLm>::type;      // the kernels' model argument: empty without a model

// launch(std::bool_constant<kLm>, model argument): the instantiation with a model when lm has nodes, else the one without
template <typename Launch>
void launch_with_lm(const NgramLm* lm, Launch&& launch) {
  if (lm && lm->n_nodes > 0) launch(std::true_type{}, *lm);
  else launch(std::false_type{}, NoLm{});
}

// ---- candidates: thread e < topk holds column e of the next row in registers (nx_id, nx_lp), fetched one row ahead of its use
__device__ __forceinline__ void cand_fetch(const int32_t* __restrict__ cand_id, const float* __restrict__ cand_lp, int topk, int row, bool any, int& nx_id, float& nx_lp) {
  const int e = threadIdx.x;
  if (e < topk && any) { nx_id = cand_id[(size_t)row * topk + e]; nx_lp = cand_lp[(size_t)row * topk + e]; }
}
// the fetched row goes to c_id / c_lp (the caller's barrier follows), `next_row` is fetched when has_next
__device__ __forceinline__ void cand_advance(const int32_t* __restrict__ cand_id, const float* __restrict__ cand_lp, int topk, int next_row, bool has_next, int& nx_id,
                                             float& nx_lp, int* c_id, float* c_lp) {
  const int e = threadIdx.x;
  if (e < topk) {
    c_id[e] = nx_id; c_lp[e] = nx_lp;
    if (has_next) { nx_id = cand_id[(size_t)next_row * topk + e]; nx_lp = cand_lp[(size_t)next_row * topk + e]; }
  }
}

// rank of entry e with score sc among scores[0 .. n): how many entries have a higher score, or an equal one and a lower index
// (the CTC row ranking writes this loop in place; ctc_beam.hip says why)
__device__ __forceinline__ int beam_rank(const float* scores, int n, float sc, int e) {
  int rank = 0;
  for (int q = 0; q < n; ++q) {
    const float o = scores[q];
    rank += (o > sc || (o == sc && q < e)) ? 1 : 0;
  }
  return rank;
}

// the second ranking, by final score (stable over the live rank order): f_order[i] is the live rank of the i-th best. Barriers before and behind are the caller's.
__device__ __forceinline__ void beam_final_order(const float* f_score, int n_live, int* f_order) {
  const int e = threadIdx.x;
  if (e < n_live) f_order[beam_rank(f_score, n_live, f_score[e], e)] = e;
}

// the bonus at the end of an utterance: a hypothesis still inside a phrase gives its partial match back, product and difference in one rounding
__device__ __forceinline__ float beam_end_bonus(const HotTrie& tr, float bonus, int node) {
  if (tr.n_nodes > 1 && node != 0) bonus = fmaf(-(float)tr.depth[node], tr.boost, bonus);
  return bonus;
}

// lm_total + (alpha * log P(c | state) + beta), the product and both sums rounded on their own; state moves behind c (an out-of-vocabulary token costs oov and
// keeps it). The NAR searches' term; the CTC search fuses its own (ctc_beam.hip).
__device__ __forceinline__ float lm_extend(const NgramLm& lmod, float lm_total, int& state, int c) {
  const float lp = lm_step(lmod, state, c);
  return lm_total + __fadd_rn(__fmul_rn(lmod.alpha, lp), lmod.beta);
}

// ---- the NAR searches (no blank, no merging: every hypothesis picks one candidate per row)
template <bool kLm>
struct NarLive : LmLive<kLm> {        // the live hypotheses of one row, in rank order
  float am[TOKEN_BEAM_MAX], bonus[TOKEN_BEAM_MAX];
  int node[TOKEN_BEAM_MAX];
};
constexpr int NAR_BEAM_THREADS = TOKEN_BEAM_MAX * TOKEN_BEAM_MAX;      // one thread per extension of a row

template <bool kLm>
__device__ __forceinline__ void nar_live_start(NarLive<kLm>& live, const LmArg<kLm>& lmod) {       // the one empty hypothesis (thread 0)
  if (threadIdx.x == 0) {
    live.am[0] = 0.0f; live.bonus[0] = 0.0f; live.node[0] = 0;
    if constexpr (kLm) { live.lm[0] = 0.0f; live.lmstate[0] = lmod.start_node; }
  }
}

// One token row: entry e = p * topk + j extends live hypothesis p of cur (rank order) by candidate column j of c_id / c_lp; a candidate with lp = -inf (or NaN)
// makes no entry. Every entry carries, all in f32 and in this order of operations:
//   am' = am[p] + lp[j]                                      (the running acoustic sum, in row order)
//   (node', bonus') = trie_step(node[p], bonus[p], token)
//   lm' = lm_extend(lm[p], state[p], token)                  (kLm)
//   key = (am' + bonus') + lm'
// The best min(beam, entries) survive into nxt by key descending, ties to the lower e; their rank is their index at the next row. parent_of(p) is read
// beside hypothesis p's state, in front of the barrier (the stream's rank of p before a commit closed ranks; a search that stores p itself returns nothing
// worth a register), and keep(rank, p, parent, j, token, lp) stores a surviving entry in what the caller walks back through. Returns the number of live
// hypotheses of nxt. Holds one barrier (the entry count); the caller's barrier follows before nxt is read.
template <bool kLm, typename ParentOf, typename Keep>
__device__ __forceinline__ int nar_row_step(const HotTrie& tr, const LmArg<kLm>& lmod, const NarLive<kLm>& cur, NarLive<kLm>& nxt, const int* c_id, const float* c_lp,
                                            float* e_score, int n_live, int topk, int beam, ParentOf parent_of, Keep keep) {
  const int e = threadIdx.x;
  const int n_ent = n_live * topk;
  const int p = e / topk, j = e - p * topk;
  bool active = e < n_ent;
  float am = 0.0f, bonus = 0.0f, nlm = 0.0f, sc = -INFINITY, lp = 0.0f;
  int node = 0, nstate = 0, c = 0, parent = 0;
  if (active) {
    lp = c_lp[j];
    active = lp > -INFINITY;                             // (a NaN makes no entry either)
    if (active) {
      c = c_id[j];
      parent = parent_of(p);
      am = cur.am[p] + lp;
      node = cur.node[p]; bonus = cur.bonus[p];
      trie_step(tr, node, bonus, c);
      sc = am + bonus;
      if constexpr (kLm) {
        nstate = cur.lmstate[p];
        nlm = lm_extend(lmod, cur.lm[p], nstate, c);
        sc += nlm;
      }
      active = sc > -INFINITY;
      if (!active) sc = -INFINITY;
    }
  }
  e_score[e] = sc;
  const int n_valid = __syncthreads_count(active ? 1 : 0);
  if (active) {
    const int rank = beam_rank(e_score, n_ent, sc, e);
    if (rank < beam) {
      keep(rank, p, parent, j, c, lp);
      nxt.am[rank] = am; nxt.bonus[rank] = bonus; nxt.node[rank] = node;
      if constexpr (kLm) { nxt.lm[rank] = nlm; nxt.lmstate[rank] = nstate; }
    }
  }
  return min(beam, n_valid);
}

// The end of an utterance: an open partial phrase gives its bonus back, (kLm) alpha * log P(</s> | state) is added when the model lists </s>, and the n_live
// hypotheses of fin are ranked again by (am + bonus) + lm, ties to the lower rank: f_order[i] is the i-th best, f_score / f_am its figures by live rank.
// Holds two barriers; f_order is ready behind the second.
template <bool kLm>
__device__ __forceinline__ void nar_end_rank(const HotTrie& tr, const LmArg<kLm>& lmod, const NarLive<kLm>& fin, int n_live, float* f_score, float* f_am, int* f_order) {
  const int e = threadIdx.x;
  if (e < n_live) {
    float sc = fin.am[e] + beam_end_bonus(tr, fin.bonus[e], fin.node[e]);
    if constexpr (kLm) {
      float lm = fin.lm[e];
      if (lmod.eos >= 0) { int st = fin.lmstate[e]; lm += __fmul_rn(lmod.alpha, lm_step(lmod, st, lmod.eos)); }
      sc += lm;
    }
    f_am[e] = fin.am[e]; f_score[e] = sc;
  }
  __syncthreads();
  beam_final_order(f_score, n_live, f_order);
  __syncthreads();
}
