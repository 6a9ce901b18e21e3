// The beam search of nar_beam.hip for a stream that arrives in chunks: the search state is carried in HBM per stream and per hypothesis, and
// tokens are committed with a fixed lag. The rule of one token row -- entries, the trie and language-model walks, the key, the ranking -- is
// nar_beam_kernel's, in the same order of f32 operations, so a stream of at most pend_cap rows followed by a finish has the offline search's bits however it
// was cut into chunks. The build's own mode: the reference graph returns the per-row arg-max. The float64 statement is tests/nar_stream_beam_ref.py.
//
// State of one stream, int32 words (nar_stream_beam_state_words):
//   [0] L   rows searched since the stream's search was last cleared; L == 0 IS the cleared state (nothing else is read then: zeroed memory is a cleared stream)
//   [1] C   how many of them are committed (L - C <= pend_cap)
//   [2] the number of live hypotheses, [3] unused
//   am, bonus (f32), node, lm (f32), lmstate: [NAR_BEAM_MAX] each, the live hypotheses in rank order (lm / lmstate only with a model)
//   ring: parent rank, token id, token log-probability (f32): three planes [pend_cap][beam]; row (pos % pend_cap) holds position pos, entry r of the row at
//   L - 1 is live hypothesis r, and `parent` indexes the row below
#include <type_traits>

#include "engine.h"
#include "hot_trie.h"
#include "kernels.h"
#include "ngram_lm.h"

namespace {

constexpr int NAR_BEAM_MAX = 16;
constexpr int NAR_BEAM_THREADS = NAR_BEAM_MAX * NAR_BEAM_MAX;        // one thread per extension of a row
constexpr int NAR_RING_MAX = NAR_STREAM_PEND_MAX * NAR_BEAM_MAX;     // 12 KB of LDS for the three planes
constexpr int ST_HEADER = 4, ST_LIVE = 5 * NAR_BEAM_MAX;

template <bool kLm> struct StreamLmState {};
template <> struct StreamLmState<true> {
  float lm[NAR_BEAM_MAX];
  int lmstate[NAR_BEAM_MAX];
};
template <bool kLm>
struct StreamLive : StreamLmState<kLm> {             // the live hypotheses, in rank order
  float am[NAR_BEAM_MAX], bonus[NAR_BEAM_MAX];
  int node[NAR_BEAM_MAX];
};
struct StreamNoLm {};

// One workgroup per stream of the call; the stream id is plan[u].lang, its rows are plan[u].row_off .. + n_lfr of the candidate arrays (cut at *m_dev when
// given; 0 rows are legal). Before the row at position L is extended, L - C == cap commits position C: every live hypothesis walks back to its ancestor entry
// there, the entry of hypothesis 0 is committed, hypotheses with another ancestor are dropped and the survivors close ranks in order. The ring row at L - 1
// stays indexed by the ranks before the drop, so the survivors' old ranks are what the next row stores as parents. A stream whose flag in final_flags is set
// ends after its rows: the end terms and the second ranking of nar_beam_kernel, the tail of the best hypothesis committed, the state cleared.
template <bool kLm>
__global__ __launch_bounds__(NAR_BEAM_THREADS) void nar_stream_beam_kernel(const int32_t* __restrict__ cand_id, const float* __restrict__ cand_lp, int topk,
                                                                           const UttPlan* __restrict__ plan, const int32_t* __restrict__ m_dev,
                                                                           const int32_t* __restrict__ final_flags, int beam, int nbest, int cap, HotTrie tr,
                                                                           typename std::conditional<kLm, NgramLm, StreamNoLm>::type lmod,
                                                                           int32_t* __restrict__ state_all, int state_stride, NarStreamOut out) {
  __shared__ StreamLive<kLm> live[2];
  __shared__ float e_score[NAR_BEAM_THREADS];
  __shared__ int r_par[NAR_RING_MAX], r_tok[NAR_RING_MAX];
  __shared__ float r_lp[NAR_RING_MAX];
  __shared__ int c_id[NAR_BEAM_MAX], f_order[NAR_BEAM_MAX], anc[NAR_BEAM_MAX], old_rank[NAR_BEAM_MAX];
  __shared__ float c_lp[NAR_BEAM_MAX], f_score[NAR_BEAM_MAX], f_am[NAR_BEAM_MAX];
  const int u = blockIdx.x, e = threadIdx.x;
  const int row0 = plan[u].row_off;
  int N = plan[u].n_lfr;
  if (m_dev) N = min(N, max(*m_dev - row0, 0));
  N = max(N, 0);
  const int ring_n = cap * beam;
  int32_t* st = state_all + (size_t)plan[u].lang * state_stride;
  int32_t* st_live = st + ST_HEADER;
  int32_t* st_ring = st + ST_HEADER + ST_LIVE;
  // ---- the carried state
  int L = st[0], C = st[1], n_live = st[2];
  if (L <= 0) {                                          // cleared: the one empty hypothesis, as nar_beam_kernel starts
    L = 0; C = 0; n_live = 1;
    if (e == 0) {
      live[0].am[0] = 0.0f; live[0].bonus[0] = 0.0f; live[0].node[0] = 0;
      if constexpr (kLm) { live[0].lm[0] = 0.0f; live[0].lmstate[0] = lmod.start_node; }
    }
    for (int i = e; i < ring_n; i += NAR_BEAM_THREADS) { r_par[i] = 0; r_tok[i] = 0; r_lp[i] = 0.0f; }
  } else {
    n_live = max(min(n_live, beam), 0);
    C = max(min(C, L), max(L - cap, 0));
    if (e < n_live) {
      live[0].am[e] = __int_as_float(st_live[e]); live[0].bonus[e] = __int_as_float(st_live[NAR_BEAM_MAX + e]);
      live[0].node[e] = min(max(st_live[2 * NAR_BEAM_MAX + e], 0), max(tr.n_nodes - 1, 0));          // (indices are clamped: the state is memory the walks index with)
      if constexpr (kLm) { live[0].lm[e] = __int_as_float(st_live[3 * NAR_BEAM_MAX + e]); live[0].lmstate[e] = min(max(st_live[4 * NAR_BEAM_MAX + e], 0), lmod.n_nodes - 1); }
    }
    for (int i = e; i < ring_n; i += NAR_BEAM_THREADS) {
      r_par[i] = min(max(st_ring[i], 0), beam - 1); r_tok[i] = st_ring[ring_n + i]; r_lp[i] = __int_as_float(st_ring[2 * ring_n + i]);
    }
  }
  if (e < NAR_BEAM_MAX) old_rank[e] = e;
  const size_t c_at = (size_t)u * out.commit_cap;
  int n_commit = 0, b = 0;
  int nx_id = 0; float nx_lp = 0.0f;                    // the next row's candidate of this thread (threads < topk), fetched a row ahead
  if (e < topk && N > 0) { nx_id = cand_id[(size_t)row0 * topk + e]; nx_lp = cand_lp[(size_t)row0 * topk + e]; }
  for (int k = 0; k < N; ++k) {
    StreamLive<kLm>& cur = live[b];
    StreamLive<kLm>& nxt = live[b ^ 1];
    if (e < topk) {
      c_id[e] = nx_id; c_lp[e] = nx_lp;
      if (k + 1 < N) { nx_id = cand_id[(size_t)(row0 + k + 1) * topk + e]; nx_lp = cand_lp[(size_t)(row0 + k + 1) * topk + e]; }
    }
    __syncthreads();
    // 0. the fixed-lag commit of position C (uniform over the workgroup)
    if (L - C == cap && n_live > 0) {
      if (e < n_live) {
        int a = e;
        for (int pos = L - 1; pos > C; --pos) a = r_par[(pos % cap) * beam + a];
        anc[e] = a;
      }
      __syncthreads();
      const int a0 = anc[0];
      const bool keep = e < n_live && anc[e] == a0;
      int n_keep = 0, rank = 0;
      for (int q = 0; q < n_live; ++q) {
        const int same = anc[q] == a0 ? 1 : 0;
        n_keep += same; rank += (same && q < e) ? 1 : 0;
      }
      float am = 0.0f, bonus = 0.0f, lm = 0.0f;
      int node = 0, lmstate = 0;
      if (keep) {
        am = cur.am[e]; bonus = cur.bonus[e]; node = cur.node[e];
        if constexpr (kLm) { lm = cur.lm[e]; lmstate = cur.lmstate[e]; }
      }
      if (e == 0 && n_commit < out.commit_cap) {
        const int at = (C % cap) * beam + a0;
        out.commit_ids[c_at + n_commit] = r_tok[at]; out.commit_lp[c_at + n_commit] = r_lp[at];
      }
      __syncthreads();
      if (keep) {
        cur.am[rank] = am; cur.bonus[rank] = bonus; cur.node[rank] = node; old_rank[rank] = e;
        if constexpr (kLm) { cur.lm[rank] = lm; cur.lmstate[rank] = lmstate; }
      }
      __syncthreads();
      n_live = n_keep; ++C; ++n_commit;
    }
    // 1. every entry's state and key (nar_beam_kernel's)
    const int n_ent = n_live * topk;
    const int p = e / topk, j = e - p * topk;
    bool active = e < n_ent;
    float am = 0.0f, bonus = 0.0f, nlm = 0.0f, sc = -INFINITY, lp = 0.0f;
    int node = 0, nstate = 0, c = 0, parent = 0;
    if (active) {
      lp = c_lp[j];
      active = lp > -INFINITY;                           // (a NaN makes no entry either)
      if (active) {
        c = c_id[j];
        parent = old_rank[p];
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
    // 2. rank by (key descending, entry ascending); the best `beam` are the next row's live hypotheses and the ring's row at position L
    if (active) {
      int rank = 0;
      for (int q = 0; q < n_ent; ++q) {
        const float o = e_score[q];
        rank += (o > sc || (o == sc && q < e)) ? 1 : 0;
      }
      if (rank < beam) {
        const int at = (L % cap) * beam + rank;
        r_par[at] = parent; r_tok[at] = c; r_lp[at] = lp;
        nxt.am[rank] = am; nxt.bonus[rank] = bonus; nxt.node[rank] = node;
        if constexpr (kLm) { nxt.lm[rank] = nlm; nxt.lmstate[rank] = nstate; }
      }
    }
    if (e < NAR_BEAM_MAX) old_rank[e] = e;               // (read before the barrier above)
    __syncthreads();
    n_live = min(beam, n_valid);
    ++L; b ^= 1;
  }
  const StreamLive<kLm>& fin = live[b];
  const bool last = final_flags && final_flags[u] != 0;
  if (e == 0) out.total[u] = L;
  if (!last) {
    // ---- the state goes back, the pending tails of the best nbest go out: live order is key order, no end terms
    __syncthreads();
    if (e == 0) { st[0] = L; st[1] = C; st[2] = n_live; st[3] = 0; out.commit_num[u] = n_commit; }
    if (e < n_live) {
      st_live[e] = __float_as_int(fin.am[e]); st_live[NAR_BEAM_MAX + e] = __float_as_int(fin.bonus[e]); st_live[2 * NAR_BEAM_MAX + e] = fin.node[e];
      if constexpr (kLm) { st_live[3 * NAR_BEAM_MAX + e] = __float_as_int(fin.lm[e]); st_live[4 * NAR_BEAM_MAX + e] = fin.lmstate[e]; }
    }
    for (int i = e; i < ring_n; i += NAR_BEAM_THREADS) {
      st_ring[i] = r_par[i]; st_ring[ring_n + i] = r_tok[i]; st_ring[2 * ring_n + i] = __float_as_int(r_lp[i]);
    }
    if (e < nbest) {
      const size_t o = (size_t)u * nbest + e;
      if (e < n_live) {
        float sc = fin.am[e] + fin.bonus[e];
        if constexpr (kLm) sc += fin.lm[e];
        out.pend_num[o] = L - C; out.pend_score[o] = sc; out.pend_am[o] = fin.am[e];
        int r = e;
        for (int pos = L - 1; pos >= C; --pos) {
          const int at = (pos % cap) * beam + r;
          out.pend_ids[o * cap + (pos - C)] = r_tok[at]; out.pend_lp[o * cap + (pos - C)] = r_lp[at];
          r = r_par[at];
        }
      } else { out.pend_num[o] = 0; out.pend_score[o] = -INFINITY; out.pend_am[o] = -INFINITY; }
    }
    return;
  }
  // ---- finish: an open partial phrase gives its bonus back; (kLm) the </s> term; rank again (stable over the rank order), as nar_beam_kernel ends
  if (e < n_live) {
    float bonus = fin.bonus[e];
    if (tr.n_nodes > 1 && fin.node[e] != 0) bonus -= (float)tr.depth[fin.node[e]] * tr.boost;
    float sc = fin.am[e] + bonus;
    if constexpr (kLm) {
      float lm = fin.lm[e];
      if (lmod.eos >= 0) { int s = fin.lmstate[e]; lm += __fmul_rn(lmod.alpha, lm_step(lmod, s, lmod.eos)); }
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
  if (e == 0) {                                          // the search is cleared; the tail of the best hypothesis is committed below
    st[0] = 0; st[1] = 0; st[2] = 1; st[3] = 0;
    out.commit_num[u] = min(n_commit + (n_live > 0 ? L - C : 0), out.commit_cap);
  }
  if (e < nbest) {
    const size_t o = (size_t)u * nbest + e;
    if (e < n_live) {
      int r = f_order[e];
      out.pend_num[o] = L - C; out.pend_score[o] = f_score[r]; out.pend_am[o] = f_am[r];
      for (int pos = L - 1; pos >= C; --pos) {
        const int at = (pos % cap) * beam + r;
        out.pend_ids[o * cap + (pos - C)] = r_tok[at]; out.pend_lp[o * cap + (pos - C)] = r_lp[at];
        if (e == 0 && n_commit + (pos - C) < out.commit_cap) {
          out.commit_ids[c_at + n_commit + (pos - C)] = r_tok[at]; out.commit_lp[c_at + n_commit + (pos - C)] = r_lp[at];
        }
        r = r_par[at];
      }
    } else { out.pend_num[o] = 0; out.pend_score[o] = -INFINITY; out.pend_am[o] = -INFINITY; }
  }
}

}  // namespace

int nar_stream_beam_state_words(int beam, int pend_cap) { return ST_HEADER + ST_LIVE + 3 * pend_cap * beam; }

void launch_nar_stream_beam(const int32_t* cand_id, const float* cand_lp, int topk, const UttPlan* token_plan, const int32_t* m_dev, const int32_t* final_flags,
                            int n_streams, int beam, int nbest, int pend_cap, const HotTrie& trie, int32_t* state, int state_stride, const NarStreamOut& out,
                            hipStream_t s, const NgramLm* lm) {
  ASR_REQUIRE(beam >= 1 && beam <= NAR_BEAM_MAX && topk >= 1 && topk <= NAR_BEAM_MAX && nbest >= 1 && nbest <= beam && pend_cap >= 1 && pend_cap <= NAR_STREAM_PEND_MAX,
              "nar_stream_beam: beam %d, topk %d, nbest %d (1..16, nbest <= beam), pend_cap %d (1..%d)", beam, topk, nbest, pend_cap, NAR_STREAM_PEND_MAX);
  ASR_REQUIRE(n_streams > 0 && state && state_stride >= nar_stream_beam_state_words(beam, pend_cap) && out.commit_cap >= 1 && out.commit_ids && out.commit_lp &&
                  out.commit_num && out.pend_ids && out.pend_lp && out.pend_num && out.pend_score && out.pend_am && out.total,
              "nar_stream_beam: bad argument");
  if (lm && lm->n_nodes > 0)
    hipLaunchKernelGGL(nar_stream_beam_kernel<true>, dim3(n_streams), dim3(NAR_BEAM_THREADS), 0, s, cand_id, cand_lp, topk, token_plan, m_dev, final_flags, beam, nbest,
                       pend_cap, trie, *lm, state, state_stride, out);
  else
    hipLaunchKernelGGL(nar_stream_beam_kernel<false>, dim3(n_streams), dim3(NAR_BEAM_THREADS), 0, s, cand_id, cand_lp, topk, token_plan, m_dev, final_flags, beam, nbest,
                       pend_cap, trie, StreamNoLm{}, state, state_stride, out);
  HIP_CHECK(hipGetLastError());
}
