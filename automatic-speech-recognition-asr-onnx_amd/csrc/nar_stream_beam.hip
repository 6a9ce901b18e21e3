// The beam search of nar_beam.hip for a stream that arrives in chunks: the search state is carried in HBM per stream and per hypothesis, and
// tokens are committed with a fixed lag. The rule of one token row and the end of a stream are nar_beam_kernel's very code (nar_row_step, nar_end_rank:
// beam_dev.h), so a stream of at most pend_cap rows followed by a finish has the offline search's bits however it was cut into chunks. What is this file's
// own: loading and clamping the state, the fixed-lag commit, writing the state and the pending tails back, the finish bookkeeping. The build's own mode: the
// reference graph returns the per-row arg-max. The float64 statement is tests/nar_stream_beam_ref.py. The state of one stream, 4 + 5 * 16 + 3 * pend_cap * beam
// int32 words, is laid out in nar_stream_state.h.
#include "beam_dev.h"
#include "engine.h"
#include "nar_stream_state.h"

namespace {

namespace S = nar_stream_state;
constexpr int NAR_RING_MAX = NAR_STREAM_PEND_MAX * TOKEN_BEAM_MAX;   // 12 KB of LDS for the three planes

// One workgroup per stream of the call; the stream id is plan[u].lang, its rows are plan[u].row_off .. + n_lfr of the candidate arrays (cut at *m_dev when
// given; 0 rows are legal). Before the row at position L is extended, L - C == cap commits position C: every live hypothesis walks back to its ancestor entry
// there, the entry of hypothesis 0 is committed, hypotheses with another ancestor are dropped and the survivors close ranks in order. The ring row at L - 1
// stays indexed by the ranks before the drop, so the survivors' old ranks are what the next row stores as parents. A stream whose flag in final_flags is set
// ends after its rows: nar_end_rank, the tail of the best hypothesis committed, the state cleared.
template <bool kLm>
__global__ __launch_bounds__(NAR_BEAM_THREADS) void nar_stream_beam_kernel(const int32_t* __restrict__ cand_id, const float* __restrict__ cand_lp, int topk,
                                                                           const UttPlan* __restrict__ plan, const int32_t* __restrict__ m_dev,
                                                                           const int32_t* __restrict__ final_flags, int beam, int nbest, int cap, HotTrie tr,
                                                                           LmArg<kLm> lmod, int32_t* __restrict__ state_all, int state_stride, NarStreamOut out) {
  __shared__ NarLive<kLm> live[2];
  __shared__ float e_score[NAR_BEAM_THREADS];
  __shared__ int r_par[NAR_RING_MAX], r_tok[NAR_RING_MAX];
  __shared__ float r_lp[NAR_RING_MAX];
  __shared__ int c_id[TOKEN_BEAM_MAX], f_order[TOKEN_BEAM_MAX], anc[TOKEN_BEAM_MAX], old_rank[TOKEN_BEAM_MAX];
  __shared__ float c_lp[TOKEN_BEAM_MAX], f_score[TOKEN_BEAM_MAX], f_am[TOKEN_BEAM_MAX];
  const int u = blockIdx.x, e = threadIdx.x;
  const int row0 = plan[u].row_off;
  int N = plan[u].n_lfr;
  if (m_dev) N = min(N, max(*m_dev - row0, 0));
  N = max(N, 0);
  const int ring_n = S::ring_plane_words(beam, cap);
  int32_t* st = state_all + (size_t)plan[u].lang * state_stride;
  int32_t* st_ring = st + S::RING;                       // the three ring planes are walked from their first word, one stride apart
  // ---- the carried state
  int L = st[S::L], C = st[S::C], n_live = st[S::N_LIVE];
  if (L <= 0) {                                          // cleared: the one empty hypothesis, as nar_beam_kernel starts
    L = 0; C = 0; n_live = 1;
    nar_live_start<kLm>(live[0], lmod);
    for (int i = e; i < ring_n; i += NAR_BEAM_THREADS) { r_par[i] = 0; r_tok[i] = 0; r_lp[i] = 0.0f; }
  } else {
    n_live = max(min(n_live, beam), 0);
    C = max(min(C, L), max(L - cap, 0));
    if (e < n_live) {
      live[0].am[e] = __int_as_float(st[S::AM + e]); live[0].bonus[e] = __int_as_float(st[S::BONUS + e]);
      live[0].node[e] = min(max(st[S::NODE + e], 0), max(tr.n_nodes - 1, 0));          // (indices are clamped: the state is memory the walks index with)
      if constexpr (kLm) { live[0].lm[e] = __int_as_float(st[S::LM + e]); live[0].lmstate[e] = min(max(st[S::LMSTATE + e], 0), lmod.n_nodes - 1); }
    }
    for (int i = e; i < ring_n; i += NAR_BEAM_THREADS) {
      r_par[i] = min(max(st_ring[i], 0), beam - 1); r_tok[i] = st_ring[S::RING_TOKEN * ring_n + i]; r_lp[i] = __int_as_float(st_ring[S::RING_LOGPROB * ring_n + i]);
    }
  }
  if (e < TOKEN_BEAM_MAX) old_rank[e] = e;
  const size_t c_at = (size_t)u * out.commit_cap;
  int n_commit = 0, b = 0;
  int nx_id = 0; float nx_lp = 0.0f;
  cand_fetch(cand_id, cand_lp, topk, row0, N > 0, nx_id, nx_lp);
  for (int k = 0; k < N; ++k) {
    NarLive<kLm>& cur = live[b];
    cand_advance(cand_id, cand_lp, topk, row0 + k + 1, k + 1 < N, nx_id, nx_lp, c_id, c_lp);
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
    // the row at position L: the survivors' parents are their ranks before the commit's drop, the ring's row at L takes parent, token and log-probability
    n_live = nar_row_step<kLm>(tr, lmod, cur, live[b ^ 1], c_id, c_lp, e_score, n_live, topk, beam, [&](int p) { return old_rank[p]; },
                               [&](int rank, int, int parent, int, int c, float lp) {
                                 const int at = (L % cap) * beam + rank;
                                 r_par[at] = parent; r_tok[at] = c; r_lp[at] = lp;
                               });
    if (e < TOKEN_BEAM_MAX) old_rank[e] = e;               // (read in front of nar_row_step's barrier)
    __syncthreads();
    ++L; b ^= 1;
  }
  const NarLive<kLm>& fin = live[b];
  const bool last = final_flags && final_flags[u] != 0;
  if (e == 0) out.total[u] = L;
  if (!last) {
    // ---- the state goes back, the pending tails of the best nbest go out: live order is key order, no end terms
    __syncthreads();
    if (e == 0) { st[S::L] = L; st[S::C] = C; st[S::N_LIVE] = n_live; st[S::UNUSED] = 0; out.commit_num[u] = n_commit; }
    if (e < n_live) {
      st[S::AM + e] = __float_as_int(fin.am[e]); st[S::BONUS + e] = __float_as_int(fin.bonus[e]); st[S::NODE + e] = fin.node[e];
      if constexpr (kLm) { st[S::LM + e] = __float_as_int(fin.lm[e]); st[S::LMSTATE + e] = fin.lmstate[e]; }
    }
    for (int i = e; i < ring_n; i += NAR_BEAM_THREADS) {
      st_ring[i] = r_par[i]; st_ring[S::RING_TOKEN * ring_n + i] = r_tok[i]; st_ring[S::RING_LOGPROB * ring_n + i] = __float_as_int(r_lp[i]);
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
  // ---- finish: the end terms and the second ranking, as nar_beam_kernel ends
  nar_end_rank<kLm>(tr, lmod, fin, n_live, f_score, f_am, f_order);
  if (e == 0) {                                          // the search is cleared; the tail of the best hypothesis is committed below
    st[S::L] = 0; st[S::C] = 0; st[S::N_LIVE] = 1; st[S::UNUSED] = 0;
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

int nar_stream_beam_state_words(int beam, int pend_cap) { return nar_stream_state::words(beam, pend_cap); }

void launch_nar_stream_beam(const int32_t* cand_id, const float* cand_lp, int topk, const UttPlan* token_plan, const int32_t* m_dev, const int32_t* final_flags,
                            int n_streams, int beam, int nbest, int pend_cap, const HotTrie& trie, int32_t* state, int state_stride, const NarStreamOut& out,
                            hipStream_t s, const NgramLm* lm) {
  ASR_REQUIRE(beam >= 1 && beam <= TOKEN_BEAM_MAX && topk >= 1 && topk <= TOKEN_BEAM_MAX && nbest >= 1 && nbest <= beam && pend_cap >= 1 && pend_cap <= NAR_STREAM_PEND_MAX,
              "nar_stream_beam: beam %d, topk %d, nbest %d (1..16, nbest <= beam), pend_cap %d (1..%d)", beam, topk, nbest, pend_cap, NAR_STREAM_PEND_MAX);
  ASR_REQUIRE(n_streams > 0 && state && state_stride >= nar_stream_beam_state_words(beam, pend_cap) && out.commit_cap >= 1 && out.commit_ids && out.commit_lp &&
                  out.commit_num && out.pend_ids && out.pend_lp && out.pend_num && out.pend_score && out.pend_am && out.total,
              "nar_stream_beam: bad argument");
  launch_with_lm(lm, [&](auto k_lm, const auto& lmod) {
    hipLaunchKernelGGL(nar_stream_beam_kernel<decltype(k_lm)::value>, dim3(n_streams), dim3(NAR_BEAM_THREADS), 0, s, cand_id, cand_lp, topk, token_plan, m_dev, final_flags,
                       beam, nbest, pend_cap, trie, lmod, state, state_stride, out);
  });
  HIP_CHECK(hipGetLastError());
}
