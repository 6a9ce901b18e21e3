// CTC prefix beam search over the top-k tokens of every frame, with a hotword context graph. Two kernels behind the timed CTC head
// (GemmArgs::amax_sum): ctc_topk_kernel picks each row's candidates from the head's per-slab partials without the logits ever being stored,
// ctc_prefix_beam_kernel runs the search, one workgroup per utterance. The float64 statement of the search is tests/ctc_beam_ref.py; with a back-off n-gram
// language model fused in (the kLm instantiation) it is tests/ctc_lm_ref.py.
#include <map>

#include "beam_dev.h"
#include "ctc_dev.h"
#include "engine.h"

namespace {

// ---- candidates ----------------------------------------------------------------------------------------------------------------------------------
// A token of value v lies in a slab whose maximum is >= v, and fewer than k slabs can have a maximum above the k-th best token: the row's top k
// tokens all lie in the k slabs with the largest maxima (ties to the lower slab). One wave per row: rank the slab maxima, recompute the 64 biased
// logits of each chosen slab (lane = column, f32 accumulation in ascending k), take the top k of those 64 k values (higher value, then lower id).
constexpr int TOPK_ROWS = 4;          // rows (waves) per workgroup

__device__ __forceinline__ void wave_best(float& v, int& i) {        // (higher value, lower index) over the wave; i < 0: no entry
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) { v = ov; i = oi; }
  }
}

// kDev (the token rows of the Paraformer decoder, nar_beam.hip): the row count is known on the device only. Rows at or past *m_dev were never computed and
// their partials hold nothing defined: a wave there repeats the last computed row, like a wave past M, and stores nothing. The kDev = false instantiation is
// the kernel as it was; its (empty) last argument is never read.
struct TopkHostRows {};
struct TopkDevRows { const int32_t* m_dev; };
template <typename T, bool kDev>
__global__ __launch_bounds__(64 * TOPK_ROWS) void ctc_topk_kernel(const T* __restrict__ h, int ldh, const T* __restrict__ W, int ldw, const float* __restrict__ bias,
                                                                  int K, const float* __restrict__ amax_val, const float* __restrict__ amax_sum, int n_slabs, int M_host,
                                                                  int n_valid, int topk, int32_t* __restrict__ cand_id, float* __restrict__ cand_lp,
                                                                  typename std::conditional<kDev, TopkDevRows, TopkHostRows>::type dev_rows) {
  extern __shared__ float topk_lds[];                 // [TOPK_ROWS][K] activation rows, then [TOPK_ROWS][16][64] slab logits
  __shared__ int sel[TOPK_ROWS][16];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int m_raw = blockIdx.x * TOPK_ROWS + wv;
  int M = M_host;
  if constexpr (kDev) M = max(min(M_host, *dev_rows.m_dev), 1);      // (the compact token plan has at least 16 rows)
  const int m = min(m_raw, M - 1);                    // (a wave past the last row repeats it and stores nothing: every wave reaches the barriers)
  float* hs = topk_lds + (size_t)wv * K;
  float* vals = topk_lds + (size_t)TOPK_ROWS * K + (size_t)wv * 16 * 64;
  for (int k = lane; k < K; k += 64) hs[k] = elem_f32(h[(size_t)m * ldh + k]);
  const float* rv = amax_val + (size_t)m * n_slabs;
  const float* rs = amax_sum + (size_t)m * n_slabs;
  // the k slabs with the largest maxima, in (maximum descending, slab ascending) order: each pass takes the best slab strictly behind the previous pick
  float pv = INFINITY; int ps = -1;
  float best_row = -INFINITY;
  for (int j = 0; j < topk; ++j) {
    float bv = -INFINITY; int bs = -1;
    for (int s = lane; s < n_slabs; s += 64) {
      const float v = rv[s];
      const bool behind = v < pv || (v == pv && s > ps);
      if (behind && (bs < 0 || v > bv)) { bv = v; bs = s; }       // ascending s inside the lane: the first maximum is the lowest slab
    }
    wave_best(bv, bs);
    if (lane == 0) sel[wv][j] = bs;
    if (j == 0) best_row = bv;
    pv = bv; ps = bs;
    if (bs < 0) { for (int q = j + 1; q < topk; ++q) if (lane == 0) sel[wv][q] = -1; break; }
  }
  const float lse = ctc_row_lse(rv, rs, n_slabs, best_row, lane);      // the row's log-sum-exp, as argmax_lse_reduce_kernel forms it
  __syncthreads();
  for (int j = 0; j < topk; ++j) {
    const int s = sel[wv][j];
    const int col = s * 64 + lane;
    float v = -INFINITY;
    if (s >= 0 && col < n_valid) {
      v = ctc_logit(hs, W + (size_t)col * ldw, K, bias[col]);
    }
    vals[j * 64 + lane] = v;
  }
  __syncthreads();
  pv = INFINITY;
  int pid = -1;
  for (int i = 0; i < topk; ++i) {
    float bv = -INFINITY; int bid = -1;
    for (int j = 0; j < topk; ++j) {
      const int s = sel[wv][j];
      const int id = s * 64 + lane;
      if (s < 0 || id >= n_valid) continue;
      const float v = vals[j * 64 + lane];
      const bool behind = v < pv || (v == pv && id > pid);
      if (behind && (bid < 0 || v > bv || (v == bv && id < bid))) { bv = v; bid = id; }
    }
    wave_best(bv, bid);
    if (lane == 0 && m_raw < M) {
      cand_id[(size_t)m * topk + i] = bid;
      cand_lp[(size_t)m * topk + i] = bid >= 0 ? bv - lse : -INFINITY;
    }
    pv = bv; pid = bid;
  }
}

// ---- search --------------------------------------------------------------------------------------------------------------------------------------
constexpr int CTC_BEAM_THREADS = TOKEN_BEAM_MAX + TOKEN_BEAM_MAX * TOKEN_BEAM_MAX + 48;     // one thread per entry of a frame (16 stays + 256 extensions), rounded up to whole waves

// identity of a prefix is its content: a 64-bit rolling hash (splitmix64 finaliser over hash * golden + token + 1) beside its length and last token
__device__ __forceinline__ uint64_t hash_step(uint64_t h, int c) {
  uint64_t z = h * 0x9E3779B97F4A7C15ull + (uint64_t)(uint32_t)c + 1ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

template <bool kLm>
struct BeamLive : LmLive<kLm> {       // the live prefixes of one frame, in rank order
  float pb[TOKEN_BEAM_MAX], pnb[TOKEN_BEAM_MAX], bonus[TOKEN_BEAM_MAX];
  uint64_t hash[TOKEN_BEAM_MAX];
  int len[TOKEN_BEAM_MAX], last[TOKEN_BEAM_MAX], pool[TOKEN_BEAM_MAX], node[TOKEN_BEAM_MAX];
};

// One workgroup per utterance, sequential over its rows plan[u].row_off .. + T. Entry e of a frame: e < 16 the "stay" of live prefix e (blank, and a repeat of
// its last token), e = 16 + p * topk + j the extension of live prefix p by candidate column j. An extension that spells a live prefix (same hash, length and
// last token) is folded into that prefix's stay -- at most one extension can reach a given stay (its parent is the prefix minus its last token), so a stay's
// pnb' has at most two terms and logaddexp of two terms does not depend on their order. The best `beam` entries by logaddexp(pb', pnb') + bonus survive,
// ties to the lower entry index; their rank is their index in the next frame. Kept extensions append a (parent, token) node to the utterance's pool at
// [t * beam + rank], which the final backtrace walks. Candidates of a row must have distinct ids; a candidate with lp = -inf is ignored.
// kLm: every prefix also carries lm, the sum of alpha * log P(token | state) + beta over its tokens, and the model's state. Both are functions of the prefix's
// content, as the bonus is, so merging by content is unchanged: a stay keeps them, an extension walks the image (lm_step) beside the trie, one dependent chain
// per frame on all extension threads at once. The ranking score gains + lm; at the end a prefix adds alpha * log P(</s> | state) when the model lists </s>.
// This search fuses its LM terms, fmaf(alpha, logp, beta) and fmaf(alpha, logp(</s>), lm): the NAR searches (beam_dev.h: lm_extend) round the product first.
// Candidate ids must lie in [0, vocab) of the image. The kLm = false instantiation is the search without a model: the instructions it had, the
// arguments behind the (empty) model argument 8 bytes further on.
template <bool kLm>
__global__ __launch_bounds__(CTC_BEAM_THREADS) void ctc_prefix_beam_kernel(const int32_t* __restrict__ cand_id, const float* __restrict__ cand_lp, int topk,
                                                                       const UttPlan* __restrict__ plan, int blank, int beam, int nbest, HotTrie tr,
                                                                       LmArg<kLm> lmod, int2* __restrict__ pool_all, int pool_stride,
                                                                       int32_t* __restrict__ tok_out, int max_tokens,
                                                                       int32_t* __restrict__ num_out, float* __restrict__ score_out, float* __restrict__ ctc_out) {
  __shared__ BeamLive<kLm> live[2];
  __shared__ float s_pb[TOKEN_BEAM_MAX], s_pnb[TOKEN_BEAM_MAX], e_score[TOKEN_BEAM_MAX + TOKEN_BEAM_MAX * TOKEN_BEAM_MAX];
  __shared__ int c_id[TOKEN_BEAM_MAX], n_valid_entries, f_order[TOKEN_BEAM_MAX];
  __shared__ float c_lp[TOKEN_BEAM_MAX], f_score[TOKEN_BEAM_MAX], f_ctc[TOKEN_BEAM_MAX];
  const int u = blockIdx.x, e = threadIdx.x;
  const int T = plan[u].T, row0 = plan[u].row_off;
  int2* pool = pool_all + (size_t)u * pool_stride;
  constexpr int N_ENT = TOKEN_BEAM_MAX + TOKEN_BEAM_MAX * TOKEN_BEAM_MAX;
  if (e == 0) {
    live[0].pb[0] = 0.0f; live[0].pnb[0] = -INFINITY; live[0].bonus[0] = 0.0f; live[0].hash[0] = 0; live[0].len[0] = 0; live[0].last[0] = -1;
    live[0].pool[0] = -1; live[0].node[0] = 0;
    if constexpr (kLm) { live[0].lm[0] = 0.0f; live[0].lmstate[0] = lmod.start_node; }
  }
  int n_live = 1;
  int nx_id = 0; float nx_lp = 0.0f;
  cand_fetch(cand_id, cand_lp, topk, row0, T > 0, nx_id, nx_lp);
  for (int t = 0; t < T; ++t) {
    const BeamLive<kLm>& cur = live[t & 1];
    BeamLive<kLm>& nxt = live[(t + 1) & 1];
    cand_advance(cand_id, cand_lp, topk, row0 + t + 1, t + 1 < T, nx_id, nx_lp, c_id, c_lp);
    if (e == 0) n_valid_entries = 0;
    __syncthreads();
    // 1. every entry's own contribution
    const bool is_stay = e < TOKEN_BEAM_MAX;
    const int x = e - TOKEN_BEAM_MAX;
    const int p = is_stay ? e : x / topk, j = is_stay ? 0 : x % topk;
    bool active = e < N_ENT && p < n_live;
    float val = -INFINITY, nb_bonus = 0.0f;
    uint64_t nh = 0;
    int c = -1, merge_to = -1, nnode = 0;
    float nlm = 0.0f;                                  // (kLm) the language-model total and state of this thread's extension
    int nstate = 0;
    if (active && is_stay) {
      const float pb = cur.pb[p], pnb = cur.pnb[p], tot = lae(pb, pnb);
      const int last = cur.last[p];
      float npb = -INFINITY, npnb = -INFINITY;
      for (int q = 0; q < topk; ++q) {
        const float lp = c_lp[q];
        if (lp == -INFINITY) continue;
        if (c_id[q] == blank) npb = lae(npb, tot + lp);
        else if (c_id[q] == last) npnb = lae(npnb, pnb + lp);
      }
      s_pb[p] = npb; s_pnb[p] = npnb;
    } else if (active) {
      c = c_id[j];
      const float lp = c_lp[j];
      const float pb = cur.pb[p], pnb = cur.pnb[p];
      if (lp == -INFINITY || c == blank) active = false;
      else if (c == cur.last[p]) { if (pb == -INFINITY) active = false; else val = pb + lp; }
      else val = lae(pb, pnb) + lp;
      if (active) {
        nh = hash_step(cur.hash[p], c);
        const int nl = cur.len[p] + 1;
        for (int q = 0; q < n_live; ++q)
          if (cur.hash[q] == nh && cur.len[q] == nl && cur.last[q] == c) merge_to = q;
      }
    }
    __syncthreads();
    // 2. an extension that spells a live prefix joins that prefix's stay
    if (active && !is_stay && merge_to >= 0) { s_pnb[merge_to] = lae(s_pnb[merge_to], val); active = false; }
    __syncthreads();
    // 3. scores
    float sc = -INFINITY;
    if (active && is_stay) {
      sc = lae(s_pb[p], s_pnb[p]) + cur.bonus[p];
      if constexpr (kLm) sc += cur.lm[p];
    } else if (active) {
      nnode = cur.node[p]; nb_bonus = cur.bonus[p];
      trie_step(tr, nnode, nb_bonus, c);
      sc = val + nb_bonus;
      if constexpr (kLm) {
        nstate = cur.lmstate[p];
        const float lp = lm_step(lmod, nstate, c);
        nlm = cur.lm[p] + fmaf(lmod.alpha, lp, lmod.beta);
        sc += nlm;
      }
    }
    if (sc == -INFINITY) active = false;
    if (e < N_ENT) e_score[e] = sc;
    if (active) atomicAdd(&n_valid_entries, 1);
    __syncthreads();
    // 4. rank by (score descending, entry ascending); the best `beam` are the next frame's live prefixes
    if (active) {
      // beam_rank's rule, written in place: through the helper this one loop leaves the compiler short of scalar registers for the constants of lae in
      // the steps above, which it then reloads per use (measured 2 % on the kernel with a model)
      const int n_ent = TOKEN_BEAM_MAX + n_live * topk;
      int rank = 0;
      for (int q = 0; q < n_ent; ++q) {
        const float o = e_score[q];
        rank += (o > sc || (o == sc && q < e)) ? 1 : 0;
      }
      if (rank < beam) {
        if (is_stay) {
          nxt.pb[rank] = s_pb[p]; nxt.pnb[rank] = s_pnb[p]; nxt.bonus[rank] = cur.bonus[p]; nxt.hash[rank] = cur.hash[p]; nxt.len[rank] = cur.len[p];
          nxt.last[rank] = cur.last[p]; nxt.pool[rank] = cur.pool[p]; nxt.node[rank] = cur.node[p];
          if constexpr (kLm) { nxt.lm[rank] = cur.lm[p]; nxt.lmstate[rank] = cur.lmstate[p]; }
        } else {
          const int idx = t * beam + rank;
          pool[idx] = make_int2(cur.pool[p], c);
          nxt.pb[rank] = -INFINITY; nxt.pnb[rank] = val; nxt.bonus[rank] = nb_bonus; nxt.hash[rank] = nh; nxt.len[rank] = cur.len[p] + 1;
          nxt.last[rank] = c; nxt.pool[rank] = idx; nxt.node[rank] = nnode;
          if constexpr (kLm) { nxt.lm[rank] = nlm; nxt.lmstate[rank] = nstate; }
        }
      }
    }
    __syncthreads();
    n_live = min(beam, n_valid_entries);
    __syncthreads();                                   // (n_valid_entries is cleared at the top of the next frame)
  }
  // ---- the end of the utterance: a prefix still inside a phrase gives its partial bonus back; sort by ctc + bonus (stable over the rank order);
  // (kLm) + lm, which gains alpha * log P(</s> | state) when the model lists </s>
  const BeamLive<kLm>& fin = live[T & 1];
  if (e < n_live) {
    const float bonus = beam_end_bonus(tr, fin.bonus[e], fin.node[e]);
    const float ctc = lae(fin.pb[e], fin.pnb[e]);
    float sc = ctc + bonus;
    if constexpr (kLm) {
      float lm = fin.lm[e];
      if (lmod.eos >= 0) { int st = fin.lmstate[e]; lm = fmaf(lmod.alpha, lm_step(lmod, st, lmod.eos), lm); }
      sc += lm;
    }
    f_ctc[e] = ctc; f_score[e] = sc;
  }
  __syncthreads();
  beam_final_order(f_score, n_live, f_order);
  __syncthreads();
  if (e < nbest) {
    const size_t o = (size_t)u * nbest + e;
    if (e < n_live) {
      const int i = f_order[e];
      const int len = fin.len[i];
      num_out[o] = len; score_out[o] = f_score[i]; ctc_out[o] = f_ctc[i];
      int node = fin.pool[i];
      for (int k = len - 1; k >= 0 && node >= 0; --k) {
        const int2 nd = pool[node];
        if (k < max_tokens) tok_out[o * max_tokens + k] = nd.y;
        node = nd.x;
      }
    } else { num_out[o] = 0; score_out[o] = -INFINITY; ctc_out[o] = -INFINITY; }
  }
}

}  // namespace

template <typename T>
void launch_ctc_topk(const T* h, int ldh, const T* W, int ldw, const float* bias, int K, const float* amax_val, const float* amax_sum, int n_slabs, int M,
                     int n_valid, int topk, int32_t* cand_id, float* cand_lp, hipStream_t s, const int32_t* m_dev) {
  ASR_REQUIRE(topk >= 1 && topk <= 16 && topk <= n_valid && n_valid <= n_slabs * 64, "ctc_topk: topk %d of %d valid columns (1..16)", topk, n_valid);
  ASR_REQUIRE(K % 8 == 0 && K <= 2048 && (ldw * sizeof(T)) % 16 == 0 && M > 0, "ctc_topk: K = %d, ldw = %d", K, ldw);
  const size_t lds = ((size_t)TOPK_ROWS * K + (size_t)TOPK_ROWS * 16 * 64) * 4;
  if (m_dev)
    hipLaunchKernelGGL((ctc_topk_kernel<T, true>), dim3((M + TOPK_ROWS - 1) / TOPK_ROWS), dim3(64 * TOPK_ROWS), lds, s, h, ldh, W, ldw, bias, K, amax_val, amax_sum, n_slabs,
                       M, n_valid, topk, cand_id, cand_lp, TopkDevRows{m_dev});
  else
    hipLaunchKernelGGL((ctc_topk_kernel<T, false>), dim3((M + TOPK_ROWS - 1) / TOPK_ROWS), dim3(64 * TOPK_ROWS), lds, s, h, ldh, W, ldw, bias, K, amax_val, amax_sum, n_slabs,
                       M, n_valid, topk, cand_id, cand_lp, TopkHostRows{});
  HIP_CHECK(hipGetLastError());
}
template void launch_ctc_topk<float>(const float*, int, const float*, int, const float*, int, const float*, const float*, int, int, int, int, int32_t*, float*, hipStream_t, const int32_t*);
template void launch_ctc_topk<bf16_t>(const bf16_t*, int, const bf16_t*, int, const float*, int, const float*, const float*, int, int, int, int, int32_t*, float*, hipStream_t, const int32_t*);

void launch_ctc_prefix_beam(const int32_t* cand_id, const float* cand_lp, int topk, const UttPlan* plan, int n_utts, int blank_id, int beam, int nbest,
                            const HotTrie& trie, int2* pool, int pool_stride, int32_t* token_ids, int max_tokens, int32_t* num_id, float* score, float* ctc_score,
                            hipStream_t s, const NgramLm* lm) {
  ASR_REQUIRE(beam >= 1 && beam <= TOKEN_BEAM_MAX && topk >= 1 && topk <= TOKEN_BEAM_MAX && nbest >= 1 && nbest <= beam, "ctc_prefix_beam: beam %d, topk %d, nbest %d (1..16, nbest <= beam)",
              beam, topk, nbest);
  ASR_REQUIRE(n_utts > 0 && max_tokens >= 1 && pool && pool_stride >= beam, "ctc_prefix_beam: bad argument");
  launch_with_lm(lm, [&](auto k_lm, const auto& lmod) {
    hipLaunchKernelGGL(ctc_prefix_beam_kernel<decltype(k_lm)::value>, dim3(n_utts), dim3(CTC_BEAM_THREADS), 0, s, cand_id, cand_lp, topk, plan, blank_id, beam, nbest, trie, lmod,
                       pool, pool_stride, token_ids, max_tokens, num_id, score, ctc_score);
  });
  HIP_CHECK(hipGetLastError());
}

// phrases (flattened ids + offsets) -> [depth n][is_end n][child_off n + 1][child_tok n - 1][child_node n - 1], nodes numbered breadth first, children by token
std::vector<int32_t> build_hot_trie(const int32_t* ids, const int32_t* offsets, int n_phrases, int* n_nodes_out) {
  std::vector<std::map<int32_t, int>> kids(1);
  std::vector<int32_t> depth(1, 0), is_end(1, 0);
  for (int p = 0; p < n_phrases; ++p) {
    int n = 0;
    for (int32_t i = offsets[p]; i < offsets[p + 1]; ++i) {
      auto it = kids[n].find(ids[i]);
      if (it == kids[n].end()) {
        it = kids[n].emplace(ids[i], (int)kids.size()).first;
        const int dn = depth[n] + 1;                      // (read before the vectors grow)
        kids.emplace_back(); depth.push_back(dn); is_end.push_back(0);
        n = (int)kids.size() - 1;
        continue;
      }
      n = it->second;
    }
    is_end[n] = 1;
  }
  const int n = (int)kids.size();
  std::vector<int> order(1, 0), remap(n, 0);
  for (size_t q = 0; q < order.size(); ++q)
    for (const auto& kv : kids[order[q]]) { remap[kv.second] = (int)order.size(); order.push_back(kv.second); }
  std::vector<int32_t> out((size_t)2 * n + (n + 1) + 2 * (size_t)(n - 1));
  int32_t *o_depth = out.data(), *o_end = o_depth + n, *o_off = o_end + n, *o_tok = o_off + n + 1, *o_node = o_tok + (n - 1);
  int e = 0;
  for (int q = 0; q < n; ++q) {
    o_depth[q] = depth[order[q]]; o_end[q] = is_end[order[q]]; o_off[q] = e;
    for (const auto& kv : kids[order[q]]) { o_tok[e] = kv.first; o_node[e] = remap[kv.second]; ++e; }
  }
  o_off[n] = e;
  *n_nodes_out = n;
  return out;
}

HotTrie hot_trie_view(const int32_t* dev_words, int n_nodes, float boost) {
  HotTrie t{};
  if (!dev_words || n_nodes <= 1) return t;
  t.depth = dev_words; t.is_end = t.depth + n_nodes; t.child_off = t.is_end + n_nodes; t.child_tok = t.child_off + n_nodes + 1; t.child_node = t.child_tok + (n_nodes - 1);
  t.n_nodes = n_nodes; t.boost = boost;
  return t;
}
