// n-gram LM shallow fusion of the autoregressive decoders (Whisper, Qwen3-ASR): the wide candidate list of a logits row, the greedy head's fused pick and
// the beam ranker's merge (kernels.h: launch_lm_*). The walk is ngram_lm.h's lm_step, shared with the CTC and Paraformer searches; the trie walk
// is hot_trie.h. The float64 statement is tests/decoder_lm_ref.py.
#include "engine.h"
#include "hot_trie.h"
#include "kernels.h"

namespace {

constexpr int LM_LIST = 8;            // per-thread list length of the one-pass top-M (beam_topk_kernel's)
constexpr int LM_PICK_ROWS = 4;       // rows (waves) per workgroup of the pick kernel
constexpr int LM_CACHE = 512;         // candidates of a re-rank row whose fused scores are kept in LDS between the rounds

// (higher value, lower id) over the workgroup's 16 waves: every thread returns the winner. sv / si: [2][16], `par` alternates so one barrier serves a round
// (a wave writes buffer par again only after the barrier of the round between, which every thread passes after its reads of this one).
__device__ __forceinline__ void block_better(float& bv, int& bi, float (*sv)[16], int (*si)[16], int par, int lane, int wave) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  if (lane == 0) { sv[par][wave] = bv; si[par][wave] = bi; }
  __syncthreads();
  bv = sv[par][0]; bi = si[par][0];
#pragma unroll
  for (int w = 1; w < 16; ++w) {
    const float ov = sv[par][w]; const int oi = si[par][w];
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
}

// Per row: the log-sum-exp and the M best (value, id) pairs, value descending then id ascending. One pass in beam_topk_kernel's geometry: every thread keeps
// a running (max, sum), its sorted best-8 list (columns arrive in ascending id order and only a strictly larger value displaces one, so equal values stay in
// id order) and `ev`, the largest value it saw and did not keep. The lists merge in M rounds of a block-wide arg-max. Everything a thread dropped is behind
// everything it kept, so the merge is the row's true order unless a thread ran out of list: that takes a dropped value at or above the M-th winner (or
// fewer than M winners with anything dropped at all). Such a row is redone by M passes that each take the best column strictly behind the last winner.
__global__ __launch_bounds__(1024) void lm_topk_kernel(const float* __restrict__ logits, int ld, int n_valid, const float* __restrict__ bias, int M,
                                                       float* __restrict__ cand_v, int32_t* __restrict__ cand_i, float* __restrict__ lse_out,
                                                       int32_t* __restrict__ slow_rows) {
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* p = logits + (size_t)row * ld;
  float* out_v = cand_v + (size_t)row * M;
  int32_t* out_i = cand_i + (size_t)row * M;
  float tv[LM_LIST]; int ti[LM_LIST];
#pragma unroll
  for (int j = 0; j < LM_LIST; ++j) { tv[j] = -INFINITY; ti[j] = INT32_MAX; }
  float m = -INFINITY, sum = 0.0f, ev = -INFINITY;
  for (int v0 = tid * 4; v0 < n_valid; v0 += 4096) {
    const float4 q = *reinterpret_cast<const float4*>(p + v0);
    const float xs[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float x = xs[e];
      if (v0 + e >= n_valid) continue;
      if (bias) x += bias[v0 + e];
      if (x == -INFINITY) continue;                        // zero weight, no candidate
      if (x > m) { sum = sum * __expf(m - x) + 1.0f; m = x; } else { sum += __expf(x - m); }
      if (x > tv[LM_LIST - 1]) {
        ev = fmaxf(ev, tv[LM_LIST - 1]);
        tv[LM_LIST - 1] = x; ti[LM_LIST - 1] = v0 + e;
#pragma unroll
        for (int j = LM_LIST - 1; j > 0; --j)
          if (tv[j] > tv[j - 1]) { const float a = tv[j]; tv[j] = tv[j - 1]; tv[j - 1] = a; const int c = ti[j]; ti[j] = ti[j - 1]; ti[j - 1] = c; }
      } else {
        ev = fmaxf(ev, x);
      }
    }
  }
  __shared__ float sm[16], ss[16], sv[2][16];
  __shared__ int si[2][16];
  auto merge = [](float& m1, float& s1, float m2, float s2) {
    const float Mx = fmaxf(m1, m2);
    const float a = m1 == -INFINITY ? 0.0f : s1 * __expf(m1 - Mx), b = m2 == -INFINITY ? 0.0f : s2 * __expf(m2 - Mx);
    m1 = Mx; s1 = a + b;
  };
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) merge(m, sum, __shfl_xor(m, o, 64), __shfl_xor(sum, o, 64));
  if (lane == 0) { sm[wave] = m; ss[wave] = sum; }
  __syncthreads();
  if (tid == 0) {
    float Mx = sm[0], S = ss[0];
    for (int w = 1; w < 16; ++w) merge(Mx, S, sm[w], ss[w]);
    lse_out[row] = Mx + logf(S);                           // (a row without a finite column: -inf + logf(0) = -inf, not NaN)
  }
  int par = 0;
  float last_v = -INFINITY;                                // the M-th winner's value; -inf when the lists held fewer than M
  for (int k = 0; k < M; ++k, par ^= 1) {
    float bv = tv[0]; int bi = ti[0];
    block_better(bv, bi, sv, si, par, lane, wave);
    const bool none = bi == INT32_MAX;
    if (tid == 0) { out_v[k] = none ? -INFINITY : bv; out_i[k] = none ? 0 : bi; }
    last_v = none ? -INFINITY : bv;
    if (none) {                                            // (uniform: every thread holds the same winner)
      if (tid == 0) for (int j = k + 1; j < M; ++j) { out_v[j] = -INFINITY; out_i[j] = 0; }
      break;
    }
    if (ti[0] == bi) {                                     // the owner pops its head
#pragma unroll
      for (int j = 0; j < LM_LIST - 1; ++j) { tv[j] = tv[j + 1]; ti[j] = ti[j + 1]; }
      tv[LM_LIST - 1] = -INFINITY; ti[LM_LIST - 1] = INT32_MAX;
    }
  }
  if (!__syncthreads_or(ev > -INFINITY && ev >= last_v)) return;
  // ---- the strict-order passes (a thread held more than 8 of the row's best, or ties reach past a list's end)
  if (tid == 0 && slow_rows) atomicAdd(slow_rows, 1);
  float pv = INFINITY; int pid = -1;
  for (int k = 0; k < M; ++k, par ^= 1) {
    float bv = -INFINITY; int bi = INT32_MAX;
    for (int v0 = tid * 4; v0 < n_valid; v0 += 4096) {
      const float4 q = *reinterpret_cast<const float4*>(p + v0);
      const float xs[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float x = xs[e];
        const int id = v0 + e;
        if (id >= n_valid) continue;
        if (bias) x += bias[id];
        if (x == -INFINITY) continue;
        const bool behind = x < pv || (x == pv && id > pid);
        if (behind && (x > bv || (x == bv && id < bi))) { bv = x; bi = id; }
      }
    }
    block_better(bv, bi, sv, si, par, lane, wave);
    const bool none = bi == INT32_MAX;
    if (tid == 0) { out_v[k] = none ? -INFINITY : bv; out_i[k] = none ? 0 : bi; }
    if (none) {
      if (tid == 0) for (int j = k + 1; j < M; ++j) { out_v[j] = -INFINITY; out_i[j] = 0; }
      break;
    }
    pv = bv; pid = bi;
  }
}

__device__ __forceinline__ void wave_better(float& v, int& i) {      // (higher value, lower id) over the wave; i < 0: no entry
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) { v = ov; i = oi; }
  }
}

__device__ __forceinline__ int lm_state_or_start(const NgramLm& lm, int st) { return st < 0 || st >= lm.n_nodes ? lm.start_node : st; }

// One wave per row, one candidate per lane: value + LM term, a wave arg-max (ties to the lower id; ids of a row are distinct), and the winner's lane writes
// the pick, its state and its log-probability.
__global__ __launch_bounds__(64 * LM_PICK_ROWS) void lm_pick_kernel(const float* __restrict__ cand_v, const int32_t* __restrict__ cand_i,
                                                                   const float* __restrict__ lse, int rows, int M, NgramLm lm, LmEnds ends,
                                                                   int32_t* __restrict__ state, const int32_t* __restrict__ n_saved,
                                                                   int32_t* __restrict__ next, float* __restrict__ logprob, int ld_save) {
  const int r = blockIdx.x * LM_PICK_ROWS + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const int n = *n_saved;
  const int s0 = n == 0 ? lm.start_node : lm_state_or_start(lm, state[r]);
  float x = -INFINITY, v = -INFINITY; int id = -1, st = s0;
  if (lane < M) {
    x = cand_v[(size_t)r * M + lane];
    if (x > -INFINITY) {
      id = cand_i[(size_t)r * M + lane];
      v = __fadd_rn(x, lm_token_term(lm, ends, st, id));
    }
  }
  float wv = v; int wi = id;
  wave_better(wv, wi);
  const bool mine = wi >= 0 ? id == wi : lane == 0;        // no candidate: lane 0 writes id 0, the state as it stands and -inf
  if (mine) {
    next[r] = wi >= 0 ? wi : 0;
    state[r] = wi >= 0 ? st : s0;
    if (logprob && n >= 0 && n < ld_save) logprob[(size_t)r * ld_save + n] = wi >= 0 ? __fsub_rn(x, lse[r]) : -INFINITY;
  }
}

// candidate q of a re-rank row -> its fused score and id; false: no candidate (a missing top-M rank, a trie column that is out of range, listed twice, among
// the top M already, or at -inf)
struct RerankRow {
  const float *p, *bias, *cand_v;
  const int* ki;                       // the row's top-M ids in LDS (-1: rank without a candidate)
  float L, d_other, d_root, d_child;
  int M, n0, nd, s0, n_valid;
  bool hot;
};
__device__ __forceinline__ bool rerank_cand(const RerankRow& r, const HotTrie& tr, const NgramLm& lm, const LmEnds& ends, int q, float& sc, int& id) {
  float x, d;
  if (q < r.M) {
    id = r.ki[q];
    if (id < 0) return false;
    x = r.cand_v[q];
    d = !r.hot ? 0.0f : trie_child(tr, r.nd, id) >= 0 ? r.d_child : (r.nd != 0 && trie_child(tr, 0, id) >= 0 ? r.d_root : r.d_other);
  } else {
    const bool of_node = q - r.M < r.n0;
    id = of_node ? tr.child_tok[tr.child_off[r.nd] + (q - r.M)] : tr.child_tok[tr.child_off[0] + (q - r.M - r.n0)];
    if (id < 0 || id >= r.n_valid) return false;
    if (!of_node && trie_child(tr, r.nd, id) >= 0) return false;             // in both lists: the node's entry stands
    bool in_top = false;
    for (int j = 0; j < r.M; ++j) in_top = in_top || r.ki[j] == id;
    if (in_top) return false;
    x = r.p[id];
    if (r.bias) x += r.bias[id];
    if (x == -INFINITY) return false;
    d = of_node ? r.d_child : r.d_root;
  }
  int st = r.s0;
  sc = __fadd_rn(__fadd_rn(__fsub_rn(x, r.L), d), lm_token_term(lm, ends, st, id));
  return sc > -INFINITY;
}

// One wave per row. Candidate index space: [0, M) the top-M pairs, then (with a trie) the node's children and the root's children, as
// hotword_rerank_kernel lists them. Every candidate's fused score is formed once (the first LM_CACHE into LDS, a longer list's tail again per round); each
// of the K rounds takes the best candidate strictly behind the previous winner in (score descending, id ascending) order.
__global__ __launch_bounds__(64) void lm_rerank_kernel(const float* __restrict__ logits, int ld, int n_valid, const float* __restrict__ bias,
                                                       const float* __restrict__ cand_v, const int32_t* __restrict__ cand_i, const float* __restrict__ lse,
                                                       int M, HotTrie tr, const int32_t* __restrict__ node, NgramLm lm, LmEnds ends,
                                                       const int32_t* __restrict__ state, int stride, int K, float* __restrict__ topv,
                                                       int32_t* __restrict__ topi) {
  const int row = blockIdx.x, lane = threadIdx.x;
  __shared__ float qs[LM_CACHE];
  __shared__ int qi[LM_CACHE], ki[LM_TOPK_MAX];
  const bool hot = tr.n_nodes > 1;
  int nd = hot ? node[(size_t)row * stride] : 0;
  if (nd < 0 || nd >= tr.n_nodes) nd = 0;
  const int s0 = state ? lm_state_or_start(lm, state[(size_t)row * stride]) : lm.start_node;
  const float* p = logits + (size_t)row * ld;
  const float L = lse[row];
  float d_other = 0.0f, d_root = 0.0f, d_child = 0.0f;     // trie_step's bonus arithmetic from 0, as hotword_rerank_kernel forms it
  int n0 = 0, n1 = 0;
  if (hot) {
    d_other = __fsub_rn(0.0f, __fmul_rn((float)tr.depth[nd], tr.boost)); d_root = __fadd_rn(d_other, tr.boost); d_child = tr.boost;
    n0 = tr.child_off[nd + 1] - tr.child_off[nd]; n1 = nd != 0 ? tr.child_off[1] - tr.child_off[0] : 0;
  }
  if (lane < M) ki[lane] = cand_v[(size_t)row * M + lane] > -INFINITY ? cand_i[(size_t)row * M + lane] : -1;
  __syncthreads();
  const int total = M + n0 + n1;
  const RerankRow rr{p, bias, cand_v + (size_t)row * M, ki, L, d_other, d_root, d_child, M, n0, nd, s0, n_valid, hot};
  for (int q = lane; q < total && q < LM_CACHE; q += 64) {
    float sc = -INFINITY; int id = -1;
    const bool ok = rerank_cand(rr, tr, lm, ends, q, sc, id);
    qs[q] = sc; qi[q] = ok ? id : -1;
  }
  __syncthreads();
  float pv = INFINITY; int pid = -1;
  float wv = -INFINITY; int wi = -1;                        // lane k keeps the winner of round k
  for (int k = 0; k < K; ++k) {
    float bv = -INFINITY; int bi = -1;
    for (int q = lane; q < total; q += 64) {
      float sc; int id;
      if (q < LM_CACHE) { sc = qs[q]; id = qi[q]; if (id < 0) continue; }
      else if (!rerank_cand(rr, tr, lm, ends, q, sc, id)) continue;
      const bool behind = sc < pv || (sc == pv && id > pid);
      if (behind && (bi < 0 || sc > bv || (sc == bv && id < bi))) { bv = sc; bi = id; }
    }
    wave_better(bv, bi);
    if (lane == k) { wv = bv; wi = bi; }
    pv = bv; pid = bi;
    if (bi < 0) break;                                      // nothing left: the later ranks keep (-inf, no id)
  }
  if (lane < K) {
    topv[(size_t)row * K + lane] = wi >= 0 ? wv : -INFINITY;
    topi[(size_t)row * K + lane] = wi >= 0 ? wi : 0;
  }
}

}  // namespace

void launch_lm_topk(const float* logits, int ld, int rows, int n_valid, const float* bias, int M, float* cand_v, int32_t* cand_i, float* lse, hipStream_t s,
                    int32_t* slow_rows) {
  ASR_REQUIRE(M >= 1 && M <= LM_TOPK_MAX && ld % 4 == 0 && rows > 0 && n_valid >= 1 && n_valid <= ld && logits && cand_v && cand_i && lse,
              "lm_topk: M %d (1..%d), ld %d, n_valid %d", M, LM_TOPK_MAX, ld, n_valid);
  hipLaunchKernelGGL(lm_topk_kernel, dim3(rows), dim3(1024), 0, s, logits, ld, n_valid, bias, M, cand_v, cand_i, lse, slow_rows);
  HIP_CHECK(hipGetLastError());
}

void launch_lm_pick(const float* cand_v, const int32_t* cand_i, const float* lse, int rows, int M, const NgramLm& lm, const LmEnds& ends, int32_t* state,
                    const int32_t* n_saved, int32_t* next, float* logprob, int ld_save, hipStream_t s) {
  ASR_REQUIRE(lm.n_nodes > 0 && M >= 1 && M <= LM_TOPK_MAX && rows > 0 && ends.n >= 0 && ends.n <= LM_ENDS_MAX && cand_v && cand_i && lse && state && n_saved && next &&
                  (!logprob || ld_save >= 1), "lm_pick: bad argument (M %d)", M);
  hipLaunchKernelGGL(lm_pick_kernel, dim3((rows + LM_PICK_ROWS - 1) / LM_PICK_ROWS), dim3(64 * LM_PICK_ROWS), 0, s, cand_v, cand_i, lse, rows, M, lm, ends, state, n_saved,
                     next, logprob, ld_save);
  HIP_CHECK(hipGetLastError());
}

void launch_lm_rerank(const float* logits, int ld, int rows, int n_valid, const float* bias, const float* cand_v, const int32_t* cand_i, const float* lse, int M,
                      const HotTrie& trie, const int32_t* node, const NgramLm& lm, const LmEnds& ends, const int32_t* state, int stride, int K, float* topv,
                      int32_t* topi, hipStream_t s) {
  ASR_REQUIRE(lm.n_nodes > 0 && M >= 1 && M <= LM_TOPK_MAX && K >= 1 && K <= BEAM_MAX && K <= M && rows > 0 && n_valid <= ld && stride >= 1 && ends.n >= 0 &&
                  ends.n <= LM_ENDS_MAX && logits && cand_v && cand_i && lse && topv && topi && (trie.n_nodes <= 1 || node),
              "lm_rerank: bad argument (M %d, K %d)", M, K);
  hipLaunchKernelGGL(lm_rerank_kernel, dim3(rows), dim3(64), 0, s, logits, ld, n_valid, bias, cand_v, cand_i, lse, M, trie, node, lm, ends, state, stride, K, topv, topi);
  HIP_CHECK(hipGetLastError());
}
