// Hotword boosting of the autoregressive decoders (Whisper, Qwen3-ASR): the selection head's sparse logit bias, the per-row trie state and the beam
// ranker's merge (kernels.h: launch_hotword_*). The trie walk is hot_trie.h, shared with the CTC prefix beam search. The float64 statement is
// tests/hotword_heads_ref.py.
#include "engine.h"
#include "hot_trie.h"
#include "kernels.h"

namespace {

constexpr int HOT_ROWS = 4;           // rows (waves) per workgroup of the bias / restore kernels

// One wave per row. Root children first (skipping those the node list will write), then the node's children: every touched column is written once.
__global__ __launch_bounds__(64 * HOT_ROWS) void hotword_bias_kernel(float* __restrict__ logits, int ld, int rows, int n_valid, HotTrie tr,
                                                                     const int32_t* __restrict__ node, const int32_t* __restrict__ n_saved,
                                                                     float* __restrict__ root_save) {
  const int r = blockIdx.x * HOT_ROWS + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const bool fresh = *n_saved == 0;
  int nd = fresh ? 0 : node[r];
  if (nd < 0 || nd >= tr.n_nodes) nd = 0;
  float* p = logits + (size_t)r * ld;
  const int r0 = tr.child_off[0], r1 = tr.child_off[1];
  for (int j = r0 + lane; j < r1; j += 64) {
    const int c = tr.child_tok[j];
    if (c < 0 || c >= n_valid) continue;
    const float x = p[c];
    if (fresh && root_save) root_save[(size_t)r * (r1 - r0) + (j - r0)] = x;
    if (nd == 0 || trie_child(tr, nd, c) < 0) p[c] = __fadd_rn(x, tr.boost);  // (at the root: depth 0, (float)(0 + 1) * boost == boost)
  }
  if (nd != 0) {
    const float add = __fmul_rn((float)(tr.depth[nd] + 1), tr.boost);   // (rounded on its own: no contraction into the add)
    for (int j = tr.child_off[nd] + lane; j < tr.child_off[nd + 1]; j += 64) {
      const int c = tr.child_tok[j];
      if (c >= 0 && c < n_valid) p[c] = __fadd_rn(p[c], add);
    }
  }
}

__global__ __launch_bounds__(64 * HOT_ROWS) void hotword_restore_kernel(float* __restrict__ logits, int ld, int rows, int n_valid, HotTrie tr,
                                                                        const float* __restrict__ root_save) {
  const int r = blockIdx.x * HOT_ROWS + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const int r0 = tr.child_off[0], r1 = tr.child_off[1];
  for (int j = r0 + lane; j < r1; j += 64) {
    const int c = tr.child_tok[j];
    if (c >= 0 && c < n_valid) logits[(size_t)r * ld + c] = root_save[(size_t)r * (r1 - r0) + (j - r0)];
  }
}

__global__ __launch_bounds__(64) void hotword_advance_kernel(const int32_t* __restrict__ next, int rows, HotTrie tr, int32_t* __restrict__ node,
                                                             const int32_t* __restrict__ n_saved, int32_t* __restrict__ save_ids, int ld_save) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= rows) return;
  const int n = *n_saved;
  if (save_ids && n < ld_save) save_ids[(size_t)r * ld_save + n] = next[r];       // append_ids_kernel's rule: a full table drops the id, the node moves on
  int nd = n == 0 ? 0 : node[r];
  if (nd < 0 || nd >= tr.n_nodes) nd = 0;
  float bonus = 0.0f;
  trie_step(tr, nd, bonus, next[r]);
  node[r] = nd;
}

__device__ __forceinline__ void wave_better(float& v, int& i) {      // (higher value, lower id) over the wave; i < 0: no entry
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) { v = ov; i = oi; }
  }
}

// One wave per row. Candidate index space: [0, K) the top-K pairs, then the node's children, then the root's children (skipped at the root, where the two
// lists are one). Each of the K rounds takes the best candidate strictly behind the previous winner in (score descending, id ascending) order -- ids are
// distinct after the de-duplication, so "behind" is a strict total order and nothing is taken twice.
__global__ __launch_bounds__(64) void hotword_rerank_kernel(const float* __restrict__ logits, int ld, int n_valid, const float* __restrict__ bias,
                                                            const float* __restrict__ lse, HotTrie tr, const int32_t* __restrict__ node, int node_stride,
                                                            int K, float* __restrict__ topv, int32_t* __restrict__ topi) {
  const int row = blockIdx.x, lane = threadIdx.x;
  __shared__ float kv[BEAM_MAX];
  __shared__ int ki[BEAM_MAX];
  int nd = node[(size_t)row * node_stride];
  if (nd < 0 || nd >= tr.n_nodes) nd = 0;
  const float* p = logits + (size_t)row * ld;
  const float L = lse[row];
  // trie_step's bonus arithmetic from 0: the refund first, the child's boost second
  const float d_other = __fsub_rn(0.0f, __fmul_rn((float)tr.depth[nd], tr.boost)), d_root = __fadd_rn(d_other, tr.boost), d_child = tr.boost;
  if (lane < K) {
    const float v = topv[(size_t)row * K + lane];
    const int id = topi[(size_t)row * K + lane];
    float sc = -INFINITY;
    if (v > -INFINITY) sc = __fadd_rn(v, trie_child(tr, nd, id) >= 0 ? d_child : (nd != 0 && trie_child(tr, 0, id) >= 0 ? d_root : d_other));
    kv[lane] = sc; ki[lane] = sc > -INFINITY ? id : -1;
  }
  __syncthreads();
  const int n0 = tr.child_off[nd + 1] - tr.child_off[nd], n1 = nd != 0 ? tr.child_off[1] - tr.child_off[0] : 0;
  const int total = K + n0 + n1;
  float pv = INFINITY; int pid = -1;
  float wv = -INFINITY; int wi = -1;                        // lane k keeps the winner of round k
  for (int k = 0; k < K; ++k) {
    float bv = -INFINITY; int bi = -1;
    for (int q = lane; q < total; q += 64) {
      float sc; int id;
      if (q < K) { sc = kv[q]; id = ki[q]; if (id < 0) continue; }
      else {
        const bool of_node = q - K < n0;
        id = of_node ? tr.child_tok[tr.child_off[nd] + (q - K)] : tr.child_tok[tr.child_off[0] + (q - K - n0)];
        if (id < 0 || id >= n_valid) continue;
        if (!of_node && trie_child(tr, nd, id) >= 0) continue;           // in both lists: the node's entry stands
        bool in_top = false;
        for (int j = 0; j < K; ++j) in_top = in_top || ki[j] == id;
        if (in_top) continue;
        float x = p[id];
        if (bias) x += bias[id];
        if (x == -INFINITY) continue;
        sc = __fadd_rn(__fsub_rn(x, L), of_node ? d_child : d_root);
      }
      const bool behind = sc < pv || (sc == pv && id > pid);
      if (behind && (bi < 0 || sc > bv || (sc == bv && id < bi))) { bv = sc; bi = id; }
    }
    wave_better(bv, bi);
    if (lane == k) { wv = bv; wi = bi; }
    pv = bv; pid = bi;
    if (bi < 0) break;                                        // nothing left: the later ranks keep (-inf, no id)
  }
  if (lane < K) {
    topv[(size_t)row * K + lane] = wi >= 0 ? wv : -INFINITY;
    topi[(size_t)row * K + lane] = wi >= 0 ? wi : 0;
  }
}

}  // namespace

void launch_hotword_bias(float* logits, int ld, int rows, int n_valid, const HotTrie& trie, const int32_t* node, const int32_t* n_saved, float* root_save,
                         hipStream_t s) {
  ASR_REQUIRE(trie.n_nodes > 1 && rows > 0 && n_valid <= ld && node && n_saved, "hotword_bias: bad argument");
  hipLaunchKernelGGL(hotword_bias_kernel, dim3((rows + HOT_ROWS - 1) / HOT_ROWS), dim3(64 * HOT_ROWS), 0, s, logits, ld, rows, n_valid, trie, node, n_saved, root_save);
  HIP_CHECK(hipGetLastError());
}

void launch_hotword_restore(float* logits, int ld, int rows, int n_valid, const HotTrie& trie, const float* root_save, hipStream_t s) {
  ASR_REQUIRE(trie.n_nodes > 1 && rows > 0 && n_valid <= ld && root_save, "hotword_restore: bad argument");
  hipLaunchKernelGGL(hotword_restore_kernel, dim3((rows + HOT_ROWS - 1) / HOT_ROWS), dim3(64 * HOT_ROWS), 0, s, logits, ld, rows, n_valid, trie, root_save);
  HIP_CHECK(hipGetLastError());
}

void launch_hotword_advance(const int32_t* next, int rows, const HotTrie& trie, int32_t* node, const int32_t* n_saved, hipStream_t s, int32_t* save_ids,
                            int ld_save) {
  ASR_REQUIRE(trie.n_nodes > 1 && rows > 0 && next && node && n_saved && (!save_ids || ld_save >= 1), "hotword_advance: bad argument");
  hipLaunchKernelGGL(hotword_advance_kernel, dim3((rows + 63) / 64), dim3(64), 0, s, next, rows, trie, node, n_saved, save_ids, ld_save);
  HIP_CHECK(hipGetLastError());
}

void launch_hotword_rerank(const float* logits, int ld, int rows, int n_valid, const float* bias, const float* lse, const HotTrie& trie, const int32_t* node,
                           int node_stride, int K, float* topv, int32_t* topi, hipStream_t s) {
  ASR_REQUIRE(trie.n_nodes > 1 && rows > 0 && n_valid <= ld && K >= 1 && K <= BEAM_MAX && lse && node && node_stride >= 1, "hotword_rerank: bad argument (K %d)", K);
  hipLaunchKernelGGL(hotword_rerank_kernel, dim3(rows), dim3(64), 0, s, logits, ld, n_valid, bias, lse, trie, node, node_stride, K, topv, topi);
  HIP_CHECK(hipGetLastError());
}
