// CTC forced alignment of a transcript the caller supplies. Two kernels behind the timed CTC head (GemmArgs::amax_sum):
// ctc_target_logprob_kernel gathers every row's log soft-max at the blank and at the utterance's target columns without the logits ever being stored
// (the recomputed logit and the row's log-sum-exp are ctc_topk_kernel's, ctc_dev.h), ctc_align_kernel runs the Viterbi and the forward trellis over those
// emissions, one workgroup per utterance, and walks the best path back into per-token spans. The float64 and f32 statements are tests/ctc_align_ref.py.
#include "ctc_dev.h"
#include "engine.h"
#include "kernels.h"

namespace {

// ---- emissions -----------------------------------------------------------------------------------------------------------------------------------
// One wave per row, lane = slot: slot 0 the blank, slot j the utterance's target j - 1, slots past the utterance's length -inf up to ld_em.
constexpr int EM_ROWS = 4;            // rows (waves) per workgroup

template <typename T>
__global__ __launch_bounds__(64 * EM_ROWS) void ctc_target_logprob_kernel(const T* __restrict__ h, int ldh, const T* __restrict__ W, int ldw, const float* __restrict__ bias,
                                                                          int K, const float* __restrict__ amax_val, const float* __restrict__ amax_sum, int n_slabs, int M,
                                                                          const int32_t* __restrict__ row_utt, const int32_t* __restrict__ tgt_ids,
                                                                          const int32_t* __restrict__ tgt_off, int blank, float* __restrict__ em, int ld_em) {
  extern __shared__ float em_lds[];                   // [EM_ROWS][K] activation rows
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int m_raw = blockIdx.x * EM_ROWS + wv;
  const int m = min(m_raw, M - 1);                    // (a wave past the last row repeats it up to the barrier and stores nothing)
  float* hs = em_lds + (size_t)wv * K;
  for (int k = lane; k < K; k += 64) hs[k] = elem_f32(h[(size_t)m * ldh + k]);
  __syncthreads();
  const int u = row_utt[m];
  if (m_raw >= M || u < 0) return;                    // a pad row behind the last utterance keeps what it held
  const float* rv = amax_val + (size_t)m * n_slabs;
  const float* rs = amax_sum + (size_t)m * n_slabs;
  float best_row = -INFINITY;
  for (int s = lane; s < n_slabs; s += 64) best_row = fmaxf(best_row, rv[s]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best_row = fmaxf(best_row, __shfl_xor(best_row, o, 64));
  const float lse = ctc_row_lse(rv, rs, n_slabs, best_row, lane);
  const int o = tgt_off[u], L = tgt_off[u + 1] - o;
  for (int j = lane; j < ld_em; j += 64) {
    float v = -INFINITY;
    if (j <= L) {
      const int col = j == 0 ? blank : tgt_ids[o + j - 1];
      v = ctc_logit(hs, W + (size_t)col * ldw, K, bias[col]) - lse;
    }
    em[(size_t)m * ld_em + j] = v;
  }
}

// ---- trellis -------------------------------------------------------------------------------------------------------------------------------------
// States s = 0 .. 2 L (even: blank, odd 2 j + 1: target j). Thread j owns the pair (2 j, 2 j + 1) in registers -- thread L the final blank alone -- so a row
// costs one LDS exchange (the left neighbour's odd state, double buffered: one barrier per row) and two emission loads fetched a row ahead.
//   v_t[s] = best(v_t-1[s], v_t-1[s - 1], v_t-1[s - 2]) + em[t][slot(s)],   s - 2 only for odd s whose target differs from target j - 1;
// a larger jump is taken only if strictly greater (stay, then 1, then 2). Only additions and comparisons: the path and its score are bit-defined given em.
// A second pair carries the forward sum with lae, in the order lae(lae(stay, step 1), step 2). Backpointers: 2 bits per (row, state), the four bits of a
// thread's pair for eight consecutive rows in one word, [ceil(rows / 8)][L + 1] words -- in dynamic LDS behind the exchange buffers when the launch's largest
// utterance fits (launch_ctc_align), else in the caller's workspace. Thread 0 walks the path back (one word per row), then thread j averages its span.
constexpr int ALIGN_MAX_L = 1023;                     // L + 1 threads
constexpr size_t ALIGN_LDS_BYTES = 64 * 1024 - 256;   // dynamic LDS a launch may ask for without an attribute (a few static words beside it)

__global__ __launch_bounds__(1024) void ctc_align_kernel(const float* __restrict__ em, int ld_em, const UttPlan* __restrict__ plan, int row0,
                                                         const int32_t* __restrict__ tgt_ids, const int32_t* __restrict__ tgt_off, uint32_t* __restrict__ bp_ws,
                                                         size_t bp_stride, int bp_in_lds, int32_t* __restrict__ first_frame, int32_t* __restrict__ last_frame,
                                                         float* __restrict__ token_logprob, int max_tokens, float* __restrict__ path_score, float* __restrict__ loglik,
                                                         int32_t* __restrict__ status) {
  extern __shared__ uint32_t align_lds[];             // float2 [2][blockDim + 1] exchange (v, f of the odd state), then the backpointer words
  __shared__ int s_ok;
  const int u = blockIdx.x, j = threadIdx.x, nx = blockDim.x + 1;
  const int T = plan[u].T - row0;
  const size_t base = (size_t)plan[u].row_off + row0;
  const int o = tgt_off[u], L = tgt_off[u + 1] - o, Wd = L + 1;
  if (T <= 0) {                                       // no row to align against (uniform over the workgroup)
    if (j == 0) { path_score[u] = -INFINITY; loglik[u] = -INFINITY; status[u] = 1; }
    return;
  }
  float2* x = reinterpret_cast<float2*>(align_lds);
  uint32_t* bp = bp_in_lds ? align_lds + 4 * (size_t)nx : bp_ws + (size_t)u * bp_stride;
  const bool has_t = j < L;                           // this thread owns a target state
  const bool skip_ok = has_t && j >= 1 && tgt_ids[o + j] != tgt_ids[o + j - 1];
  const float NINF = -INFINITY;
  if (j == 0) { x[0] = make_float2(NINF, NINF); x[nx] = make_float2(NINF, NINF); }     // state -1 of both buffers
  const float* e = em + base * ld_em;
  float eb = j <= L ? e[0] : NINF, et = has_t ? e[j + 1] : NINF;
  float vb = j == 0 ? eb : NINF, vt = j == 0 ? et : NINF;       // start: v[0] = em[blank], v[1] = em[target 0]
  float fb = vb, ft = vt;
  uint32_t word = 0;
  if (T > 1) { e += ld_em; eb = j <= L ? e[0] : NINF; et = has_t ? e[j + 1] : NINF; }
  for (int t = 1; t < T; ++t) {
    float2* xb = x + (t & 1) * nx;
    xb[j + 1] = make_float2(vt, ft);
    const float ceb = eb, cet = et;
    if (t + 1 < T) { e += ld_em; eb = j <= L ? e[0] : NINF; et = has_t ? e[j + 1] : NINF; }
    __syncthreads();
    const float2 p = xb[j];                           // state 2 j - 1 of row t - 1
    float best = vb; uint32_t bits = 0;
    if (p.x > best) { best = p.x; bits = 1; }
    const float nvb = best + ceb;
    const float nfb = lae(fb, p.y) + ceb;
    best = vt; uint32_t bt = 0;
    if (vb > best) { best = vb; bt = 1; }
    if (skip_ok && p.x > best) { best = p.x; bt = 2; }
    const float nvt = best + cet;
    const float nft = lae(lae(ft, fb), skip_ok ? p.y : NINF) + cet;
    vb = nvb; vt = nvt; fb = nfb; ft = nft;
    word |= (bits | (bt << 2)) << ((t & 7) * 4);
    if ((t & 7) == 7 || t == T - 1) {
      if (j <= L) bp[(size_t)(t >> 3) * Wd + j] = word;
      word = 0;
    }
  }
  __syncthreads();
  if (j == L) { x[1] = make_float2(vb, fb); if (L == 0) x[0] = make_float2(NINF, NINF); }    // state 2 L
  if (j == L - 1) x[0] = make_float2(vt, ft);                                               // state 2 L - 1
  __threadfence_block();
  __syncthreads();
  if (j == 0) {
    const float2 a = x[0], b = x[1];
    const bool odd_end = L > 0 && a.x >= b.x;         // state 2 L - 1 wins a tie
    const float score = odd_end ? a.x : b.x;
    const bool ok = score != NINF;
    s_ok = ok ? 1 : 0;
    path_score[u] = ok ? score : NINF;
    loglik[u] = ok ? lae(a.y, b.y) : NINF;
    status[u] = ok ? 0 : 1;
    if (ok) {
      int s = odd_end ? 2 * L - 1 : 2 * L;
      bool in_run = false;
      const size_t ob = (size_t)u * max_tokens;
      for (int t = T - 1; t >= 0; --t) {
        const int jj = s >> 1;
        if ((s & 1) && !in_run) { last_frame[ob + jj] = t + row0; in_run = true; }
        const uint32_t bits = t > 0 ? (bp[(size_t)(t >> 3) * Wd + jj] >> ((t & 7) * 4 + (s & 1) * 2)) & 3u : 0u;
        if ((s & 1) && (bits != 0 || t == 0)) { first_frame[ob + jj] = t + row0; in_run = false; }
        s = max(s - (int)bits, 0);
      }
    }
  }
  __threadfence_block();
  __syncthreads();
  if (s_ok && has_t) {                                // the mean of the span's emissions: f32 sum in ascending row order / f32 count
    const size_t ob = (size_t)u * max_tokens + j;
    const int f = first_frame[ob] - row0, l = last_frame[ob] - row0;
    float sum = 0.0f;
    for (int t = f; t <= l; ++t) sum += em[(base + t) * ld_em + j + 1];
    token_logprob[ob] = sum / (float)(l - f + 1);
  }
}

inline size_t align_bp_words(int max_rows, int row0, int max_L) { return (size_t)((std::max(max_rows - row0, 1) + 7) / 8) * (max_L + 1); }
inline int align_threads(int max_L) { return (max_L + 1 + 63) / 64 * 64; }
inline bool align_bp_in_lds(int max_rows, int row0, int max_L) {
  return (size_t)16 * (align_threads(max_L) + 1) + align_bp_words(max_rows, row0, max_L) * 4 <= ALIGN_LDS_BYTES;
}

}  // namespace

template <typename T>
void launch_ctc_target_logprob(const T* h, int ldh, const T* W, int ldw, const float* bias, int K, const float* amax_val, const float* amax_sum, int n_slabs, int M,
                               const int32_t* row_utt, const int32_t* target_ids, const int32_t* target_offsets, int blank_id, float* em, int ld_em, hipStream_t s) {
  ASR_REQUIRE(K % 8 == 0 && K <= 2048 && (ldw * sizeof(T)) % 16 == 0 && M > 0, "ctc_target_logprob: K = %d, ldw = %d", K, ldw);
  ASR_REQUIRE(ld_em >= 1 && ld_em <= ALIGN_MAX_L + 1 && blank_id >= 0 && blank_id < n_slabs * 64 && row_utt && target_ids && target_offsets && em,
              "ctc_target_logprob: ld_em = %d, blank %d", ld_em, blank_id);
  hipLaunchKernelGGL(ctc_target_logprob_kernel<T>, dim3((M + EM_ROWS - 1) / EM_ROWS), dim3(64 * EM_ROWS), (size_t)EM_ROWS * K * 4, s, h, ldh, W, ldw, bias, K, amax_val,
                     amax_sum, n_slabs, M, row_utt, target_ids, target_offsets, blank_id, em, ld_em);
  HIP_CHECK(hipGetLastError());
}
template void launch_ctc_target_logprob<float>(const float*, int, const float*, int, const float*, int, const float*, const float*, int, int, const int32_t*, const int32_t*,
                                               const int32_t*, int, float*, int, hipStream_t);
template void launch_ctc_target_logprob<bf16_t>(const bf16_t*, int, const bf16_t*, int, const float*, int, const float*, const float*, int, int, const int32_t*, const int32_t*,
                                                const int32_t*, int, float*, int, hipStream_t);

size_t ctc_align_ws_bytes(int n_utts, int max_rows, int row0, int max_L) {
  return align_bp_in_lds(max_rows, row0, max_L) ? 0 : (size_t)n_utts * align_bp_words(max_rows, row0, max_L) * 4;
}

void launch_ctc_align(const float* em, int ld_em, const UttPlan* plan, int n_utts, int row0, int max_rows, const int32_t* target_ids, const int32_t* target_offsets,
                      int max_L, uint32_t* bp_ws, int32_t* first_frame, int32_t* last_frame, float* token_logprob, int max_tokens, float* path_score, float* loglik,
                      int32_t* status, hipStream_t s) {
  ASR_REQUIRE(max_L >= 0 && max_L <= ALIGN_MAX_L, "ctc_align: a transcript of %d tokens (at most %d)", max_L, ALIGN_MAX_L);
  ASR_REQUIRE(n_utts > 0 && row0 >= 0 && max_rows >= 1 && ld_em >= max_L + 1 && max_tokens >= std::max(max_L, 1), "ctc_align: bad argument");
  ASR_REQUIRE(em && plan && target_ids && target_offsets && first_frame && last_frame && token_logprob && path_score && loglik && status, "ctc_align: null argument");
  const bool in_lds = align_bp_in_lds(max_rows, row0, max_L);
  ASR_REQUIRE(in_lds || bp_ws, "ctc_align: the backpointers of %d rows x %d tokens need the workspace", max_rows - row0, max_L);
  const int threads = align_threads(max_L);
  const size_t words = align_bp_words(max_rows, row0, max_L);
  const size_t lds = (size_t)16 * (threads + 1) + (in_lds ? words * 4 : 0);
  hipLaunchKernelGGL(ctc_align_kernel, dim3(n_utts), dim3(threads), lds, s, em, ld_em, plan, row0, target_ids, target_offsets, bp_ws, words, in_lds ? 1 : 0, first_frame,
                     last_frame, token_logprob, max_tokens, path_score, loglik, status);
  HIP_CHECK(hipGetLastError());
}
