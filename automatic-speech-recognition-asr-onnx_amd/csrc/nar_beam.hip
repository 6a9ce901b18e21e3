// Token-synchronous beam search over the token rows of a non-autoregressive decoder (offline Paraformer), with the hotword context graph
// (hot_trie.h) and, in the kLm instantiation, a back-off n-gram language model (ngram_lm.h) fused into the ranking. Not a CTC search: there is no blank, no
// collapse and no merging -- every hypothesis of an utterance picks exactly one candidate per token row, so all of them have the utterance's token count and
// two hypotheses with different picks differ in content. The candidates come from ctc_topk_kernel (ctc_beam.hip) behind the decoder's vocabulary GEMM. The
// float64 statement is tests/nar_beam_ref.py.
#include "beam_dev.h"
#include "engine.h"

namespace {

// One workgroup per utterance, sequential over its N token rows plan[u].row_off .. + N of the compact token plan, N = plan[u].n_lfr read here (rows at or
// past *m_dev are never read: N is cut there). The rule of one row is nar_row_step's (beam_dev.h). A kept entry appends (parent rank, candidate column) to
// the utterance's pool at [k * beam + rank]: the walk back reads the token and its log-probability from the candidate arrays at (row k, column). After the
// last row the end terms and the second ranking are nar_end_rank's, and the best nbest are walked back. An utterance without tokens yields the one empty
// hypothesis. Candidate ids of a row must be distinct and, with a model, lie in [0, vocab) of the image.
template <bool kLm>
__global__ __launch_bounds__(NAR_BEAM_THREADS) void nar_beam_kernel(const int32_t* __restrict__ cand_id, const float* __restrict__ cand_lp, int topk,
                                                                    const UttPlan* __restrict__ plan, const int32_t* __restrict__ m_dev, int beam, int nbest,
                                                                    HotTrie tr, LmArg<kLm> lmod, int2* __restrict__ pool_all, int pool_stride,
                                                                    int32_t* __restrict__ tok_out, int max_tokens, int32_t* __restrict__ num_out,
                                                                    float* __restrict__ score_out, float* __restrict__ am_out, float* __restrict__ tlp_out) {
  __shared__ NarLive<kLm> live[2];
  __shared__ float e_score[NAR_BEAM_THREADS];
  __shared__ int c_id[TOKEN_BEAM_MAX], f_order[TOKEN_BEAM_MAX];
  __shared__ float c_lp[TOKEN_BEAM_MAX], f_score[TOKEN_BEAM_MAX], f_am[TOKEN_BEAM_MAX];
  const int u = blockIdx.x, e = threadIdx.x;
  const int row0 = plan[u].row_off;
  int N = plan[u].n_lfr;
  if (m_dev) N = min(N, max(*m_dev - row0, 0));
  N = max(min(N, pool_stride / beam), 0);
  int2* pool = pool_all + (size_t)u * pool_stride;
  nar_live_start<kLm>(live[0], lmod);
  int n_live = 1;
  int nx_id = 0; float nx_lp = 0.0f;
  cand_fetch(cand_id, cand_lp, topk, row0, N > 0, nx_id, nx_lp);
  for (int k = 0; k < N; ++k) {
    cand_advance(cand_id, cand_lp, topk, row0 + k + 1, k + 1 < N, nx_id, nx_lp, c_id, c_lp);
    __syncthreads();
    n_live = nar_row_step<kLm>(tr, lmod, live[k & 1], live[(k + 1) & 1], c_id, c_lp, e_score, n_live, topk, beam, [](int) { return 0; },
                               [&](int rank, int p, int, int j, int, float) { pool[k * beam + rank] = make_int2(p, j); });
    __syncthreads();
  }
  nar_end_rank<kLm>(tr, lmod, live[N & 1], n_live, f_score, f_am, f_order);
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
  ASR_REQUIRE(beam >= 1 && beam <= TOKEN_BEAM_MAX && topk >= 1 && topk <= TOKEN_BEAM_MAX && nbest >= 1 && nbest <= beam, "nar_beam: beam %d, topk %d, nbest %d (1..16, nbest <= beam)",
              beam, topk, nbest);
  ASR_REQUIRE(n_utts > 0 && max_tokens >= 1 && pool && pool_stride >= beam, "nar_beam: bad argument");
  launch_with_lm(lm, [&](auto k_lm, const auto& lmod) {
    hipLaunchKernelGGL(nar_beam_kernel<decltype(k_lm)::value>, dim3(n_utts), dim3(NAR_BEAM_THREADS), 0, s, cand_id, cand_lp, topk, token_plan, m_dev, beam, nbest, trie, lmod,
                       pool, pool_stride, token_ids, max_tokens, num_id, score, am_score, token_logprob);
  });
  HIP_CHECK(hipGetLastError());
}
