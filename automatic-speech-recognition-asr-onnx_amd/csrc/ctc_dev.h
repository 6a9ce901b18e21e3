// Device helpers shared by the CTC kernels behind the timed head (ctc_beam.hip: candidates and prefix beam search; ctc_align.hip: gathered emissions and
// forced alignment): log-add-exp, the recomputed logit of one (row, column) and the row's log-sum-exp from the head's per-slab partials. Both files get
// their numbers from these, so a column that is a top-k candidate and an alignment target has the same bits in both.
#pragma once
#include "common.h"

__device__ __forceinline__ float lae(float a, float b) {
  if (a == -INFINITY) return b;
  if (b == -INFINITY) return a;
  return fmaxf(a, b) + log1pf(expf(-fabsf(a - b)));
}

__device__ __forceinline__ float dot8(const float* hs, const bf16_t* w) {
  const uint4 q = *reinterpret_cast<const uint4*>(w);
  const uint32_t u[4] = {q.x, q.y, q.z, q.w};
  float a = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    a = fmaf(hs[2 * i], __uint_as_float(u[i] << 16), a);
    a = fmaf(hs[2 * i + 1], __uint_as_float(u[i] & 0xffff0000u), a);
  }
  return a;
}
__device__ __forceinline__ float dot8(const float* hs, const float* w) {
  const float4 p = *reinterpret_cast<const float4*>(w), q = *reinterpret_cast<const float4*>(w + 4);
  float a = 0.0f;
  a = fmaf(hs[0], p.x, a); a = fmaf(hs[1], p.y, a); a = fmaf(hs[2], p.z, a); a = fmaf(hs[3], p.w, a);
  a = fmaf(hs[4], q.x, a); a = fmaf(hs[5], q.y, a); a = fmaf(hs[6], q.z, a); a = fmaf(hs[7], q.w, a);
  return a;
}
__device__ __forceinline__ float elem_f32(float v) { return v; }
__device__ __forceinline__ float elem_f32(bf16_t v) { return bf16_to_f32(v); }

// hs . wr + bias_col: one lane, f32 accumulation in ascending k, two interleaved partial sums of eight-element dot products (K a multiple of 8)
template <typename T>
__device__ __forceinline__ float ctc_logit(const float* hs, const T* wr, int K, float bias_col) {
  float a0 = 0.0f, a1 = 0.0f;
  int k = 0;
  for (; k + 16 <= K; k += 16) { a0 += dot8(hs + k, wr + k); a1 += dot8(hs + k + 8, wr + k + 8); }
  for (; k < K; k += 8) a0 += dot8(hs + k, wr + k);
  return a0 + a1 + bias_col;
}

// The row's log-sum-exp over the whole wave, as argmax_lse_reduce_kernel forms it: slab maxima rv, slab sums of exponentials rs (relative to the slab's
// maximum), best_row = the largest slab maximum.
__device__ __forceinline__ float ctc_row_lse(const float* rv, const float* rs, int n_slabs, float best_row, int lane) {
  float tot = 0.0f;
  for (int s = lane; s < n_slabs; s += 64) tot += rs[s] * expf(rv[s] - best_row);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
  return best_row + logf(tot);
}
