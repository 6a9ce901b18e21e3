// Whisper token / word timestamps: OpenAI Whisper's cross-attention DTW (openai-whisper timing.py) on the device. Five kernels (kernels.h):
//   align_scores    inside the decoder step: raw q . k of the selected (layer, head) pairs for the step's last query row, one row of the capture buffer per position
//   align_softmax   after generation: soft-max over the frames that hold audio, in place
//   align_colstats  mean and 1 / std over the token axis per (pair, frame)
//   align_cost      standardise, median-filter along frames (sorting network in registers), mean over the pairs, negate
//   align_dtw       dynamic time warping over the tokens x frames cost matrix, anti-diagonal wavefront, three rolling diagonals in LDS
// The reference has no alignment (it always decodes behind <|notimestamps|>): the specification is OpenAI's algorithm, restated in tests/whisper_align_ref.py.
#include <cmath>

#include "engine.h"
#include "kernels.h"

namespace {

// ---- capture. A 64-key tile per workgroup of 256 threads. A key row (64 elements) is read by LPK lanes with one 16-byte load each (bf16: 8 lanes x 8
// elements, f32: 16 lanes x 4), so a wave's load covers 1 KiB of consecutive slab bytes; the lanes' partial dot products meet through shuffles. q stays in
// registers (each lane keeps the slice of the row it multiplies): no LDS.
template <typename T> struct AlignVec;
template <> struct AlignVec<bf16_t> {
  static constexpr int E = 8;
  static __device__ __forceinline__ void load(const bf16_t* p, float* v) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = __uint_as_float(w[i] << 16); v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
  }
};
template <> struct AlignVec<float> {
  static constexpr int E = 4;
  static __device__ __forceinline__ void load(const float* p, float* v) {
    const float4 u = *reinterpret_cast<const float4*>(p);
    v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
  }
};

template <typename T>
__global__ __launch_bounds__(256) void align_scores_kernel(const T* __restrict__ q, int ld_q, int n, const T* __restrict__ k_base, int64_t stride_h,
                                                           const UttPlan* __restrict__ plan, const int32_t* __restrict__ sel, const int32_t* __restrict__ pos_dev,
                                                           int row_bias, float* __restrict__ out, int n_pairs, int max_rows, int ld) {
  constexpr int E = AlignVec<T>::E, LPK = 64 / E, KPP = 256 / LPK;      // elements per lane, lanes per key, keys per pass
  const int b = blockIdx.z, head = sel[2 * blockIdx.y], slot = sel[2 * blockIdx.y + 1];
  const int row = pos_dev[0] + row_bias;
  const int n_keys = min(plan[b].n_lfr, ld), key0 = blockIdx.x * 64;
  if (row < 0 || row >= max_rows || key0 >= n_keys) return;
  const int part = threadIdx.x % LPK, kk = threadIdx.x / LPK;
  float qv[E];
  AlignVec<T>::load(q + ((size_t)b * n + n - 1) * ld_q + head * 64 + part * E, qv);
  const T* slab = k_base + (size_t)head * stride_h + (size_t)plan[b].row_off * 64;
  float* dst = out + (((size_t)b * n_pairs + slot) * max_rows + row) * ld;
#pragma unroll
  for (int p = 0; p < 64 / KPP; ++p) {
    const int key = key0 + p * KPP + kk;
    float acc = 0.0f;
    if (key < n_keys) {
      float kv[E];
      AlignVec<T>::load(slab + (size_t)key * 64 + part * E, kv);
#pragma unroll
      for (int e = 0; e < E; ++e) acc = fmaf(qv[e], kv[e], acc);
    }
#pragma unroll
    for (int o = LPK / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (part == 0 && key < n_keys) dst[key] = acc;
  }
}

// ---- 1. row soft-max in place: a workgroup per (row, pair, sequence)
__device__ __forceinline__ float block_reduce(float v, bool is_max, float* red) {
  v = is_max ? wave_max(v) : wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();                                  // (red may still be read from the previous reduction)
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float r = red[0];
  for (int i = 1; i < (int)(blockDim.x >> 6); ++i) r = is_max ? fmaxf(r, red[i]) : r + red[i];
  return r;
}

__global__ __launch_bounds__(256) void align_softmax_kernel(float* __restrict__ scores, int n_pairs, int max_rows, int ld, const int32_t* __restrict__ n_rows,
                                                            const int32_t* __restrict__ n_frames) {
  __shared__ float red[4];
  const int b = blockIdx.z, pair = blockIdx.y, r = blockIdx.x;
  const int N = min(n_rows[b], max_rows), M = min(n_frames[b], ld);
  if (r >= N || M <= 0) return;
  float* x = scores + (((size_t)b * n_pairs + pair) * max_rows + r) * ld;
  float m = -INFINITY;
  for (int j = threadIdx.x; j < M; j += blockDim.x) m = fmaxf(m, x[j]);
  m = block_reduce(m, true, red);
  float sum = 0.0f;
  for (int j = threadIdx.x; j < M; j += blockDim.x) sum += expf(x[j] - m);
  sum = block_reduce(sum, false, red);
  const float inv = 1.0f / sum;
  for (int j = threadIdx.x; j < M; j += blockDim.x) x[j] = expf(x[j] - m) * inv;
}

// ---- 2. column statistics over the token axis: a thread per (frame, pair, sequence); consecutive threads read consecutive frames of a row
__global__ __launch_bounds__(256) void align_colstats_kernel(const float* __restrict__ scores, int n_pairs, int max_rows, int ld, const int32_t* __restrict__ n_rows,
                                                             const int32_t* __restrict__ n_frames, float* __restrict__ stats) {
  const int b = blockIdx.z, pair = blockIdx.y, j = blockIdx.x * blockDim.x + threadIdx.x;
  const int N = min(n_rows[b], max_rows), M = min(n_frames[b], ld);
  if (N <= 0 || j >= M) return;
  const float* x = scores + ((size_t)b * n_pairs + pair) * max_rows * ld + j;
  float sum = 0.0f, lo = INFINITY, hi = -INFINITY;
  for (int r = 0; r < N; ++r) { const float v = x[(size_t)r * ld]; sum += v; lo = fminf(lo, v); hi = fmaxf(hi, v); }
  const float mean = sum / (float)N;
  float ss = 0.0f;
  for (int r = 0; r < N; ++r) { const float d = x[(size_t)r * ld] - mean; ss = fmaf(d, d, ss); }
  const float var = ss / (float)N;
  float* st = stats + ((size_t)b * n_pairs + pair) * 2 * ld;
  st[j] = mean;
  // variance 0 -- all rows equal, judged on the values themselves: a rounded mean of equal values need not equal them --: the column standardises to 0
  // (OpenAI divides by zero there)
  st[ld + j] = (hi > lo && var > 0.0f) ? 1.0f / sqrtf(var) : 0.0f;
}

// ---- 3. standardise, median of W reflect-padded neighbours (odd-even transposition network over W registers), mean over the pairs, negate
template <int W>
__global__ __launch_bounds__(256) void align_cost_kernel(const float* __restrict__ scores, const float* __restrict__ stats, int n_pairs, int max_rows, int ld,
                                                         const int32_t* __restrict__ n_rows, const int32_t* __restrict__ n_frames, float* __restrict__ cost) {
  const int b = blockIdx.z, r = blockIdx.y, j = blockIdx.x * blockDim.x + threadIdx.x;
  const int N = min(n_rows[b], max_rows), M = min(n_frames[b], ld);
  if (r >= N || j >= M) return;
  constexpr int P = W / 2;
  const bool filter = M > P;                                 // OpenAI / HF: a row no longer than the pad is returned as it is
  float acc = 0.0f;
  for (int pair = 0; pair < n_pairs; ++pair) {
    const float* x = scores + (((size_t)b * n_pairs + pair) * max_rows + r) * ld;
    const float* st = stats + ((size_t)b * n_pairs + pair) * 2 * ld;
    float v[W];
#pragma unroll
    for (int t = 0; t < W; ++t) {
      int c = filter ? j + t - P : j;
      c = c < 0 ? -c : c >= M ? 2 * (M - 1) - c : c;         // reflect (M > P keeps it inside)
      v[t] = (x[c] - st[c]) * st[ld + c];
    }
    if (filter) {
#pragma unroll
      for (int pass = 0; pass < W; ++pass)
#pragma unroll
        for (int t = pass & 1; t + 1 < W; t += 2) {
          const float lo = fminf(v[t], v[t + 1]), hi = fmaxf(v[t], v[t + 1]);
          v[t] = lo; v[t + 1] = hi;
        }
    }
    acc += v[P];
  }
  cost[((size_t)b * max_rows + r) * ld + j] = -(acc / (float)n_pairs);
}

// ---- 4. DTW. D[i][j] (i tokens, j frames, one-based; D[0][0] = 0, the rest of row 0 and column 0 +inf) lives on three rolling anti-diagonals in LDS,
// indexed by i: diagonal d = i + j needs d - 1 and d - 2 only. One __syncthreads per diagonal; the threads stride over its cells. One trace byte per cell
// goes to global memory; lane 0 walks it back and writes, per row, the smallest frame on the path.
__global__ __launch_bounds__(256) void align_dtw_kernel(const float* __restrict__ cost, int max_rows, int ld, const int32_t* __restrict__ n_rows,
                                                        const int32_t* __restrict__ n_frames, int rows_max, unsigned char* __restrict__ trace, size_t trace_stride,
                                                        int32_t* __restrict__ frames_out, int out_stride, int32_t* __restrict__ path_out, int path_stride,
                                                        int32_t* __restrict__ path_len) {
  extern __shared__ float align_diag[];                     // three diagonals of rows_max + 1 floats
  const int b = blockIdx.x;
  const int N = n_rows[b], M = n_frames[b];
  if (path_len && threadIdx.x == 0) path_len[b] = 0;
  if (N <= 0 || M <= 0 || N > max_rows || N > rows_max || M > ld || N > out_stride || (size_t)(N + 1) * (M + 1) > trace_stride) return;
  const float* x = cost + (size_t)b * max_rows * ld;
  unsigned char* tr = trace + (size_t)b * trace_stride;
  const int Ms = M + 1;
  // the value of D at (i, d - i) from the diagonal buffer that holds d
  auto at = [&](const float* buf, int d, int i) -> float {
    const int j = d - i;
    return (i == 0 || j == 0) ? ((i == 0 && j == 0) ? 0.0f : INFINITY) : buf[i];
  };
  for (int d = 2; d <= N + M; ++d) {
    float* cur = align_diag + (size_t)(d % 3) * (rows_max + 1);
    const float* p1 = align_diag + (size_t)((d + 2) % 3) * (rows_max + 1);                      // d - 1
    const float* p2 = align_diag + (size_t)((d + 1) % 3) * (rows_max + 1);                      // d - 2
    const int lo = max(1, d - M), hi = min(N, d - 1);
    for (int i = lo + threadIdx.x; i <= hi; i += blockDim.x) {
      const int j = d - i;
      const float c0 = at(p2, d - 2, i - 1), c1 = at(p1, d - 1, i - 1), c2 = at(p1, d - 1, i);
      float c; unsigned char t;
      if (c0 < c1 && c0 < c2) { c = c0; t = 0; }
      else if (c1 < c0 && c1 < c2) { c = c1; t = 1; }
      else { c = c2; t = 2; }
      cur[i] = x[(size_t)(i - 1) * ld + (j - 1)] + c;
      tr[(size_t)i * Ms + j] = t;
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  int i = N, j = M, len = 0;
  while (i > 0 || j > 0) {
    const int t = i == 0 ? 2 : j == 0 ? 1 : tr[(size_t)i * Ms + j];      // OpenAI's backtrace: trace[0, :] = 2, trace[:, 0] = 1
    if (i > 0 && j > 0) frames_out[(size_t)b * out_stride + i - 1] = j - 1;      // walking back, the last write of a row is its smallest frame
    if (path_out && len < path_stride) { path_out[((size_t)b * path_stride + len) * 2] = i - 1; path_out[((size_t)b * path_stride + len) * 2 + 1] = j - 1; }
    ++len;
    if (t == 0) { --i; --j; }
    else if (t == 1) --i;
    else --j;
  }
  if (path_len) path_len[b] = len;
}

}  // namespace

template <typename T>
void launch_align_scores(const AlignScoresArgs& a, int B, hipStream_t s) {
  ASR_REQUIRE(a.n_sel >= 1 && a.max_keys >= 1 && a.max_keys <= a.ld && a.n >= 1 && B >= 1 && a.ld_q % 8 == 0, "align_scores: bad launch geometry");
  hipLaunchKernelGGL(align_scores_kernel<T>, dim3((a.max_keys + 63) / 64, a.n_sel, B), dim3(256), 0, s, (const T*)a.q, a.ld_q, a.n, (const T*)a.k_base, a.stride_h,
                     a.plan, a.sel, a.pos_dev, a.row_bias, a.out, a.n_pairs, a.max_rows, a.ld);
  HIP_CHECK(hipGetLastError());
}
template void launch_align_scores<bf16_t>(const AlignScoresArgs&, int, hipStream_t);
template void launch_align_scores<float>(const AlignScoresArgs&, int, hipStream_t);

void launch_align_softmax(float* scores, int B, int n_pairs, int max_rows, int ld, const int32_t* n_rows, const int32_t* n_frames, int rows_max, hipStream_t s) {
  ASR_REQUIRE(B >= 1 && n_pairs >= 1 && rows_max >= 1 && rows_max <= max_rows, "align_softmax: bad launch geometry");
  hipLaunchKernelGGL(align_softmax_kernel, dim3(rows_max, n_pairs, B), dim3(256), 0, s, scores, n_pairs, max_rows, ld, n_rows, n_frames);
  HIP_CHECK(hipGetLastError());
}

void launch_align_colstats(const float* scores, int B, int n_pairs, int max_rows, int ld, const int32_t* n_rows, const int32_t* n_frames, int frames_max,
                           float* stats, hipStream_t s) {
  ASR_REQUIRE(B >= 1 && n_pairs >= 1 && frames_max >= 1 && frames_max <= ld, "align_colstats: bad launch geometry");
  hipLaunchKernelGGL(align_colstats_kernel, dim3((frames_max + 255) / 256, n_pairs, B), dim3(256), 0, s, scores, n_pairs, max_rows, ld, n_rows, n_frames, stats);
  HIP_CHECK(hipGetLastError());
}

void launch_align_cost(const float* scores, const float* stats, int B, int n_pairs, int max_rows, int ld, const int32_t* n_rows, const int32_t* n_frames,
                       int rows_max, int frames_max, int width, float* cost, hipStream_t s) {
  ASR_REQUIRE(B >= 1 && n_pairs >= 1 && rows_max >= 1 && rows_max <= max_rows && frames_max >= 1 && frames_max <= ld, "align_cost: bad launch geometry");
  ASR_REQUIRE(width >= 1 && width <= 9 && (width & 1), "align_cost: median filter width %d (odd, 1..9)", width);
  const dim3 grid((frames_max + 255) / 256, rows_max, B);
#define ALIGN_COST(W) hipLaunchKernelGGL(align_cost_kernel<W>, grid, dim3(256), 0, s, scores, stats, n_pairs, max_rows, ld, n_rows, n_frames, cost)
  switch (width) {
    case 1: ALIGN_COST(1); break;
    case 3: ALIGN_COST(3); break;
    case 5: ALIGN_COST(5); break;
    case 7: ALIGN_COST(7); break;
    default: ALIGN_COST(9); break;
  }
#undef ALIGN_COST
  HIP_CHECK(hipGetLastError());
}

void launch_align_dtw(const float* cost, int B, int max_rows, int ld, const int32_t* n_rows, const int32_t* n_frames, int rows_max, unsigned char* trace, size_t trace_stride,
                      int32_t* frames_out, int out_stride, int32_t* path_out, int path_stride, int32_t* path_len, hipStream_t s) {
  ASR_REQUIRE(B >= 1 && max_rows >= 1 && ld >= 1 && out_stride >= 1 && trace_stride >= 4 && rows_max >= 1 && rows_max <= max_rows && rows_max <= 4000, "align_dtw: bad launch geometry");
  hipLaunchKernelGGL(align_dtw_kernel, dim3(B), dim3(256), (size_t)3 * (rows_max + 1) * sizeof(float), s, cost, max_rows, ld, n_rows, n_frames, rows_max, trace, trace_stride, frames_out, out_stride, path_out,
                     path_stride, path_len);
  HIP_CHECK(hipGetLastError());
}
