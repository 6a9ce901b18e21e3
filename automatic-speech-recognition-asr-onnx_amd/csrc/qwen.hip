// Qwen3-ASR hot path on one MI355X (Qwen_ASR/Export_Qwen_ASR.py).
//   prefill : packed ragged batch -> Whisper-style log-mel (shared fbank kernel) -> 100-frame chunks -> 3 x Conv2d(k3, s2, p1) +
//             tanh-GELU as GEMMs over gathered (channel-last) patches -> conv_out + positions -> windowed-attention encoder
//             layers (windows of n_window_infer / 100 chunks are the attention units) -> proj1 / tanh-GELU / proj2 -> prompt rows
//             [head | query | suffix | audio | tail | language tail] gathered into the decoder's residual stream -> Qwen3 decoder
//             layers over the whole prompt (RMSNorm folded into q|k|v, per-head q/k RMSNorm, RoPE, causal GQA attention with an
//             in-place KV cache, SwiGLU) -> final RMSNorm of each sequence's last row -> lm_head -> arg-max.
//             Follows QWEN3_ASR_ENCODER.forward (:850-927), ROTARY_MASK_PREFILL (:933-1002), DECODER_MAIN.forward (:1265-1336).
//   decode  : one token per sequence with per-sequence history lengths (ROTARY_MASK_DECODE :1005-1028).
// The reference shuttles 2 x 28 KV tensors through Python per token and re-concatenates them (:1306-1309); here the cache is
// appended in place and token ids / history lengths stay on the device between steps.
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/asr_mi355x.h"
#include "decode_head.h"
#include "engine.h"
#include "gemm.h"
#include "kernels.h"
#include "qwen_attn.h"

namespace {

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// tokens after the three stride-2 convolutions of n mel frames (_get_feat_extract_output_lengths, :519-527)
inline int feat_lengths(int n) {
  const int leave = n % 100;
  const int f1 = leave > 0 ? (std::max(leave - 1, 0) / 2 + 1) : 0;
  const int f2 = f1 > 0 ? (std::max(f1 - 1, 0) / 2 + 1) : 0;
  const int f3 = f2 > 0 ? (std::max(f2 - 1, 0) / 2 + 1) : 0;
  return f3 + (n / 100) * 13;
}

// rows handed to the GEMMs must be readable up to the next row-tile edge (128- or 144-row tiles)
inline size_t pad_rows(size_t r) { return (r + 127) / 128 * 128 + 144; }

// ------------------------------------------------------------------------------------ kernels
template <typename T> __device__ __forceinline__ void load8(const T* p, float* o);
template <> __device__ __forceinline__ void load8<float>(const float* p, float* o) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}
template <> __device__ __forceinline__ void load8<bf16_t>(const bf16_t* p, float* o) {
  const uint4 r = *reinterpret_cast<const uint4*>(p);
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) { o[2 * e] = __uint_as_float(w[e] << 16); o[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u); }
}
// log-mel finish: clamp to (clip max - 8), x * 0.25 + 1, laid out per 100-frame chunk slot [slot][frame][mel]; frames past the clip
// (and whole padding slots) are zero (:855-866)
template <typename T>
__global__ void qw_mel_finish_kernel(const float* __restrict__ mel, const float* __restrict__ blk_max, const UttPlan* __restrict__ plan,
                                     const int32_t* __restrict__ slot_utt, const int32_t* __restrict__ slot_local, int n_mels, int chunk,
                                     T* __restrict__ out) {
  const int j = blockIdx.x, slot = j / chunk, t = j - slot * chunk, u = slot_utt[slot];
  T* o = out + (size_t)j * n_mels;
  int f = -1;
  UttPlan up{};
  if (u >= 0) { up = plan[u]; f = slot_local[slot] * chunk + t; if (f >= up.n_frames) f = -1; }
  if (f < 0) {
    for (int c = threadIdx.x; c < n_mels; c += blockDim.x) Elem<T>::store(o + c, 0.0f);
    return;
  }
  float gmax = -INFINITY;
  const int nblk = (up.n_frames + 63) / 64;
  for (int k = 0; k < nblk; ++k) gmax = fmaxf(gmax, blk_max[up.blk0 + k]);
  for (int c = threadIdx.x; c < n_mels; c += blockDim.x) {
    const float v = fmaxf(mel[(size_t)(up.frame_off + f) * n_mels + c], gmax - 8.0f);
    Elem<T>::store(o + c, v * 0.25f + 1.0f);
  }
}

// conv1 patches: row (slot, t1, f1) <- the 3 x 3 neighbourhood of feat[slot][2 t1 + kw - 1][2 f1 + kh - 1]; K = 64 (9 used, k = kh*3+kw)
template <typename T>
__global__ void qw_im2col1_kernel(const T* __restrict__ feat, int n_mels, int chunk, int t_out, int f_out, T* __restrict__ out) {
  const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int k = threadIdx.x & 63;
  const int per = t_out * f_out;
  const int slot = (int)(r / per), rem = (int)(r % per), t1 = rem / f_out, f1 = rem % f_out;
  float v = 0.0f;
  if (k < 9) {
    const int kh = k / 3, kw = k % 3, fi = 2 * f1 + kh - 1, ti = 2 * t1 + kw - 1;
    if (fi >= 0 && fi < n_mels && ti >= 0 && ti < chunk) v = Elem<T>::load(feat + ((size_t)slot * chunk + ti) * n_mels + fi);
  }
  Elem<T>::store(out + r * 64 + k, v);
}

// channel-last patches of a stride-2 3 x 3 convolution: out row (unit, t_o, f_o), column (kh*3+kw) * C + c <- src row
// (src_unit, 2 t_o + kw - 1, 2 f_o + kh - 1) (zero outside [0, t_in) x [0, f_in)). `slots` > 0 describes conv3's window layout: the
// unit is a window of `slots` token rows; slot s maps to source unit unit * cpw + s / t_tok, t_o = s % t_tok (pad slots are zero).
template <typename T>
__global__ __launch_bounds__(256) void qw_im2col_cl_kernel(const T* __restrict__ src, int C, int t_in, int f_in, int t_o_n, int f_o_n, int slots,
                                                           int cpw, int t_tok, T* __restrict__ out) {
  const size_t r = blockIdx.x;
  int unit, t_o, f_o, src_unit;
  bool live = true;
  if (slots > 0) {
    const int per = slots * f_o_n;
    unit = (int)(r / per);
    const int rem = (int)(r % per), s = rem / f_o_n;
    f_o = rem % f_o_n;
    live = s < cpw * t_tok;
    src_unit = unit * cpw + s / t_tok;
    t_o = s % t_tok;
  } else {
    const int per = t_o_n * f_o_n;
    unit = (int)(r / per);
    const int rem = (int)(r % per);
    t_o = rem / f_o_n; f_o = rem % f_o_n;
    src_unit = unit;
  }
  constexpr int V = 16 / sizeof(T);                    // elements per 16-byte move
  const int vec_per_tap = C / V;
  for (int e = threadIdx.x; e < 9 * vec_per_tap; e += 256) {
    const int tap = e / vec_per_tap, cv = e - tap * vec_per_tap, kh = tap / 3, kw = tap % 3;
    const int ti = 2 * t_o + kw - 1, fi = 2 * f_o + kh - 1;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (live && ti >= 0 && ti < t_in && fi >= 0 && fi < f_in)
      v = *reinterpret_cast<const uint4*>(src + (((size_t)src_unit * t_in + ti) * f_in + fi) * C + cv * V);
    *reinterpret_cast<uint4*>(out + r * 9 * C + (size_t)tap * C + cv * V) = v;
  }
}

// y = x * rsqrt(mean(x^2) + eps) [* weight]; one wave per row
template <typename OutT>
__global__ __launch_bounds__(256) void qw_rmsnorm_kernel(const float* __restrict__ x, int ld_x, int rows, int D, const float* __restrict__ w,
                                                         float eps, OutT* __restrict__ out, int ld_out, const int32_t* __restrict__ src_rows) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* xr = x + (size_t)(src_rows ? src_rows[row] : row) * ld_x;
  float ss = 0.0f;
  for (int i = lane * 4; i < D; i += 256) {
    const float4 v = *reinterpret_cast<const float4*>(xr + i);
    ss += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
  }
  const float r = rsqrtf(wave_sum(ss) / (float)D + eps);
  OutT* o = out + (size_t)row * ld_out;
  for (int i = lane * 4; i < D; i += 256) {
    const float4 v = *reinterpret_cast<const float4*>(xr + i);
    float y[4] = {v.x * r, v.y * r, v.z * r, v.w * r};
    if (w) { y[0] *= w[i]; y[1] *= w[i + 1]; y[2] *= w[i + 2]; y[3] *= w[i + 3]; }
#pragma unroll
    for (int e = 0; e < 4; ++e) Elem<OutT>::store(o + i + e, y[e]);
  }
}

// (KvAddr, the cache addressing of both layouts: qwen_attn.h)
template <typename T>
__device__ __forceinline__ T* kv_row(T* base, const KvAddr& a, int b, int kvh, int n_kv, int s) {
  if (a.table) return base + (size_t)a.table[(size_t)b * a.pps + (s >> 4)] * a.page_stride + ((size_t)kvh * 16 + (s & 15)) * 128;
  return base + (((size_t)b * n_kv + kvh) * a.S_max + s) * 128;
}

__device__ __forceinline__ void qw_store4(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void qw_store4(bf16_t* p, const float (&v)[4]) { *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])); }

// per-head RMSNorm of q and k (weight * d^-1/4 folded), RoPE (half-split convention, position = hist + t), then q -> operand
// buffer, k / v -> the KV cache [layer-local base][seq][kv head][S][128] at that position (:1283-1309). Sixteen lanes per (row, head) -- four heads per wave --,
// a lane holds four consecutive elements of each rotary half (16-byte loads; the one-element-per-lane form of rounds 3-5 moved 280 MB per prefill layer at 2 TB/s).
template <typename T>
__global__ __launch_bounds__(256) void qw_qk_rope_kernel(const float* __restrict__ qkv, int n_heads, int n_kv, const float* __restrict__ qn,
                                                         const float* __restrict__ kn, const float* __restrict__ rope, float eps,
                                                         const int32_t* __restrict__ row_seq, const int32_t* __restrict__ row_t,
                                                         const int32_t* __restrict__ hist, int rows, T* __restrict__ q_out, T* __restrict__ kc,
                                                         T* __restrict__ vc, KvAddr ka, T* __restrict__ k_rows) {
  constexpr int HD = 128;
  const int heads = n_heads + 2 * n_kv;
  const int gid = blockIdx.x * 16 + (threadIdx.x >> 4), l = threadIdx.x & 15;          // (row, head) unit; a row's heads are consecutive units
  const int row = gid / heads, hh = gid - row * heads;
  const bool live = row < rows && row_seq[min(row, rows - 1)] >= 0;
  const int b = live ? row_seq[row] : 0;
  const int pos = live ? hist[b] + row_t[row] : 0;
  const float* src = qkv + (size_t)(live ? row : 0) * heads * HD + hh * HD + 4 * l;
  const float4 lo = *reinterpret_cast<const float4*>(src), hi = *reinterpret_cast<const float4*>(src + 64);
  const float x0[4] = {lo.x, lo.y, lo.z, lo.w}, x1[4] = {hi.x, hi.y, hi.z, hi.w};              // the two rotary halves of this lane's four pairs
  // (explicit fmaf here and in the rotation below: which product of a * b + c * d gets fused is otherwise the compiler's choice per kernel, and the fused decode
  //  kernel has to round exactly like this one -- a fused step and an unfused one cache the same bits, tests/test_qwen_attn_gpu.py::test_forms_agree)
  auto sq2 = [](float a, float b) { return fmaf(a, a, b * b); };
  float ss = (sq2(x0[0], x1[0]) + sq2(x0[1], x1[1])) + (sq2(x0[2], x1[2]) + sq2(x0[3], x1[3]));
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);                                  // (every lane of the wave takes part: no early exit above)
  if (!live) return;
  if (hh >= n_heads + n_kv) {                                  // v: cached as is
    T* dst = kv_row(vc, ka, b, hh - n_heads - n_kv, n_kv, pos) + 4 * l;
    qw_store4(dst, x0); qw_store4(dst + 64, x1);
    return;
  }
  const float r = rsqrtf(ss / (float)HD + eps);
  const float* w = (hh < n_heads ? qn : kn) + 4 * l;
  const float4 w0 = *reinterpret_cast<const float4*>(w), w1 = *reinterpret_cast<const float4*>(w + 64);
  const float* rp = rope + (size_t)pos * HD + 4 * l;
  const float4 c4 = *reinterpret_cast<const float4*>(rp), s4 = *reinterpret_cast<const float4*>(rp + 64);
  const float wa[4] = {w0.x, w0.y, w0.z, w0.w}, wb[4] = {w1.x, w1.y, w1.z, w1.w}, cs[4] = {c4.x, c4.y, c4.z, c4.w}, sn[4] = {s4.x, s4.y, s4.z, s4.w};
  float y0[4], y1[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float a0 = x0[e] * r * wa[e], a1 = x1[e] * r * wb[e];
    y0[e] = fmaf(a0, cs[e], -(a1 * sn[e])); y1[e] = fmaf(a1, cs[e], a0 * sn[e]);
  }
  T* dst = (hh < n_heads ? q_out + (size_t)row * n_heads * HD + hh * HD : kv_row(kc, ka, b, hh - n_heads, n_kv, pos)) + 4 * l;
  qw_store4(dst, y0); qw_store4(dst + 64, y1);
  if (k_rows && hh >= n_heads) {                         // row-major copy of the new keys for the prefill attention kernel
    T* kr = k_rows + (size_t)row * n_kv * HD + (hh - n_heads) * HD + 4 * l;
    qw_store4(kr, y0); qw_store4(kr + 64, y1);
  }
}

// causal GQA attention over the cache: workgroup = (sequence, q head), 128 threads; query t of the sequence sees keys [0, hist + t]
template <typename T>
__global__ __launch_bounds__(128) void qw_attn_kernel(const T* __restrict__ q, int n_heads, int n_kv, const T* __restrict__ kc,
                                                      const T* __restrict__ vc, KvAddr ka, const UttPlan* __restrict__ plan,
                                                      const int32_t* __restrict__ hist, T* __restrict__ ctx) {
  constexpr int HD = 128;
  extern __shared__ float qw_sc[];                       // [S_max] scores / probabilities
  __shared__ float qs[HD];
  __shared__ float red[2];
  const int b = blockIdx.x, h = blockIdx.y, tid = threadIdx.x, kvh = h / (n_heads / n_kv);
  const UttPlan p = plan[b];
  const int nq = p.T, row0 = p.row_off, h0 = hist[b];
  for (int t = 0; t < nq; ++t) {
    const int nk = h0 + t + 1;
    __syncthreads();
    qs[tid] = Elem<T>::load(q + (size_t)(row0 + t) * n_heads * HD + h * HD + tid);
    __syncthreads();
    float mx = -INFINITY;
    for (int s = tid; s < nk; s += 128) {
      const T* kr = kv_row(kc, ka, b, kvh, n_kv, s);
      float acc = 0.0f;
      for (int e = 0; e < HD; e += 8) {
        float kv8[8];
        load8<T>(kr + e, kv8);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = fmaf(qs[e + u], kv8[u], acc);
      }
      qw_sc[s] = acc;
      mx = fmaxf(mx, acc);
    }
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(red[0], red[1]);
    __syncthreads();
    float sum = 0.0f;
    for (int s = tid; s < nk; s += 128) { const float e = expf(qw_sc[s] - mx); qw_sc[s] = e; sum += e; }
    sum = wave_sum(sum);
    if ((tid & 63) == 0) red[tid >> 6] = sum;
    __syncthreads();
    const float inv = 1.0f / (red[0] + red[1]);
    float acc = 0.0f;
    for (int s = 0; s < nk; ++s) acc = fmaf(qw_sc[s], Elem<T>::load(kv_row(vc, ka, b, kvh, n_kv, s) + tid), acc);
    Elem<T>::store(ctx + (size_t)(row0 + t) * n_heads * HD + h * HD + tid, acc * inv);
  }
}

// sum over the 16 lanes of a DPP row in four VALU moves (xor 1, xor 2, mirror within 8, mirror within 16): no LDS-crossbar shuffles
__device__ __forceinline__ float dpp_sum16(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true));    // quad_perm [1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, true));    // quad_perm [2,3,0,1]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, true));   // row_half_mirror
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xf, 0xf, true));   // row_mirror
  return v;
}

// 8 consecutive elements of a cache row, kept raw in registers while the load is in flight
template <typename T> struct Raw8;
template <> struct Raw8<bf16_t> {
  uint4 r;
  __device__ __forceinline__ void load(const bf16_t* p) { r = *reinterpret_cast<const uint4*>(p); }
  __device__ __forceinline__ void unpack(float* o) const {
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[2 * e] = __uint_as_float(w[e] << 16); o[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u); }
  }
};
template <> struct Raw8<float> {
  float4 a, b;
  __device__ __forceinline__ void load(const float* p) { a = *reinterpret_cast<const float4*>(p); b = *reinterpret_cast<const float4*>(p + 4); }
  __device__ __forceinline__ void unpack(float* o) const { o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w; }
};

// One decode position per sequence, everything between the q|k|v GEMM and the o_proj GEMM in one launch: workgroup = (sequence,
// kv head), 4 waves. The cache rows of the first key block are requested before anything else, so the HBM round trip overlaps
// the new position's work -- per-head RMSNorm + RoPE of k (-> cache, LDS), v (-> cache, LDS) and of the group's q heads (-> LDS).
// Attention: 16 lanes share a key (8 head-dim elements each: one coalesced 256-byte row per 16 lanes), every 16-lane group keeps
// its own online soft-max state over keys s = 16 j + group, blocks of KPI keys per group are double-buffered in registers, and
// the 16 partial states merge through LDS. K and V are read once per kv head and serve the whole GQA group.
// BEAM: the sequences are beam-search hypotheses, `beam` rows per utterance. Positions below p0[b] (the prompt) are read from the
// utterance's prefill cache (kc_p / vc_p, shared by its rows: one HBM read serves the whole beam when the rows sit on one XCD -- see
// the workgroup order below); generated position p0[b] + j lives in slot j of the hypothesis cache kc / vc (S_max slots per row), in
// the row that wrote it on the hypothesis' ancestry, src[b][j] -- nothing is re-ordered between steps.
template <typename T, int G, bool BEAM = false>
__global__ __launch_bounds__(256) void qw_decode_attn_kernel(const float* __restrict__ qkv, int n_heads, int n_kv, const float* __restrict__ qn,
                                                             const float* __restrict__ kn, const float* __restrict__ rope, float eps,
                                                             const int32_t* __restrict__ hist, T* __restrict__ kc, T* __restrict__ vc, KvAddr ka,
                                                             T* __restrict__ ctx, const int32_t* __restrict__ src = nullptr, int ld_src = 0,
                                                             const int32_t* __restrict__ p0 = nullptr, const T* __restrict__ kc_p = nullptr,
                                                             const T* __restrict__ vc_p = nullptr, KvAddr kap = KvAddr{nullptr, 0, 0, 0}, int beam = 1) {
  constexpr int HD = 128, KPI = BEAM ? 2 : 4, NTASK = (2 + G + 3) / 4;     // (beam search: 5 x the workgroups -- fewer rows in flight per wave, 128 registers, four workgroups per CU instead of three)
  __shared__ float qsh[G][HD];
  __shared__ float knew[HD], vnew[HD];
  __shared__ float pm[16][G], pl[16][G];
  __shared__ float pacc[16][G][HD];
  int b = blockIdx.x, kvh = blockIdx.y;
  if constexpr (BEAM) {
    // 1-D grid. Consecutive workgroup ids go to consecutive XCDs: the `beam` rows of one (utterance, kv head) unit take ids that are
    // 8 apart, so they share an L2 and the prompt keys come from HBM once per unit. (Needs units % 8 == 0; plain order otherwise.)
    const int w = blockIdx.x, units = (gridDim.x / beam);
    int u, r;
    if (units % 8 == 0) { const int x = w & 7, q = w >> 3; u = (q / beam) * 8 + x; r = q % beam; }
    else { u = w / beam; r = w % beam; }
    b = (u / n_kv) * beam + r; kvh = u % n_kv;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pos = hist[b];                               // keys [0, pos) are in the cache; key pos is made here
  const int heads = n_heads + 2 * n_kv;
  const int base = BEAM ? p0[b] : 0;
  const int S_max = ka.S_max;
  // the sequence's slice of the block table goes to LDS once (one coalesced load): a lookup per 16-key block in front of every cache request would put a
  // dependent L2 round trip into each turn of the key loop (measured: + 4.5 us per launch, 1.64 -> 1.77 ms per token at 64 sequences)
  constexpr int PG_MAX = 256;
  __shared__ int32_t pg_sh[PG_MAX];
  const KvAddr& kt = BEAM ? kap : ka;                     // the paged part: the session's own cache, or (beam search) the utterance's prompt
  const int tb = BEAM ? b / beam : b, n_pg = kt.table ? min(((BEAM ? base : pos + 1) + 15) >> 4, PG_MAX) : 0;
  for (int i = threadIdx.x; i < n_pg; i += 256) pg_sh[i] = kt.table[(size_t)tb * kt.pps + i];
  if (n_pg) __syncthreads();
  auto paged_row = [&](auto* base_ptr, int s) {           // kv_row() through the LDS copy of the table
    const int pi = s >> 4;
    const int32_t page = pi < PG_MAX ? pg_sh[pi] : kt.table[(size_t)tb * kt.pps + pi];
    return base_ptr + (size_t)page * kt.page_stride + ((size_t)kvh * 16 + (s & 15)) * HD;
  };
  // BEAM: the hypothesis rows' caches are extents indexed by position, slot = position - base; the prompt is the utterance's prefill cache (extents or pages)
  T* K = BEAM ? kc + ((size_t)b * n_kv + kvh) * S_max * HD - (size_t)base * HD : nullptr;
  T* V = BEAM ? vc + ((size_t)b * n_kv + kvh) * S_max * HD - (size_t)base * HD : nullptr;
  const float* row = qkv + (size_t)b * heads * HD;
  const int lg = lane >> 4, li = lane & 15, gid = wave * 4 + lg;
  auto row_ptrs = [&](int s, const T*& kp, const T*& vp) {   // where position s of this sequence lives
    if constexpr (BEAM) {
      if (s < base) {
        if (kap.table) { kp = paged_row(kc_p, s); vp = paged_row(vc_p, s); }
        else { kp = kv_row(kc_p, kap, b / beam, kvh, n_kv, s); vp = kv_row(vc_p, kap, b / beam, kvh, n_kv, s); }
        return;
      }
      const ptrdiff_t o = (ptrdiff_t)(src[(size_t)b * ld_src + (s - base)] - b) * n_kv * S_max * HD + (ptrdiff_t)s * HD;
      kp = K + o; vp = V + o;
      return;
    }
    if (ka.table) { kp = paged_row(kc, s); vp = paged_row(vc, s); }
    else { kp = kv_row(kc, ka, b, kvh, n_kv, s); vp = kv_row(vc, ka, b, kvh, n_kv, s); }
  };
  T* k_new = BEAM ? K + (size_t)pos * HD : (ka.table ? paged_row(kc, pos) : kv_row(kc, ka, b, kvh, n_kv, pos));      // where this step's key / value go
  T* v_new = BEAM ? V + (size_t)pos * HD : (ka.table ? paged_row(vc, pos) : kv_row(vc, ka, b, kvh, n_kv, pos));
  // ---- requests: the new position's inputs first (L2), then the first block of cache rows (HBM)
  float x0[NTASK], x1[NTASK];
#pragma unroll
  for (int t = 0; t < NTASK; ++t) {
    const int task = wave + 4 * t;
    const int hh = task == 0 ? n_heads + kvh : task == 1 ? n_heads + n_kv + kvh : kvh * G + (task - 2);
    if (task < 2 + G) { x0[t] = row[hh * HD + lane]; x1[t] = row[hh * HD + lane + 64]; }
  }
  Raw8<T> kb[KPI], vb[KPI];
#pragma unroll
  for (int u = 0; u < KPI; ++u) {
    const int s = u * 16 + gid;
    if (s < pos) { const T *kp, *vp; row_ptrs(s, kp, vp); kb[u].load(kp + li * 8); vb[u].load(vp + li * 8); }
  }
  // ---- the new position: task 0 = k, 1 = v, 2.. = the group's q heads
  const float cs = rope[(size_t)pos * HD + lane], sn = rope[(size_t)pos * HD + 64 + lane];
#pragma unroll
  for (int t = 0; t < NTASK; ++t) {
    const int task = wave + 4 * t;
    if (task >= 2 + G) continue;
    T t0, t1;
    if (task == 1) {
      Elem<T>::store(&t0, x0[t]);
      Elem<T>::store(&t1, x1[t]);
      v_new[lane] = t0;
      v_new[lane + 64] = t1;
      vnew[lane] = Elem<T>::load(&t0);
      vnew[lane + 64] = Elem<T>::load(&t1);
      continue;
    }
    // the sum of squares in qw_qk_rope_kernel's association (a lane there adds four consecutive pairs as (p0 + p1) + (p2 + p3), then its sixteen lanes combine
    // by xor 8, 4, 2, 1 = element strides 32, 16, 8, 4) and with its explicit fmaf, so a fused step and an unfused one cache the same bits
    float ss = fmaf(x0[t], x0[t], x1[t] * x1[t]);
    ss += __shfl_xor(ss, 1, 64); ss += __shfl_xor(ss, 2, 64);
#pragma unroll
    for (int o = 32; o > 2; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const float r = rsqrtf(ss / (float)HD + eps);
    const float* w = task == 0 ? kn : qn;
    const float a0 = x0[t] * r * w[lane], a1 = x1[t] * r * w[lane + 64];
    Elem<T>::store(&t0, fmaf(a0, cs, -(a1 * sn)));       // through the operand dtype, like the unfused path
    Elem<T>::store(&t1, fmaf(a1, cs, a0 * sn));
    float* dst = task == 0 ? knew : qsh[task - 2];
    dst[lane] = Elem<T>::load(&t0);
    dst[lane + 64] = Elem<T>::load(&t1);
    if (task == 0) { k_new[lane] = t0; k_new[lane + 64] = t1; }
  }
  __syncthreads();
  float qr[G][8], m[G], l[G], acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -INFINITY; l[g] = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { qr[g][e] = qsh[g][li * 8 + e]; acc[g][e] = 0.0f; }
  }
  // one block of NB keys of this 16-lane group: all the dot products first (independent chains), one soft-max rescale per block
  auto block = [&](const float (*k8)[8], const float (*v8)[8], const bool* valid, auto nb_tag) {
    constexpr int NB = decltype(nb_tag)::value;
    float sc[NB][G];
#pragma unroll
    for (int u = 0; u < NB; ++u)
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float t = 0.0f;
#pragma unroll
        for (int e = 0; e < 8; ++e) t = fmaf(qr[g][e], k8[u][e], t);
        sc[u][g] = t;
      }
#pragma unroll
    for (int u = 0; u < NB; ++u)
#pragma unroll
      for (int g = 0; g < G; ++g) sc[u][g] = dpp_sum16(sc[u][g]);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float mn = m[g];
#pragma unroll
      for (int u = 0; u < NB; ++u) if (valid[u]) mn = fmaxf(mn, sc[u][g]);
      const float scale = m[g] == -INFINITY ? 0.0f : __expf(m[g] - mn);
      m[g] = mn;
      l[g] *= scale;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[g][e] *= scale;
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const float p = valid[u] ? __expf(sc[u][g] - mn) : 0.0f;
        l[g] += p;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[g][e] = fmaf(p, v8[u][e], acc[g][e]);
      }
    }
  };
  for (int s0 = 0; s0 < pos; s0 += 16 * KPI) {
    Raw8<T> kn2[KPI], vn2[KPI];
#pragma unroll
    for (int u = 0; u < KPI; ++u) {                      // next block's rows while this one is consumed
      const int s = s0 + (KPI + u) * 16 + gid;
      if (s < pos) { const T *kp, *vp; row_ptrs(s, kp, vp); kn2[u].load(kp + li * 8); vn2[u].load(vp + li * 8); }
    }
    float k8[KPI][8], v8[KPI][8];
    bool valid[KPI];
#pragma unroll
    for (int u = 0; u < KPI; ++u) {
      valid[u] = s0 + u * 16 + gid < pos;                // uniform per 16-lane group
      if (valid[u]) { kb[u].unpack(k8[u]); vb[u].unpack(v8[u]); }
      else {
#pragma unroll
        for (int e = 0; e < 8; ++e) { k8[u][e] = 0.0f; v8[u][e] = 0.0f; }
      }
    }
    block(k8, v8, valid, std::integral_constant<int, KPI>{});
#pragma unroll
    for (int u = 0; u < KPI; ++u) { kb[u] = kn2[u]; vb[u] = vn2[u]; }
  }
  {                                                      // the new key / value, from LDS (group 0 only)
    float k8[1][8], v8[1][8];
    const bool valid[1] = {gid == 0};
#pragma unroll
    for (int e = 0; e < 8; ++e) { k8[0][e] = knew[li * 8 + e]; v8[0][e] = vnew[li * 8 + e]; }
    block(k8, v8, valid, std::integral_constant<int, 1>{});
  }
  // ---- merge the 16 partial soft-max states
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (li == 0) { pm[gid][g] = m[g]; pl[gid][g] = l[g]; }
#pragma unroll
    for (int e = 0; e < 8; ++e) pacc[gid][g][li * 8 + e] = acc[g][e];
  }
  __syncthreads();
  for (int i = tid; i < G * HD; i += 256) {
    const int g = i / HD, e = i - g * HD;
    float mx = pm[0][g];
#pragma unroll
    for (int q = 1; q < 16; ++q) mx = fmaxf(mx, pm[q][g]);
    float num = 0.0f, den = 0.0f;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float w = __expf(pm[q][g] - mx);
      num = fmaf(pacc[q][g][e], w, num);
      den = fmaf(pl[q][g], w, den);
    }
    Elem<T>::store(ctx + (size_t)b * n_heads * HD + (kvh * G + g) * HD + e, num / den);
  }
}

}  // namespace

// ------------------------------------------------------------------------------------ the attention stage of a decoder layer (qwen_attn.h)
QwAttnForm qwen_attention_form(const QwAttnArgs& a) {
  const int G = a.H / a.KV;
  const bool fused_attn = a.step && (G == 1 || G == 2 || G == 4) && !a.no_fuse;
  if (fused_attn) return a.beam_src ? QW_ATTN_FUSED_BEAM : QW_ATTN_FUSED_DECODE;
  const bool mfma_attn = a.bf16 && !a.step && a.n_qb > 0;
  return mfma_attn ? QW_ATTN_ROPE_MFMA : QW_ATTN_ROPE_SCALAR;
}

template <typename T>
const char* launch_qwen_attention(const QwAttnArgs& a, Profiler& prof, hipStream_t stream) {
  const int H = a.H, KV = a.KV, B = a.B, rows = a.rows, hd = 128, G = H / KV;
  const float* qkv = a.qkv;
  const int32_t* hist = a.hist;
  T *q = (T*)a.q, *kc = (T*)a.kc, *vc = (T*)a.vc, *ctx = (T*)a.ctx;
  const KvAddr ka = a.ka;
  const QwAttnForm form = qwen_attention_form(a);
  if (form == QW_ATTN_FUSED_DECODE || form == QW_ATTN_FUSED_BEAM) {
    ProfScope ps(prof, "dec_attn", stream);
    const size_t lds = 0;
    if (a.beam_src) {
      const T *kc_p = (const T*)a.kc_p, *vc_p = (const T*)a.vc_p;
      const KvAddr kap = a.kap;
      if (G == 1) hipLaunchKernelGGL((qw_decode_attn_kernel<T, 1, true>), dim3(B * KV), dim3(256), lds, stream, qkv, H, KV, a.qn, a.kn, a.rope, a.eps, hist, kc, vc, ka, ctx, a.beam_src, a.ld_src, a.beam_p0, kc_p, vc_p, kap, a.beam);
      else if (G == 2) hipLaunchKernelGGL((qw_decode_attn_kernel<T, 2, true>), dim3(B * KV), dim3(256), lds, stream, qkv, H, KV, a.qn, a.kn, a.rope, a.eps, hist, kc, vc, ka, ctx, a.beam_src, a.ld_src, a.beam_p0, kc_p, vc_p, kap, a.beam);
      else hipLaunchKernelGGL((qw_decode_attn_kernel<T, 4, true>), dim3(B * KV), dim3(256), lds, stream, qkv, H, KV, a.qn, a.kn, a.rope, a.eps, hist, kc, vc, ka, ctx, a.beam_src, a.ld_src, a.beam_p0, kc_p, vc_p, kap, a.beam);
      return G == 1 ? "beam_g1" : G == 2 ? "beam_g2" : "beam_g4";
    }
    if (G == 1) hipLaunchKernelGGL((qw_decode_attn_kernel<T, 1, false>), dim3(B, KV), dim3(256), lds, stream, qkv, H, KV, a.qn, a.kn, a.rope, a.eps, hist, kc, vc, ka, ctx, (const int32_t*)nullptr, 0, (const int32_t*)nullptr, (const T*)nullptr, (const T*)nullptr, KvAddr{nullptr, 0, 0, 0}, 1);
    else if (G == 2) hipLaunchKernelGGL((qw_decode_attn_kernel<T, 2, false>), dim3(B, KV), dim3(256), lds, stream, qkv, H, KV, a.qn, a.kn, a.rope, a.eps, hist, kc, vc, ka, ctx, (const int32_t*)nullptr, 0, (const int32_t*)nullptr, (const T*)nullptr, (const T*)nullptr, KvAddr{nullptr, 0, 0, 0}, 1);
    else hipLaunchKernelGGL((qw_decode_attn_kernel<T, 4, false>), dim3(B, KV), dim3(256), lds, stream, qkv, H, KV, a.qn, a.kn, a.rope, a.eps, hist, kc, vc, ka, ctx, (const int32_t*)nullptr, 0, (const int32_t*)nullptr, (const T*)nullptr, (const T*)nullptr, KvAddr{nullptr, 0, 0, 0}, 1);
    return G == 1 ? "fused_g1" : G == 2 ? "fused_g2" : "fused_g4";
  }
  const bool mfma_attn = form == QW_ATTN_ROPE_MFMA;
  { ProfScope ps(prof, "dec_rope", stream);
    const int units = rows * (H + 2 * KV);           // sixteen lanes each
    hipLaunchKernelGGL(qw_qk_rope_kernel<T>, dim3((units + 15) / 16), dim3(256), 0, stream, qkv, H, KV, a.qn, a.kn, a.rope, a.eps, a.row_seq, a.row_t,
                       hist, rows, q, kc, vc, ka, mfma_attn ? (T*)a.k_rows : (T*)nullptr); }
  ProfScope ps(prof, "dec_attn", stream);
  if (mfma_attn) {
    AttnArgs aa; aa.q = q; aa.ld_q = H * hd; aa.k = a.k_rows; aa.ld_qk = KV * hd; aa.vt = a.vt; aa.ld_vt = a.ld_vt; aa.ctx = ctx; aa.ld_ctx = H * hd;
    aa.plan = a.plan; aa.qb_utt = a.qb_utt; aa.qb_q0 = a.qb_q0; aa.n_qblocks = a.n_qb; aa.n_heads = H; aa.qt = a.qt; aa.n_waves = a.nw; aa.max_T = a.max_T;
    aa.causal = 1; aa.kv_group = G;
    launch_attention_bf16_hd128(aa, stream);
    return "rope_mfma";
  }
  hipLaunchKernelGGL(qw_attn_kernel<T>, dim3(B, H), dim3(128), (size_t)a.S * 4, stream, q, H, KV, kc, vc, ka, a.plan, hist, ctx);
  return "rope_scalar";
}
template const char* launch_qwen_attention<float>(const QwAttnArgs&, Profiler&, hipStream_t);
template const char* launch_qwen_attention<bf16_t>(const QwAttnArgs&, Profiler&, hipStream_t);

namespace {

// decoder input rows: src >= 0 -> embedding of token src; src < 0 -> audio embedding row -1 - src; pad rows are zero
template <typename T>
__global__ void qw_gather_prompt_kernel(const int32_t* __restrict__ src, const T* __restrict__ embed, const float* __restrict__ audio, int d,
                                        int32_t pad_marker, float* __restrict__ x, T* __restrict__ x_lo) {
  const int row = blockIdx.x, s = src[row];
  float* o = x + (size_t)row * d;
  for (int c = threadIdx.x; c < d; c += blockDim.x) {
    const float v = s == pad_marker ? 0.0f : (s >= 0 ? Elem<T>::load(embed + (size_t)s * d + c) : audio[(size_t)(-1 - s) * d + c]);
    o[c] = v;
    if (x_lo) Elem<T>::store(x_lo + (size_t)row * d + c, v);
  }
}

// cap: a finished sequence that generate() keeps stepping beside unfinished ones stops advancing at the last cache slot (its outputs are
// ignored; rows that still matter never reach the cap -- the host checks them before every step)
__global__ void qw_hist_add_kernel(int32_t* __restrict__ hist, const UttPlan* __restrict__ plan, int B, int cap) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) hist[b] = min(hist[b] + plan[b].T, cap);
}

// ------------------------------------------------------------------------------------ forced-aligner head
// Row selection of asr_qwen_align (Inference_Qwen_ForcedAligner_ONNX.py:565-567 gathers the positions whose prompt id is <timestamp>): one workgroup
// per utterance over its prompt rows [row_off, row_off + T) of the packed decoder layout; `tid` < 0 selects every position (the graph's output_ids).
__device__ __forceinline__ bool qw_slot_hit(const int32_t* src, int row, int tid) { return tid < 0 || src[row] == tid; }

__global__ __launch_bounds__(256) void qw_slot_count_kernel(const int32_t* __restrict__ src, const UttPlan* __restrict__ plan, int tid, int32_t* __restrict__ cnt) {
  __shared__ int total;
  const UttPlan p = plan[blockIdx.x];
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  int n = 0;
  for (int t = threadIdx.x; t < p.T; t += 256) n += qw_slot_hit(src, p.row_off + t, tid) ? 1 : 0;
  atomicAdd(&total, n);
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

// utterance b's slots go to rows[off[b] ...] in position order, off[b] = sum of the counts before it; writes stop at `cap` (the host's count)
__global__ __launch_bounds__(256) void qw_slot_compact_kernel(const int32_t* __restrict__ src, const UttPlan* __restrict__ plan, int tid,
                                                              const int32_t* __restrict__ cnt, int B, int cap, int32_t* __restrict__ off,
                                                              int32_t* __restrict__ rows) {
  __shared__ int base_sh, wave_n[4];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) base_sh = 0;
  __syncthreads();
  int s = 0;
  for (int i = threadIdx.x; i < b; i += 256) s += cnt[i];
  atomicAdd(&base_sh, s);
  __syncthreads();
  int base = base_sh;
  if (threadIdx.x == 0) { off[b] = base; if (b == B - 1) off[B] = base + cnt[b]; }
  const UttPlan p = plan[b];
  for (int t0 = 0; t0 < p.T; t0 += 256) {
    const int t = t0 + threadIdx.x;
    const bool hit = t < p.T && qw_slot_hit(src, p.row_off + t, tid);
    const unsigned long long m = __ballot(hit);
    if (lane == 0) wave_n[wave] = __popcll(m);
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += wave_n[w];
    const int at = base + before + __popcll(m & ((1ull << lane) - 1ull));
    if (hit && at < cap) rows[at] = p.row_off + t;
    base += wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
    __syncthreads();                                     // (wave_n is rewritten by the next block of rows)
  }
}

// ------------------------------------------------------------------------------------ beam search
// Width-`beam` search over summed log-probabilities (README.md:38 names a beam mode for Qwen3-ASR; the reference ships no code for it, the
// semantics are those of oracle/qwen_asr_oracle.py:beam_search_core). Hypotheses of utterance b are the decoder rows b * beam + r. The
// ranking kernels (launch_beam_topk / launch_beam_select) live in kernels.hip: the Whisper session ranks its hypotheses with them too.
__global__ void qw_beam_init_kernel(const int32_t* __restrict__ hist_in, int B, int beam, int32_t* __restrict__ hist_out, int32_t* __restrict__ p0) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n < B * beam) { hist_out[n] = hist_in[n / beam]; p0[n] = hist_in[n / beam]; }
}

// ------------------------------------------------------------------------------------ session
struct QwEncLayer { const void *wqkv, *wo, *w1, *w2; const float *bqkv, *bo, *b1, *b2; };
struct QwDecLayer { const void *wqkv, *wo, *gate_up, *down; const float *qn, *kn; };

// one decoder pass: the packed rows (T new positions per sequence) and, for the bf16 prefill, the MFMA attention geometry
struct DecPass {
  const UttPlan* plan = nullptr; const int32_t *row_seq = nullptr, *row_t = nullptr, *last_rows = nullptr;
  int rows = 0, B = 0; bool step = false, hist_done = false;   // hist_done: the history counters were advanced already
  const int32_t *qb_utt = nullptr, *qb_q0 = nullptr; int n_qb = 0, qt = 0, nw = 0, max_T = 0, ld_vt = 0;
  // beam search: the rows are hypotheses with their own cache (slot stride S), history counters and generated-slot ancestry table
  void *kc = nullptr, *vc = nullptr; int S = 0; int32_t* hist = nullptr; const int32_t *beam_src = nullptr, *beam_p0 = nullptr; int ld_src = 0, beam = 1;
  bool head = true;        // false: stop after the last layer (the forced aligner runs its own head on selected rows)
};

// asr_qwen_align's head request: row selection + host outputs
struct AlignReq { int32_t tid = -1; int32_t* slot_off = nullptr; int32_t* buckets = nullptr; int64_t cap = 0; float* logits = nullptr; };

struct QwSession : asr_session {
  asr_qwen_config cfg;
  int vpad = 0, hpad = 0, cpad = 0, chunk = 0, cpw = 0, rpw = 0, t_tok = 13;
  std::vector<QwEncLayer> enc;
  std::vector<QwDecLayer> dec;
  FrontEnd fe;
  const float *conv1_b = nullptr, *conv2_b = nullptr, *conv3_b = nullptr, *enc_pos = nullptr,
              *proj1_b = nullptr, *proj2_b = nullptr, *rope = nullptr, *final_norm = nullptr;
  const void *conv1_w = nullptr, *conv2_w = nullptr, *conv3_w = nullptr, *conv_out_w = nullptr, *proj1_w = nullptr, *proj2_w = nullptr,
             *embed = nullptr, *lm_head = nullptr;
  int batch = 0;
  std::vector<int> seq_len;                              // positions in the cache per sequence (host mirror)
  DeviceBuffer d_plan, d_audio, d_mel, d_blkmax, d_feat, d_col, d_c1, d_c2, d_c3, d_xa, d_xb, d_h, d_qk, d_vt, d_ctx, d_ffn, d_aud_out;
  std::vector<char> frozen;      // generate(): finished sequences, allowed to sit at max_seq_len while the others go on
  DeviceBuffer d_dplan, d_x, d_x2, d_dh, d_qkv, d_q, d_dctx, d_act, d_last, d_logits, d_next, d_kc, d_vc, d_hist, d_stepplan, d_vt2, d_krows, d_xlo, d_x2lo;
  bool no_fuse = false, use_graph = true;
  // precision mode ASR_PRECISION_FP8W (opt-in; everything else as in bf16 mode; the MI355X counterpart of the reference's q4f32 / q8f32 decoders, README.md:70,
  // Optimize_ONNX_Common.py:27,55-60): the four projections of every decoder layer as e4m3 bytes with one power-of-two scale per output row, streamed by the
  // weight-streaming GEMM of the decode step (<= 64 rows; gemm.hip: gemm_bf16_skinny<.., W8>); their exact bf16 dequantisation serves every other path (prefill, beam
  // search above 64 rows), so all steps of a session see the same effective weights. ASR_FP8_FAKE=1: same quantisation, bf16 kernels throughout (the tests' exact twin).
  bool fp4 = false;                    // precision mode ASR_PRECISION_MXFP4W: the four projections as OCP MXFP4 (nibbles in d_w8, e8m0 block scales in d_wscale) instead of e4m3
  bool fp8 = false, fp8_fake = false;
  bool use_decode_gemm = true;         // ASR_QWEN_DECODE_GEMM=0: o_proj / down_proj of a decode step through the tiled split-K pass + reduce launch (rounds 1-4) instead of csrc/decode_gemm.hip
  LowBitWeights dec8;                  // wqkv, wo, gate_up, down of every decoder layer
  // ---- paged KV cache (the default; ASR_QWEN_KV_PAGED=0 and the persistent decode kernel keep extents). Pool [page][layer][kv head][16][128] for K and for V,
  // one block table [sequence][pps] for all layers, a free list on the host: a sequence holds pages for the positions it has, gets one more when it crosses a
  // page boundary, and gives all of them back the step after it finishes (its table row then points at page 0, a scratch page nobody reads meaningfully).
  bool kv_paged = true, kv_shuffle = false;
  int kv_pps = 0, kv_pool_pages = 0, kv_high_water = 0;
  std::vector<int32_t> kv_free, kv_table;                 // free page ids (LIFO); host mirror of the block table
  std::vector<std::vector<int32_t>> kv_owned;             // pages of every sequence, in position order
  std::vector<char> kv_released;
  DeviceBuffer d_kvtab;
  PinnedBuffer h_kvtab;
  bool kv_table_dirty = false;
  size_t kv_page_elems() const { return (size_t)cfg.n_layers * cfg.n_kv_heads * 16 * cfg.d_head; }
  void kv_begin(int B, const std::vector<int>& lens, size_t eT);
  void kv_prepare_step(size_t eT);
  int kv_take(size_t eT);
  void kv_upload();
  KvAddr kv_addr() const {
    if (kv_paged) return KvAddr{d_kvtab.as<int32_t>(), kv_pps, kv_page_elems(), cfg.max_seq_len};
    return KvAddr{nullptr, 0, 0, cfg.max_seq_len};
  }
  TokenHead head;                      // decode head (Inference_Qwen_ASR_ONNX.py:369-376) + the history of generated ids [B][max_seq_len]
  DeviceBuffer d_sel, d_amax_v, d_amax_i, d_bucket;      // forced-aligner head: counts / offsets / rows, arg-max partials, buckets
  DeviceBuffer d_bkc, d_bvc, d_bhist, d_bp0, d_bplan;    // beam search: the hypothesis rows' caches, counters and row plan; scores and tables are the ranker's
  BeamRanker ranker;
  StepGraph dec_graph;
  PinnedBuffer h_plan, h_stepplan, h_io, h_ids;
  SplitKGemm sk;
  void gemm(const GemmArgs& g) { sk.run(g, precision, stream); }
  // the plan of a pass with one row per sequence (a decode step, a beam step over hypothesis rows): uploaded into `dev`, staged in h_stepplan
  DecPass step_plan(DeviceBuffer& dev, int rows);
  DecPass step_pass;                   // ... of the decode steps that follow a prefill
  void init();
  bool aligner() const { return cfg.classify_num > 0; }
  template <typename T> void prefill(const void* audio, int audio_mem, const int64_t* offs, int B, const int32_t* pre_ids, const int32_t* pre_off,
                                     const int32_t* post_ids, const int32_t* post_off, int32_t* next_out, float* logits_out, int32_t* ids_len_out,
                                     const AlignReq* al = nullptr);
  template <typename T> void align_head(int B, const UttPlan* ddp, const int32_t* d_src, int n_sel, const AlignReq& al);
  template <typename T> void decoder_pass(const DecPass& P);
  template <typename T> void logits_head(const DecPass& P);
  template <typename T> void step(const int32_t* ids_host, int32_t* next_out, float* logits_out);
  void finish(int B, int32_t* next_out, float* logits_out, bool sync);
  template <typename T> void beam_search(int beam, int max_new, const int32_t* stop_ids, int n_stop, int32_t* tokens_out, int32_t* n_out, float* scores_out);
};

void QwSession::init() {
  const auto& c = cfg;
  ASR_REQUIRE(c.nfft == 400 && c.hop_length == 160 && c.n_mels == 128, "qwen: front-end is built for n_fft 400 / hop 160 / 128 mels");
  ASR_REQUIRE(c.d_head == 128 && c.n_heads % c.n_kv_heads == 0, "qwen: decoder head_dim must be 128");
  ASR_REQUIRE(c.enc_d % 128 == 0 && c.enc_d / c.enc_heads == 64 && c.enc_ffn % 128 == 0, "qwen: encoder needs 64-wide heads and widths that are multiples of 128");
  ASR_REQUIRE(c.d_model % 128 == 0 && c.d_ffn % 64 == 0 && (2 * c.d_ffn) % 128 == 0, "qwen: decoder widths must be multiples of 128");
  ASR_REQUIRE(c.n_window == 50, "qwen: the conv stem is built for 100-frame chunks (n_window 50)");
  chunk = 2 * c.n_window;
  cpw = c.n_window_infer / chunk;
  rpw = round_up(cpw * t_tok, 16);
  ASR_REQUIRE(cpw >= 1 && rpw <= 1024, "qwen: bad attention window");
  vpad = round_up(c.vocab, 128);
  head.init(c.max_seq_len, 1, 10, 1024);
  head.prof = &prof; ranker.prof = &prof;
  ASR_REQUIRE(c.classify_num >= 0, "qwen: classify_num %d", c.classify_num);
  hpad = aligner() ? round_up(c.classify_num, 128) : vpad;   // rows of dec.lm_head: the vocabulary, or the aligner's timestamp buckets
  cpad = round_up(c.conv_channels, 128);
  fe.init(c.nfft, c.nfft, c.hop_length, c.n_mels, 1, 1e-10f);
  model_rate = c.sample_rate;
  const int wt = precision == ASR_PRECISION_BF16 ? ARENA_BF16 : ARENA_F32;
  const int de = c.enc_d, d = c.d_model, qkvn = (c.n_heads + 2 * c.n_kv_heads) * c.d_head;
  auto F = [&](const std::string& n, std::initializer_list<int64_t> sh) { return (const float*)arena.get(n, ARENA_F32, sh).ptr; };
  auto W = [&](const std::string& n, std::initializer_list<int64_t> sh) { return arena.get(n, wt, sh).ptr; };
  fe.dft = F("fe.dft", {(int64_t)fe.n_bin_tiles * 2 * fe.n_kchunks * 64 * 4});
  fe.melp = F("fe.mel", {(int64_t)(c.n_mels / 16) * fe.n_bin_tiles * 64 * 4});
  conv1_w = W("enc.conv1_w", {cpad, 64});          conv1_b = F("enc.conv1_b", {cpad});
  conv2_w = W("enc.conv2_w", {cpad, 9 * cpad});    conv2_b = F("enc.conv2_b", {cpad});
  conv3_w = W("enc.conv3_w", {cpad, 9 * cpad});    conv3_b = F("enc.conv3_b", {cpad});
  conv_out_w = W("enc.conv_out_w", {de, 16 * cpad});
  enc_pos = F("enc.pos", {t_tok, de});
  enc.resize(c.n_enc_layers);
  for (int i = 0; i < c.n_enc_layers; ++i) {
    const std::string q = "enc" + std::to_string(i) + ".";
    enc[i] = {W(q + "wqkv", {3 * de, de}), W(q + "wo", {de, de}), W(q + "w1", {c.enc_ffn, de}), W(q + "w2", {de, c.enc_ffn}),
              F(q + "bqkv", {3 * de}), F(q + "bo", {de}), F(q + "b1", {c.enc_ffn}), F(q + "b2", {de})};
  }
  proj1_w = W("enc.proj1_w", {de, de});   proj1_b = F("enc.proj1_b", {de});
  proj2_w = W("enc.proj2_w", {d, de});    proj2_b = F("enc.proj2_b", {d});
  embed = W("dec.embed", {vpad, d});
  lm_head = W("dec.lm_head", {hpad, d});
  rope = F("dec.rope", {c.max_seq_len, c.d_head});             // [position][cos(64) | sin(64)] (ROTARY_MASK_PREFILL tables, :933-1002)
  final_norm = F("dec.final_norm", {d});
  dec.resize(c.n_layers);
  for (int i = 0; i < c.n_layers; ++i) {
    const std::string q = "dec" + std::to_string(i) + ".";
    dec[i] = {W(q + "wqkv", {qkvn, d}), W(q + "wo", {d, c.n_heads * c.d_head}), W(q + "gate_up", {2 * c.d_ffn, d}), W(q + "down", {d, c.d_ffn}),
              F(q + "qn", {c.d_head}), F(q + "kn", {c.d_head})};
  }
  if (fp8) {
    const int I = c.d_ffn, od = c.n_heads * c.d_head;
    ASR_REQUIRE(d % 256 == 0 && I % 256 == 0 && od % 256 == 0, "qwen: FP8 mode needs d_model, d_ffn and heads x head_dim to be multiples of 256");
    dec8.build(c.n_layers, fp4, [&](int i) {
      QwDecLayer& L = dec[i];
      return std::vector<LowBitWeights::Slot>{{&L.wqkv, qkvn, d}, {&L.wo, d, od}, {&L.gate_up, 2 * I, d}, {&L.down, d, I}};
    }, stream);
    HIP_CHECK(hipStreamSynchronize(stream));
  }
}

// ---- paged KV cache: host side
void QwSession::kv_upload() {
  if (!kv_table_dirty) return;
  const size_t bytes = kv_table.size() * 4;
  h_kvtab.reserve(bytes);
  int32_t* st = h_kvtab.as<int32_t>();
  memcpy(st, kv_table.data(), bytes);
  HIP_CHECK(hipMemcpyAsync(d_kvtab.ptr, st, bytes, hipMemcpyHostToDevice, stream));
  HIP_CHECK(hipStreamSynchronize(stream));               // (the staging buffer is reused by the next change)
  kv_table_dirty = false;
}
// one free page; the pool doubles when the list is empty (page-major layout: the old pool is a prefix of the new one)
int QwSession::kv_take(size_t eT) {
  if (kv_free.empty()) {
    const int old_pages = kv_pool_pages, new_pages = std::max(2 * old_pages, old_pages + 64);
    DeviceBuffer nk, nv;
    nk.reserve((size_t)new_pages * kv_page_elems() * eT, stream);
    nv.reserve((size_t)new_pages * kv_page_elems() * eT, stream);
    HIP_CHECK(hipMemcpyAsync(nk.ptr, d_kc.ptr, (size_t)old_pages * kv_page_elems() * eT, hipMemcpyDeviceToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(nv.ptr, d_vc.ptr, (size_t)old_pages * kv_page_elems() * eT, hipMemcpyDeviceToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    d_kc = std::move(nk); d_vc = std::move(nv);           // (the decode graph is keyed on these pointers: it is captured again)
    for (int p = new_pages - 1; p >= old_pages; --p) kv_free.push_back(p);
    kv_pool_pages = new_pages;
  }
  const int p = kv_free.back();
  kv_free.pop_back();
  kv_high_water = std::max(kv_high_water, kv_pool_pages - (int)kv_free.size());
  return p;
}
// a new batch: every page back to the list, then pages for the prompts (+ the first generated position)
void QwSession::kv_begin(int B, const std::vector<int>& lens, size_t eT) {
  const auto& c = cfg;
  kv_pps = (c.max_seq_len + 15) / 16;
  // pages of a prompt + the first generated position, never more than a sequence can hold: a prompt of exactly max_seq_len positions (prefill accepts it)
  // has no next position to reserve -- (S + 16) / 16 would be kv_pps + 1 and the fill loop would write one entry past the sequence's table row
  auto prompt_pages = [&](int len) { return std::min((len + 1 + 15) / 16, kv_pps); };
  int need = 1;
  for (int b = 0; b < B; ++b) need += prompt_pages(lens[b]);
  if (need > kv_pool_pages) {                             // nothing to keep across batches: a fresh pool
    d_kc.release(); d_vc.release();
    d_kc.reserve((size_t)need * kv_page_elems() * eT, stream);
    d_vc.reserve((size_t)need * kv_page_elems() * eT, stream);
    kv_pool_pages = need;
  }
  kv_free.clear();
  for (int p = kv_pool_pages - 1; p >= 1; --p) kv_free.push_back(p);          // page 0: the scratch page of finished sequences
  if (kv_shuffle) {                                       // tests: hand the pages out in a scrambled order
    uint64_t x = 0x9e3779b97f4a7c15ull;
    for (size_t i = kv_free.size(); i > 1; --i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; std::swap(kv_free[i - 1], kv_free[x % i]); }
  }
  kv_table.assign((size_t)B * kv_pps, 0);
  kv_owned.assign(B, {});
  kv_released.assign(B, 0);
  kv_high_water = 0;
  for (int b = 0; b < B; ++b)
    for (int j = 0; j < prompt_pages(lens[b]); ++j) { const int p = kv_take(eT); kv_owned[b].push_back(p); kv_table[(size_t)b * kv_pps + j] = p; }
  d_kvtab.reserve(kv_table.size() * 4, stream);
  kv_table_dirty = true;
  kv_upload();
}
// before a decode step: finished sequences give their pages back (their row points at the scratch page from now on), the others get a page when the position
// this step writes opens a new one
void QwSession::kv_prepare_step(size_t eT) {
  if (!kv_paged) return;
  for (int b = 0; b < batch; ++b) {
    const bool fz = b < (int)frozen.size() && frozen[b];
    if (fz) {
      if (!kv_released[b]) {
        for (int p : kv_owned[b]) kv_free.push_back(p);
        kv_owned[b].clear();
        for (int j = 0; j < kv_pps; ++j) kv_table[(size_t)b * kv_pps + j] = 0;
        kv_released[b] = 1;
        kv_table_dirty = true;
      }
      continue;
    }
  }
  // a sequence whose next position opens a page it does not own triggers a refill for EVERY running sequence up to two pages past its position: the table
  // changes (and is uploaded) about every 16 steps, not every time one of 64 sequences crosses a boundary
  bool need = false;
  for (int b = 0; b < batch; ++b)
    need = need || (!kv_released[b] && (seq_len[b] >> 4) >= (int)kv_owned[b].size());
  if (need) {
    for (int b = 0; b < batch; ++b) {
      if (kv_released[b]) continue;
      const int upto = std::min((seq_len[b] + 32) >> 4, kv_pps - 1);
      while ((int)kv_owned[b].size() <= upto) {
        const int p = kv_take(eT);
        kv_table[(size_t)b * kv_pps + kv_owned[b].size()] = p;
        kv_owned[b].push_back(p);
      }
    }
    kv_table_dirty = true;
  }
  kv_upload();
}

// one pass of the decoder stack over `rows` packed rows described by `plan` (T new positions per sequence, appended at hist[b])
template <typename T>
void QwSession::decoder_pass(const DecPass& P) {
  const auto& c = cfg;
  const int d = c.d_model, H = c.n_heads, KV = c.n_kv_heads, hd = c.d_head, I = c.d_ffn, qkvn = (H + 2 * KV) * hd, S = P.S ? P.S : c.max_seq_len;
  const int rows = P.rows, B = P.B;
  const bool bf = precision == ASR_PRECISION_BF16;
  float* x = d_x.as<float>();
  float* x2 = d_x2.as<float>();
  T* h = d_dh.as<T>();
  float* qkv = d_qkv.as<float>();
  T* q = d_q.as<T>();
  T* ctx = d_dctx.as<T>();
  T* act = d_act.as<T>();
  // the session's own cache is paged (per-layer offset inside a page) or extents; beam hypothesis caches (P.kc) are always extents of S slots
  const bool own_paged = kv_paged && !P.kc;
  const size_t layer_kv = own_paged ? (size_t)KV * 16 * hd : (size_t)B * KV * S * hd;
  const KvAddr ka = own_paged ? kv_addr() : KvAddr{nullptr, 0, 0, S};
  const int32_t* hist = P.hist ? P.hist : d_hist.as<int32_t>();
  // single-position steps of small batches (bf16): RMSNorm(x) W^T = rstd(x) (x W^T) -- the weight-streaming GEMM reads the raw residual
  // rows (bf16 copy written by the producing GEMM), sums x^2 from the fragments it streams anyway and scales its output rows
  const bool rms_in_gemm = P.step && bf && rows <= 64 && d % 256 == 0 && !no_fuse;
  const bool norm_in_reduce = bf && !rms_in_gemm && !no_fuse && d == 1024;
  const bool w8 = fp8 && !fp8_fake && rms_in_gemm;           // byte weights: the weight-streaming launches of a decode step
  auto bytes_of = [&](GemmArgs& g, int layer, int wi) {
    if (!w8) return;
    dec8.select(g, layer, wi);
    if (!fp4) g.ldw8 = g.K;
  };
  // o_proj / down_proj of a decode step (<= 64 rows, + residual, f32 and bf16 copies of the stream): the decode GEMM of csrc/decode_gemm.hip -- K split across workgroups
  // with the hand-over inside the launch -- instead of the tiled split-K pass and its reduce launch (6.3 + 4.8 us per projection at 64 rows)
  // (the decode GEMM has its own shape limits -- K % 32, K >= 256, 16-byte rows: a geometry outside them keeps the tiled pass)
  auto dgm_shape_ok = [&](int K, int lda) {
    DecGemmArgs a;
    a.A = (const bf16_t*)ctx; a.lda = lda; a.W = (const bf16_t*)ctx; a.ldw = K; a.M = rows; a.N = d; a.K = K;
    // (a shape question without a layer: stand-in pointers, not dec8.select)
    if (w8 && fp4) { a.W = nullptr; a.W4 = (const unsigned char*)ctx; a.w_scale4 = (const unsigned char*)ctx; }
    else if (w8) { a.W = nullptr; a.W8 = (const unsigned char*)ctx; a.w_scale = (const float*)ctx; }
    return decode_gemm_supported(a);
  };
  const bool dgm = rms_in_gemm && use_decode_gemm && dgm_shape_ok(H * hd, H * hd) && dgm_shape_ok(I, I);
  auto dg = [&](const T* A, int lda, const void* Wt, int layer, int wi, int N, int K, const float* add, float* of32, T* olo) {
    ProfScope ps(prof, "dec_gemm", stream);
    sk.ensure(stream);
    DecGemmArgs a;
    a.A = (const bf16_t*)A; a.lda = lda; a.W = (const bf16_t*)Wt; a.ldw = K; a.M = rows; a.N = N; a.K = K;
    if (w8) { a.W = nullptr; dec8.select(a, layer, wi); }
    a.add = add; a.ld_add = d; a.out_f32 = of32; a.ld_out_f32 = d; a.out_lo = (bf16_t*)olo; a.ld_out_lo = d;
    a.ws = sk.ws.as<float>(); a.ws_bytes = SplitKGemm::WS_BYTES; a.cnt = sk.cnt.as<int32_t>();
    launch_decode_gemm(a, stream);
  };
  auto can_norm = [&](const GemmArgs& g0) { return gemm_reduce_can_norm(sk.attach(g0, stream)); };     // (the session's gemm() adds the split-K workspace: ask with it in place)
  T* xlo = d_xlo.as<T>();
  T* x2lo = d_x2lo.as<T>();
  // 65+ rows (beam search, prefill of short prompts): o_proj / down_proj take the tiled split-K pass; its reduce launch then also writes
  // RMSNorm(row) as the operand rows of the next projection (GemmArgs.rms_out), so the stand-alone RMSNorm launches disappear
  bool h_is_norm = false;                     // `h` already holds RMSNorm of the stream the next normed_gemm will ask for
  auto normed_gemm = [&](const float* src, const T* src_lo, GemmArgs& g) {          // g = RMSNorm(src) W^T
    if (rms_in_gemm) { g.A = src_lo; g.lda = d; g.a_rms_eps = c.rms_eps; }
    else if (h_is_norm) { g.A = h; g.lda = d; h_is_norm = false; }
    else {
      ProfScope ps(prof, "dec_norm", stream);
      hipLaunchKernelGGL(qw_rmsnorm_kernel<T>, dim3((rows + 3) / 4), dim3(256), 0, stream, src, d, rows, d, (const float*)nullptr, c.rms_eps, h, d, (const int32_t*)nullptr);
      g.A = h; g.lda = d;
    }
    ProfScope ps(prof, "dec_gemm", stream);
    gemm(g);
  };
  for (int i = 0; i < c.n_layers; ++i) {
    const QwDecLayer& L = dec[i];
    T* kc = (P.kc ? (T*)P.kc : d_kc.as<T>()) + (size_t)i * layer_kv;
    T* vc = (P.vc ? (T*)P.vc : d_vc.as<T>()) + (size_t)i * layer_kv;
    { GemmArgs g; g.W = L.wqkv; g.ldw = d; g.M = rows; g.N = qkvn; g.K = d; g.out_f32 = qkv; g.ld_out_f32 = qkvn; bytes_of(g, i, 0); normed_gemm(x, xlo, g); }
    QwAttnArgs at;
    at.bf16 = bf; at.step = P.step; at.no_fuse = no_fuse;
    at.qkv = qkv; at.rows = rows; at.B = B; at.H = H; at.KV = KV; at.qn = L.qn; at.kn = L.kn; at.rope = rope; at.eps = c.rms_eps;
    at.hist = hist; at.row_seq = P.row_seq; at.row_t = P.row_t; at.plan = P.plan;
    at.q = q; at.kc = kc; at.vc = vc; at.ctx = ctx; at.ka = ka; at.S = S;
    at.k_rows = d_krows.ptr; at.vt = d_vt2.ptr; at.ld_vt = P.ld_vt;
    at.qb_utt = P.qb_utt; at.qb_q0 = P.qb_q0; at.n_qb = P.n_qb; at.qt = P.qt; at.nw = P.nw; at.max_T = P.max_T;
    if (P.beam_src) {
      const size_t prompt_kv = kv_paged ? (size_t)KV * 16 * hd : (size_t)(B / P.beam) * KV * c.max_seq_len * hd;    // the utterances' prefill cache, one layer
      at.beam_src = P.beam_src; at.beam_p0 = P.beam_p0; at.ld_src = P.ld_src; at.beam = P.beam;
      at.kc_p = d_kc.as<T>() + (size_t)i * prompt_kv; at.vc_p = d_vc.as<T>() + (size_t)i * prompt_kv; at.kap = kv_addr();
    }
    if (qwen_attention_form(at) == QW_ATTN_ROPE_MFMA) {    // V^T for the MFMA attention kernel (the cache gets V from the q|k|v GEMM)
      ProfScope ps(prof, "dec_gemm", stream);
      GemmArgs gv; gv.A = h; gv.lda = d; gv.W = (const T*)L.wqkv + (size_t)(H + KV) * hd * d; gv.ldw = d; gv.M = rows; gv.N = KV * hd; gv.K = d;
      gv.out_t = d_vt2.ptr; gv.ld_out_t = P.ld_vt; gemm(gv);
    }
    launch_qwen_attention<T>(at, prof, stream);
    if constexpr (sizeof(T) == 2) { if (dgm) dg(ctx, H * hd, L.wo, i, 1, d, H * hd, x, x2, x2lo); }
    if (!(sizeof(T) == 2 && dgm))
    { ProfScope ps(prof, "dec_gemm", stream);
      GemmArgs g; g.A = ctx; g.lda = H * hd; g.W = L.wo; g.ldw = H * hd; g.M = rows; g.N = d; g.K = H * hd; g.add = x; g.ld_add = d;
      g.out_f32 = x2; g.ld_out_f32 = d;
      if (rms_in_gemm) { g.out_lo = x2lo; g.ld_out_lo = d; }
      else if (norm_in_reduce && can_norm(g)) { g.rms_out = h; g.ld_rms_out = d; g.rms_eps = c.rms_eps; h_is_norm = true; }
      bytes_of(g, i, 1);
      gemm(g); }
    // gate|up rows are interleaved in the arena: the epilogue stores silu(gate) * up directly (:1322-1325)
    { GemmArgs g; g.W = L.gate_up; g.ldw = d; g.M = rows; g.N = 2 * I; g.K = d; g.act = ACT_SWIGLU; g.out_lo = act; g.ld_out_lo = I; bytes_of(g, i, 2); normed_gemm(x2, x2lo, g); }
    if constexpr (sizeof(T) == 2) { if (dgm) dg(act, I, L.down, i, 3, d, I, x2, x, xlo); }
    if (!(sizeof(T) == 2 && dgm))
    { ProfScope ps(prof, "dec_gemm", stream);
      GemmArgs g2; g2.A = act; g2.lda = I; g2.W = L.down; g2.ldw = I; g2.M = rows; g2.N = d; g2.K = I; g2.add = x2; g2.ld_add = d;
      g2.out_f32 = x; g2.ld_out_f32 = d;
      if (rms_in_gemm) { g2.out_lo = xlo; g2.ld_out_lo = d; }
      else if (norm_in_reduce && i + 1 < c.n_layers && can_norm(g2)) { g2.rms_out = h; g2.ld_rms_out = d; g2.rms_eps = c.rms_eps; h_is_norm = true; }
      bytes_of(g2, i, 3);
      gemm(g2); }
  }
  if (P.head) logits_head<T>(P);
}

// final RMSNorm (learned weight) of every sequence's last row, lm_head (:1331-1335), decode head
template <typename T>
void QwSession::logits_head(const DecPass& P) {
  const auto& c = cfg;
  const int d = c.d_model, B = P.B;
  float* x = d_x.as<float>();
  { ProfScope ps(prof, "dec_logits", stream);
    T* last = d_last.as<T>();
    hipLaunchKernelGGL(qw_rmsnorm_kernel<T>, dim3((B + 3) / 4), dim3(256), 0, stream, x, d, B, d, final_norm, c.rms_eps, last, d, P.last_rows);
    GemmArgs g; g.A = last; g.lda = d; g.W = lm_head; g.ldw = d; g.M = B; g.N = vpad; g.K = d; g.out_f32 = d_logits.as<float>(); g.ld_out_f32 = vpad; gemm(g);
    // a beam pass ranks the rows' extensions itself
    if (!P.beam_src) head.enqueue(d_logits.as<float>(), vpad, B, c.vocab, nullptr, P.step, d_next.as<int32_t>(), stream); }
  if (!P.hist_done) hipLaunchKernelGGL(qw_hist_add_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, P.hist ? P.hist : d_hist.as<int32_t>(), P.plan, B,
                                       P.step ? cfg.max_seq_len - 1 : INT32_MAX);
  HIP_CHECK(hipGetLastError());
}

void QwSession::finish(int B, int32_t* next_out, float* logits_out, bool sync) {
  if (taps_enabled) save_tap("logits", d_logits.ptr, B, cfg.vocab, vpad, 4);
  if (next_out || logits_out || sync || prof.enabled) download_step(h_io, d_next.ptr, d_logits.ptr, vpad, B, cfg.vocab, next_out, logits_out, stream);
  if (prof.enabled) prof.collect();
}

DecPass QwSession::step_plan(DeviceBuffer& dev, int rows) {
  const int Mb = round_up(rows, 128);
  PlanBlob pb(h_stepplan, dev);
  const auto s_plan = pb.add<UttPlan>(rows);
  const auto s_seq = pb.add<int32_t>(Mb), s_t = pb.add<int32_t>(Mb), s_last = pb.add<int32_t>(Mb);
  pb.commit(stream);
  int32_t *seq = pb.host(s_seq), *t = pb.host(s_t), *last = pb.host(s_last);
  for (int r = 0; r < Mb; ++r) { seq[r] = r < rows ? r : -1; t[r] = 0; last[r] = r < rows ? r : 0; }
  for (int r = 0; r < rows; ++r) { UttPlan p{}; p.T = 1; p.n_lfr = 1; p.row_off = r; pb.host(s_plan)[r] = p; }
  pb.upload(stream);
  DecPass P;
  P.plan = pb.dev(s_plan); P.row_seq = pb.dev(s_seq); P.row_t = pb.dev(s_t); P.last_rows = pb.dev(s_last); P.rows = rows; P.B = rows; P.step = true;
  return P;
}

template <typename T>
void QwSession::prefill(const void* audio, int audio_mem, const int64_t* audio_offs, int B, const int32_t* pre_ids, const int32_t* pre_off,
                        const int32_t* post_ids, const int32_t* post_off, int32_t* next_out, float* logits_out, int32_t* ids_len_out,
                        const AlignReq* al) {
  const auto& c = cfg;
  ASR_REQUIRE(audio && audio_offs && B >= 1 && pre_off && post_off, "qwen_prefill: bad argument");
  HIP_CHECK(hipSetDevice(device));
  const AudioIn in = stage_input(*this, true, audio, audio_mem, audio_offs, B);     // default input format: the caller's own; else model-rate f32 and its offsets
  const int64_t* const offs = in.offs;
  const int de = c.enc_d, d = c.d_model, H = c.enc_heads, dff = c.enc_ffn;
  const size_t eT = sizeof(T);
  // ---- host plan: per utterance frames / chunk slots / windows; per window an attention unit
  std::vector<UttPlan> up(B);
  std::vector<int> n_chunks(B), n_win(B), slot0(B), win0(B), n_audio(B);
  int frames = 0, n_fb = 0, slots = 0, wins = 0;
  const int64_t base0 = offs[0];
  for (int b = 0; b < B; ++b) {
    UttPlan& p = up[b];
    fe.plan_utt("qwen", b, offs, c.max_audio_len, p, frames, n_fb);
    n_chunks[b] = (p.n_frames + chunk - 1) / chunk;
    n_win[b] = (n_chunks[b] + cpw - 1) / cpw;
    slot0[b] = slots; win0[b] = wins;
    n_audio[b] = feat_lengths(p.n_frames);
    p.n_lfr = n_audio[b]; p.T = n_audio[b]; p.row_off = wins * rpw;
    slots += n_win[b] * cpw; wins += n_win[b];
  }
  const int rows_e = wins * rpw, Me = (int)pad_rows(rows_e);
  int att_qt = 0, att_nw = 4, q_rows = 64, max_T = cpw * t_tok, n_qb = 0;
  if (precision == ASR_PRECISION_BF16) { attention_geometry(max_T, 64, &att_qt, &att_nw); q_rows = 16 * att_qt * att_nw; }
  // window plans (attention units) + tables
  std::vector<UttPlan> wp(wins);
  for (int b = 0; b < B; ++b) {
    for (int w = 0; w < n_win[b]; ++w) {
      int valid = 0;
      for (int k = 0; k < cpw; ++k) {
        const int ch = w * cpw + k;
        if (ch < n_chunks[b]) valid += feat_lengths(std::min(std::max(up[b].n_frames - ch * chunk, 0), chunk));
      }
      UttPlan& p = wp[win0[b] + w];
      p = up[b];
      p.T = valid; p.n_lfr = valid; p.row_off = (win0[b] + w) * rpw;
      n_qb += (valid + q_rows - 1) / q_rows;
    }
  }
  // decoder prompt rows
  std::vector<int> ids_len(B), drow0(B);
  int rows_d = 0;
  int64_t n_sel = 0;                                     // aligner: rows the head will classify (the device's selection must agree)
  for (int b = 0; b < B; ++b) {
    ids_len[b] = (pre_off[b + 1] - pre_off[b]) + n_audio[b] + (post_off[b + 1] - post_off[b]);
    ASR_REQUIRE(ids_len[b] >= 1 && ids_len[b] <= c.max_seq_len, "qwen: prompt of %d positions exceeds max_seq_len %d", ids_len[b], c.max_seq_len);
    drow0[b] = rows_d;
    rows_d += round_up(ids_len[b], 16);
    if (ids_len_out) ids_len_out[b] = ids_len[b];
    if (al && al->tid < 0) n_sel += ids_len[b];
    else if (al) {
      for (int i = pre_off[b]; i < pre_off[b + 1]; ++i) n_sel += pre_ids[i] == al->tid;
      for (int i = post_off[b]; i < post_off[b + 1]; ++i) n_sel += post_ids[i] == al->tid;
    }
  }
  if (al) ASR_REQUIRE(n_sel <= al->cap, "qwen_align: %lld selected rows but buckets_cap is %lld", (long long)n_sel, (long long)al->cap);
  const int Md = (int)pad_rows(rows_d);
  int dqt = 0, dnw = 4, dq_rows = 0, n_dqb = 0, max_len = 0;
  for (int b = 0; b < B; ++b) max_len = std::max(max_len, ids_len[b]);
  if (precision == ASR_PRECISION_BF16) {
    attention_geometry(max_len, 128, &dqt, &dnw);
    dq_rows = 16 * dqt * dnw;
    for (int b = 0; b < B; ++b) n_dqb += (ids_len[b] + dq_rows - 1) / dq_rows;
  }
  // plan blob: [UttPlan B][win plans][dec plans B][blk_utt][blk_f0][qb_utt][qb_q0][slot_utt][slot_local][pos_rows Me][src Md][row_seq Md][row_t Md][last B][dqb_utt][dqb_q0]
  PlanBlob pb(h_plan, d_plan);
  const auto s_up = pb.add<UttPlan>(B), s_wp = pb.add<UttPlan>(wins), s_dp = pb.add<UttPlan>(B);
  const auto s_blk_utt = pb.add<int32_t>(n_fb), s_blk_f0 = pb.add<int32_t>(n_fb), s_qb_utt = pb.add<int32_t>(n_qb), s_qb_q0 = pb.add<int32_t>(n_qb);
  const auto s_slot_utt = pb.add<int32_t>(slots), s_slot_local = pb.add<int32_t>(slots), s_pos_rows = pb.add<int32_t>(Me);
  const auto s_src = pb.add<int32_t>(Md), s_row_seq = pb.add<int32_t>(Md), s_row_t = pb.add<int32_t>(Md), s_last = pb.add<int32_t>(B);
  const auto s_dqb_utt = pb.add<int32_t>(n_dqb), s_dqb_q0 = pb.add<int32_t>(n_dqb);
  pb.commit(stream, 16);
  UttPlan* h_dp = pb.host(s_dp);
  int32_t *slot_utt = pb.host(s_slot_utt), *slot_local = pb.host(s_slot_local), *pos_rows = pb.host(s_pos_rows), *src = pb.host(s_src);
  int32_t *row_seq = pb.host(s_row_seq), *row_t = pb.host(s_row_t), *last = pb.host(s_last), *dqb_utt = pb.host(s_dqb_utt), *dqb_q0 = pb.host(s_dqb_q0);
  memcpy(pb.host(s_up), up.data(), sizeof(UttPlan) * B);
  memcpy(pb.host(s_wp), wp.data(), sizeof(UttPlan) * wins);
  fill_fbank_blocks(up.data(), B, pb.host(s_blk_utt), pb.host(s_blk_f0));
  fill_query_blocks(wp.data(), wins, q_rows, pb.host(s_qb_utt), pb.host(s_qb_q0));     // attention units are windows
  constexpr int32_t PAD = INT32_MIN;
  {
    for (int b = 0; b < B; ++b)
      for (int k = 0; k < n_win[b] * cpw; ++k) { slot_utt[slot0[b] + k] = k < n_chunks[b] ? b : -1; slot_local[slot0[b] + k] = k; }
    for (int r = 0; r < Me; ++r) pos_rows[r] = (r < rows_e && (r % rpw) < cpw * t_tok) ? (r % rpw) % t_tok : 0;
    for (int r = 0; r < Md; ++r) { src[r] = PAD; row_seq[r] = -1; row_t[r] = 0; }
    for (int b = 0; b < B; ++b) {
      int r = drow0[b];
      for (int i = pre_off[b]; i < pre_off[b + 1]; ++i) {
        ASR_REQUIRE(pre_ids[i] >= 0 && pre_ids[i] < c.vocab, "qwen: token id %d out of range", pre_ids[i]);
        src[r++] = pre_ids[i];
      }
      // audio tokens: window w of the utterance holds tokens [w * cpw * 13, ...) at rows win * rpw + s
      for (int j = 0; j < n_audio[b]; ++j) src[r++] = -1 - ((win0[b] + j / (cpw * t_tok)) * rpw + j % (cpw * t_tok));
      for (int i = post_off[b]; i < post_off[b + 1]; ++i) {
        ASR_REQUIRE(post_ids[i] >= 0 && post_ids[i] < c.vocab, "qwen: token id %d out of range", post_ids[i]);
        src[r++] = post_ids[i];
      }
      for (int t = 0; t < ids_len[b]; ++t) { row_seq[drow0[b] + t] = b; row_t[drow0[b] + t] = t; }
      last[b] = drow0[b] + ids_len[b] - 1;
      if (dq_rows)
        for (int q0 = 0; q0 < ids_len[b]; q0 += dq_rows) { *dqb_utt++ = b; *dqb_q0++ = q0; }
      UttPlan& p = h_dp[b];
      p = up[b];
      p.T = ids_len[b]; p.n_lfr = ids_len[b]; p.row_off = drow0[b];
    }
  }
  pb.upload(stream);
  const UttPlan *dup = pb.dev(s_up), *dwp = pb.dev(s_wp), *ddp = pb.dev(s_dp);
  const int32_t *d_blk_utt = pb.dev(s_blk_utt), *d_blk_f0 = pb.dev(s_blk_f0), *d_qb_utt = pb.dev(s_qb_utt), *d_qb_q0 = pb.dev(s_qb_q0);
  const int32_t *d_slot_utt = pb.dev(s_slot_utt), *d_slot_local = pb.dev(s_slot_local), *d_pos_rows = pb.dev(s_pos_rows), *d_src = pb.dev(s_src);
  const int32_t *d_row_seq = pb.dev(s_row_seq), *d_row_t = pb.dev(s_row_t), *d_last_rows = pb.dev(s_last), *d_dqb_utt = pb.dev(s_dqb_utt), *d_dqb_q0 = pb.dev(s_dqb_q0);

  const void* d_aud = stage_audio(*this, d_audio, in, base0, offs[B] - base0);
  // ---- front-end + conv stem
  const size_t r1 = (size_t)slots * 50 * 64, r2 = (size_t)slots * 25 * 32, r3 = (size_t)wins * rpw * 16;
  d_mel.reserve((size_t)frames * c.n_mels * 4, stream);
  d_blkmax.reserve((size_t)n_fb * 4, stream);
  d_feat.reserve((size_t)slots * chunk * c.n_mels * eT, stream);
  d_col.reserve(std::max(std::max(pad_rows(r1) * 64, pad_rows(r2) * 9 * cpad), pad_rows(r3) * 9 * cpad) * eT, stream);
  d_c1.reserve(pad_rows(r1) * cpad * eT, stream);
  d_c2.reserve(pad_rows(r2) * cpad * eT, stream);
  d_c3.reserve((r3 + 16 * 288) * cpad * eT, stream);
  d_xa.reserve((size_t)Me * de * 4, stream);
  d_xb.reserve((size_t)Me * de * 4, stream);
  d_h.reserve((size_t)Me * de * eT, stream);
  d_qk.reserve((size_t)Me * 2 * de * eT, stream);
  d_vt.reserve((size_t)Me * de * eT, stream);
  d_ctx.reserve((size_t)Me * de * eT, stream);
  d_ffn.reserve((size_t)Me * dff * eT, stream);
  d_aud_out.reserve((size_t)Me * d * 4, stream);
  {
    ProfScope ps(prof, "logmel", stream);
    const FbankArgs fa = fe.args(d_aud, in.dtype, dup, d_blk_utt, d_blk_f0, d_mel.as<float>(), d_blkmax.as<float>());
    launch_fbank(fa, n_fb, stream);
    if (taps_enabled) save_tap("mel", d_mel.ptr, frames, c.n_mels, c.n_mels, 4);       // log10 mel before the per-utterance clamp: what the front end made of the samples
    hipLaunchKernelGGL(qw_mel_finish_kernel<T>, dim3(slots * chunk), dim3(128), 0, stream, d_mel.as<float>(), d_blkmax.as<float>(), dup, d_slot_utt,
                       d_slot_local, c.n_mels, chunk, d_feat.as<T>());
    if (taps_enabled) save_tap("feat", d_feat.ptr, (int64_t)slots * chunk, c.n_mels, c.n_mels, (int)eT);   // what the conv stem reads: [slot][frame][mel]
  }
  {
    ProfScope ps(prof, "conv_stem", stream);
    T* col = d_col.as<T>();
    hipLaunchKernelGGL(qw_im2col1_kernel<T>, dim3((unsigned)(r1 / 4)), dim3(256), 0, stream, d_feat.as<T>(), c.n_mels, chunk, 50, 64, col);
    GemmArgs g1; g1.A = col; g1.lda = 64; g1.W = conv1_w; g1.ldw = 64; g1.M = (int)r1; g1.N = cpad; g1.K = 64; g1.bias = conv1_b; g1.act = ACT_GELU_TANH;
    g1.out_lo = d_c1.ptr; g1.ld_out_lo = cpad; gemm(g1);
    hipLaunchKernelGGL(qw_im2col_cl_kernel<T>, dim3((unsigned)r2), dim3(256), 0, stream, d_c1.as<T>(), cpad, 50, 64, 25, 32, 0, 0, 0, col);
    GemmArgs g2; g2.A = col; g2.lda = 9 * cpad; g2.W = conv2_w; g2.ldw = 9 * cpad; g2.M = (int)r2; g2.N = cpad; g2.K = 9 * cpad; g2.bias = conv2_b;
    g2.act = ACT_GELU_TANH; g2.out_lo = d_c2.ptr; g2.ld_out_lo = cpad; gemm(g2);
    hipLaunchKernelGGL(qw_im2col_cl_kernel<T>, dim3((unsigned)r3), dim3(256), 0, stream, d_c2.as<T>(), cpad, 25, 32, 13, 16, rpw, cpw, t_tok, col);
    GemmArgs g3; g3.A = col; g3.lda = 9 * cpad; g3.W = conv3_w; g3.ldw = 9 * cpad; g3.M = (int)r3; g3.N = cpad; g3.K = 9 * cpad; g3.bias = conv3_b;
    g3.act = ACT_GELU_TANH; g3.out_lo = d_c3.ptr; g3.ld_out_lo = cpad; gemm(g3);
    // conv_out over rows (window slot) x [f3][channel], + sinusoidal positions of the slot's token index (:867-872)
    GemmArgs g4; g4.A = d_c3.ptr; g4.lda = 16 * cpad; g4.W = conv_out_w; g4.ldw = 16 * cpad; g4.M = rows_e; g4.N = de; g4.K = 16 * cpad;
    g4.add2 = enc_pos; g4.ld_add2 = de; g4.add2_rows = d_pos_rows; g4.out_f32 = d_xa.as<float>(); g4.ld_out_f32 = de; gemm(g4);
  }
  if (taps_enabled) save_tap("stem", d_xa.ptr, rows_e, de, de, 4);
  // ---- encoder layers over windows (:885-917)
  float* xa = d_xa.as<float>();
  float* xb = d_xb.as<float>();
  T* h = d_h.as<T>();
  T* qk = d_qk.as<T>();
  T* vt = d_vt.as<T>();
  T* ctx = d_ctx.as<T>();
  T* ffn = d_ffn.as<T>();
  for (int i = 0; i < c.n_enc_layers; ++i) {
    const QwEncLayer& L = enc[i];
    { ProfScope ps(prof, "layernorm", stream); launch_layernorm<T>(xa, de, rows_e, de, nullptr, nullptr, 1e-5f, h, de, de, stream); }
    { ProfScope ps(prof, "gemm_qkv", stream);
      GemmArgs g; g.A = h; g.lda = de; g.W = L.wqkv; g.ldw = de; g.M = rows_e; g.N = 2 * de; g.K = de; g.bias = L.bqkv; g.out_lo = qk; g.ld_out_lo = 2 * de; gemm(g);
      GemmArgs gv; gv.A = h; gv.lda = de; gv.W = (const T*)L.wqkv + (size_t)2 * de * de; gv.ldw = de; gv.M = rows_e; gv.N = de; gv.K = de;
      gv.bias = L.bqkv + 2 * de; gv.out_t = vt; gv.ld_out_t = Me; gemm(gv); }
    { ProfScope ps(prof, "attention", stream);
      AttnArgs aa; aa.q = qk; aa.k = qk + de; aa.ld_qk = 2 * de; aa.vt = vt; aa.ld_vt = Me; aa.ctx = ctx; aa.ld_ctx = de; aa.plan = dwp;
      aa.qb_utt = d_qb_utt; aa.qb_q0 = d_qb_q0; aa.n_qblocks = n_qb; aa.n_heads = H; aa.qt = att_qt; aa.n_waves = att_nw; aa.max_T = max_T;
      if (precision == ASR_PRECISION_BF16) launch_attention_bf16_hd64(aa, stream); else launch_attention_f32(aa, 64, stream); }
    { ProfScope ps(prof, "gemm_out", stream);
      GemmArgs g; g.A = ctx; g.lda = de; g.W = L.wo; g.ldw = de; g.M = rows_e; g.N = de; g.K = de; g.bias = L.bo; g.add = xa; g.ld_add = de;
      g.out_f32 = xb; g.ld_out_f32 = de; gemm(g); }
    { ProfScope ps(prof, "layernorm", stream); launch_layernorm<T>(xb, de, rows_e, de, nullptr, nullptr, 1e-5f, h, de, de, stream); }
    { ProfScope ps(prof, "gemm_ffn1", stream);
      GemmArgs g; g.A = h; g.lda = de; g.W = L.w1; g.ldw = de; g.M = rows_e; g.N = dff; g.K = de; g.bias = L.b1; g.act = ACT_GELU_TANH; g.out_lo = ffn;
      g.ld_out_lo = dff; gemm(g); }
    { ProfScope ps(prof, "gemm_ffn2", stream);
      GemmArgs g; g.A = ffn; g.lda = dff; g.W = L.w2; g.ldw = dff; g.M = rows_e; g.N = de; g.K = dff; g.bias = L.b2; g.add = xb; g.ld_add = de;
      g.out_f32 = xa; g.ld_out_f32 = de; gemm(g); }
  }
  { ProfScope ps(prof, "proj", stream);
    launch_layernorm<T>(xa, de, rows_e, de, nullptr, nullptr, 1e-5f, h, de, de, stream);                  // ln_post, affine folded into proj1
    GemmArgs g; g.A = h; g.lda = de; g.W = proj1_w; g.ldw = de; g.M = rows_e; g.N = de; g.K = de; g.bias = proj1_b; g.act = ACT_GELU_TANH; g.out_lo = ctx;
    g.ld_out_lo = de; gemm(g);
    GemmArgs g2; g2.A = ctx; g2.lda = de; g2.W = proj2_w; g2.ldw = de; g2.M = rows_e; g2.N = d; g2.K = de; g2.bias = proj2_b; g2.out_f32 = d_aud_out.as<float>();
    g2.ld_out_f32 = d; gemm(g2); }
  if (taps_enabled) save_tap("audio_hidden", d_aud_out.ptr, rows_e, d, d, 4);
  // ---- decoder prefill over the assembled prompts
  const int KV = c.n_kv_heads, hd = c.d_head, Hq = c.n_heads, I = c.d_ffn, qkvn = (Hq + 2 * KV) * hd, S = c.max_seq_len;
  batch = B;
  seq_len.assign(ids_len.begin(), ids_len.end());
  if (kv_paged) kv_begin(B, ids_len, eT);
  else {
    d_kc.reserve((size_t)c.n_layers * B * KV * S * hd * eT, stream);
    d_vc.reserve((size_t)c.n_layers * B * KV * S * hd * eT, stream);
  }
  d_hist.reserve((size_t)std::max(B, 64) * 4, stream);
  HIP_CHECK(hipMemsetAsync(d_hist.ptr, 0, (size_t)B * 4, stream));
  const int Mmax = std::max(Md, (int)pad_rows(B));
  d_x.reserve((size_t)Mmax * d * 4, stream);
  d_x2.reserve((size_t)Mmax * d * 4, stream);
  d_dh.reserve((size_t)Mmax * d * eT, stream);
  d_qkv.reserve((size_t)Mmax * qkvn * 4, stream);
  d_q.reserve((size_t)Mmax * Hq * hd * eT, stream);
  d_dctx.reserve((size_t)Mmax * Hq * hd * eT, stream);
  d_xlo.reserve(pad_rows(B) * d * eT, stream);
  d_x2lo.reserve(pad_rows(B) * d * eT, stream);
  d_act.reserve((size_t)Mmax * I * eT, stream);
  d_last.reserve(pad_rows(B) * d * eT, stream);
  d_logits.reserve(pad_rows(B) * (size_t)vpad * 4, stream);
  d_next.reserve((size_t)std::max(B, 64) * 4, stream);
  head.reserve(B, stream);
  head.restart(stream);
  { ProfScope ps(prof, "dec_embed", stream);
    hipLaunchKernelGGL(qw_gather_prompt_kernel<T>, dim3(Md), dim3(256), 0, stream, d_src, (const T*)embed, d_aud_out.as<float>(), d, PAD, d_x.as<float>(), (T*)nullptr); }
  if (taps_enabled) save_tap("prompt", d_x.ptr, rows_d, d, d, 4);
  if (precision == ASR_PRECISION_BF16) {
    d_vt2.reserve((size_t)KV * hd * Md * eT, stream);
    d_krows.reserve((size_t)Md * KV * hd * eT, stream);
  }
  DecPass P;
  P.plan = ddp; P.row_seq = d_row_seq; P.row_t = d_row_t; P.last_rows = d_last_rows; P.rows = rows_d; P.B = B; P.step = false;
  P.qb_utt = d_dqb_utt; P.qb_q0 = d_dqb_q0; P.n_qb = no_fuse ? 0 : n_dqb; P.qt = dqt; P.nw = dnw; P.max_T = max_len; P.ld_vt = Md;
  P.head = al == nullptr;
  decoder_pass<T>(P);
  if (al) { align_head<T>(B, ddp, d_src, (int)n_sel, *al); return; }
  step_pass = step_plan(d_stepplan, B);                   // for the decode calls that follow
  head.consumed();
  finish(B, next_out, logits_out, true);
}

// Forced-aligner head (FORCED_ALIGNER_DECODER_MAIN :1104-1109 on the selected rows only): device-side row selection -> final RMSNorm of those
// rows (learned weight) -> classify GEMM with the row arg-max. A few rows stream the weights (skinny GEMM to f32 logits + row arg-max); more
// rows take the MFMA tiles with the fused arg-max epilogue (per 64-column partials, reduced afterwards), the CTC head's form.
template <typename T>
void QwSession::align_head(int B, const UttPlan* ddp, const int32_t* d_src, int n_sel, const AlignReq& al) {
  const auto& c = cfg;
  const int d = c.d_model, n_slabs = hpad / 64;
  const bool want_logits = al.logits != nullptr;
  d_sel.reserve((size_t)(2 * B + 1 + std::max(n_sel, 64)) * 4, stream);
  int32_t* cnt = d_sel.as<int32_t>();
  int32_t* off = cnt + B;
  int32_t* rows = off + B + 1;
  d_bucket.reserve((size_t)std::max(n_sel, 64) * 4, stream);
  const bool stream_w = precision == ASR_PRECISION_BF16 && n_sel <= 64;
  { ProfScope ps(prof, "align_head", stream);
    hipLaunchKernelGGL(qw_slot_count_kernel, dim3(B), dim3(256), 0, stream, d_src, ddp, al.tid, cnt);
    hipLaunchKernelGGL(qw_slot_compact_kernel, dim3(B), dim3(256), 0, stream, d_src, ddp, al.tid, (const int32_t*)cnt, B, n_sel, off, rows);
    if (n_sel > 0) {
      d_last.reserve(pad_rows(n_sel) * d * sizeof(T), stream);
      T* last = d_last.as<T>();
      hipLaunchKernelGGL(qw_rmsnorm_kernel<T>, dim3((n_sel + 3) / 4), dim3(256), 0, stream, d_x.as<float>(), d, n_sel, d, final_norm, c.rms_eps, last, d,
                         (const int32_t*)rows);
      GemmArgs g; g.A = last; g.lda = d; g.W = lm_head; g.ldw = d; g.M = n_sel; g.N = hpad; g.K = d;
      if (stream_w || want_logits) {
        d_logits.reserve(pad_rows(n_sel) * (size_t)hpad * 4, stream);
        g.out_f32 = d_logits.as<float>(); g.ld_out_f32 = hpad;
      }
      if (stream_w) {
        gemm(g);
        launch_argmax_rows(d_logits.as<float>(), hpad, n_sel, c.classify_num, nullptr, d_bucket.as<int32_t>(), stream);
      } else {
        d_amax_v.reserve(pad_rows(n_sel) * n_slabs * 4, stream);
        d_amax_i.reserve(pad_rows(n_sel) * n_slabs * 4, stream);
        g.amax_val = d_amax_v.as<float>(); g.amax_idx = d_amax_i.as<int32_t>(); g.n_valid = c.classify_num;
        gemm(g);
        launch_argmax_reduce(d_amax_v.as<float>(), d_amax_i.as<int32_t>(), n_sel, n_slabs, d_bucket.as<int32_t>(), stream);
      }
    }
    HIP_CHECK(hipGetLastError()); }
  if (taps_enabled && n_sel > 0 && want_logits) save_tap("logits", d_logits.ptr, n_sel, c.classify_num, hpad, 4);
  const size_t lbytes = want_logits ? (size_t)n_sel * c.classify_num * 4 : 0;
  h_io.reserve((size_t)(B + 1 + n_sel) * 4 + 64 + lbytes);
  unsigned char* st = h_io.as<unsigned char>();
  int32_t* h_off = (int32_t*)st;
  int32_t* h_bk = h_off + B + 1;
  float* h_lg = (float*)(st + (size_t)(B + 1 + n_sel) * 4 + 64);
  HIP_CHECK(hipMemcpyAsync(h_off, off, (size_t)(B + 1) * 4, hipMemcpyDeviceToHost, stream));
  if (n_sel > 0) {
    HIP_CHECK(hipMemcpyAsync(h_bk, d_bucket.ptr, (size_t)n_sel * 4, hipMemcpyDeviceToHost, stream));
    if (want_logits)
      HIP_CHECK(hipMemcpy2DAsync(h_lg, (size_t)c.classify_num * 4, d_logits.ptr, (size_t)hpad * 4, (size_t)c.classify_num * 4, n_sel, hipMemcpyDeviceToHost, stream));
  }
  HIP_CHECK(hipStreamSynchronize(stream));
  ASR_REQUIRE(h_off[B] == n_sel, "qwen_align: the device selected %d rows, the host counted %d", h_off[B], n_sel);
  memcpy(al.slot_off, h_off, (size_t)(B + 1) * 4);
  if (n_sel > 0) memcpy(al.buckets, h_bk, (size_t)n_sel * 4);
  if (want_logits && n_sel > 0) memcpy(al.logits, h_lg, lbytes);
  if (prof.enabled) prof.collect();
}

template <typename T>
void QwSession::step(const int32_t* ids_host, int32_t* next_out, float* logits_out) {
  const auto& c = cfg;
  ASR_REQUIRE(batch > 0, "qwen_decode: prefill first");
  HIP_CHECK(hipSetDevice(device));
  const int B = batch, d = c.d_model;
  head.reserve(B, stream);                               // (token scores switched on since the prefill: their history covers this batch before anything is enqueued)
  for (int b = 0; b < B; ++b) {
    ASR_REQUIRE(seq_len[b] + 1 <= c.max_seq_len || (b < (int)frozen.size() && frozen[b]), "qwen_decode: sequence %d is at max_seq_len %d", b, c.max_seq_len);
    // a sequence that generate() finished has given its cache pages back (its table row points at the scratch page): it cannot be stepped again outside that
    // generate() call -- fail loudly instead of decoding against page 0
    ASR_REQUIRE(!(kv_paged && b < (int)kv_released.size() && kv_released[b]) || (b < (int)frozen.size() && frozen[b]),
                "qwen_decode: sequence %d was finished by generate() and its cache pages were returned; prefill again", b);
  }
  if (ids_host) {
    h_ids.reserve((size_t)B * 4);
    int32_t* st = h_ids.as<int32_t>();
    for (int b = 0; b < B; ++b) {
      ASR_REQUIRE(ids_host[b] >= 0 && ids_host[b] < c.vocab, "qwen_decode: token id %d out of range", ids_host[b]);
      st[b] = ids_host[b];
    }
    HIP_CHECK(hipMemcpyAsync(d_next.ptr, st, (size_t)B * 4, hipMemcpyHostToDevice, stream));
  }
  kv_prepare_step(sizeof(T));
  const DecPass P = step_pass;                           // (one row per sequence: uploaded by prefill)
  auto enqueue = [&] {
    { ProfScope ps(prof, "dec_embed", stream);
      hipLaunchKernelGGL(qw_gather_prompt_kernel<T>, dim3(B), dim3(256), 0, stream, (const int32_t*)d_next.ptr, (const T*)embed, (const float*)nullptr, d,
                         INT32_MIN, d_x.as<float>(), precision == ASR_PRECISION_BF16 ? d_xlo.as<T>() : (T*)nullptr); }
    decoder_pass<T>(P);
  };
  // every step reads its position from the device-side history counters => one captured graph replays for all of them
  const bool graphable = use_graph && !taps_enabled && !prof.enabled && !head.noise_armed;
  GraphKey key;
  for (const void* q : {d_x.ptr, d_x2.ptr, d_dh.ptr, d_qkv.ptr, d_q.ptr, d_dctx.ptr, d_xlo.ptr, d_x2lo.ptr, d_act.ptr, d_last.ptr, d_logits.ptr, d_next.ptr, d_kc.ptr,
                        d_vc.ptr, d_kvtab.ptr, d_hist.ptr, d_stepplan.ptr, sk.ws.ptr, (void*)stream, (void*)(uintptr_t)B})
    key.mix(q);
  key.mix(head.epoch);
  dec_graph.run(stream, graphable, key.h, enqueue);
  head.consumed();
  for (int b = 0; b < B; ++b) seq_len[b] = std::min(seq_len[b] + 1, c.max_seq_len);
  finish(B, next_out, logits_out, ids_host != nullptr);
}

// Beam search after a prefill: every step runs the decoder over all B * beam hypothesis rows. The prompts stay where the prefill wrote
// them (one copy per utterance, shared by its rows); generated positions go to a small per-row cache and the attention kernel follows
// each row's ancestry through it, so nothing is copied or re-ordered between steps. The extensions are ranked on the device; the host
// reads back only the per-utterance "best hypothesis has ended" flags.
// Output: per utterance its `beam` hypotheses best-first -- tokens_out [B][beam][max_new], n_out [B][beam], scores_out [B][beam].
template <typename T>
void QwSession::beam_search(int beam, int max_new, const int32_t* stop_ids, int n_stop, int32_t* tokens_out, int32_t* n_out, float* scores_out) {
  const auto& c = cfg;
  ASR_REQUIRE(batch > 0, "qwen_beam_search: prefill first");
  ASR_REQUIRE(beam >= 1 && beam <= BEAM_MAX, "qwen_beam_search: beam width %d outside 1..%d", beam, BEAM_MAX);
  ASR_REQUIRE(!no_fuse && (c.n_heads / c.n_kv_heads == 1 || c.n_heads / c.n_kv_heads == 2 || c.n_heads / c.n_kv_heads == 4),
              "qwen_beam_search: needs the fused decode attention kernel");
  ASR_REQUIRE(head.plain(), "qwen_beam_search: the penalty / sampling heads do not combine with beam search");
  HIP_CHECK(hipSetDevice(device));
  const int B = batch, N = B * beam, KV = c.n_kv_heads, hd = c.d_head, d = c.d_model, H = c.n_heads, I = c.d_ffn, qkvn = (H + 2 * KV) * hd;
  const size_t eT = sizeof(T);
  int max_len = 0;
  for (int b = 0; b < B; ++b) max_len = std::max(max_len, seq_len[b]);
  ASR_REQUIRE(max_len + 1 <= c.max_seq_len, "qwen_beam_search: no room after the prompt (max_seq_len %d)", c.max_seq_len);
  const int out_stride = max_new;
  max_new = std::min(max_new, c.max_seq_len - max_len);  // positions (RoPE rows) end at max_seq_len
  const int Sb = round_up(max_new, 16), ld = Sb;         // generated slots per hypothesis row; the prompts stay in the prefill cache
  // ---- the first ranking reads the prefill logits; do it before any buffer grows
  ranker.begin(B, beam, ld, stop_ids, n_stop, TimestampRule{}, head.hot_view("qwen_beam_search"), stream, head.lm, "qwen_beam_search");
  ranker.rank_first(d_logits.as<float>(), vpad, c.vocab, nullptr, stream);
  // ---- hypothesis rows: caches, counters, row buffers, the one-row-per-hypothesis plan
  for (DeviceBuffer* q : {&d_bhist, &d_bp0}) q->reserve((size_t)std::max(N, 64) * 4, stream);
  d_bkc.reserve((size_t)c.n_layers * N * KV * Sb * hd * eT, stream);
  d_bvc.reserve((size_t)c.n_layers * N * KV * Sb * hd * eT, stream);
  hipLaunchKernelGGL(qw_beam_init_kernel, dim3((N + 63) / 64), dim3(64), 0, stream, d_hist.as<int32_t>(), B, beam, d_bhist.as<int32_t>(), d_bp0.as<int32_t>());
  const size_t Mn = pad_rows(N);
  d_x.reserve(Mn * d * 4, stream); d_x2.reserve(Mn * d * 4, stream); d_dh.reserve(Mn * d * eT, stream); d_qkv.reserve(Mn * qkvn * 4, stream);
  d_dctx.reserve(Mn * H * hd * eT, stream); d_xlo.reserve(Mn * d * eT, stream); d_x2lo.reserve(Mn * d * eT, stream); d_act.reserve(Mn * I * eT, stream);
  d_last.reserve(Mn * d * eT, stream); d_logits.reserve(Mn * (size_t)vpad * 4, stream);
  DecPass P = step_plan(d_bplan, N);
  P.kc = d_bkc.ptr; P.vc = d_bvc.ptr; P.S = Sb; P.hist = d_bhist.as<int32_t>(); P.beam_p0 = d_bp0.as<int32_t>(); P.ld_src = ld; P.beam = beam;
  for (int t = 0; t + 1 < max_new && !ranker.all_done(stream); ++t) {
    { ProfScope ps(prof, "dec_embed", stream);
      hipLaunchKernelGGL(qw_gather_prompt_kernel<T>, dim3(N), dim3(256), 0, stream, (const int32_t*)ranker.next_ids(), (const T*)embed, (const float*)nullptr, d,
                         INT32_MIN, d_x.as<float>(), precision == ASR_PRECISION_BF16 ? d_xlo.as<T>() : (T*)nullptr); }
    P.beam_src = ranker.ancestry();
    decoder_pass<T>(P);
    { ProfScope ps(prof, "beam_rank", stream);
      ranker.enqueue_rank(d_logits.as<float>(), vpad, c.vocab, t + 1, stream); }
    ranker.flip();
  }
  HIP_CHECK(hipGetLastError());
  ranker.download(tokens_out, out_stride, n_out, scores_out, stream);
  if (prof.enabled) prof.collect();
}

}  // namespace

extern "C" int asr_qwen_create(const asr_qwen_config* cfg, const void* arena, size_t arena_bytes, int arena_mem, int device_id, int precision,
                               asr_session** out) {
  return asr_guard([&] {
    ASR_REQUIRE(cfg && arena && out, "qwen_create: null argument");
    ASR_REQUIRE(precision == ASR_PRECISION_BF16 || precision == ASR_PRECISION_F32 || precision == ASR_PRECISION_FP8W || precision == ASR_PRECISION_MXFP4W, "qwen_create: bad precision %d", precision);
    asr_require_device(device_id);
    QwSession* s = new QwSession();
    try {
      s->kind = 5;
      s->device = device_id;
      asr_tenant_attach(s);
      s->fp4 = precision == ASR_PRECISION_MXFP4W;
      s->fp8 = precision == ASR_PRECISION_FP8W || s->fp4;
      s->precision = s->fp8 ? ASR_PRECISION_BF16 : precision;        // FP8 mode = bf16 mode with byte-wide decoder projections
      s->cfg = *cfg;
      ASR_REQUIRE(cfg->classify_num == 0 || !s->fp8, "qwen_create: the forced aligner runs bf16 or f32 weights (FP8W / MXFP4W aligner sessions are not supported)");
      HIP_CHECK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
      s->own_stream = true;
      gemm_reload_env();
      s->fp8_fake = env_on("ASR_FP8_FAKE", s->fp8_fake);
      s->use_decode_gemm = env_flag("ASR_QWEN_DECODE_GEMM", s->use_decode_gemm);
      s->use_graph = !env_on("ASR_NO_GRAPH", !s->use_graph);
      s->no_fuse = env_on("ASR_QWEN_NO_FUSE", s->no_fuse);
      s->kv_paged = env_flag("ASR_QWEN_KV_PAGED", s->kv_paged);
      s->kv_shuffle = env_on("ASR_KV_PAGE_SHUFFLE", s->kv_shuffle);
      s->arena.load(arena, arena_bytes, arena_mem, s->stream);
      s->init();
    } catch (...) {
      delete s;
      throw;
    }
    *out = s;
  });
}

extern "C" int asr_qwen_prefill(asr_session* s, const void* audio, int audio_mem, const int64_t* audio_offsets, int batch, const int32_t* pre_ids,
                                const int32_t* pre_offsets, const int32_t* post_ids, const int32_t* post_offsets, int32_t* next_ids_out,
                                float* logits_out, int32_t* ids_len_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 5, "qwen_prefill: not a Qwen3-ASR session");
    TenantScope tenant(s);
    QwSession* q = static_cast<QwSession*>(s);
    ASR_REQUIRE(!q->aligner(), "qwen_prefill: a forced-aligner session (classify_num %d) has no LM head; call asr_qwen_align", q->cfg.classify_num);
    if (q->precision == ASR_PRECISION_BF16)
      q->prefill<bf16_t>(audio, audio_mem, audio_offsets, batch, pre_ids, pre_offsets, post_ids, post_offsets, next_ids_out, logits_out, ids_len_out);
    else
      q->prefill<float>(audio, audio_mem, audio_offsets, batch, pre_ids, pre_offsets, post_ids, post_offsets, next_ids_out, logits_out, ids_len_out);
  });
}

extern "C" int asr_qwen_decode(asr_session* s, const int32_t* ids, int32_t* next_ids_out, float* logits_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 5, "qwen_decode: not a Qwen3-ASR session");
    TenantScope tenant(s);
    QwSession* q = static_cast<QwSession*>(s);
    ASR_REQUIRE(!q->aligner(), "qwen_decode: a forced-aligner session (classify_num %d) has no decode loop; call asr_qwen_align", q->cfg.classify_num);
    if (q->precision == ASR_PRECISION_BF16) q->step<bf16_t>(ids, next_ids_out, logits_out);
    else q->step<float>(ids, next_ids_out, logits_out);
  });
}

// the decode-head entries: the checks and the state are TokenHead's (decode_head.h)
static QwSession* qwen_session(asr_session* s, const char* who) {
  ASR_REQUIRE(s && s->kind == 5, "%s: not a Qwen3-ASR session", who);
  return static_cast<QwSession*>(s);
}

extern "C" int asr_qwen_set_penalty(asr_session* s, float repeat_penalty, int penalty_range) {
  return asr_guard([&] { qwen_session(s, "qwen_set_penalty")->head.set_penalty(repeat_penalty, penalty_range, "qwen_set_penalty"); });
}

extern "C" int asr_qwen_track_history(asr_session* s, int enable) {
  return asr_guard([&] { qwen_session(s, "qwen_track_history")->head.set_track_history(enable != 0); });
}

extern "C" int asr_qwen_set_sampling(asr_session* s, int enable, float temperature, int top_k, float top_p, float repetition_penalty, uint64_t seed) {
  return asr_guard([&] {
    qwen_session(s, "qwen_set_sampling")->head.set_sampling(enable != 0, temperature, top_k, top_p, repetition_penalty, seed, "qwen_set_sampling");
  });
}

extern "C" int asr_qwen_set_hotwords(asr_session* s, const int32_t* ids, const int32_t* offsets, int n_phrases, float boost) {
  return asr_guard([&] {
    QwSession* q = qwen_session(s, "qwen_set_hotwords");
    HIP_CHECK(hipSetDevice(q->device));
    q->head.set_hotwords(ids, offsets, n_phrases, boost, q->cfg.vocab, q->stream, "qwen_set_hotwords");
  });
}

extern "C" int asr_qwen_set_lm(asr_session* s, const int32_t* image_words, int64_t n_words, float alpha, float beta, float oov_logprob, int topk,
                               const int32_t* end_ids, int n_end_ids) {
  return asr_guard([&] {
    QwSession* q = qwen_session(s, "qwen_set_lm");
    ASR_REQUIRE(!q->aligner(), "qwen_set_lm: a forced-aligner session (classify_num %d) has no LM head to fuse a language model into", q->cfg.classify_num);
    HIP_CHECK(hipSetDevice(q->device));
    q->head.set_lm(image_words, n_words, alpha, beta, oov_logprob, topk, end_ids, n_end_ids, q->cfg.vocab, q->stream, "qwen_set_lm");
  });
}

extern "C" int asr_qwen_set_token_scores(asr_session* s, int enable) {
  return asr_guard([&] { qwen_session(s, "qwen_set_token_scores")->head.set_scores(enable != 0); });
}

extern "C" int asr_qwen_token_scores(asr_session* s, float* logprob_out, int out_stride, int32_t* n_out) {
  return asr_guard([&] {
    QwSession* q = qwen_session(s, "qwen_token_scores");
    HIP_CHECK(hipSetDevice(q->device));
    q->head.download_scores(q->batch, logprob_out, out_stride, n_out, q->stream, "qwen_token_scores");
  });
}

extern "C" int asr_qwen_set_sampling_noise(asr_session* s, const float* uniforms, int count) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 5 && uniforms && count > 0, "qwen_set_sampling_noise: bad argument");
    QwSession* q = static_cast<QwSession*>(s);
    ASR_REQUIRE(q->head.sampling && count % q->head.top_k == 0, "qwen_set_sampling_noise: expects batch x top_k uniforms for the next step");
    HIP_CHECK(hipSetDevice(q->device));
    q->head.arm_noise(uniforms, count, q->stream);
  });
}

extern "C" int asr_qwen_beam_search(asr_session* s, int beam, int max_new, const int32_t* stop_ids, int n_stop, int32_t* tokens_out, int32_t* n_out,
                                    float* scores_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 5 && tokens_out && n_out && max_new >= 1 && n_stop >= 0 && (n_stop == 0 || stop_ids), "qwen_beam_search: bad argument");
    TenantScope tenant(s);
    QwSession* q = static_cast<QwSession*>(s);
    ASR_REQUIRE(!q->aligner(), "qwen_beam_search: a forced-aligner session (classify_num %d) has no decode loop; call asr_qwen_align", q->cfg.classify_num);
    if (q->precision == ASR_PRECISION_BF16) q->beam_search<bf16_t>(beam, max_new, stop_ids, n_stop, tokens_out, n_out, scores_out);
    else q->beam_search<float>(beam, max_new, stop_ids, n_stop, tokens_out, n_out, scores_out);
  });
}

extern "C" int asr_qwen_kv_stats(asr_session* s, int32_t* out4) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 5 && out4, "qwen_kv_stats: bad argument");
    QwSession* q = static_cast<QwSession*>(s);
    int held = 0;
    for (const auto& v : q->kv_owned) held += (int)v.size();
    out4[0] = q->kv_paged ? 1 : 0; out4[1] = q->kv_pool_pages; out4[2] = q->kv_paged ? held : 0; out4[3] = q->kv_high_water;
  });
}

extern "C" int asr_qwen_generate(asr_session* s, int max_new, const int32_t* stop_ids, int n_stop, int32_t* tokens_out, int32_t* n_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 5 && tokens_out && n_out && max_new >= 1 && (n_stop == 0 || stop_ids), "qwen_generate: bad argument");
    TenantScope tenant(s);
    QwSession* q = static_cast<QwSession*>(s);
    ASR_REQUIRE(!q->aligner(), "qwen_generate: a forced-aligner session (classify_num %d) has no decode loop; call asr_qwen_align", q->cfg.classify_num);
    ASR_REQUIRE(q->batch > 0, "qwen_generate: prefill first");
    const int B = q->batch;
    std::vector<int32_t> cur(B);
    HIP_CHECK(hipSetDevice(q->device));
    HIP_CHECK(hipMemcpyAsync(cur.data(), q->d_next.ptr, (size_t)B * 4, hipMemcpyDeviceToHost, q->stream));
    HIP_CHECK(hipStreamSynchronize(q->stream));
    std::vector<char> done(B, 0);
    for (int b = 0; b < B; ++b) n_out[b] = 0;
    // a sequence that an EARLIER generate() call of this batch finished has given its pages back: it stays finished (no tokens) while the others go on -- chunked generation
    // after hitting max_new must not abort the batch
    if (q->kv_paged) for (int b = 0; b < B && b < (int)q->kv_released.size(); ++b) if (q->kv_released[b]) done[b] = 1;
    struct ClearFrozen { QwSession* q; ~ClearFrozen() { q->frozen.clear(); } } clear_frozen{q};      // also when a step throws: a stale list would release live sequences' pages
    auto is_stop = [&](int32_t t) { for (int i = 0; i < n_stop; ++i) if (stop_ids[i] == t) return true; return false; };
    for (int t = 0; t < max_new; ++t) {
      bool all_done = true, room = true;
      for (int b = 0; b < B; ++b) {
        if (!done[b]) {
          if (is_stop(cur[b])) done[b] = 1;                      // a stop token ends the sequence and is not emitted
          else tokens_out[(size_t)b * max_new + n_out[b]++] = cur[b];
        }
        all_done = all_done && done[b];
        // only sequences still generating need a free position: a finished long-prompt row that has reached max_seq_len keeps
        // re-writing its last cache slot (device-side cap) instead of ending the batch for the others
        if (!done[b]) room = room && q->seq_len[b] + 1 <= q->cfg.max_seq_len;
      }
      q->frozen.assign(done.begin(), done.end());
      if (all_done || t + 1 == max_new || !room) break;
      if (q->precision == ASR_PRECISION_BF16) q->step<bf16_t>(nullptr, cur.data(), nullptr);
      else q->step<float>(nullptr, cur.data(), nullptr);
    }
  });
}

extern "C" int asr_qwen_align(asr_session* s, const void* audio, int audio_mem, const int64_t* audio_offsets, int batch, const int32_t* pre_ids,
                              const int32_t* pre_offsets, const int32_t* post_ids, const int32_t* post_offsets, int32_t timestamp_id,
                              int32_t* slot_offsets_out, int32_t* buckets_out, int64_t buckets_cap, float* logits_out, int32_t* ids_len_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && s->kind == 5, "qwen_align: not a Qwen3 session");
    TenantScope tenant(s);
    QwSession* q = static_cast<QwSession*>(s);
    ASR_REQUIRE(q->aligner(), "qwen_align: not a forced-aligner session (classify_num = 0: this session has the vocabulary LM head)");
    ASR_REQUIRE(slot_offsets_out && buckets_cap >= 0 && (buckets_out || buckets_cap == 0), "qwen_align: bad argument");
    ASR_REQUIRE(timestamp_id < q->cfg.vocab, "qwen_align: timestamp id %d out of range", timestamp_id);
    AlignReq al;
    al.tid = timestamp_id < 0 ? -1 : timestamp_id; al.slot_off = slot_offsets_out; al.buckets = buckets_out; al.cap = buckets_cap; al.logits = logits_out;
    if (q->precision == ASR_PRECISION_BF16)
      q->prefill<bf16_t>(audio, audio_mem, audio_offsets, batch, pre_ids, pre_offsets, post_ids, post_offsets, nullptr, nullptr, ids_len_out, &al);
    else
      q->prefill<float>(audio, audio_mem, audio_offsets, batch, pre_ids, pre_offsets, post_ids, post_offsets, nullptr, nullptr, ids_len_out, &al);
  });
}
