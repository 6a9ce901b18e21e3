// Prompt attention of the Whisper decoder (kernels.h: PromptAttnArgs): prefills of more than 8 ids per sequence or of ragged, left-padded lengths.
// head_dim 64. One workgroup of 256 threads per (sequence, head, tile of query rows); the keys of the tile go through LDS in blocks of 64 under an online
// soft-max that runs on exp2 of scores pre-scaled by log2(e).
//   f32  : tile of 16 query rows, thread = (row, 1 of 16): four scores of a block per thread, then four context dims per thread, all f32 FMAs.
//   bf16 : tile of 64 query rows, wave = 16 rows. The scores are computed TRANSPOSED, S^T = K Q^T (v_mfma_f32_16x16x32_bf16, K rows from LDS as the A operand,
//          the wave's Q rows held in registers as the B operand), so that a lane holds 16 keys of ONE query row: the soft-max statistics are register
//          reductions plus two shuffles, and the probabilities -- rounded to bf16 -- are already the B operand of O^T = V^T P^T without leaving the
//          registers (the k order inside a 32-key step is permuted; the V^T fragments are read from LDS in the same order).
// Causality (self): keys after the query's slot are skipped, keys below key_start[b] (the left pad) do not exist and are never loaded.
#include "kernels.h"

#include <type_traits>

namespace {

constexpr float PA_LOG2E = 1.4426950408889634f;
constexpr int PA_QT_F32 = 16, PA_QT_BF16 = 64;

template <typename T>
struct PaAddr {                      // where the keys of one (sequence, head) live
  const T* NEW;                      // self: row s at NEW + s * ld_new (+ k_col0 / v_col0)
  const T* Kc; const T* Vc;          // cross: row s at + s * 64
  T* Kw; T* Vw;                      // self: the cache to fill, row s at + crow(s)
  const int32_t* pt; int64_t page_stride;
  __device__ __forceinline__ size_t crow(int s) const { return pt ? (size_t)pt[s >> 4] * (size_t)page_stride + (size_t)(s & 15) * 64 : (size_t)s * 64; }
};

template <typename T, bool SELF>
__device__ __forceinline__ PaAddr<T> pa_addr(const PromptAttnArgs& a, int b, int h, int& k_begin, int& k_total) {
  PaAddr<T> ad{};
  if constexpr (SELF) {
    ad.pt = a.page_table ? a.page_table + (size_t)b * a.pages_per_seq : nullptr;
    ad.page_stride = a.page_stride;
    const size_t off = ad.pt ? (size_t)h * 1024 : (size_t)b * a.stride_b + (size_t)h * a.stride_h;
    ad.Kw = reinterpret_cast<T*>(a.k_base) + off;
    ad.Vw = reinterpret_cast<T*>(a.v_base) + off;
    ad.NEW = reinterpret_cast<const T*>(a.kv_new) + (size_t)b * a.n * a.ld_new + h * 64;
    k_begin = a.key_start ? a.key_start[b] : 0;
    k_total = a.n;
  } else {
    const size_t off = (size_t)b * a.stride_b + (size_t)h * a.stride_h + (size_t)a.plan[b].row_off * 64;
    ad.Kc = reinterpret_cast<const T*>(a.k_base) + off;
    ad.Vc = reinterpret_cast<const T*>(a.v_base) + off;
    k_begin = 0;
    k_total = a.plan[b].n_lfr;
  }
  return ad;
}

// ------------------------------------------------------------------------------------ f32
template <bool SELF>
__global__ __launch_bounds__(256) void prompt_attn_f32_kernel(const PromptAttnArgs a) {
  constexpr int QT = PA_QT_F32;
  __shared__ float Qs[QT][64];
  __shared__ float Ks[64][65];
  __shared__ __attribute__((aligned(16))) float Vs[64][64];
  __shared__ float Ps[QT][64];
  const int b = blockIdx.x, h = blockIdx.y, tile = blockIdx.z, tid = threadIdx.x, r = tid >> 4, c = tid & 15;
  const int n = a.n, pad = a.key_start ? a.key_start[b] : 0;
  int k_begin, k_total;
  const PaAddr<float> ad = pa_addr<float, SELF>(a, b, h, k_begin, k_total);
  const int i = tile * QT + r;                                  // this thread's query slot
  const bool active = i < n && i >= pad;
  const int k_end = SELF ? min(k_total, tile * QT + QT) : k_total;
  {                                                             // the tile's query rows, pre-scaled; rows that are not queries read nothing
    const float* Q = reinterpret_cast<const float*>(a.q) + (size_t)(b * n + i) * a.ld_q + a.q_col0 + h * 64 + c * 4;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (active) q = *reinterpret_cast<const float4*>(Q);
    Qs[r][c * 4 + 0] = q.x * PA_LOG2E; Qs[r][c * 4 + 1] = q.y * PA_LOG2E; Qs[r][c * 4 + 2] = q.z * PA_LOG2E; Qs[r][c * 4 + 3] = q.w * PA_LOG2E;
  }
  if constexpr (SELF) {                                         // the tile's own K / V rows into the cache, pad slots included (read back only by later steps)
    if (i < n) {
      const float* src = ad.NEW + (size_t)i * a.ld_new + c * 4;
      const size_t ro = ad.crow(i) + c * 4;
      *reinterpret_cast<float4*>(ad.Kw + ro) = *reinterpret_cast<const float4*>(src + a.k_col0);
      *reinterpret_cast<float4*>(ad.Vw + ro) = *reinterpret_cast<const float4*>(src + a.v_col0);
    }
  }
  float m = -INFINITY, l = 0.0f, acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int kb = k_begin; kb < k_end; kb += 64) {
    __syncthreads();                                            // (the previous block's reads; the first trip: Qs)
    {
      const int kk = tid >> 2, s = kb + kk, d0 = (tid & 3) * 16;
      float4 kv[4], vv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) { kv[e] = make_float4(0.f, 0.f, 0.f, 0.f); vv[e] = kv[e]; }
      if (s < k_end) {
        const float* kp = SELF ? ad.NEW + (size_t)s * a.ld_new + a.k_col0 + d0 : ad.Kc + (size_t)s * 64 + d0;
        const float* vp = SELF ? ad.NEW + (size_t)s * a.ld_new + a.v_col0 + d0 : ad.Vc + (size_t)s * 64 + d0;
#pragma unroll
        for (int e = 0; e < 4; ++e) { kv[e] = *reinterpret_cast<const float4*>(kp + 4 * e); vv[e] = *reinterpret_cast<const float4*>(vp + 4 * e); }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        Ks[kk][d0 + 4 * e + 0] = kv[e].x; Ks[kk][d0 + 4 * e + 1] = kv[e].y; Ks[kk][d0 + 4 * e + 2] = kv[e].z; Ks[kk][d0 + 4 * e + 3] = kv[e].w;
        *reinterpret_cast<float4*>(&Vs[kk][d0 + 4 * e]) = vv[e];
      }
    }
    __syncthreads();
    float sc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int d8 = 0; d8 < 64; d8 += 8) {                         // chains of 8 FMAs, then 8 additions: <= 16 roundings per score, as the decode kernels
      float part[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float q = Qs[r][d8 + e];
#pragma unroll
        for (int j = 0; j < 4; ++j) part[j] = fmaf(q, Ks[c + 16 * j][d8 + e], part[j]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) sc[j] += part[j];
    }
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int s = kb + c + 16 * j;
      if (!(active && s < k_end && (!SELF || s <= i))) sc[j] = -INFINITY;
      mx = fmaxf(mx, sc[j]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 1, 64)); mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 4, 64)); mx = fmaxf(mx, __shfl_xor(mx, 8, 64));
    const float m_new = fmaxf(m, mx), m_use = m_new == -INFINITY ? 0.0f : m_new;      // (a row that has seen no key yet: every term below is exp2(-inf) = 0)
    const float alpha = exp2f(m - m_use);
    float ps = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { const float p = exp2f(sc[j] - m_use); Ps[r][c + 16 * j] = p; ps += p; }
    l = l * alpha + ps;
    m = m_new;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] *= alpha;
    for (int kk = 0; kk < 64; ++kk) {
      const float p = Ps[r][kk];
      const float4 v = *reinterpret_cast<const float4*>(&Vs[kk][c * 4]);
      acc[0] = fmaf(p, v.x, acc[0]); acc[1] = fmaf(p, v.y, acc[1]); acc[2] = fmaf(p, v.z, acc[2]); acc[3] = fmaf(p, v.w, acc[3]);
    }
  }
  l += __shfl_xor(l, 1, 64); l += __shfl_xor(l, 2, 64); l += __shfl_xor(l, 4, 64); l += __shfl_xor(l, 8, 64);
  if (i < n) {
    const float inv = l > 0.0f ? 1.0f / l : 0.0f;               // a pad slot has no visible key: zeros
    float* O = reinterpret_cast<float*>(a.out) + (size_t)(b * n + i) * a.ld_out + h * 64 + c * 4;
    *reinterpret_cast<float4*>(O) = make_float4(acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[3] * inv);
  }
}

// ------------------------------------------------------------------------------------ bf16
// LDS: Ks [64 keys][72] bf16 (144-byte rows: the 16 keys of an A fragment land on 16 different 16-byte slots), Vt [64 dims][68] bf16 = V transposed
// (136-byte rows), so a V^T fragment is two 8-byte reads of four consecutive keys each.
template <bool SELF>
__global__ __launch_bounds__(256) void prompt_attn_bf16_kernel(const PromptAttnArgs a) {
  constexpr int QT = PA_QT_BF16, KS_LD = 72, VT_LD = 68;
  __shared__ __attribute__((aligned(16))) bf16_t Ks[64 * KS_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[64 * VT_LD];
  const int b = blockIdx.x, h = blockIdx.y, tile = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, g = lane >> 4;
  const int n = a.n, pad = a.key_start ? a.key_start[b] : 0;
  int k_begin, k_total;
  const PaAddr<bf16_t> ad = pa_addr<bf16_t, SELF>(a, b, h, k_begin, k_total);
  const int i = tile * QT + wave * 16 + fr;                     // this lane's query slot (the column of the transposed tiles)
  const bool active = i < n && i >= pad;
  const int k_end = SELF ? min(k_total, tile * QT + QT) : k_total;
  bf16x8_t qf[2];                                               // B operand of S^T = K Q^T: Q[i][32 ks + 8 g + j]
  qf[0] = bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0}; qf[1] = qf[0];
  if (active) {
    const bf16_t* Q = reinterpret_cast<const bf16_t*>(a.q) + (size_t)(b * n + i) * a.ld_q + a.q_col0 + h * 64 + g * 8;
    qf[0] = *reinterpret_cast<const bf16x8_t*>(Q);
    qf[1] = *reinterpret_cast<const bf16x8_t*>(Q + 32);
  }
  if constexpr (SELF) {                                         // the tile's own K / V rows into the cache, pad slots included
    const int s = tile * QT + (tid >> 2), d0 = (tid & 3) * 16;
    if (s < n) {
      const bf16_t* src = ad.NEW + (size_t)s * a.ld_new + d0;
      const size_t ro = ad.crow(s) + d0;
      *reinterpret_cast<uint4*>(ad.Kw + ro) = *reinterpret_cast<const uint4*>(src + a.k_col0);
      *reinterpret_cast<uint4*>(ad.Kw + ro + 8) = *reinterpret_cast<const uint4*>(src + a.k_col0 + 8);
      *reinterpret_cast<uint4*>(ad.Vw + ro) = *reinterpret_cast<const uint4*>(src + a.v_col0);
      *reinterpret_cast<uint4*>(ad.Vw + ro + 8) = *reinterpret_cast<const uint4*>(src + a.v_col0 + 8);
    }
  }
  float m = -INFINITY, l = 0.0f;
  f32x4_t o[4];                                                 // O^T: o[dt][r] = dim 16 dt + 4 g + r of query row i
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  for (int kb = k_begin; kb < k_end; kb += 64) {
    __syncthreads();                                            // the previous block's fragment reads
    {
      const int kk = tid >> 2, s = kb + kk, d0 = (tid & 3) * 16;
      union { uint4 v[2]; bf16_t e[16]; } kx, vx;
      kx.v[0] = make_uint4(0, 0, 0, 0); kx.v[1] = kx.v[0]; vx.v[0] = kx.v[0]; vx.v[1] = kx.v[0];      // keys past the end: zeros (0 x 0, never 0 x garbage)
      if (s < k_end) {
        const bf16_t* kp = SELF ? ad.NEW + (size_t)s * a.ld_new + a.k_col0 + d0 : ad.Kc + (size_t)s * 64 + d0;
        const bf16_t* vp = SELF ? ad.NEW + (size_t)s * a.ld_new + a.v_col0 + d0 : ad.Vc + (size_t)s * 64 + d0;
        kx.v[0] = *reinterpret_cast<const uint4*>(kp); kx.v[1] = *reinterpret_cast<const uint4*>(kp + 8);
        vx.v[0] = *reinterpret_cast<const uint4*>(vp); vx.v[1] = *reinterpret_cast<const uint4*>(vp + 8);
      }
      *reinterpret_cast<uint4*>(Ks + kk * KS_LD + d0) = kx.v[0];
      *reinterpret_cast<uint4*>(Ks + kk * KS_LD + d0 + 8) = kx.v[1];
#pragma unroll
      for (int e = 0; e < 16; ++e) Vt[(d0 + e) * VT_LD + kk] = vx.e[e];
    }
    __syncthreads();
    // ---- S^T tiles: st[t][r] = score of key kb + 16 t + 4 g + r against query row i
    f32x4_t st[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      st[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(Ks + (16 * t + fr) * KS_LD + 32 * ks + 8 * g);
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], st[t], 0, 0, 0);
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int s = kb + 16 * t + 4 * g + r;
        const bool vis = active && s < k_end && (!SELF || s <= i);
        st[t][r] = vis ? st[t][r] * PA_LOG2E : -INFINITY;
        mx = fmaxf(mx, st[t][r]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64)); mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m, mx), m_use = m_new == -INFINITY ? 0.0f : m_new;
    const float alpha = exp2f(m - m_use);
    float ps = 0.0f;
    // the probabilities, rounded to bf16, as the B operand of O^T = V^T P^T: element j of k-step u is key 32 u + 16 (j >> 2) + 4 g + (j & 3); the
    // normaliser sums the ROUNDED values, so numerator and denominator carry the same weights
    bf16x8_t pf[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      uint32_t w[4];
#pragma unroll
      for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
          const float p0 = exp2f(st[2 * u + hh][2 * pr] - m_use), p1 = exp2f(st[2 * u + hh][2 * pr + 1] - m_use);
          const uint32_t pk = pack_bf16x2(p0, p1);
          ps += __uint_as_float(pk << 16) + __uint_as_float(pk & 0xffff0000u);
          w[2 * hh + pr] = pk;
        }
      pf[u] = __builtin_bit_cast(bf16x8_t, make_uint4(w[0], w[1], w[2], w[3]));
    }
    l = l * alpha + ps;
    m = m_new;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      o[dt] *= alpha;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const bf16_t* vrow = Vt + (16 * dt + fr) * VT_LD + 32 * u + 4 * g;
        const uint2 lo = *reinterpret_cast<const uint2*>(vrow), hi = *reinterpret_cast<const uint2*>(vrow + 16);
        const bf16x8_t vf = __builtin_bit_cast(bf16x8_t, make_uint4(lo.x, lo.y, hi.x, hi.y));
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[u], o[dt], 0, 0, 0);
      }
    }
  }
  l += __shfl_xor(l, 16, 64); l += __shfl_xor(l, 32, 64);
  if (i < n) {
    const float inv = l > 0.0f ? 1.0f / l : 0.0f;               // a pad slot has no visible key: zeros
    bf16_t* O = reinterpret_cast<bf16_t*>(a.out) + (size_t)(b * n + i) * a.ld_out + h * 64 + 4 * g;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      uint2 w;
      w.x = pack_bf16x2(o[dt][0] * inv, o[dt][1] * inv);
      w.y = pack_bf16x2(o[dt][2] * inv, o[dt][3] * inv);
      *reinterpret_cast<uint2*>(O + 16 * dt) = w;
    }
  }
}

}  // namespace

template <typename T>
void launch_prompt_attention(const PromptAttnArgs& a, int batch, hipStream_t s) {
  constexpr bool lo = std::is_same<T, bf16_t>::value;
  constexpr int align = lo ? 8 : 4, QT = lo ? PA_QT_BF16 : PA_QT_F32;
  ASR_REQUIRE(batch >= 1 && a.n >= 1 && a.n_heads >= 1 && a.q && a.k_base && a.v_base && a.out, "prompt attention: bad argument");
  ASR_REQUIRE((a.kv_new != nullptr) != (a.plan != nullptr), "prompt attention: self-attention takes kv_new, cross-attention the plan");
  ASR_REQUIRE((a.ld_q % align) == 0 && (a.q_col0 % align) == 0 && (a.ld_out % align) == 0 && (a.ld_new % align) == 0 && (a.k_col0 % align) == 0 &&
              (a.v_col0 % align) == 0 && (a.stride_b % align) == 0 && (a.stride_h % align) == 0 && (a.page_stride % align) == 0,
              "prompt attention: strides and column offsets must be multiples of %d elements", align);
  const dim3 grid(batch, a.n_heads, (a.n + QT - 1) / QT);
  ASR_REQUIRE(grid.y <= 65535 && grid.z <= 65535, "prompt attention: grid too large");
  if (a.kv_new) {
    if constexpr (lo) hipLaunchKernelGGL(prompt_attn_bf16_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(prompt_attn_f32_kernel<true>, grid, dim3(256), 0, s, a);
  } else {
    ASR_REQUIRE(!a.page_table, "prompt attention: the cross-attention slabs are not paged");
    if constexpr (lo) hipLaunchKernelGGL(prompt_attn_bf16_kernel<false>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(prompt_attn_f32_kernel<false>, grid, dim3(256), 0, s, a);
  }
  HIP_CHECK(hipGetLastError());
}
template void launch_prompt_attention<float>(const PromptAttnArgs&, int, hipStream_t);
template void launch_prompt_attention<bf16_t>(const PromptAttnArgs&, int, hipStream_t);
