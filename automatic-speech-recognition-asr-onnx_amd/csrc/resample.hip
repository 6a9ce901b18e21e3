// Device resampler (kernels.h): any sample rate and channel count -> model-rate mono f32, one launch over a ragged batch.
#include "kernels.h"
#include "pcm.h"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_NF = 4;                     // frames a thread requests per staging pass
constexpr int RS_LDS_FLOATS = 15360;         // 60 KiB: the input span of a tile

double bessel_i0(double x) {                 // sum_k ((x / 2)^k / k!)^2
  const double h = 0.5 * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= h / k;
    const double t2 = term * term;
    sum += t2;
    if (t2 < 1e-20 * sum) break;
  }
  return sum;
}

int span_of(const ResampleDesign& d, int tile) { return (int)(((int64_t)(d.L - 1) + (int64_t)(tile - 1) * d.M) / d.L) + d.T; }

// The multiply-adds of a tile whose input span is staged in rs_x (slot 0 = frame floor(n0 M / L) - W, r0 = (n0 M) mod L): output j is T fused multiply-adds in
// tap order against phase (r0 + j M) mod L. The offline and the streaming kernel both end in this one function: their outputs are equal bit for bit because of it.
__device__ __forceinline__ void rs_mac(const float* rs_x, const float* tab_t, float* out, int r0, int nt, int L, int M, int T, int tid) {
  if (L == 1) {                                          // one phase: c[k] is wave-uniform, four outputs per thread share it
    const float* x[4];
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) x[r] = rs_x + min(tid + r * RS_THREADS, nt - 1) * M;      // (outputs past nt repeat the last one and are not stored)
    for (int k = 0; k < T; ++k) {
      const float ck = tab_t[k];
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = fmaf(ck, x[r][k], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (tid + r * RS_THREADS < nt) out[tid + r * RS_THREADS] = acc[r];
    return;
  }
  for (int j = tid; j < nt; j += RS_THREADS) {
    const int t = r0 + j * M, ir = t / L, p = t - ir * L;
    const float* x = rs_x + ir;
    const float* c = tab_t + p;
    float acc = 0.f;
#pragma unroll 4
    for (int k = 0; k < T; ++k) acc = fmaf(c[(size_t)k * L], x[k], acc);
    out[j] = acc;
  }
}

// One workgroup = up to d.tile consecutive outputs of one utterance. The input span they read (frames floor(n0 M / L) - W .. floor((n0 + nt - 1) M / L) + W) is
// staged in LDS as f32 once -- widening and the channel mean happen at the store, frames outside the utterance are zeros, never a neighbour's samples -- and every
// output is then T multiply-adds of LDS against its phase's coefficients. Lane j of a wave reads LDS at floor(j M / L) + k: stride M / L (3 at 48 kHz: no bank
// conflict). The table is stored tap-major, [T][L], so that at tap k a wave touches one row of L floats whatever the phases of its lanes (consecutive outputs take
// phases (n M) mod L, which are not consecutive: 160 rows apart at 44.1 kHz in a phase-major table); at L == 1 the coefficient is wave-uniform and is fetched
// once for the four outputs of a thread.
// C: interleaved channels known at compile time (1, 2), or 0 = a.channels.
template <typename S, int C>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const ResampleArgs a) {
  extern __shared__ __attribute__((aligned(16))) float rs_x[];
  typedef typename Pcm<S>::raw_t raw_t;
  const int tid = threadIdx.x;
  const int u = a.tile_utt[blockIdx.x], n0 = a.tile_n0[blockIdx.x];
  const RsUtt ut = a.utt[u];
  const int L = a.d.L, M = a.d.M, T = a.d.T;
  const int nt = min(a.d.tile, ut.n_out - n0);
  if (nt <= 0) return;                                   // (no such tile is listed)
  const int64_t nm0 = (int64_t)n0 * M;                   // 64-bit: n M passes 2^31 on long files
  const int64_t q0 = nm0 / L;
  const int r0 = (int)(nm0 - q0 * L);
  const int64_t base = q0 - a.d.W;                       // the input frame of LDS slot 0
  const int span = (r0 + (nt - 1) * M) / L + T;          // <= d.span_max
  const S* src = static_cast<const S*>(a.audio);
  const int nch = C ? C : a.channels;
  const float inv = 1.0f / (float)nch;

  for (int i0 = 0; i0 < span; i0 += RS_NF * RS_THREADS) {
    // every thread requests its raw samples of a pass before it converts the first (the load shape of fbank_kernel; 2-byte alignment only)
    if constexpr (C != 0) {
      raw_t rv[RS_NF][C];
#pragma unroll
      for (int j = 0; j < RS_NF; ++j) {
        const int i = i0 + tid + j * RS_THREADS;
        const int64_t f = base + i;
        const bool ok = i < span && f >= 0 && f < ut.n_in;
        const S* p = src + (ok ? (ut.in_off + f) * nch : 0);
#pragma unroll
        for (int c = 0; c < C; ++c) rv[j][c] = ok ? Pcm<S>::load(p, c) : (raw_t)0;
      }
#pragma unroll
      for (int j = 0; j < RS_NF; ++j)
#pragma unroll
        for (int c = 0; c < C; ++c) rv[j][c] = Pcm<S>::hold(rv[j][c]);
#pragma unroll
      for (int j = 0; j < RS_NF; ++j) {
        const int i = i0 + tid + j * RS_THREADS;
        float acc = Pcm<S>::widen(rv[j][0], a.scale);
#pragma unroll
        for (int c = 1; c < C; ++c) acc += Pcm<S>::widen(rv[j][c], a.scale);
        if (i < span) rs_x[i] = acc * inv;
      }
    } else {
      float acc[RS_NF];
      for (int c = 0; c < nch; ++c) {                    // channel by channel: the sum runs in channel order
        raw_t rv[RS_NF];
#pragma unroll
        for (int j = 0; j < RS_NF; ++j) {
          const int i = i0 + tid + j * RS_THREADS;
          const int64_t f = base + i;
          const bool ok = i < span && f >= 0 && f < ut.n_in;
          rv[j] = ok ? Pcm<S>::load(src + (ut.in_off + f) * nch, c) : (raw_t)0;
        }
#pragma unroll
        for (int j = 0; j < RS_NF; ++j) rv[j] = Pcm<S>::hold(rv[j]);
#pragma unroll
        for (int j = 0; j < RS_NF; ++j) {
          const float w = Pcm<S>::widen(rv[j], a.scale);
          acc[j] = c == 0 ? w : acc[j] + w;
        }
      }
#pragma unroll
      for (int j = 0; j < RS_NF; ++j) {
        const int i = i0 + tid + j * RS_THREADS;
        if (i < span) rs_x[i] = acc[j] * inv;
      }
    }
  }
  __syncthreads();

  rs_mac(rs_x, a.tab_t, a.out + ut.out_off + n0, r0, nt, L, M, T, tid);
}

template <typename S>
void launch_typed(const ResampleArgs& a, int n_tiles, hipStream_t s) {
  const size_t lds = (size_t)a.d.span_max * 4;
  auto k = a.channels == 1 ? resample_kernel<S, 1> : a.channels == 2 ? resample_kernel<S, 2> : resample_kernel<S, 0>;
  hipLaunchKernelGGL(k, dim3(n_tiles), dim3(RS_THREADS), lds, s, a);
  HIP_CHECK(hipGetLastError());
}

// ---- the streaming form (kernels.h, ResampleStreamArgs)
// One input frame as the offline kernel stages it: the samples widened, summed in channel order, times 1 / channels.
template <typename S, int C>
__device__ __forceinline__ float rs_mono(const S* p, int nch, float scale, float inv) {
  float acc = Pcm<S>::widen(Pcm<S>::load(p, 0), scale);
  if constexpr (C != 0) {
#pragma unroll
    for (int c = 1; c < C; ++c) acc += Pcm<S>::widen(Pcm<S>::load(p, c), scale);
  } else {
    for (int c = 1; c < nch; ++c) acc += Pcm<S>::widen(Pcm<S>::load(p, c), scale);
  }
  return acc * inv;
}

// One workgroup = up to d.tile consecutive outputs of one slot's step: outputs c S + j0 .. of stream sid, c = count[sid] read here (64-bit products, as above).
// Frame f of the span comes from the slot's row when f >= A(c), from the stream's carried frames (half c & 1) when A(c) - keep <= f < A(c), and is zero in front
// of the stream's first frame. Nothing past frame need(c) - 1 of the row is read: the last output of the step reads hi(c) = A(c) + need(c) - 1.
template <typename S, int C>
__global__ __launch_bounds__(RS_THREADS) void resample_stream_kernel(const ResampleStreamArgs a) {
  extern __shared__ __attribute__((aligned(16))) float rs_x[];
  const int tid = threadIdx.x;
  const int tps = (a.chunk + a.d.tile - 1) / a.d.tile;
  const int slot = blockIdx.x / tps, j0 = (blockIdx.x - slot * tps) * a.d.tile;
  const int sid = a.sid[(size_t)slot * a.sid_stride];
  const int64_t c = a.count[sid];
  const int L = a.d.L, M = a.d.M, T = a.d.T;
  const int nt = min(a.d.tile, a.chunk - j0);
  const int64_t nm0 = (c * a.chunk + j0) * M;
  const int64_t q0 = nm0 / L;
  const int r0 = (int)(nm0 - q0 * L);
  const int64_t base = q0 - a.d.W;
  const int span = (r0 + (nt - 1) * M) / L + T;          // <= d.span_max
  const int64_t A = resample_stream_start(a.d, a.chunk, c);
  const int keep = resample_stream_keep(a.d);
  const int nch = C ? C : a.channels;
  const float inv = 1.0f / (float)nch;
  const float* carried = a.hist + ((size_t)(c & 1) * a.streams + sid) * keep;
  const S* row = static_cast<const S*>(a.audio) + (size_t)slot * a.pitch * nch;
#pragma unroll 4
  for (int i = tid; i < span; i += RS_THREADS) {
    const int64_t f = base + i;
    float v = 0.f;
    if (f >= A) {
      const int64_t fr = f - A;
      if (fr < a.pitch) v = rs_mono<S, C>(row + fr * nch, nch, a.scale, inv);
    } else if (f >= 0) {
      const int64_t h = f - (A - keep);
      if (h >= 0) v = carried[h];
    }
    rs_x[i] = v;
  }
  __syncthreads();
  rs_mac(rs_x, a.tab_t, a.out + (size_t)slot * a.chunk + j0, r0, nt, L, M, T, tid);
}

// Behind the tiles, one workgroup per slot: the last `keep` frames of (carried | row[0, need(c))) go to the half the tiles did not read, then the count moves.
template <typename S, int C>
__global__ __launch_bounds__(RS_THREADS) void resample_stream_carry_kernel(const ResampleStreamArgs a) {
  const int tid = threadIdx.x, slot = blockIdx.x;
  const int sid = a.sid[(size_t)slot * a.sid_stride];
  const int c = a.count[sid];
  __syncthreads();                                       // every thread holds c before thread 0 moves it
  const int keep = resample_stream_keep(a.d), need = resample_stream_need(a.d, a.chunk, c);
  const int nch = C ? C : a.channels;
  const float inv = 1.0f / (float)nch;
  const float* carried = a.hist + ((size_t)(c & 1) * a.streams + sid) * keep;
  float* next = a.hist + ((size_t)((c + 1) & 1) * a.streams + sid) * keep;
  const S* row = static_cast<const S*>(a.audio) + (size_t)slot * a.pitch * nch;
  for (int j = tid; j < keep; j += RS_THREADS) {
    const int64_t at = (int64_t)need + j;                // position in (carried | row[0, need))
    float v = 0.f;
    if (at < keep) v = carried[at];
    else if (at - keep < a.pitch) v = rs_mono<S, C>(row + (at - keep) * nch, nch, a.scale, inv);
    next[j] = v;
  }
  if (tid == 0) {
    a.count[sid] = c + 1;
    if (a.need_out) a.need_out[slot] = need;
  }
}

template <typename S>
void launch_stream_typed(const ResampleStreamArgs& a, int n, hipStream_t s) {
  const size_t lds = (size_t)a.d.span_max * 4;
  const int tps = (a.chunk + a.d.tile - 1) / a.d.tile;
  auto k = a.channels == 1 ? resample_stream_kernel<S, 1> : a.channels == 2 ? resample_stream_kernel<S, 2> : resample_stream_kernel<S, 0>;
  auto kc = a.channels == 1 ? resample_stream_carry_kernel<S, 1> : a.channels == 2 ? resample_stream_carry_kernel<S, 2> : resample_stream_carry_kernel<S, 0>;
  hipLaunchKernelGGL(k, dim3(n * tps), dim3(RS_THREADS), lds, s, a);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(kc, dim3(n), dim3(RS_THREADS), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

}  // namespace

ResampleDesign resample_design(int rate_in, int rate_model) {
  ASR_REQUIRE(rate_in >= 1 && rate_model >= 1, "input format: sample rate %d (model rate %d): rates are positive", rate_in, rate_model);
  ResampleDesign d{};
  if (rate_in == rate_model) {
    d.L = d.M = d.T = 1; d.W = 0;
  } else {
    const int g = std::gcd(rate_in, rate_model);
    d.L = rate_model / g; d.M = rate_in / g;
    ASR_REQUIRE(d.L <= 1024, "input format: %d Hz -> %d Hz needs %d filter phases (at most 1024: the rates must share a larger factor)", rate_in, rate_model, d.L);
    const double fc = 0.945 * std::min(1.0, (double)d.L / d.M);
    const double w = std::ceil(32.0 / fc);
    ASR_REQUIRE(w < (double)RS_LDS_FLOATS, "input format: %d Hz is too far above the model's %d Hz (the filter of one output does not fit in LDS)", rate_in, rate_model);
    d.W = (int)w; d.T = 2 * d.W + 1;
  }
  for (int tile : {1024, 512, 256})
    if (span_of(d, tile) <= RS_LDS_FLOATS) { d.tile = tile; d.span_max = span_of(d, tile); return d; }
  ASR_THROW(ASR_ERR_INVALID, "input format: %d Hz is too far above the model's %d Hz (the input span of 256 outputs does not fit in LDS)", rate_in, rate_model);
}

void resample_table(const ResampleDesign& d, float* coeffs) {
  if (d.T == 1) { coeffs[0] = 1.0f; return; }            // the pure down-mix
  const double fc = 0.945 * std::min(1.0, (double)d.L / d.M), i0_9 = bessel_i0(9.0), pi = 3.14159265358979323846;
  for (int p = 0; p < d.L; ++p)
    for (int k = 0; k < d.T; ++k) {
      const double t = ((double)(k - d.W) - (double)p / d.L) * fc;
      double c = 0.0;
      if (std::fabs(t) < 32.0) {
        const double sinc = t == 0.0 ? 1.0 : std::sin(pi * t) / (pi * t), r = t / 32.0;
        c = fc * sinc * bessel_i0(9.0 * std::sqrt(1.0 - r * r)) / i0_9;
      }
      coeffs[(size_t)p * d.T + k] = (float)c;
    }
}

void launch_resample(const ResampleArgs& a, int n_tiles, hipStream_t s) {
  if (n_tiles <= 0) return;
  ASR_REQUIRE(a.channels >= 1 && a.channels <= 8, "resample: %d channels (1..8)", a.channels);
  ASR_REQUIRE(a.d.span_max == span_of(a.d, a.d.tile) && a.d.span_max <= RS_LDS_FLOATS && a.d.tile <= 4 * RS_THREADS, "resample: inconsistent design");
  switch (a.audio_dtype) {
    case AUDIO_F32: launch_typed<float>(a, n_tiles, s); break;
    case AUDIO_I16: launch_typed<int16_t>(a, n_tiles, s); break;
    case AUDIO_F16: launch_typed<_Float16>(a, n_tiles, s); break;
    default: ASR_THROW(ASR_ERR_INVALID, "resample: unknown audio sample type %d", a.audio_dtype);
  }
}

void launch_resample_stream(const ResampleStreamArgs& a, int n, hipStream_t s) {
  if (n <= 0) return;
  ASR_REQUIRE(a.channels >= 1 && a.channels <= 8, "resample: %d channels (1..8)", a.channels);
  ASR_REQUIRE(a.d.span_max == span_of(a.d, a.d.tile) && a.d.span_max <= RS_LDS_FLOATS && a.d.tile <= 4 * RS_THREADS, "resample: inconsistent design");
  ASR_REQUIRE(a.chunk >= 1 && a.pitch == resample_stream_pitch(a.d, a.chunk) && a.streams >= 1 && a.sid_stride >= 1 && a.audio && a.sid && a.count && a.out &&
              (a.hist || resample_stream_keep(a.d) == 0), "resample: bad streaming argument");
  switch (a.audio_dtype) {
    case AUDIO_F32: launch_stream_typed<float>(a, n, s); break;
    case AUDIO_I16: launch_stream_typed<int16_t>(a, n, s); break;
    case AUDIO_F16: launch_stream_typed<_Float16>(a, n, s); break;
    default: ASR_THROW(ASR_ERR_INVALID, "resample: unknown audio sample type %d", a.audio_dtype);
  }
}
