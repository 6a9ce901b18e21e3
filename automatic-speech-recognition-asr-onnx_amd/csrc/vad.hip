// Energy VAD (kernels.h): frame energies and levels of a ragged batch in one launch, then floor / peak / threshold, the mask, the run rules and the cuts of long
// runs in one launch with one workgroup per utterance, then one launch that packs the batch's segments in order. The statement: include/asr_mi355x.h.
#include "kernels.h"
#include "pcm.h"

namespace {

constexpr int V1_THREADS = 256;              // stage 1: 16 groups of 16 lanes, a group sums one analysis frame at a time
constexpr int V1_GROUP = 16;
constexpr int V2_THREADS = 1024;             // stage 2: 16 waves; a thread owns ceil(words / 1024) consecutive 64-frame mask words
constexpr int V2_INF = 1 << 28;              // "no delimiter on this side": a run that reaches it is endless

// ---------------------------------------------------------------- stage 1

// The samples of a 16-byte vector as Pcm<S>::raw_t
template <typename S> struct Vec16;
template <> struct Vec16<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void get(const uint4& v, float (&r)[4]) {
    r[0] = __uint_as_float(v.x); r[1] = __uint_as_float(v.y); r[2] = __uint_as_float(v.z); r[3] = __uint_as_float(v.w);
  }
};
template <> struct Vec16<int16_t> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void get(const uint4& v, int (&r)[8]) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { r[2 * i] = (int)(int16_t)(w[i] & 0xffffu); r[2 * i + 1] = (int)w[i] >> 16; }
  }
};
template <> struct Vec16<_Float16> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void get(const uint4& v, uint32_t (&r)[8]) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { r[2 * i] = w[i] & 0xffffu; r[2 * i + 1] = w[i] >> 16; }
  }
};

// x^2 of the channel mean of one input frame, loaded sample by sample (2-byte alignment only)
template <typename S, int C>
__device__ __forceinline__ float frame_sq(const S* p, int nch, float inv) {
  typedef typename Pcm<S>::raw_t raw_t;
  float m;
  if constexpr (C != 0) {
    raw_t rv[C];
#pragma unroll
    for (int c = 0; c < C; ++c) rv[c] = Pcm<S>::load(p, c);
#pragma unroll
    for (int c = 0; c < C; ++c) rv[c] = Pcm<S>::hold(rv[c]);
    m = Pcm<S>::widen(rv[0], 1.0f);
#pragma unroll
    for (int c = 1; c < C; ++c) m += Pcm<S>::widen(rv[c], 1.0f);
  } else {
    m = Pcm<S>::widen(Pcm<S>::hold(Pcm<S>::load(p, 0)), 1.0f);
    for (int c = 1; c < nch; ++c) m += Pcm<S>::widen(Pcm<S>::hold(Pcm<S>::load(p, c)), 1.0f);            // the sum runs in channel order
  }
  m *= inv;
  return m * m;
}

// One workgroup = up to VAD_TILE_F consecutive analysis frames of one utterance. A group of 16 lanes owns one analysis frame at a time: its H * channels samples
// are contiguous, so where an input frame is 2, 4 or 8 bytes and the utterance starts on a multiple of that, the group reads the 16-byte-aligned middle of the
// span as 16-byte vectors and only the few input frames before and after it sample by sample; otherwise (three channels and up, or an odd start) every input frame
// is read sample by sample, as the resampler does. Nothing outside [frame start, min(n, frame start + H)) is read. The 16 partial sums meet in wave (xor 8, 4, 2, 1);
// lane 0 of the group writes e and q and counts q in the workgroup's LDS histogram, which is flushed with integer atomics: the histogram is exact in any order.
// C: interleaved channels known at compile time (1, 2), or 0 = a.channels.
template <typename S, int C>
__global__ __launch_bounds__(V1_THREADS) void vad_energy_kernel(const VadArgs a) {
  __shared__ int hist[VAD_LEVELS];
  const int tid = threadIdx.x, sub = tid & (V1_GROUP - 1), grp = tid / V1_GROUP;
  const int u = a.tile_utt[blockIdx.x], f0 = a.tile_f0[blockIdx.x];
  const VadUtt ut = a.utt[u];
  for (int i = tid; i < VAD_LEVELS; i += V1_THREADS) hist[i] = 0;
  __syncthreads();
  const int nch = C ? C : a.channels, H = a.H;
  const float inv = 1.0f / (float)nch;
  const int nf = min(VAD_TILE_F, ut.F - f0);
  const S* src = static_cast<const S*>(a.audio) + ut.in_off * nch;
  constexpr int SFB = (C ? C : 3) * (int)sizeof(S);          // bytes of an input frame, where the vector path can apply
  const bool vec = C != 0 && (reinterpret_cast<uintptr_t>(src) % SFB) == 0;

  for (int it = 0; it * (V1_THREADS / V1_GROUP) < nf; ++it) {                   // uniform trip count: every lane takes part in the shuffles
    const int fi = it * (V1_THREADS / V1_GROUP) + grp;
    const int64_t i0 = (int64_t)(f0 + fi) * H;
    const int cnt = fi < nf ? (int)(ut.n - i0 < H ? ut.n - i0 : H) : 0;
    float acc = 0.f;
    if (cnt > 0) {
      const S* fp = src + i0 * nch;
      if (vec) {
        const uintptr_t p0 = reinterpret_cast<uintptr_t>(fp), bytes = (uintptr_t)cnt * SFB;
        const uintptr_t al = (p0 + 15) & ~(uintptr_t)15;
        const int head = (int)(al - p0 < bytes ? al - p0 : bytes);                             // a multiple of SFB: p0 is one, 16 is one
        const int nvec = (int)((bytes - head) / 16), body_end = head + nvec * 16;
        const int head_n = head / SFB, tail_n = ((int)bytes - body_end) / SFB;
        const uint4* vp = reinterpret_cast<const uint4*>(al);
        for (int v0 = 0; v0 < nvec; v0 += 4 * V1_GROUP) {                       // four vectors requested before the first is used
          uint4 rv[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int v = v0 + sub + j * V1_GROUP;
            rv[j] = v < nvec ? vp[v] : make_uint4(0, 0, 0, 0);                  // (zero bits are the sample 0 in all three types)
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            typename Pcm<S>::raw_t r[Vec16<S>::N];
            Vec16<S>::get(rv[j], r);
            constexpr int CC = C ? C : 1;
#pragma unroll
            for (int i = 0; i < Vec16<S>::N; i += CC) {
              float m = Pcm<S>::widen(r[i], 1.0f);
#pragma unroll
              for (int c = 1; c < CC; ++c) m += Pcm<S>::widen(r[i + c], 1.0f);
              m *= inv;
              acc = fmaf(m, m, acc);
            }
          }
        }
        for (int j = sub; j < head_n + tail_n; j += V1_GROUP) {
          const int sf = j < head_n ? j : body_end / SFB + (j - head_n);
          acc += frame_sq<S, C>(fp + (int64_t)sf * nch, nch, inv);
        }
      } else {
        for (int j = sub; j < cnt; j += V1_GROUP) acc += frame_sq<S, C>(fp + (int64_t)j * nch, nch, inv);
      }
    }
#pragma unroll
    for (int d = V1_GROUP / 2; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
    if (sub == 0 && fi < nf) {
      const int q = vad_level(acc);
      a.energy[ut.f_off + f0 + fi] = acc;
      a.level[ut.f_off + f0 + fi] = q;
      atomicAdd(&hist[q], 1);
    }
  }
  __syncthreads();
  for (int i = tid; i < VAD_LEVELS; i += V1_THREADS)
    if (hist[i]) atomicAdd(&a.hist[(size_t)u * VAD_LEVELS + i], hist[i]);
}

// ---------------------------------------------------------------- stage 2

__device__ __forceinline__ uint64_t bit_range(int s, int e) {                    // bits [s, e), 0 <= s < e <= 64
  const uint64_t hi = e >= 64 ? ~0ull : ((1ull << e) - 1);
  return hi & ~((1ull << s) - 1);
}

// exclusive scan over the 1024 threads (Hillis-Steele in LDS); reverse: from the last thread down. op(v, ident) == v.
template <typename Op>
__device__ int block_scan_excl(int v, int ident, int* buf, bool reverse, Op op) {
  const int t = reverse ? V2_THREADS - 1 - (int)threadIdx.x : (int)threadIdx.x;
  buf[t] = v;
  __syncthreads();
  for (int d = 1; d < V2_THREADS; d <<= 1) {
    const int o = t >= d ? buf[t - d] : ident;
    __syncthreads();
    v = op(v, o);
    buf[t] = v;
    __syncthreads();
  }
  const int r = t ? buf[t - 1] : ident;
  __syncthreads();
  return r;
}
struct OpMax { __device__ int operator()(int a, int b) const { return a > b ? a : b; } };
struct OpMin { __device__ int operator()(int a, int b) const { return a < b ? a : b; } };
struct OpAdd { __device__ int operator()(int a, int b) const { return a + b; } };

enum { RULE_MIN_SPEECH = 0, RULE_MIN_PAUSE = 1, RULE_PAD = 2 };

// One rule over the whole mask, in place. The rule looks at the runs of ones of w' -- the mask itself for MIN_SPEECH, its complement (the pauses) for the other
// two -- and keeps of each run [gs, ge) a part [ns, ne), clearing the rest:
//   MIN_SPEECH: all of it when ge - gs >= k, else nothing. Outside [0, F) there is no speech: the delimiters default to -1 and F.
//   MIN_PAUSE:  all of it when ge - gs >= k or the pause reaches an end of the utterance (it is not between two speech runs), else nothing.
//   PAD:        [gs + k, ge - k), without the + k / - k on a side that reaches an end of the utterance; nothing when that is empty (the runs touch: one run).
// A pause that reaches an end has no delimiter on that side: -V2_INF / +V2_INF. A thread learns the last delimiter before and the first after its words from two
// scans over the threads' own last / first delimiters, then walks the runs of its words with ctz; it writes only its own words, from what it read of them before.
template <int RULE>
__device__ void run_rule(uint64_t* words, int nwords, int wpt, int F, int k, int* buf) {
  const int t = threadIdx.x, w0 = min(nwords, t * wpt), w1 = min(nwords, w0 + wpt);
  const bool inv = RULE != RULE_MIN_SPEECH;
  int first = inv ? V2_INF : F, last = inv ? -V2_INF : -1;
  for (int j = w0; j < w1; ++j) {
    const uint64_t z = inv ? words[j] : ~words[j];                              // the delimiters: zeros of w' (complement: bits past F are ones of w', no delimiters)
    if (z) {
      if (first == (inv ? V2_INF : F)) first = j * 64 + __builtin_ctzll(z);
      last = j * 64 + 63 - __builtin_clzll(z);
    }
  }
  if (!inv) first = min(first, F);
  int ld = block_scan_excl(last, inv ? -V2_INF : -1, buf, false, OpMax());
  const int nd_chunk = block_scan_excl(first, inv ? V2_INF : F, buf, true, OpMin());
  for (int j = w0; j < w1; ++j) {
    const int wbase = j * 64;
    const uint64_t wp = inv ? ~words[j] : words[j];
    uint64_t x = wp, out = wp;
    while (x) {
      const int s = __builtin_ctzll(x);
      const uint64_t y = ~(x >> s);
      const int e = s + (y ? __builtin_ctzll(y) : 64);                           // (x >> s has s zeros on top, so the count stops at 64 - s)
      const int gs = s == 0 ? ld + 1 : wbase + s;
      int ge = wbase + e;
      if (e == 64) {                                                             // the run goes on: the first delimiter in my later words, or past them
        ge = nd_chunk;
        for (int jj = j + 1; jj < w1; ++jj) {
          const uint64_t z = inv ? words[jj] : ~words[jj];
          if (z) { ge = jj * 64 + __builtin_ctzll(z); break; }
        }
        if (!inv) ge = min(ge, F);
      }
      int ns = gs, ne = ge;
      if (RULE == RULE_MIN_SPEECH) { if (ge - gs < k) ne = ns; }
      else if (RULE == RULE_MIN_PAUSE) { if (gs >= 0 && ge < V2_INF && ge - gs < k) ne = ns; }
      else { if (gs >= 0) ns = gs + k; if (ge < V2_INF) ne = ge - k; }
      const uint64_t run = bit_range(s, e);
      if (ne <= ns) out &= ~run;
      else {
        const int ls = min(max(ns - wbase, s), e), le = min(max(ne - wbase, s), e);
        if (le <= ls) out &= ~run; else out &= ~run | bit_range(ls, le);
      }
      x &= ~run;
    }
    const uint64_t z = ~wp;
    if (z) ld = wbase + 63 - __builtin_clzll(z);
    uint64_t res = inv ? ~out : out;
    if (j == nwords - 1 && (F & 63)) res &= (1ull << (F & 63)) - 1;
    words[j] = res;
  }
  __syncthreads();
}

// The segments of the final mask, in order. A thread walks the run starts of its words; a run no longer than max_frames is one segment. A longer one is cut by the
// whole wave: the lanes that hold one take turns, and for each cut the 64 lanes share the window [start + max_frames / 2, start + max_frames], each keeping the
// smallest (q << 20) | (0xfffff - frame) it saw -- lowest level first, latest frame on a tie -- and the wave's minimum names the cut. WRITE == false counts
// (returns the thread's segments), WRITE == true writes them from slot idx on.
template <bool WRITE>
__device__ int emit_segments(const uint64_t* words, int nwords, int wpt, int F, int max_frames, int nd_chunk, const int32_t* q, int32_t* seg, int idx) {
  const int t = threadIdx.x, lane = t & 63, w0 = min(nwords, t * wpt), w1 = min(nwords, w0 + wpt);
  int count = 0;
  for (int jo = 0; jo < wpt; ++jo) {                                             // uniform trip counts: the wave works together below
    const int j = w0 + jo;
    const bool valid = j < w1;
    const uint64_t w = valid ? words[j] : 0;
    const uint64_t prev = valid && j > 0 ? words[j - 1] >> 63 : 0;
    uint64_t starts = w & ~((w << 1) | prev);
    while (__any(starts != 0)) {
      const bool have = starts != 0;
      int gs = 0, ge = 0;
      if (have) {
        const int s = __builtin_ctzll(starts);
        starts &= starts - 1;
        const uint64_t y = ~(w >> s);
        const int e = s + (y ? __builtin_ctzll(y) : 64);
        gs = j * 64 + s; ge = j * 64 + e;
        if (e == 64) {
          ge = nd_chunk;
          for (int jj = j + 1; jj < w1; ++jj)
            if (~words[jj]) { ge = jj * 64 + __builtin_ctzll(~words[jj]); break; }
          ge = min(ge, F);
        }
      }
      const bool is_long = have && ge - gs > max_frames;
      if (have && !is_long) {
        if (WRITE && idx + count < F) { seg[2 * (idx + count)] = gs; seg[2 * (idx + count) + 1] = ge; }
        ++count;
      }
      uint64_t todo = __ballot(is_long);
      while (todo) {
        const int srcl = __builtin_ctzll(todo);
        todo &= todo - 1;
        int rs = __shfl(gs, srcl);
        const int re = __shfl(ge, srcl), at = __shfl(idx + count, srcl);
        int n = 0;
        while (re - rs > max_frames) {
          const int lo = rs + max_frames / 2, hi = rs + max_frames;            // hi < re <= F
          int key = 0x7fffffff;
          for (int f = lo + lane; f <= hi; f += 64) key = min(key, (q[f] << 20) | (0xfffff - f));
#pragma unroll
          for (int d = 32; d >= 1; d >>= 1) key = min(key, __shfl_xor(key, d));
          const int c = 0xfffff - (key & 0xfffff);
          if (WRITE && lane == 0 && at + n < F) { seg[2 * (at + n)] = rs; seg[2 * (at + n) + 1] = c; }
          ++n;
          rs = c;
        }
        if (WRITE && lane == 0 && at + n < F) { seg[2 * (at + n)] = rs; seg[2 * (at + n) + 1] = re; }
        ++n;
        if (lane == srcl) count += n;
      }
    }
  }
  return count;
}

// One workgroup per utterance; the mask of its F frames is ceil(F / 64) 64-bit words of dynamic LDS (128 KiB at 2^20 frames).
__global__ __launch_bounds__(V2_THREADS) void vad_segment_kernel(const VadArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint64_t v2_words[];
  __shared__ int buf[V2_THREADS];
  __shared__ int s_floor, s_peak;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, u = blockIdx.x;
  const VadUtt ut = a.utt[u];
  const int F = ut.F;
  if (t == 0) { s_floor = 0; s_peak = 0; }
  // ---- floor and peak from the histogram: bin t's cumulative count, by a scan over the bins
  const int h = a.hist[(size_t)u * VAD_LEVELS + t];
  const int below = block_scan_excl(h, 0, buf, false, OpAdd());                 // (its barriers also order the two stores above)
  if (F > 0 && below < ut.need && below + h >= ut.need) s_floor = t;            // one bin
  if (h) atomicMax(&s_peak, t);
  __syncthreads();
  const int thr = max(a.r.abs_level, min(s_floor + a.r.margin, s_peak - a.r.peak_drop));
  if (t == 0) { a.stats[3 * u] = s_floor; a.stats[3 * u + 1] = s_peak; a.stats[3 * u + 2] = thr; }
  if (F == 0) { if (t == 0) a.seg_count[u] = 0; return; }
  // ---- the raw mask, 64 frames a ballot
  const int nwords = (F + 63) / 64, wpt = (nwords + V2_THREADS - 1) / V2_THREADS;
  const int32_t* q = a.level + ut.f_off;
  for (int w = wave; w < nwords; w += V2_THREADS / 64) {
    const int f = w * 64 + lane;
    const uint64_t b = __ballot(f < F && q[f] >= thr);
    if (lane == 0) v2_words[w] = b;
  }
  __syncthreads();
  run_rule<RULE_MIN_SPEECH>(v2_words, nwords, wpt, F, a.r.min_speech, buf);
  run_rule<RULE_MIN_PAUSE>(v2_words, nwords, wpt, F, a.r.min_pause, buf);
  run_rule<RULE_PAD>(v2_words, nwords, wpt, F, a.r.pad, buf);
  // ---- count, prefix sum, write
  const int w0 = min(nwords, t * wpt), w1 = min(nwords, w0 + wpt);
  int first = F;
  for (int j = w0; j < w1; ++j)
    if (~v2_words[j]) { first = min(F, j * 64 + __builtin_ctzll(~v2_words[j])); break; }
  const int nd_chunk = block_scan_excl(first, F, buf, true, OpMin());
  int32_t* seg = a.seg_tmp + 2 * ut.f_off;
  const int mine = emit_segments<false>(v2_words, nwords, wpt, F, a.r.max_frames, nd_chunk, q, seg, 0);
  const int before = block_scan_excl(mine, 0, buf, false, OpAdd());
  if (t == V2_THREADS - 1) a.seg_count[u] = before + mine;
  emit_segments<true>(v2_words, nwords, wpt, F, a.r.max_frames, nd_chunk, q, seg, before);
}

// Utterance u's segments, from analysis frames to the caller's input-frame offsets, behind those of the utterances before it; nothing at or past seg_cap.
__global__ __launch_bounds__(256) void vad_pack_kernel(const VadArgs a) {
  __shared__ long long part[256];
  const int tid = threadIdx.x, u = blockIdx.x;
  long long sum = 0;
  for (int v = tid; v < u; v += 256) sum += a.seg_count[v];
  part[tid] = sum;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if (tid < d) part[tid] += part[tid + d];
    __syncthreads();
  }
  const long long base = part[0];
  const VadUtt ut = a.utt[u];
  const int cnt = min(a.seg_count[u], ut.F);
  const int32_t* seg = a.seg_tmp + 2 * ut.f_off;
  for (int i = tid; i < cnt; i += 256) {
    const long long o = base + i;
    if (o >= a.seg_cap) break;
    a.seg_out[2 * o] = ut.abs_off + (int64_t)seg[2 * i] * a.H;
    const int64_t e = (int64_t)seg[2 * i + 1] * a.H;
    a.seg_out[2 * o + 1] = ut.abs_off + (e < ut.n ? e : (int64_t)ut.n);
    if (a.seg_utt) a.seg_utt[o] = u;
  }
}

template <typename S>
void launch_energy(const VadArgs& a, int n_tiles, hipStream_t s) {
  auto k = a.channels == 1 ? vad_energy_kernel<S, 1> : a.channels == 2 ? vad_energy_kernel<S, 2> : vad_energy_kernel<S, 0>;
  hipLaunchKernelGGL(k, dim3(n_tiles), dim3(V1_THREADS), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

}  // namespace

void launch_vad(const VadArgs& a, int n_tiles, hipStream_t s) {
  ASR_REQUIRE(a.batch >= 1 && a.H >= 1, "vad: empty batch");
  ASR_REQUIRE(a.channels >= 1 && a.channels <= 8, "vad: %d channels (1..8)", a.channels);
  ASR_REQUIRE(a.max_F >= 0 && a.max_F <= VAD_MAX_F, "vad: %d analysis frames in one utterance (at most %d)", a.max_F, VAD_MAX_F);
  ASR_REQUIRE(a.r.max_frames >= 2, "vad: max_frames %d (at least 2)", a.r.max_frames);
  ASR_REQUIRE(a.r.min_speech >= 0 && a.r.min_pause >= 0 && a.r.pad >= 0 && a.r.min_speech <= VAD_MAX_F && a.r.min_pause <= VAD_MAX_F && a.r.pad <= VAD_MAX_F &&
              a.r.max_frames <= V2_INF, "vad: a run length is negative or beyond %d frames", VAD_MAX_F);
  HIP_CHECK(hipMemsetAsync(a.hist, 0, (size_t)a.batch * VAD_LEVELS * 4, s));
  if (n_tiles > 0) switch (a.audio_dtype) {
    case AUDIO_F32: launch_energy<float>(a, n_tiles, s); break;
    case AUDIO_I16: launch_energy<int16_t>(a, n_tiles, s); break;
    case AUDIO_F16: launch_energy<_Float16>(a, n_tiles, s); break;
    default: ASR_THROW(ASR_ERR_INVALID, "vad: unknown audio sample type %d", a.audio_dtype);
  }
  const size_t lds = (size_t)((a.max_F + 63) / 64) * 8;
  static PerDeviceOnce attr_once;
  if (attr_once.first())
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(vad_segment_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, VAD_MAX_F / 8));
  hipLaunchKernelGGL(vad_segment_kernel, dim3(a.batch), dim3(V2_THREADS), lds, s, a);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(vad_pack_kernel, dim3(a.batch), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}
