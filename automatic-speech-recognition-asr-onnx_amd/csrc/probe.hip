// Probe / test-hook library (libasr_mi355x_probe.so): timing probes and kernel-selection hooks that are NOT part of the product
// C ABI (include/asr_mi355x.h). Links against libasr_mi355x.so and calls its internal launchers; declared in
// include/asr_mi355x_probe.h, bound by automatic-speech-recognition-asr-onnx_amd/_probe.py, used by tests/ and tools/ only.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/asr_mi355x.h"
#include "../../include/asr_mi355x_probe.h"
#include "decode_head.h"
#include "engine.h"
#include "gemm.h"
#include "kernels.h"
#include "qwen_attn.h"

namespace {

struct Tmp {
  std::vector<void*> ptrs;
  ~Tmp() { for (void* p : ptrs) (void)hipFree(p); }
  void* alloc(size_t bytes) {
    void* p = nullptr;
    HIP_CHECK(hipMalloc(&p, std::max<size_t>(bytes, 256)));
    HIP_CHECK(hipMemset(p, 0, std::max<size_t>(bytes, 256)));
    ptrs.push_back(p);
    return p;
  }
};

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
char g_chain_kernel[32] = "";
inline float bf16_bits_to_f32(bf16_t b) { union { uint32_t u; float f; } c; c.u = ((uint32_t)b) << 16; return c.f; }

// Guarded output buffer of asr_probe_gemm: rows x pitch elements of 2 (bf16) or 4 (f32 / int32) bytes, every byte 0xff before the launch -- a NaN in both
// formats, -1 as an index.
struct Guarded { void* dev = nullptr; size_t rows = 0, pitch = 0; int elt = 4; };
inline Guarded guarded(Tmp& t, size_t rows, size_t pitch, int elt) {
  Guarded b;
  b.rows = rows; b.pitch = pitch; b.elt = elt;
  b.dev = t.alloc(rows * pitch * elt);
  HIP_CHECK(hipMemset(b.dev, 0xff, rows * pitch * elt));
  return b;
}
inline uint32_t guard_word(int elt) { return elt == 2 ? 0xffff0000u : 0xffffffffu; }
// the whole buffer -> h (one 32-bit word per element, bf16 widened to its f32 bits); returns the elements outside the top-left rows_v x cols_v block
// that no longer hold the pattern
inline int collect(const Guarded& b, size_t rows_v, size_t cols_v, std::vector<uint32_t>& h) {
  const size_t n = b.rows * b.pitch;
  h.resize(n);
  if (b.elt == 2) {
    std::vector<uint16_t> raw(n);
    HIP_CHECK(hipMemcpy(raw.data(), b.dev, n * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) h[i] = (uint32_t)raw[i] << 16;
  } else {
    HIP_CHECK(hipMemcpy(h.data(), b.dev, n * 4, hipMemcpyDeviceToHost));
  }
  const uint32_t pat = guard_word(b.elt);
  int bad = 0;
  for (size_t r = 0; r < b.rows; ++r)
    for (size_t c = 0; c < b.pitch; ++c)
      if ((r >= rows_v || c >= cols_v) && h[r * b.pitch + c] != pat) ++bad;
  return bad;
}
// lo_group slabs [slab][Mp][G]: elements of the rows Mv .. Mp of every slab that no longer hold the pattern
inline int stale_rows(const std::vector<uint32_t>& h, size_t pitch, int slabs, int Mv, int Mp, int G, int elt) {
  int bad = 0;
  for (int s = 0; s < slabs; ++s)
    for (size_t i = (size_t)Mv * G; i < (size_t)Mp * G; ++i) bad += h[s * pitch + i] != guard_word(elt);
  return bad;
}

}  // namespace

extern "C" int asr_probe_gemm_bench(int variant, int M, int N, int K, int epilogue, int iters, float* avg_ms) {
  return asr_guard([&] {
    ASR_REQUIRE(avg_ms && iters > 0, "probe_gemm_bench: bad argument");
    asr_require_device(0);
    Tmp t;
    const int Mp = round_up(M, 128);
    auto rnd = [](size_t n, uint32_t seed) {
      std::vector<bf16_t> v(n);
      uint32_t x = seed;
      for (size_t i = 0; i < n; ++i) { x = x * 1664525u + 1013904223u; v[i] = f32_to_bf16(((int)(x >> 9) % 2001 - 1000) * 1e-3f); }
      return v;
    };
    std::vector<bf16_t> ha = rnd((size_t)Mp * K, 1), hw = rnd((size_t)N * K, 2);
    bf16_t* da = (bf16_t*)t.alloc(ha.size() * 2);
    bf16_t* dw = (bf16_t*)t.alloc(hw.size() * 2);
    HIP_CHECK(hipMemcpy(da, ha.data(), ha.size() * 2, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dw, hw.data(), hw.size() * 2, hipMemcpyHostToDevice));
    float* bias = (float*)t.alloc((size_t)N * 4);
    float* addm = (float*)t.alloc((size_t)Mp * N * 4);
    float* addt = (float*)t.alloc((size_t)Mp * N * 4);
    float* of32 = (float*)t.alloc((size_t)Mp * N * 4);
    bf16_t* olo = (bf16_t*)t.alloc((size_t)Mp * N * 2);
    bf16_t* ot = (bf16_t*)t.alloc((size_t)Mp * N * 2);
    GemmArgs g;
    g.A = da; g.lda = K; g.W = dw; g.ldw = K; g.M = M; g.N = N; g.K = K; g.bias = bias;
    switch (epilogue) {
      case 0: g.out_lo = olo; g.ld_out_lo = N; break;
      case 1: g.out_lo = olo; g.ld_out_lo = N; g.act = ACT_RELU; break;
      case 2: g.add = addm; g.ld_add = N; g.out_f32 = of32; g.ld_out_f32 = N; break;
      case 7: g.out_lo = olo; g.ld_out_lo = N; g.act = ACT_GELU_ERF; break;
      case 3: g.bias = nullptr; g.add = addt; g.ld_add = N; g.add2 = addm; g.ld_add2 = N; g.out_f32 = of32; g.ld_out_f32 = N; break;
      case 4: g.out_t = ot; g.ld_out_t = Mp; break;
      case 5: {   // FFN-1 with the LayerNorm evaluated inside (statistics handed over by the producer)
        float2* st = (float2*)t.alloc((size_t)Mp * (K / 32) * 8);
        HIP_CHECK(hipMemset(st, 0, (size_t)Mp * (K / 32) * 8));
        g.out_lo = olo; g.ld_out_lo = N; g.act = ACT_RELU; g.ln_colsum = bias; g.ln_dim = K; g.ln_stats_in = st; g.ln_slots = K / 32;
        break;
      }
      case 6: {   // out-projection writing the residual stream in f32 + bf16 + row statistics
        float2* st = (float2*)t.alloc((size_t)Mp * (N / 32) * 8);
        g.bias = nullptr; g.add = addt; g.ld_add = N; g.add2 = addm; g.ld_add2 = N; g.out_f32 = of32; g.ld_out_f32 = N;
        g.out_lo = olo; g.ld_out_lo = N; g.st_out = st;
        break;
      }
      default: ASR_THROW(ASR_ERR_INVALID, "probe_gemm_bench: unknown epilogue %d", epilogue);
    }
    g.dbg = variant < 0 ? 0 : variant >> 8;
    uint32_t* clk = nullptr;
    if (getenv("ASR_PP_CLK")) { clk = (uint32_t*)t.alloc(64 * 4); HIP_CHECK(hipMemset(clk, 0, 64 * 4)); g.dbg_clk = clk; }
    gemm_set_variant(variant < 0 ? -1 : (variant & 0xff));      // sticky: later asr_op_gemm calls use it too
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    for (int i = 0; i < 3; ++i) launch_gemm_bf16(g, nullptr);
    HIP_CHECK(hipEventRecord(e0, nullptr));
    for (int i = 0; i < iters; ++i) launch_gemm_bf16(g, nullptr);
    HIP_CHECK(hipEventRecord(e1, nullptr));
    HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    *avg_ms = ms / iters;
    if (clk) {
      uint32_t h[40];
      HIP_CHECK(hipMemcpy(h, clk, sizeof(h), hipMemcpyDeviceToHost));
      const int ksteps = K / 64 - 2;
      for (int w = 0; w < 2; ++w)
        for (int r = 0; r < 4; ++r)
          fprintf(stderr, "pp clock: group %d phase %d: reads %6.1f  vmcnt %6.1f  barrier %6.1f | mfma %6.1f  barrier %6.1f  (cycles per phase)\n", w, r,
                  h[w * 20 + r * 5] / (double)ksteps, h[w * 20 + r * 5 + 1] / (double)ksteps, h[w * 20 + r * 5 + 2] / (double)ksteps,
                  h[w * 20 + r * 5 + 3] / (double)ksteps, h[w * 20 + r * 5 + 4] / (double)ksteps);
    }
    gemm_set_variant(-1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  });
}


// Decode-shaped GEMM in a captured chain with COLD weights: `copies` weight matrices (together larger than the 256 MB Infinity Cache when
// cold_mb says so) are walked round-robin by dependent launches of one hipGraph, the way a decoder layer stack streams its weights from
// HBM once per token. Reports microseconds per launch (graph replay, device time between events).
extern "C" int asr_probe_gemm_chain(int M, int N, int K, int epilogue, int cold_mb, int replays, float* us_per_launch) {
  return asr_guard([&] {
    ASR_REQUIRE(us_per_launch && replays > 0 && M > 0 && N % 16 == 0 && K % 256 == 0, "probe_gemm_chain: bad argument");
    asr_require_device(0);
    gemm_reload_env();
    Tmp t;
    const int Mp = round_up(M, 128);
    const size_t wbytes = (size_t)N * K * 2;
    const int copies = std::max(1, std::min(512, (int)(((size_t)cold_mb << 20) / wbytes) + 1));
    std::vector<bf16_t> hw((size_t)N * K), ha((size_t)Mp * K);
    uint32_t x = 12345;
    for (auto& v : hw) { x = x * 1664525u + 1013904223u; v = f32_to_bf16(((int)(x >> 9) % 2001 - 1000) * 1e-3f); }
    for (auto& v : ha) { x = x * 1664525u + 1013904223u; v = f32_to_bf16(((int)(x >> 9) % 2001 - 1000) * 1e-3f); }
    bf16_t* dw = (bf16_t*)t.alloc(wbytes * copies);
    for (int c = 0; c < copies; ++c) HIP_CHECK(hipMemcpy((char*)dw + wbytes * c, hw.data(), wbytes, hipMemcpyHostToDevice));
    bf16_t* da = (bf16_t*)t.alloc(ha.size() * 2);
    HIP_CHECK(hipMemcpy(da, ha.data(), ha.size() * 2, hipMemcpyHostToDevice));
    float* bias = (float*)t.alloc((size_t)N * 4);
    float* addm = (float*)t.alloc((size_t)Mp * N * 4);
    float* of32 = (float*)t.alloc((size_t)Mp * N * 4);
    bf16_t* olo = (bf16_t*)t.alloc((size_t)Mp * N * 2);
    float* lnx = (float*)t.alloc((size_t)Mp * K * 4);
    GemmArgs g;
    g.A = da; g.lda = K; g.ldw = K; g.M = M; g.N = N; g.K = K; g.bias = bias;
    g.sk_ws = (float*)t.alloc((size_t)16 << 20); g.sk_ws_bytes = (size_t)16 << 20; g.sk_cnt = (int32_t*)t.alloc(4096 * 4);
    switch (epilogue >= 10 ? 0 : epilogue) {
      case 0: g.out_lo = olo; g.ld_out_lo = N; break;                                                  // bias -> bf16 (q|k|v, cross-q with a separate LayerNorm)
      case 1: g.out_lo = olo; g.ld_out_lo = N; g.act = ACT_GELU_ERF; break;                            // fc1
      case 2: g.add = addm; g.ld_add = N; g.out_f32 = of32; g.ld_out_f32 = N; break;                   // out-proj / fc2: + residual -> f32
      case 3: g.A = nullptr; g.ln_x = lnx; g.ld_ln_x = K; g.out_lo = olo; g.ld_out_lo = N; break;      // LayerNorm prologue -> bf16
      default: ASR_THROW(ASR_ERR_INVALID, "probe_gemm_chain: unknown epilogue %d", epilogue);
    }
    hipStream_t s;
    HIP_CHECK(hipStreamCreate(&s));
    const int chain = std::max(copies, 64);
    DecGemmArgs dg;                                      // epilogue >= 10: the decode GEMM (csrc/decode_gemm.hip)
    const bool use_dg = epilogue >= 10;
    if (use_dg) {
      const int e = epilogue - 10;
      float* cs = (float*)t.alloc((size_t)N * 4);
      dg.A = da; dg.lda = K; dg.ldw = K; dg.M = M; dg.N = N; dg.K = K; dg.bias = bias;
      dg.ws = g.sk_ws; dg.ws_bytes = g.sk_ws_bytes; dg.cnt = g.sk_cnt;
      if (e == 0) { dg.out_lo = olo; dg.ld_out_lo = N; }
      else if (e == 1) { dg.out_lo = olo; dg.ld_out_lo = N; dg.act = ACT_GELU_ERF; dg.colsum = cs; }
      else if (e == 2) { dg.add = addm; dg.ld_add = N; dg.out_f32 = of32; dg.ld_out_f32 = N; dg.out_lo = olo; dg.ld_out_lo = N; }
      else if (e == 3) { dg.out_lo = olo; dg.ld_out_lo = N; dg.colsum = cs; }
      else ASR_THROW(ASR_ERR_INVALID, "probe_gemm_chain: unknown decode epilogue %d", e);
      int nt = 1, sp = 1;
      decode_gemm_plan(dg, &nt, &sp);
      snprintf(g_chain_kernel, sizeof(g_chain_kernel), "decode nt%d ks%d", nt, sp);
    }
    // ASR_PROBE_PREFETCH=1: while node i runs, a side branch touches node i + 1's weights from the workgroups that will stream them (launch_decode_gemm_prefetch)
    const bool prefetch = use_dg && getenv("ASR_PROBE_PREFETCH") && getenv("ASR_PROBE_PREFETCH")[0] == '1';
    hipStream_t s2 = nullptr;
    std::vector<hipEvent_t> evs;
    if (prefetch) {
      HIP_CHECK(hipStreamCreate(&s2));
      evs.resize(chain + 1);
      for (auto& e : evs) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    // ASR_PROBE_CLK=1: every launch of the chain stamps its phase clock (decode_gemm_kernel: DecGemmArgs::dbg_clk); the breakdown of the last replay goes to stderr
    const bool clocked = use_dg && getenv("ASR_PROBE_CLK") && getenv("ASR_PROBE_CLK")[0] == '1';
    unsigned long long* dclk = clocked ? (unsigned long long*)t.alloc((size_t)chain * 10 * 8) : nullptr;
    if (dclk) HIP_CHECK(hipMemset(dclk, 0, (size_t)chain * 10 * 8));
    auto enqueue = [&] {
      for (int i = 0; i < chain; ++i) {
        if (prefetch) {
          DecGemmArgs gn = dg; gn.W = (const bf16_t*)((char*)dw + wbytes * ((i + 1) % copies));
          HIP_CHECK(hipEventRecord(evs[i], s));
          HIP_CHECK(hipStreamWaitEvent(s2, evs[i], 0));
          launch_decode_gemm_prefetch(gn, s2);
        }
        if (use_dg) { DecGemmArgs gi = dg; gi.W = (const bf16_t*)((char*)dw + wbytes * (i % copies)); gi.dbg_clk = dclk ? dclk + (size_t)i * 10 : nullptr; launch_decode_gemm(gi, s); }
        else { GemmArgs gi = g; gi.W = (char*)dw + wbytes * (i % copies); launch_gemm_bf16(gi, s); }
      }
      if (prefetch) { HIP_CHECK(hipEventRecord(evs[chain], s2)); HIP_CHECK(hipStreamWaitEvent(s, evs[chain], 0)); }
    };
    enqueue();                                                 // eager once (lazy attributes)
    HIP_CHECK(hipStreamSynchronize(s));
    if (s2) HIP_CHECK(hipStreamSynchronize(s2));
    hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
    HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    enqueue();
    HIP_CHECK(hipStreamEndCapture(s, &graph));
    HIP_CHECK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0)); HIP_CHECK(hipEventCreate(&e1));
    HIP_CHECK(hipGraphLaunch(exec, s));
    HIP_CHECK(hipEventRecord(e0, s));
    for (int r = 0; r < replays; ++r) HIP_CHECK(hipGraphLaunch(exec, s));
    HIP_CHECK(hipEventRecord(e1, s));
    HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    *us_per_launch = ms * 1e3f / ((float)replays * chain);
    if (dclk) {
      std::vector<unsigned long long> h((size_t)chain * 10);
      HIP_CHECK(hipMemcpy(h.data(), dclk, h.size() * 8, hipMemcpyDeviceToHost));
      double seg[4] = {0, 0, 0, 0}, body = 0, gap = 0, skew = 0, tail = 0;
      int n = 0;
      for (int i = 1; i + 1 < chain; ++i) {            // 100 MHz clock: 0.01 us per tick
        const unsigned long long* a = &h[(size_t)i * 10];
        const unsigned long long* b = &h[(size_t)(i + 1) * 10];
        if (!a[0] || !a[4] || !b[0] || !a[5] || !a[9]) continue;
        for (int q = 0; q < 4; ++q) seg[q] += (double)(a[q + 1] - a[q]) * 0.01;
        body += (double)(a[4] - a[0]) * 0.01;
        skew += (double)((long long)a[5] - (long long)a[0]) * 0.01;                    // the last workgroup starts this much after the first
        tail += (double)((long long)std::max(a[9], a[4]) - (long long)a[4]) * 0.01;    // ... and ends this much after the first one's end
        gap += (double)((long long)std::min(b[0], b[5]) - (long long)std::max(a[4], a[9])) * 0.01;   // last store acknowledged -> first instruction of the next launch
        ++n;
      }
      if (n) fprintf(stderr, "  [clock M=%d N=%d K=%d %s] launch %.2f us = body of workgroup 0 %.2f (setup %.2f, weights + MFMA %.2f, reduce %.2f, hand-over + epilogue + store ack %.2f) + last workgroup start skew %.2f / end tail %.2f; boundary to the next launch %.2f\n",
                     M, N, K, g_chain_kernel, *us_per_launch, body / n, seg[0] / n, seg[1] / n, seg[2] / n, seg[3] / n, skew / n, tail / n, gap / n);
    }
    if (!use_dg) snprintf(g_chain_kernel, sizeof(g_chain_kernel), "%s", gemm_last_kernel());
    (void)hipGraphExecDestroy(exec); (void)hipGraphDestroy(graph); (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipStreamDestroy(s);
    if (s2) (void)hipStreamDestroy(s2);
    for (auto& e : evs) (void)hipEventDestroy(e);
  });
}

// ---- FP8 mode (ASR_PRECISION_FP8W): the row quantiser and the decode GEMM over byte weights, on host arrays
// w_bf16 is [N][ld] with ld >= K: the quantiser must read K columns of every row and nothing of the gap
extern "C" int asr_probe_quantize_fp8_ld(const uint16_t* w_bf16, int ld, int N, int K, uint8_t* out8, float* scale, uint16_t* dq_bf16) {
  return asr_guard([&] {
    ASR_REQUIRE(w_bf16 && out8 && scale && N > 0 && K > 0 && K % 8 == 0 && ld >= K, "probe_quantize_fp8: bad argument");
    asr_require_device(0);
    DeviceBuffer w, q, sc, dq;
    w.reserve((size_t)N * ld * 2, nullptr); q.reserve((size_t)N * K, nullptr); sc.reserve((size_t)N * 4, nullptr); dq.reserve((size_t)N * K * 2, nullptr);
    HIP_CHECK(hipMemcpy(w.ptr, w_bf16, (size_t)N * ld * 2, hipMemcpyHostToDevice));
    launch_quantize_rows_fp8(w.as<bf16_t>(), ld, N, K, q.as<unsigned char>(), sc.as<float>(), dq.as<bf16_t>(), nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out8, q.ptr, (size_t)N * K, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(scale, sc.ptr, (size_t)N * 4, hipMemcpyDeviceToHost));
    if (dq_bf16) HIP_CHECK(hipMemcpy(dq_bf16, dq.ptr, (size_t)N * K * 2, hipMemcpyDeviceToHost));
  });
}
extern "C" int asr_probe_quantize_fp8(const uint16_t* w_bf16, int N, int K, uint8_t* out8, float* scale, uint16_t* dq_bf16) {
  return asr_probe_quantize_fp8_ld(w_bf16, K, N, K, out8, scale, dq_bf16);
}

// out[M][N] (f32) = decode GEMM of a[M][K] (bf16) with EITHER w_bf16[N][K] OR (w8[N][K], scale[N]); fold != 0: LayerNorm folded in
// (column sums taken from w_bf16, which a byte-weight caller passes as the dequantised copy); bias may be null
extern "C" int asr_probe_decode_gemm(int M, int N, int K, const uint16_t* a, const uint16_t* w_bf16, const uint8_t* w8, const float* scale,
                                     const float* bias, int fold, float* out) {
  return asr_guard([&] {
    ASR_REQUIRE(a && out && (w_bf16 || w8) && !(w8 && !scale) && !(fold && !w_bf16), "probe_decode_gemm: bad argument");
    asr_require_device(0);
    DeviceBuffer da, dw, dw8, dsc, db, dcs, dout, ws, cnt;
    da.reserve((size_t)64 * K * 2, nullptr); dout.reserve((size_t)64 * N * 4, nullptr); ws.reserve((size_t)16 << 20, nullptr); cnt.reserve(4096 * 4, nullptr);
    HIP_CHECK(hipMemset(da.ptr, 0, (size_t)64 * K * 2)); HIP_CHECK(hipMemset(cnt.ptr, 0, 4096 * 4));
    HIP_CHECK(hipMemcpy(da.ptr, a, (size_t)M * K * 2, hipMemcpyHostToDevice));
    DecGemmArgs g;
    g.A = da.as<bf16_t>(); g.lda = K; g.ldw = K; g.M = M; g.N = N; g.K = K; g.out_f32 = dout.as<float>(); g.ld_out_f32 = N;
    g.ws = ws.as<float>(); g.ws_bytes = ws.cap; g.cnt = cnt.as<int32_t>();
    if (w_bf16) { dw.reserve((size_t)N * K * 2, nullptr); HIP_CHECK(hipMemcpy(dw.ptr, w_bf16, (size_t)N * K * 2, hipMemcpyHostToDevice)); g.W = dw.as<bf16_t>(); }
    if (w8) {
      dw8.reserve((size_t)N * K, nullptr); dsc.reserve((size_t)N * 4, nullptr);
      HIP_CHECK(hipMemcpy(dw8.ptr, w8, (size_t)N * K, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dsc.ptr, scale, (size_t)N * 4, hipMemcpyHostToDevice));
      g.W = nullptr; g.W8 = dw8.as<unsigned char>(); g.w_scale = dsc.as<float>();
    }
    if (bias) { db.reserve((size_t)N * 4, nullptr); HIP_CHECK(hipMemcpy(db.ptr, bias, (size_t)N * 4, hipMemcpyHostToDevice)); g.bias = db.as<float>(); }
    if (fold) { dcs.reserve((size_t)N * 4, nullptr); launch_colsum_bf16(dw.as<bf16_t>(), K, N, K, dcs.as<float>(), nullptr); g.colsum = dcs.as<float>(); }
    launch_decode_gemm(g, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, dout.ptr, (size_t)M * N * 4, hipMemcpyDeviceToHost));
  });
}

// ---- MXFP4 mode (ASR_PRECISION_MXFP4W): the block quantiser and the decode GEMM over nibble weights, on host arrays
extern "C" int asr_probe_quantize_mxfp4_ld(const uint16_t* w_bf16, int ld, int N, int K, uint8_t* out4, uint8_t* scale8, uint16_t* dq_bf16) {
  return asr_guard([&] {
    ASR_REQUIRE(w_bf16 && out4 && scale8 && N > 0 && K > 0 && K % 32 == 0 && ld >= K, "probe_quantize_mxfp4: bad argument");
    asr_require_device(0);
    DeviceBuffer w, q, sc, dq;
    w.reserve((size_t)N * ld * 2, nullptr); q.reserve((size_t)N * K / 2, nullptr); sc.reserve((size_t)N * K / 32, nullptr); dq.reserve((size_t)N * K * 2, nullptr);
    HIP_CHECK(hipMemcpy(w.ptr, w_bf16, (size_t)N * ld * 2, hipMemcpyHostToDevice));
    launch_quantize_rows_mxfp4(w.as<bf16_t>(), ld, N, K, q.as<unsigned char>(), sc.as<unsigned char>(), dq.as<bf16_t>(), nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out4, q.ptr, (size_t)N * K / 2, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(scale8, sc.ptr, (size_t)N * K / 32, hipMemcpyDeviceToHost));
    if (dq_bf16) HIP_CHECK(hipMemcpy(dq_bf16, dq.ptr, (size_t)N * K * 2, hipMemcpyDeviceToHost));
  });
}
extern "C" int asr_probe_quantize_mxfp4(const uint16_t* w_bf16, int N, int K, uint8_t* out4, uint8_t* scale8, uint16_t* dq_bf16) {
  return asr_probe_quantize_mxfp4_ld(w_bf16, K, N, K, out4, scale8, dq_bf16);
}

// out[M][N] (f32) = decode GEMM of a[M][K] (bf16) with the MXFP4 weights (w4 [N][K / 2], scale8 [N][K / 32]); fold != 0: LayerNorm folded in, column sums
// taken from w_dq (the dequantised bf16 copy, as the session does)
extern "C" int asr_probe_decode_gemm_mxfp4(int M, int N, int K, const uint16_t* a, const uint8_t* w4, const uint8_t* scale8, const uint16_t* w_dq,
                                           const float* bias, int fold, float* out) {
  return asr_guard([&] {
    ASR_REQUIRE(a && out && w4 && scale8 && !(fold && !w_dq), "probe_decode_gemm_mxfp4: bad argument");
    asr_require_device(0);
    DeviceBuffer da, dw, dw4, dsc, db, dcs, dout, ws, cnt;
    da.reserve((size_t)64 * K * 2, nullptr); dout.reserve((size_t)64 * N * 4, nullptr); ws.reserve((size_t)16 << 20, nullptr); cnt.reserve(4096 * 4, nullptr);
    HIP_CHECK(hipMemset(da.ptr, 0, (size_t)64 * K * 2)); HIP_CHECK(hipMemset(cnt.ptr, 0, 4096 * 4));
    HIP_CHECK(hipMemcpy(da.ptr, a, (size_t)M * K * 2, hipMemcpyHostToDevice));
    DecGemmArgs g;
    g.A = da.as<bf16_t>(); g.lda = K; g.ldw = K; g.M = M; g.N = N; g.K = K; g.out_f32 = dout.as<float>(); g.ld_out_f32 = N;
    g.ws = ws.as<float>(); g.ws_bytes = ws.cap; g.cnt = cnt.as<int32_t>();
    dw4.reserve((size_t)N * K / 2, nullptr); dsc.reserve((size_t)N * K / 32, nullptr);
    HIP_CHECK(hipMemcpy(dw4.ptr, w4, (size_t)N * K / 2, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dsc.ptr, scale8, (size_t)N * K / 32, hipMemcpyHostToDevice));
    g.W4 = dw4.as<unsigned char>(); g.w_scale4 = dsc.as<unsigned char>();
    if (bias) { db.reserve((size_t)N * 4, nullptr); HIP_CHECK(hipMemcpy(db.ptr, bias, (size_t)N * 4, hipMemcpyHostToDevice)); g.bias = db.as<float>(); }
    if (fold) {
      dw.reserve((size_t)N * K * 2, nullptr); HIP_CHECK(hipMemcpy(dw.ptr, w_dq, (size_t)N * K * 2, hipMemcpyHostToDevice));
      dcs.reserve((size_t)N * 4, nullptr); launch_colsum_bf16(dw.as<bf16_t>(), K, N, K, dcs.as<float>(), nullptr); g.colsum = dcs.as<float>();
    }
    launch_decode_gemm(g, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, dout.ptr, (size_t)M * N * 4, hipMemcpyDeviceToHost));
  });
}

// FP8 matrix-pipe GEMM on host arrays (csrc/gemm_fp8.hip): a8 [M][K], w8 [N][K] e4m3 bytes, w_scale [N], bias [N]; either out8 [M][N] (act, bytes) or
// out_f32 [M][N] (+ add [M][N]). iters > 0: also times that many launches (microseconds per launch in *us).
extern "C" int asr_probe_gemm_fp8(int M, int N, int K, const uint8_t* a8, const uint8_t* w8, const float* w_scale, float a_scale, const float* bias,
                                  const float* add, int act, uint8_t* out8, float* out_f32, int iters, float* us) {
  return asr_guard([&] {
    ASR_REQUIRE(a8 && w8 && w_scale && bias && (out8 || out_f32), "probe_gemm_fp8: bad argument");
    asr_require_device(0);
    DeviceBuffer da, dw, dsc, db, dadd, dout;
    da.reserve((size_t)M * K, nullptr); dw.reserve((size_t)N * K, nullptr); dsc.reserve((size_t)N * 4, nullptr); db.reserve((size_t)N * 4, nullptr);
    HIP_CHECK(hipMemcpy(da.ptr, a8, (size_t)M * K, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dw.ptr, w8, (size_t)N * K, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dsc.ptr, w_scale, (size_t)N * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(db.ptr, bias, (size_t)N * 4, hipMemcpyHostToDevice));
    Fp8GemmArgs g;
    g.A = da.as<unsigned char>(); g.lda = K; g.W = dw.as<unsigned char>(); g.ldw = K; g.M = M; g.N = N; g.K = K; g.w_scale = dsc.as<float>(); g.a_scale = a_scale;
    g.bias = db.as<float>(); g.act = act;
    if (out8) { dout.reserve((size_t)M * N, nullptr); g.out8 = dout.as<unsigned char>(); g.ld_out8 = N; }
    else {
      ASR_REQUIRE(add, "probe_gemm_fp8: the f32 output needs the residual rows");
      dadd.reserve((size_t)M * N * 4, nullptr); HIP_CHECK(hipMemcpy(dadd.ptr, add, (size_t)M * N * 4, hipMemcpyHostToDevice));
      dout.reserve((size_t)M * N * 4, nullptr); g.add = dadd.as<float>(); g.ld_add = N; g.out_f32 = dout.as<float>(); g.ld_out_f32 = N;
    }
    launch_gemm_fp8(g, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    if (out8) HIP_CHECK(hipMemcpy(out8, dout.ptr, (size_t)M * N, hipMemcpyDeviceToHost));
    else HIP_CHECK(hipMemcpy(out_f32, dout.ptr, (size_t)M * N * 4, hipMemcpyDeviceToHost));
    if (iters > 0 && us) {
      hipEvent_t e0, e1;
      HIP_CHECK(hipEventCreate(&e0)); HIP_CHECK(hipEventCreate(&e1));
      for (int i = 0; i < 3; ++i) launch_gemm_fp8(g, nullptr);
      HIP_CHECK(hipEventRecord(e0, nullptr));
      for (int i = 0; i < iters; ++i) launch_gemm_fp8(g, nullptr);
      HIP_CHECK(hipEventRecord(e1, nullptr));
      HIP_CHECK(hipEventSynchronize(e1));
      float ms = 0.f;
      HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
      *us = ms * 1e3f / iters;
      (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    }
  });
}

// ---- the decode GEMM with every DecGemmArgs term, a forced plan and guarded buffers (tests/test_decode_gemm_ref_gpu.py)
namespace {
// rows x `pitch` elements of `elt` bytes, every byte 0xff (a NaN in bf16, f32 and e4m3), the top-left rows_v x cols_v block copied in from the host
void* nan_padded(Tmp& t, const void* host, size_t rows_v, size_t cols_v, size_t rows, size_t pitch, int elt) {
  void* p = t.alloc(rows * pitch * elt);
  HIP_CHECK(hipMemset(p, 0xff, rows * pitch * elt));
  if (rows_v && cols_v) HIP_CHECK(hipMemcpy2D(p, pitch * elt, host, cols_v * elt, cols_v * elt, rows_v, hipMemcpyHostToDevice));
  return p;
}
}  // namespace

extern "C" int asr_probe_decode_gemm_desc(asr_probe_dec_gemm_args* d) {
  return asr_guard([&] {
    ASR_REQUIRE(d && d->a && d->w_bf16 && (d->out_f32 || d->out_lo) && d->M >= 1 && d->M <= 64 && d->N >= 16 && d->N <= 65536 && d->K >= 32 && d->repeats >= 1,
                "probe_decode_gemm_desc: bad argument");
    ASR_REQUIRE(d->wkind == 0 || (d->wkind == 1 && d->wq && d->w_scale) || (d->wkind == 2 && d->wq && d->w_scale8), "probe_decode_gemm_desc: weight kind %d", d->wkind);
    asr_require_device(0);
    const int M = d->M, N = d->N, K = d->K;
    const int lda = d->lda ? d->lda : K, ldw = d->ldw ? d->ldw : K, ld_add = d->ld_add ? d->ld_add : N;
    const int ld_f32 = d->ld_out_f32 ? d->ld_out_f32 : N, ld_lo = d->ld_out_lo ? d->ld_out_lo : N;
    ASR_REQUIRE(lda >= K && ldw >= K && ld_add >= N && ld_f32 >= N && ld_lo >= N && ld_add % 4 == 0 && ld_f32 % 4 == 0 && ld_lo % 4 == 0 && N % 16 == 0,
                "probe_decode_gemm_desc: a pitch below the extent or off the vector alignment");
    ASR_REQUIRE(d->pre_M >= 0 && d->pre_M <= 64, "probe_decode_gemm_desc: pre_M");
    Tmp t;
    const int SLACK = 16;                                 // NaN rows behind the M rows of A and add: the kernel must not need zeros past M
    DecGemmArgs g;
    g.M = M; g.N = N; g.K = K; g.plan_M = d->plan_M; g.lda = lda; g.ldw = ldw; g.act = d->act; g.ln_eps = d->ln_eps;
    g.A = (const bf16_t*)nan_padded(t, d->a, M, K, M + SLACK, lda, 2);
    const bf16_t* w_dense = nullptr;                      // the bf16 weights (or the dequantised copy) the column sums come from
    if (d->wkind == 0) { g.W = (const bf16_t*)nan_padded(t, d->w_bf16, N, K, N, ldw, 2); }
    else if (d->wkind == 1) {
      g.W8 = (const unsigned char*)nan_padded(t, d->wq, N, K, N, ldw, 1);
      float* sc = (float*)t.alloc((size_t)N * 4); HIP_CHECK(hipMemcpy(sc, d->w_scale, (size_t)N * 4, hipMemcpyHostToDevice)); g.w_scale = sc;
    } else {
      ASR_REQUIRE(ldw % 2 == 0, "probe_decode_gemm_desc: ldw");
      g.W4 = (const unsigned char*)nan_padded(t, d->wq, N, K / 2, N, ldw / 2, 1);
      unsigned char* sc = (unsigned char*)t.alloc((size_t)N * (K / 32)); HIP_CHECK(hipMemcpy(sc, d->w_scale8, (size_t)N * (K / 32), hipMemcpyHostToDevice)); g.w_scale4 = sc;
    }
    if (d->fold) {
      int ld_dense = ldw;
      if (d->wkind == 0) w_dense = g.W;
      else { w_dense = (const bf16_t*)nan_padded(t, d->w_bf16, N, K, N, K, 2); ld_dense = K; }
      float* cs = (float*)t.alloc((size_t)N * 4);
      launch_colsum_bf16(w_dense, ld_dense, N, K, cs, nullptr);
      g.colsum = cs;
    }
    if (d->bias) { float* b = (float*)t.alloc((size_t)N * 4); HIP_CHECK(hipMemcpy(b, d->bias, (size_t)N * 4, hipMemcpyHostToDevice)); g.bias = b; }
    if (d->add) { g.add = (const float*)nan_padded(t, d->add, M, N, M + SLACK, ld_add, 4); g.ld_add = ld_add; }
    const size_t out_rows = 64 + 16;
    Guarded of32, olo;
    if (d->out_f32) { of32 = guarded(t, out_rows, ld_f32, 4); g.out_f32 = (float*)of32.dev; g.ld_out_f32 = ld_f32; }
    if (d->out_lo) { olo = guarded(t, out_rows, ld_lo, 2); g.out_lo = (bf16_t*)olo.dev; g.ld_out_lo = ld_lo; }
    const int n_tickets = 4096;
    ASR_REQUIRE(N / 16 <= n_tickets, "probe_decode_gemm_desc: N");
    int32_t* cnt = nullptr;
    if (d->with_ws) {                                     // partials hold NaN before the first launch, the tickets 0
      const size_t ws_bytes = std::max<size_t>((size_t)1 << 20, (size_t)16 * 64 * N * 4 + (size_t)(N / 16) * 16 * 64 * 8);
      g.ws = (float*)t.alloc(ws_bytes); g.ws_bytes = ws_bytes;
      HIP_CHECK(hipMemset(g.ws, 0xff, ws_bytes));
      cnt = (int32_t*)t.alloc((size_t)n_tickets * 4); g.cnt = cnt;
    }
    ASR_REQUIRE(decode_gemm_supported(g), "probe_decode_gemm_desc: unsupported shape (M = %d, N = %d, K = %d)", M, N, K);
    int nt = 1, splits = 1, rb = 1;
    decode_gemm_plan(g, &nt, &splits, &rb);
    if (d->force_nt || d->force_splits || d->force_row_blocks) {
      if (d->force_nt) nt = d->force_nt;
      if (d->force_splits) splits = d->force_splits; else if (d->force_row_blocks == 2) splits = 1;
      if (d->force_row_blocks) rb = d->force_row_blocks; else if (d->force_splits) rb = 1;
      ASR_REQUIRE(decode_gemm_plan_admissible(g, nt, splits, rb), "probe_decode_gemm_desc: the forced plan (nt %d, splits %d, row blocks %d) is not admissible", nt, splits, rb);
    }
    if (d->pre_M > 0) {                                   // a launch of pre_M rows (row i = row i % M of A and add) and pre_splits splits on the same workspace first
      ASR_REQUIRE(d->with_ws && d->pre_splits >= 1, "probe_decode_gemm_desc: the launch before needs the workspace");
      const int P = d->pre_M;
      std::vector<uint16_t> ha((size_t)P * K);
      for (int r = 0; r < P; ++r) memcpy(&ha[(size_t)r * K], d->a + (size_t)(r % M) * K, (size_t)K * 2);
      DecGemmArgs p = g;
      p.M = P; p.plan_M = 0;
      p.A = (const bf16_t*)nan_padded(t, ha.data(), P, K, P + SLACK, lda, 2);
      if (d->add) {
        std::vector<float> hadd((size_t)P * N);
        for (int r = 0; r < P; ++r) memcpy(&hadd[(size_t)r * N], d->add + (size_t)(r % M) * N, (size_t)N * 4);
        p.add = (const float*)nan_padded(t, hadd.data(), P, N, P + SLACK, ld_add, 4);
      }
      if (g.out_f32) p.out_f32 = (float*)t.alloc(out_rows * ld_f32 * 4);
      if (g.out_lo) p.out_lo = (bf16_t*)t.alloc(out_rows * ld_lo * 2);
      ASR_REQUIRE(decode_gemm_plan_admissible(p, nt, d->pre_splits, 1), "probe_decode_gemm_desc: the launch before (%d rows, %d splits) is not admissible", P, d->pre_splits);
      launch_decode_gemm_planned(p, nt, d->pre_splits, 1, nullptr);
      HIP_CHECK(hipDeviceSynchronize());
    }
    int launched[4] = {0, 0, 0, 0};
    for (int r = 0; r < d->repeats; ++r) launch_decode_gemm_planned(g, nt, splits, rb, nullptr, launched);
    HIP_CHECK(hipDeviceSynchronize());
    d->mt = launched[0]; d->nt = launched[1]; d->splits = launched[2]; d->row_blocks = launched[3];
    std::vector<uint32_t> h;
    d->stray = 0;
    if (d->out_f32) {
      d->stray += collect(of32, M, N, h);
      for (int m = 0; m < M; ++m) memcpy(d->out_f32 + (size_t)m * N, &h[(size_t)m * ld_f32], (size_t)N * 4);
    }
    if (d->out_lo) {
      d->stray += collect(olo, M, N, h);
      for (int m = 0; m < M; ++m) memcpy(d->out_lo + (size_t)m * N, &h[(size_t)m * ld_lo], (size_t)N * 4);
    }
    d->tickets_zero = 1;
    if (cnt) {
      std::vector<int32_t> hc(n_tickets);
      HIP_CHECK(hipMemcpy(hc.data(), cnt, (size_t)n_tickets * 4, hipMemcpyDeviceToHost));
      for (int32_t v : hc) if (v != 0) d->tickets_zero = 0;
    }
  });
}

// launch_quantize_crosskv_fp8 on host arrays: slabs [n_slabs][rows][64] bf16 bits (returned as the launch leaves them), sequence b at rows
// [row_off[b], row_off[b] + n_lfr[b]); out8 [n_slabs][rows][64] (0xa5 where the kernel wrote nothing), scale [n_slabs][batch]
extern "C" int asr_probe_quantize_crosskv_fp8(uint16_t* slabs, int n_slabs, int rows, const int32_t* row_off, const int32_t* n_lfr, int batch, int dq_in_place,
                                              uint8_t* out8, float* scale) {
  return asr_guard([&] {
    ASR_REQUIRE(slabs && row_off && n_lfr && out8 && scale && n_slabs >= 1 && rows >= 1 && batch >= 1, "probe_quantize_crosskv_fp8: bad argument");
    for (int b = 0; b < batch; ++b)
      ASR_REQUIRE(row_off[b] >= 0 && n_lfr[b] >= 0 && row_off[b] % 16 == 0 && row_off[b] + n_lfr[b] <= rows, "probe_quantize_crosskv_fp8: sequence %d leaves the slab", b);
    asr_require_device(0);
    Tmp t;
    const size_t elems = (size_t)n_slabs * rows * 64;
    bf16_t* ds = (bf16_t*)t.alloc(elems * 2);
    unsigned char* d8 = (unsigned char*)t.alloc(elems);
    float* dsc = (float*)t.alloc((size_t)n_slabs * batch * 4);
    UttPlan* dp = (UttPlan*)t.alloc((size_t)batch * sizeof(UttPlan));
    std::vector<UttPlan> hp(batch);
    for (int b = 0; b < batch; ++b) { memset(&hp[b], 0, sizeof(UttPlan)); hp[b].row_off = row_off[b]; hp[b].n_lfr = n_lfr[b]; hp[b].T = n_lfr[b]; }
    HIP_CHECK(hipMemcpy(dp, hp.data(), (size_t)batch * sizeof(UttPlan), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(ds, slabs, elems * 2, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemset(d8, 0xa5, elems));
    HIP_CHECK(hipMemset(dsc, 0xff, (size_t)n_slabs * batch * 4));
    launch_quantize_crosskv_fp8(ds, (size_t)rows * 64, n_slabs, dp, batch, d8, dsc, dq_in_place, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(slabs, ds, elems * 2, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(out8, d8, elems, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(scale, dsc, (size_t)n_slabs * batch * 4, hipMemcpyDeviceToHost));
  });
}

// launch_layernorm_fp8 on host arrays: x [rows][ld_x] f32 -> out [rows + 4][ld_out] bytes, every byte 0xa5 before the launch (the sentinel)
extern "C" int asr_probe_layernorm_fp8(const float* x, int ld_x, int rows, int D, float eps, float inv_scale, int ld_out, uint8_t* out) {
  return asr_guard([&] {
    ASR_REQUIRE(x && out && rows >= 1 && D >= 1 && ld_x >= D && ld_out >= D, "probe_layernorm_fp8: bad argument");
    asr_require_device(0);
    Tmp t;
    float* dx = (float*)t.alloc((size_t)rows * ld_x * 4);
    unsigned char* dout = (unsigned char*)t.alloc((size_t)(rows + 4) * ld_out);
    HIP_CHECK(hipMemcpy(dx, x, (size_t)rows * ld_x * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemset(dout, 0xa5, (size_t)(rows + 4) * ld_out));
    launch_layernorm_fp8(dx, ld_x, rows, D, eps, inv_scale, dout, ld_out, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, dout, (size_t)(rows + 4) * ld_out, hipMemcpyDeviceToHost));
  });
}

// asr_probe_gemm_fp8 with pitches on every operand, out_inv_scale and the saturation count. Outputs are returned as laid out, 8 rows past M included:
// out8 [M + 8][ld_out8] (0xa5 before the launch) or out_f32 [M + 8][ld_out_f32] (every byte 0xff before the launch); the gaps of a8 / w8 / add hold 0xff
extern "C" int asr_probe_gemm_fp8_v2(int M, int N, int K, const uint8_t* a8, int lda, const uint8_t* w8, int ldw, const float* w_scale, float a_scale, const float* bias,
                                     const float* add, int ld_add, int act, float out_inv_scale, uint8_t* out8, int ld_out8, float* out_f32, int ld_out_f32,
                                     uint64_t* sat_count) {
  return asr_guard([&] {
    ASR_REQUIRE(a8 && w8 && w_scale && bias && (out8 || out_f32) && !(out8 && out_f32) && M >= 1 && lda >= K && ldw >= K, "probe_gemm_fp8_v2: bad argument");
    asr_require_device(0);
    Tmp t;
    Fp8GemmArgs g;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldw = ldw; g.a_scale = a_scale; g.act = act; g.out_inv_scale = out_inv_scale;
    g.A = (const unsigned char*)nan_padded(t, a8, M, K, M, lda, 1);
    g.W = (const unsigned char*)nan_padded(t, w8, N, K, N, ldw, 1);
    float* sc = (float*)t.alloc((size_t)N * 4); HIP_CHECK(hipMemcpy(sc, w_scale, (size_t)N * 4, hipMemcpyHostToDevice)); g.w_scale = sc;
    float* b = (float*)t.alloc((size_t)N * 4); HIP_CHECK(hipMemcpy(b, bias, (size_t)N * 4, hipMemcpyHostToDevice)); g.bias = b;
    unsigned long long* sat = (unsigned long long*)t.alloc(8);
    void* dout = nullptr;
    const size_t R = (size_t)M + 8;
    if (out8) {
      ASR_REQUIRE(ld_out8 >= N && !add, "probe_gemm_fp8_v2: byte output");
      dout = t.alloc(R * ld_out8); HIP_CHECK(hipMemset(dout, 0xa5, R * ld_out8));
      g.out8 = (unsigned char*)dout; g.ld_out8 = ld_out8; g.sat_count = sat;
    } else {
      ASR_REQUIRE(add && ld_add >= N && ld_out_f32 >= N, "probe_gemm_fp8_v2: the f32 output needs the residual rows");
      g.add = (const float*)nan_padded(t, add, M, N, M, ld_add, 4); g.ld_add = ld_add;
      dout = t.alloc(R * ld_out_f32 * 4); HIP_CHECK(hipMemset(dout, 0xff, R * ld_out_f32 * 4));
      g.out_f32 = (float*)dout; g.ld_out_f32 = ld_out_f32;
    }
    launch_gemm_fp8(g, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    if (out8) HIP_CHECK(hipMemcpy(out8, dout, R * ld_out8, hipMemcpyDeviceToHost));
    else HIP_CHECK(hipMemcpy(out_f32, dout, R * ld_out_f32 * 4, hipMemcpyDeviceToHost));
    unsigned long long hs = 0;
    HIP_CHECK(hipMemcpy(&hs, sat, 8, hipMemcpyDeviceToHost));
    if (sat_count) *sat_count = hs;
  });
}

extern "C" const char* asr_probe_last_kernel(void) { return g_chain_kernel; }

extern "C" int asr_probe_live_device_bytes(int64_t* bytes) {
  return asr_guard([&] {
    ASR_REQUIRE(bytes, "probe_live_device_bytes: null argument");
    *bytes = asr_live_device_bytes();
  });
}

extern "C" int asr_probe_gemm_counts(int reset, char* buf, int cap) {
  return asr_guard([&] {
    if (buf && cap > 0) gemm_kernel_counts(buf, cap);
    if (reset) gemm_kernel_counts_reset();
  });
}

// Parity hook for the epilogue families the product's batch-64 path uses and asr_op_gemm cannot express: the LayerNorm folded into
// the product (row statistics handed over in 32-column groups, column sums of the bf16 weights), the fused row arg-max, and the
// producer epilogue (f32 + bf16 stores + row statistics) -- and every other GemmArgs term at op level (the transposed store, per-head slabs, the
// post-activation term with its row table, SwiGLU, the RMSNorm fold, rms_out, the device-side row count, pitches wider than the matrix, a launch without
// the split-K workspace, the f32 kernel). Every output buffer reaches the documented edge plus its pitch gap and is filled with a NaN pattern first;
// d->stray counts what changed outside valid rows x valid columns. Reports which kernel family the dispatcher chose.
extern "C" int asr_probe_gemm(asr_probe_gemm_desc* d) {
  return asr_guard([&] {
    ASR_REQUIRE(d && d->a && d->w && d->M > 0 && d->N > 0 && d->K > 0 && d->N % 16 == 0 && d->K % 16 == 0, "probe_gemm: bad argument");
    ASR_REQUIRE(d->pad_a >= 0 && d->pad_w >= 0 && d->pad_out >= 0 && d->pad_out % 8 == 0, "probe_gemm: pad_out must be a multiple of 8");
    asr_require_device(0);
    gemm_reload_env();
    d->stray = 0;
    Tmp t;
    const bool f32 = d->precision != 0;
    const int elt = f32 ? 4 : 2;
    ASR_REQUIRE((d->pad_a * elt) % 16 == 0 && (d->pad_w * elt) % 16 == 0, "probe_gemm: pad_a / pad_w must keep the rows 16-byte aligned");
    ASR_REQUIRE(!(f32 && (d->ln || d->a_rms_eps > 0.0f || d->m_dev >= 0 || d->out_stats || d->out_rms)),
                "probe_gemm: the f32 kernel has no LayerNorm / RMSNorm fold, device-side row count or row statistics, and gemm_reduce_can_norm describes the bf16 dispatcher");
    const int M = d->M, N = d->N, K = d->K, Mp = round_up(M, 128), Mv = d->m_dev >= 0 ? std::min(M, d->m_dev) : M, pad = d->pad_out;
    const int lda = K + d->pad_a, ldw = K + d->pad_w;
    // operands: A [round_up(M, 128)][lda], W [N][ldw]; the pitch gaps and A's rows from M to the tile edge hold NaN (every byte 0xff)
    std::vector<float> ra((size_t)M * K), rw((size_t)N * K);      // the operand values the kernels see
    std::vector<unsigned char> ha((size_t)Mp * lda * elt, 0xff), hw((size_t)N * ldw * elt, 0xff);
    auto put = [&](std::vector<unsigned char>& h, std::vector<float>& r, const float* src, int rows, int ld) {
      for (int m = 0; m < rows; ++m)
        for (int k = 0; k < K; ++k) {
          const float v = src[(size_t)m * K + k];
          if (f32) { memcpy(&h[((size_t)m * ld + k) * 4], &v, 4); r[(size_t)m * K + k] = v; }
          else { const bf16_t b = f32_to_bf16(v); memcpy(&h[((size_t)m * ld + k) * 2], &b, 2); r[(size_t)m * K + k] = bf16_bits_to_f32(b); }
        }
    };
    put(ha, ra, d->a, M, lda);
    put(hw, rw, d->w, N, ldw);
    void* da = t.alloc(ha.size());
    void* dw = t.alloc(hw.size());
    HIP_CHECK(hipMemcpy(da, ha.data(), ha.size(), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dw, hw.data(), hw.size(), hipMemcpyHostToDevice));
    GemmArgs g;
    g.A = da; g.lda = lda; g.W = dw; g.ldw = ldw; g.M = M; g.N = N; g.K = K; g.act = d->act; g.a_rms_eps = d->a_rms_eps;
    if (d->bias) {
      float* db = (float*)t.alloc((size_t)N * 4);
      HIP_CHECK(hipMemcpy(db, d->bias, (size_t)N * 4, hipMemcpyHostToDevice));
      g.bias = db;
    }
    if (d->with_ws) { g.sk_ws = (float*)t.alloc((size_t)16 << 20); g.sk_ws_bytes = (size_t)16 << 20; g.sk_cnt = (int32_t*)t.alloc(4096 * 4); }
    if (d->m_dev >= 0) {
      int32_t* dm = (int32_t*)t.alloc(4);
      HIP_CHECK(hipMemcpy(dm, &d->m_dev, 4, hipMemcpyHostToDevice));
      g.m_dev = dm;
    }
    if (d->ln) {            // LayerNorm(no affine, eps) of the bf16-rounded A rows folded into the product
      ASR_REQUIRE(K % 64 == 0 && N % 128 == 0, "probe_gemm: the LayerNorm fold needs K %% 64 == 0 and N %% 128 == 0");
      std::vector<float> cs(N);
      for (int n = 0; n < N; ++n) { double s = 0.0; for (int k = 0; k < K; ++k) s += rw[(size_t)n * K + k]; cs[n] = (float)s; }
      std::vector<float> st((size_t)Mp * (K / 32) * 2, 0.0f);
      for (int m = 0; m < M; ++m)
        for (int q = 0; q < K / 32; ++q) {
          float s1 = 0.0f, s2 = 0.0f;
          for (int k = 0; k < 32; ++k) { const float v = ra[(size_t)m * K + q * 32 + k]; s1 += v; s2 += v * v; }
          st[((size_t)m * (K / 32) + q) * 2] = s1; st[((size_t)m * (K / 32) + q) * 2 + 1] = s2;
        }
      float* dcs = (float*)t.alloc((size_t)N * 4);
      float2* dst = (float2*)t.alloc(st.size() * 4);
      HIP_CHECK(hipMemcpy(dcs, cs.data(), (size_t)N * 4, hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(dst, st.data(), st.size() * 4, hipMemcpyHostToDevice));
      g.ln_colsum = dcs; g.ln_dim = K; g.ln_stats_in = dst; g.ln_slots = K / 32; g.ln_eps = d->ln_eps;
      ASR_REQUIRE(gemm_ln_fusable(g), "probe_gemm: shape cannot take the LayerNorm-folded kernels");
    }
    // f32 terms [rows][N + pad]: the pitch gap and the rows the kernels may touch without using them hold NaN
    auto upload_rows = [&](const float* src, int rows, int rows_alloc) {
      const int ld = N + pad;
      std::vector<uint32_t> h((size_t)rows_alloc * ld, 0xffffffffu);
      for (int m = 0; m < rows; ++m) memcpy(&h[(size_t)m * ld], src + (size_t)m * N, (size_t)N * 4);
      float* p = (float*)t.alloc(h.size() * 4);
      HIP_CHECK(hipMemcpy(p, h.data(), h.size() * 4, hipMemcpyHostToDevice));
      return p;
    };
    if (d->add) { g.add = upload_rows(d->add, M, Mp); g.ld_add = N + pad; }      // readable to the tile edge
    if (d->add2) {
      const int R = d->add2_table_rows > 0 ? d->add2_table_rows : M;
      ASR_REQUIRE(d->add2_rows || R >= M, "probe_gemm: the add2 table has fewer rows than the product");
      g.add2 = upload_rows(d->add2, R, R); g.ld_add2 = N + pad;
      if (d->add2_rows) {
        for (int m = 0; m < M; ++m) ASR_REQUIRE(d->add2_rows[m] >= 0 && d->add2_rows[m] < R, "probe_gemm: add2_rows[%d] = %d outside the table", m, d->add2_rows[m]);
        int32_t* dr = (int32_t*)t.alloc((size_t)M * 4);
        HIP_CHECK(hipMemcpy(dr, d->add2_rows, (size_t)M * 4, hipMemcpyHostToDevice));
        g.add2_rows = dr;
      }
    }
    // outputs: every buffer reaches the documented edge (round_up(M, 128) rows) plus its pitch gap and holds the NaN pattern before the launch
    Guarded lo, o32, ot, rms, st, av, ai, ids;
    const int n_slabs = N / 64, G = d->lo_group, n_lo = d->act == ACT_SWIGLU ? N / 2 : N;
    if (d->argmax) {
      ASR_REQUIRE(N % 128 == 0 && d->out_ids, "probe_gemm: the arg-max head needs N %% 128 == 0 and out_ids");
      av = guarded(t, Mp, n_slabs, 4); ai = guarded(t, Mp, n_slabs, 4); ids = guarded(t, Mp, 1, 4);
      g.amax_val = (float*)av.dev; g.amax_idx = (int32_t*)ai.dev; g.n_valid = d->n_valid > 0 ? d->n_valid : N;
    }
    if (d->out_lo) {
      if (G > 0) {                                             // [N / G] slabs of [Mp][G] (+ gap)
        ASR_REQUIRE(N % G == 0 && d->act != ACT_SWIGLU, "probe_gemm: lo_group must divide N");
        lo = guarded(t, N / G, (size_t)Mp * G + pad, elt); g.lo_group = G;
      } else lo = guarded(t, Mp, n_lo + pad, elt);
      g.out_lo = lo.dev; g.ld_out_lo = (int)lo.pitch;
    }
    if (d->out_f32) { o32 = guarded(t, Mp, N + pad, 4); g.out_f32 = (float*)o32.dev; g.ld_out_f32 = N + pad; }
    if (d->out_t) {
      const int ld = d->ld_out_t > 0 ? d->ld_out_t : round_up(M, 4) + pad;
      ASR_REQUIRE(ld >= M, "probe_gemm: ld_out_t = %d below M", ld);
      ot = guarded(t, N, ld, elt); g.out_t = ot.dev; g.ld_out_t = ld;
    }
    if (d->out_rms) { rms = guarded(t, Mp, N + pad, elt); g.rms_out = rms.dev; g.ld_rms_out = N + pad; g.rms_eps = d->rms_eps; }
    if (d->out_stats) {
      ASR_REQUIRE(d->out_lo && N % 32 == 0, "probe_gemm: row statistics describe the bf16 output");
      st = guarded(t, Mp, (size_t)(N / 32) * 2, 4); g.st_out = (float2*)st.dev;
    }
    if (f32) {
      launch_gemm_f32(g, nullptr);
    } else {
      if (g.rms_out) ASR_REQUIRE(gemm_reduce_can_norm(g), "probe_gemm: this shape does not take the split-K reduce that writes rms_out (gemm_reduce_can_norm)");
      gemm_set_variant(d->variant);
      try { launch_gemm_bf16(g, nullptr); } catch (...) { gemm_set_variant(-1); throw; }
      gemm_set_variant(-1);
    }
    snprintf(d->kernel, sizeof(d->kernel), "%s", gemm_last_kernel());
    if (d->argmax && Mv > 0) launch_argmax_reduce((const float*)av.dev, (const int32_t*)ai.dev, Mv, n_slabs, (int32_t*)ids.dev, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    std::vector<uint32_t> h;
    int stray = 0;
    auto fetch = [&](const Guarded& b, size_t rows_v, size_t cols_v) { if (b.dev) stray += collect(b, rows_v, cols_v, h); return b.dev != nullptr; };
    auto block = [&](const Guarded& b, void* dst, size_t rows, size_t cols) {       // the top-left rows x cols words of h -> dst
      for (size_t r = 0; r < rows; ++r) memcpy((uint32_t*)dst + r * cols, &h[r * b.pitch], cols * 4);
    };
    if (fetch(ids, Mv, 1)) block(ids, d->out_ids, Mv, 1);
    fetch(av, Mv, n_slabs);
    fetch(ai, Mv, n_slabs);
    if (G > 0) { if (fetch(lo, N / G, (size_t)Mp * G)) { stray += stale_rows(h, lo.pitch, N / G, Mv, Mp, G, elt); block(lo, d->out_lo, N / G, (size_t)Mp * G); } }
    else if (fetch(lo, Mv, n_lo)) block(lo, d->out_lo, Mv, n_lo);
    if (fetch(o32, Mv, N)) block(o32, d->out_f32, Mv, N);
    if (fetch(ot, N, Mv)) block(ot, d->out_t, N, Mv);
    if (fetch(rms, Mv, N)) block(rms, d->out_rms, Mv, N);
    if (fetch(st, Mv, (size_t)(N / 32) * 2)) block(st, d->out_stats, Mv, (size_t)(N / 32) * 2);
    d->stray = stray;
  });
}

// The CTC head with frame log-probabilities: the arg-max GEMM with the third partial (GemmArgs::amax_sum) and launch_argmax_lse_reduce, operands set up
// as asr_probe_gemm does with `argmax`. Every output buffer is padded to the 128-row tile edge and filled with a NaN pattern first; *stray counts the words
// of rows >= M that no longer hold it.
extern "C" int asr_probe_ctc_head(int M, int N, int K, const float* a, const float* w, const float* bias, int n_valid, int variant, int32_t* out_ids,
                                  float* out_logprob, int32_t* stray, char* kernel32) {
  return asr_guard([&] {
    ASR_REQUIRE(a && w && bias && out_ids && out_logprob && M > 0 && N > 0 && K > 0 && N % 128 == 0 && K % 64 == 0 && n_valid >= 0 && n_valid <= N, "probe_ctc_head: bad argument");
    asr_require_device(0);
    gemm_reload_env();
    Tmp t;
    const int Mp = round_up(M, 128) + 128, n_slabs = N / 64;      // one whole spare tile of rows behind the padded operand
    std::vector<bf16_t> ha((size_t)Mp * K, 0), hw((size_t)N * K);
    for (size_t i = 0; i < (size_t)M * K; ++i) ha[i] = f32_to_bf16(a[i]);
    for (size_t i = 0; i < (size_t)N * K; ++i) hw[i] = f32_to_bf16(w[i]);
    bf16_t* da = (bf16_t*)t.alloc(ha.size() * 2);
    bf16_t* dw = (bf16_t*)t.alloc(hw.size() * 2);
    float* db = (float*)t.alloc((size_t)N * 4);
    HIP_CHECK(hipMemcpy(da, ha.data(), ha.size() * 2, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dw, hw.data(), hw.size() * 2, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(db, bias, (size_t)N * 4, hipMemcpyHostToDevice));
    const size_t part = (size_t)Mp * n_slabs;
    uint32_t* dav = (uint32_t*)t.alloc(part * 4); uint32_t* dai = (uint32_t*)t.alloc(part * 4); uint32_t* das = (uint32_t*)t.alloc(part * 4);
    uint32_t* dids = (uint32_t*)t.alloc((size_t)Mp * 4); uint32_t* dlp = (uint32_t*)t.alloc((size_t)Mp * 4);
    for (uint32_t* p : {dav, dai, das}) HIP_CHECK(hipMemset(p, 0xff, part * 4));       // 0xffffffff: a NaN as f32, -1 as an index
    for (uint32_t* p : {dids, dlp}) HIP_CHECK(hipMemset(p, 0xff, (size_t)Mp * 4));
    GemmArgs g;
    g.A = da; g.lda = K; g.W = dw; g.ldw = K; g.M = M; g.N = N; g.K = K; g.bias = db;
    g.sk_ws = (float*)t.alloc((size_t)16 << 20); g.sk_ws_bytes = (size_t)16 << 20; g.sk_cnt = (int32_t*)t.alloc(4096 * 4);
    g.amax_val = (float*)dav; g.amax_idx = (int32_t*)dai; g.amax_sum = (float*)das; g.n_valid = n_valid > 0 ? n_valid : N;
    gemm_set_variant(variant);
    try { launch_gemm_bf16(g, nullptr); } catch (...) { gemm_set_variant(-1); throw; }
    gemm_set_variant(-1);
    if (kernel32) snprintf(kernel32, 32, "%s", gemm_last_kernel());
    launch_argmax_lse_reduce((const float*)dav, (const int32_t*)dai, (const float*)das, M, n_slabs, (int32_t*)dids, (float*)dlp, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out_ids, dids, (size_t)M * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(out_logprob, dlp, (size_t)M * 4, hipMemcpyDeviceToHost));
    if (stray) {
      int bad = 0;
      std::vector<uint32_t> h;
      auto tail = [&](const uint32_t* p, size_t per_row) {
        h.resize((size_t)(Mp - M) * per_row);
        HIP_CHECK(hipMemcpy(h.data(), p + (size_t)M * per_row, h.size() * 4, hipMemcpyDeviceToHost));
        for (uint32_t v : h) bad += v != 0xffffffffu;
      };
      tail(dav, n_slabs); tail(dai, n_slabs); tail(das, n_slabs); tail(dids, 1); tail(dlp, 1);
      *stray = bad;
    }
  });
}

// The candidate kernel behind the same head (launch_ctc_topk): operands and `variant` as asr_probe_ctc_head; precision ASR_PRECISION_BF16 rounds a / w to
// bf16 as that entry does, ASR_PRECISION_F32 keeps them and runs the f32 GEMM (variant is then ignored). out_ids / out_logprob [M][topk].
extern "C" int asr_probe_ctc_topk(int M, int N, int K, const float* a, const float* w, const float* bias, int n_valid, int variant, int precision, int topk,
                                  int32_t* out_ids, float* out_logprob, char* kernel32) {
  return asr_guard([&] {
    ASR_REQUIRE(a && w && bias && out_ids && out_logprob && M > 0 && N > 0 && K > 0 && N % 128 == 0 && K % 64 == 0 && n_valid >= 0 && n_valid <= N, "probe_ctc_topk: bad argument");
    ASR_REQUIRE(precision == ASR_PRECISION_BF16 || precision == ASR_PRECISION_F32, "probe_ctc_topk: precision %d (bf16 or f32)", precision);
    asr_require_device(0);
    gemm_reload_env();
    Tmp t;
    const bool lo = precision == ASR_PRECISION_BF16;
    const int Mp = round_up(M, 128) + 128, n_slabs = N / 64, nv = n_valid > 0 ? n_valid : N;
    void *da = nullptr, *dw = nullptr;
    if (lo) {
      std::vector<bf16_t> ha((size_t)Mp * K, 0), hw((size_t)N * K);
      for (size_t i = 0; i < (size_t)M * K; ++i) ha[i] = f32_to_bf16(a[i]);
      for (size_t i = 0; i < (size_t)N * K; ++i) hw[i] = f32_to_bf16(w[i]);
      da = t.alloc(ha.size() * 2); dw = t.alloc(hw.size() * 2);
      HIP_CHECK(hipMemcpy(da, ha.data(), ha.size() * 2, hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(dw, hw.data(), hw.size() * 2, hipMemcpyHostToDevice));
    } else {
      da = t.alloc((size_t)Mp * K * 4); dw = t.alloc((size_t)N * K * 4);
      HIP_CHECK(hipMemcpy(da, a, (size_t)M * K * 4, hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(dw, w, (size_t)N * K * 4, hipMemcpyHostToDevice));
    }
    float* db = (float*)t.alloc((size_t)N * 4);
    HIP_CHECK(hipMemcpy(db, bias, (size_t)N * 4, hipMemcpyHostToDevice));
    const size_t part = (size_t)Mp * n_slabs;
    float* dav = (float*)t.alloc(part * 4); int32_t* dai = (int32_t*)t.alloc(part * 4); float* das = (float*)t.alloc(part * 4);
    int32_t* dci = (int32_t*)t.alloc((size_t)Mp * topk * 4); float* dcl = (float*)t.alloc((size_t)Mp * topk * 4);
    GemmArgs g;
    g.A = da; g.lda = K; g.W = dw; g.ldw = K; g.M = M; g.N = N; g.K = K; g.bias = db;
    g.amax_val = dav; g.amax_idx = dai; g.amax_sum = das; g.n_valid = nv;
    if (lo) {
      g.sk_ws = (float*)t.alloc((size_t)16 << 20); g.sk_ws_bytes = (size_t)16 << 20; g.sk_cnt = (int32_t*)t.alloc(4096 * 4);
      gemm_set_variant(variant);
      try { launch_gemm_bf16(g, nullptr); } catch (...) { gemm_set_variant(-1); throw; }
      gemm_set_variant(-1);
      if (kernel32) snprintf(kernel32, 32, "%s", gemm_last_kernel());
      launch_ctc_topk<bf16_t>((const bf16_t*)da, K, (const bf16_t*)dw, K, db, K, dav, das, n_slabs, M, nv, topk, dci, dcl, nullptr);
    } else {
      launch_gemm_f32(g, nullptr);
      if (kernel32) snprintf(kernel32, 32, "f32");
      launch_ctc_topk<float>((const float*)da, K, (const float*)dw, K, db, K, dav, das, n_slabs, M, nv, topk, dci, dcl, nullptr);
    }
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out_ids, dci, (size_t)M * topk * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(out_logprob, dcl, (size_t)M * topk * 4, hipMemcpyDeviceToHost));
  });
}

// The emission kernel of the forced alignment behind the same head (launch_ctc_target_logprob): operands, `variant` and `precision` as asr_probe_ctc_topk.
// row_utt [M] maps every row to one of n_utts transcripts (or -1: the row is left alone), target_ids / target_offsets are ragged over the transcripts.
// out_em [M][ld_em]. The device buffer is padded to the tile edge and NaN-filled first; *stray counts the words of rows >= M that no longer hold the pattern.
extern "C" int asr_probe_ctc_target_logprob(int M, int N, int K, const float* a, const float* w, const float* bias, int n_valid, int variant, int precision,
                                            const int32_t* row_utt, int n_utts, const int32_t* target_ids, const int32_t* target_offsets, int blank_id, int ld_em,
                                            float* out_em, int32_t* stray, char* kernel32) {
  return asr_guard([&] {
    ASR_REQUIRE(a && w && bias && out_em && row_utt && target_ids && target_offsets && M > 0 && N > 0 && K > 0 && N % 128 == 0 && K % 64 == 0 && n_valid >= 0 && n_valid <= N && n_utts > 0,
                "probe_ctc_target_logprob: bad argument");
    ASR_REQUIRE(precision == ASR_PRECISION_BF16 || precision == ASR_PRECISION_F32, "probe_ctc_target_logprob: precision %d (bf16 or f32)", precision);
    const int nv = n_valid > 0 ? n_valid : N;
    ASR_REQUIRE(target_offsets[0] == 0 && blank_id >= 0 && blank_id < nv, "probe_ctc_target_logprob: target_offsets[0] = %d, blank %d", target_offsets[0], blank_id);
    for (int u = 0; u < n_utts; ++u) {
      ASR_REQUIRE(target_offsets[u + 1] >= target_offsets[u] && target_offsets[u + 1] - target_offsets[u] < ld_em, "probe_ctc_target_logprob: transcript %d does not fit ld_em = %d", u, ld_em);
      for (int32_t i = target_offsets[u]; i < target_offsets[u + 1]; ++i) ASR_REQUIRE(target_ids[i] >= 0 && target_ids[i] < nv, "probe_ctc_target_logprob: target %d outside the valid columns", target_ids[i]);
    }
    for (int m = 0; m < M; ++m) ASR_REQUIRE(row_utt[m] >= -1 && row_utt[m] < n_utts, "probe_ctc_target_logprob: row_utt[%d] = %d", m, row_utt[m]);
    asr_require_device(0);
    gemm_reload_env();
    Tmp t;
    const bool lo = precision == ASR_PRECISION_BF16;
    const int Mp = round_up(M, 128) + 128, n_slabs = N / 64;
    void *da = nullptr, *dw = nullptr;
    if (lo) {
      std::vector<bf16_t> ha((size_t)Mp * K, 0), hw((size_t)N * K);
      for (size_t i = 0; i < (size_t)M * K; ++i) ha[i] = f32_to_bf16(a[i]);
      for (size_t i = 0; i < (size_t)N * K; ++i) hw[i] = f32_to_bf16(w[i]);
      da = t.alloc(ha.size() * 2); dw = t.alloc(hw.size() * 2);
      HIP_CHECK(hipMemcpy(da, ha.data(), ha.size() * 2, hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(dw, hw.data(), hw.size() * 2, hipMemcpyHostToDevice));
    } else {
      da = t.alloc((size_t)Mp * K * 4); dw = t.alloc((size_t)N * K * 4);
      HIP_CHECK(hipMemcpy(da, a, (size_t)M * K * 4, hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(dw, w, (size_t)N * K * 4, hipMemcpyHostToDevice));
    }
    float* db = (float*)t.alloc((size_t)N * 4);
    HIP_CHECK(hipMemcpy(db, bias, (size_t)N * 4, hipMemcpyHostToDevice));
    const size_t part = (size_t)Mp * n_slabs, n_tgt = (size_t)target_offsets[n_utts];
    float* dav = (float*)t.alloc(part * 4); int32_t* dai = (int32_t*)t.alloc(part * 4); float* das = (float*)t.alloc(part * 4);
    std::vector<int32_t> hru(Mp, -1);
    memcpy(hru.data(), row_utt, (size_t)M * 4);
    int32_t* dru = (int32_t*)t.alloc((size_t)Mp * 4);
    int32_t* dtgt = (int32_t*)t.alloc(n_tgt * 4);
    int32_t* doff = (int32_t*)t.alloc((size_t)(n_utts + 1) * 4);
    uint32_t* dem = (uint32_t*)t.alloc((size_t)Mp * ld_em * 4);
    HIP_CHECK(hipMemcpy(dru, hru.data(), (size_t)Mp * 4, hipMemcpyHostToDevice));
    if (n_tgt) HIP_CHECK(hipMemcpy(dtgt, target_ids, n_tgt * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(doff, target_offsets, (size_t)(n_utts + 1) * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemset(dem, 0xff, (size_t)Mp * ld_em * 4));
    GemmArgs g;
    g.A = da; g.lda = K; g.W = dw; g.ldw = K; g.M = M; g.N = N; g.K = K; g.bias = db;
    g.amax_val = dav; g.amax_idx = dai; g.amax_sum = das; g.n_valid = nv;
    if (lo) {
      g.sk_ws = (float*)t.alloc((size_t)16 << 20); g.sk_ws_bytes = (size_t)16 << 20; g.sk_cnt = (int32_t*)t.alloc(4096 * 4);
      gemm_set_variant(variant);
      try { launch_gemm_bf16(g, nullptr); } catch (...) { gemm_set_variant(-1); throw; }
      gemm_set_variant(-1);
      if (kernel32) snprintf(kernel32, 32, "%s", gemm_last_kernel());
      launch_ctc_target_logprob<bf16_t>((const bf16_t*)da, K, (const bf16_t*)dw, K, db, K, dav, das, n_slabs, M, dru, dtgt, doff, blank_id, (float*)dem, ld_em, nullptr);
    } else {
      launch_gemm_f32(g, nullptr);
      if (kernel32) snprintf(kernel32, 32, "f32");
      launch_ctc_target_logprob<float>((const float*)da, K, (const float*)dw, K, db, K, dav, das, n_slabs, M, dru, dtgt, doff, blank_id, (float*)dem, ld_em, nullptr);
    }
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out_em, dem, (size_t)M * ld_em * 4, hipMemcpyDeviceToHost));
    if (stray) {
      std::vector<uint32_t> h((size_t)(Mp - M) * ld_em);
      HIP_CHECK(hipMemcpy(h.data(), dem + (size_t)M * ld_em, h.size() * 4, hipMemcpyDeviceToHost));
      int bad = 0;
      for (uint32_t v : h) bad += v != 0xffffffffu;
      *stray = bad;
    }
  });
}

// ---- decoder attention (launch_decode_attention) on host arrays: self-attention over a contiguous or paged cache, cross-attention over
// packed slabs (optionally FP8 through the product's quantiser). Reports which form the dispatcher chose (asr_mi355x_probe.h).
namespace {
template <typename T> T elem_from_f32(float v);
template <> float elem_from_f32<float>(float v) { return v; }
template <> bf16_t elem_from_f32<bf16_t>(float v) { return f32_to_bf16(v); }
inline float elem_to_f32(float v) { return v; }
inline float elem_to_f32(bf16_t v) { return bf16_bits_to_f32(v); }
template <typename T> T elem_nan();
template <> float elem_nan<float>() { return std::nanf(""); }
template <> bf16_t elem_nan<bf16_t>() { return (bf16_t)0x7fc0; }
template <typename T> bool same_bits(T x, T y) { return std::memcmp(&x, &y, sizeof(T)) == 0; }

// key_start (host [B], nullable): the single-token self forms with DecAttnArgs::key_start; prompt: the call goes to launch_prompt_attention instead
// (any n, whole batch, empty cache), with key_start as the per-sequence left pad.
template <typename T>
void probe_decode_attention(asr_probe_decode_attn_desc* d, const int32_t* key_start = nullptr, bool prompt = false) {
  Tmp t;
  const int B = d->B, H = d->H, n = d->n, D = H * 64, nb = d->nb > 0 ? d->nb : d->B - d->b0;
  ASR_REQUIRE(B > 0 && H > 0 && n >= 1 && n <= (prompt ? 1536 : 8) && d->b0 >= 0 && nb > 0 && d->b0 + nb <= B && d->q && d->out, "probe_decode_attention: bad geometry");
  ASR_REQUIRE(!prompt || (d->b0 == 0 && nb == B && !d->fp8 && !d->hist_dev && (d->cross || d->hist == 0)), "probe_prompt_attention: whole batch, empty cache, bf16 / f32 slabs");
  ASR_REQUIRE(!key_start || prompt || (!d->cross && n == 1), "probe_decode_attention_ks: key_start belongs to single-token self-attention");
  if (key_start)
    for (int b = 0; b < B; ++b)
      ASR_REQUIRE(key_start[b] >= 0 && key_start[b] <= (prompt ? n : d->hist), "probe: key_start[%d] = %d outside 0..%d", b, key_start[b], prompt ? n : d->hist);
  int32_t* dks = nullptr;
  if (key_start) {
    dks = (int32_t*)t.alloc((size_t)B * 4);
    HIP_CHECK(hipMemcpy(dks, key_start, (size_t)B * 4, hipMemcpyHostToDevice));
  }
  ASR_REQUIRE(d->ld_q >= d->q_col0 + D && d->q_col0 >= 0, "probe_decode_attention: q columns [%d, %d) past ld_q %d", d->q_col0, d->q_col0 + D, d->ld_q);
  auto up = [&](const float* src, size_t count) -> T* {
    std::vector<T> h(count);
    for (size_t i = 0; i < count; ++i) h[i] = elem_from_f32<T>(src[i]);
    T* p = (T*)t.alloc(count * sizeof(T));
    HIP_CHECK(hipMemcpy(p, h.data(), count * sizeof(T), hipMemcpyHostToDevice));
    return p;
  };
  DecAttnArgs a{};
  a.q = up(d->q, (size_t)B * n * d->ld_q); a.ld_q = d->ld_q; a.q_col0 = d->q_col0;
  a.n = n; a.n_heads = H; a.causal = d->causal; a.b0 = d->b0;
  T* out = (T*)t.alloc((size_t)B * n * D * sizeof(T));
  a.out = out; a.ld_out = D;
  std::vector<T> cache;                 // self: host image of the cache (NaN wherever no cached row was placed)
  T* dcache = nullptr;
  std::vector<size_t> kpos, vpos;       // self: element offset of (b, h, s) row in the image, [B][H][hist + n]
  const int S = d->hist + n;
  if (!d->cross) {
    ASR_REQUIRE(d->kv_new && (d->hist == 0 || (d->k_hist && d->v_hist)) && d->hist >= 0, "probe_decode_attention: self mode needs kv_new and the cached rows");
    a.kv_new = up(d->kv_new, (size_t)B * n * 2 * D); a.ld_new = 2 * D; a.k_col0 = 0; a.v_col0 = D;
    int cap;
    if (d->paged) {
      ASR_REQUIRE(d->page_table && d->n_pages > 0 && d->pages_per_seq > 0, "probe_decode_attention: paged cache without a page table");
      for (int i = 0; i < B * d->pages_per_seq; ++i)
        ASR_REQUIRE(d->page_table[i] >= 0 && d->page_table[i] < d->n_pages, "probe_decode_attention: page id %d outside the pool of %d", d->page_table[i], d->n_pages);
      cap = d->pages_per_seq * 16;
      cache.assign((size_t)d->n_pages * 2 * H * 1024, elem_nan<T>());     // pool [page][K | V][head][16][64], as whisper.hip lays it out
    } else {
      ASR_REQUIRE(d->max_pos > 0, "probe_decode_attention: contiguous cache without max_pos");
      cap = d->max_pos;
      cache.assign((size_t)2 * B * H * cap * 64, elem_nan<T>());          // K [B][H][max_pos][64], then V
    }
    a.max_keys = d->max_keys > 0 ? d->max_keys : cap;
    ASR_REQUIRE(S <= cap && S <= a.max_keys && a.max_keys <= 1536, "probe_decode_attention: %d keys, cache of %d, max_keys %d", S, cap, a.max_keys);
    kpos.resize((size_t)B * H * S); vpos.resize((size_t)B * H * S);
    for (int b = 0; b < B; ++b)
      for (int h = 0; h < H; ++h)
        for (int s = 0; s < S; ++s) {
          const size_t i = ((size_t)b * H + h) * S + s;
          if (d->paged) {
            kpos[i] = (size_t)d->page_table[(size_t)b * d->pages_per_seq + (s >> 4)] * 2 * H * 1024 + (size_t)h * 1024 + (size_t)(s & 15) * 64;
            vpos[i] = kpos[i] + (size_t)H * 1024;
          } else {
            kpos[i] = (((size_t)b * H + h) * cap + s) * 64;
            vpos[i] = kpos[i] + (size_t)B * H * cap * 64;
          }
          if (s < d->hist)
            for (int e = 0; e < 64; ++e) {
              const size_t src = (((size_t)b * H + h) * d->hist + s) * 64 + e;
              cache[kpos[i] + e] = elem_from_f32<T>(d->k_hist[src]);
              cache[vpos[i] + e] = elem_from_f32<T>(d->v_hist[src]);
            }
        }
    dcache = (T*)t.alloc(cache.size() * sizeof(T));
    HIP_CHECK(hipMemcpy(dcache, cache.data(), cache.size() * sizeof(T), hipMemcpyHostToDevice));
    if (d->paged) {
      int32_t* pt = (int32_t*)t.alloc((size_t)B * d->pages_per_seq * 4);
      HIP_CHECK(hipMemcpy(pt, d->page_table, (size_t)B * d->pages_per_seq * 4, hipMemcpyHostToDevice));
      a.k_base = dcache; a.v_base = dcache + (size_t)H * 1024;
      a.page_table = pt; a.pages_per_seq = d->pages_per_seq; a.page_stride = (int64_t)2 * H * 1024;
    } else {
      a.k_base = dcache; a.v_base = dcache + (size_t)B * H * cap * 64;
      a.stride_b = (int64_t)H * cap * 64; a.stride_h = (int64_t)cap * 64;
    }
    a.hist = d->hist;
    if (d->hist_dev) {                  // graph-replay form: the by-value history is deliberately wrong
      int32_t* hd = (int32_t*)t.alloc(4);
      HIP_CHECK(hipMemcpy(hd, &d->hist, 4, hipMemcpyHostToDevice));
      a.hist_dev = hd; a.hist = 0;
    }
  } else {
    ASR_REQUIRE(d->k_slab && d->v_slab && d->row_off && d->n_lfr && d->rows > 0 && !d->causal, "probe_decode_attention: cross mode needs slabs and a plan");
    std::vector<UttPlan> plan(B);
    std::memset(plan.data(), 0, plan.size() * sizeof(UttPlan));
    int longest = 0;
    for (int b = 0; b < B; ++b) {
      ASR_REQUIRE(d->n_lfr[b] >= 1 && d->row_off[b] >= 0 && d->row_off[b] + d->n_lfr[b] <= d->rows, "probe_decode_attention: sequence %d rows [%d, %d) outside the slab of %d",
                  b, d->row_off[b], d->row_off[b] + d->n_lfr[b], d->rows);
      plan[b].n_lfr = d->n_lfr[b]; plan[b].row_off = d->row_off[b]; plan[b].T = d->n_lfr[b];
      longest = std::max(longest, d->n_lfr[b]);
    }
    a.max_keys = d->max_keys > 0 ? d->max_keys : longest;
    ASR_REQUIRE(longest <= a.max_keys && a.max_keys <= 1536, "probe_decode_attention: %d keys, max_keys %d", longest, a.max_keys);
    UttPlan* dp = (UttPlan*)t.alloc(plan.size() * sizeof(UttPlan));
    HIP_CHECK(hipMemcpy(dp, plan.data(), plan.size() * sizeof(UttPlan), hipMemcpyHostToDevice));
    const size_t slab = (size_t)d->rows * 64, half = (size_t)H * slab;
    std::vector<float> kv(2 * half);
    std::memcpy(kv.data(), d->k_slab, half * 4);
    std::memcpy(kv.data() + half, d->v_slab, half * 4);
    a.plan = dp; a.stride_b = 0; a.stride_h = (int64_t)slab;
    if (d->fp8) {
      ASR_REQUIRE(sizeof(T) == 2, "probe_decode_attention: FP8 slabs need a bf16 session");
      std::vector<bf16_t> hb(kv.size());
      for (size_t i = 0; i < kv.size(); ++i) hb[i] = f32_to_bf16(kv[i]);
      bf16_t* src = (bf16_t*)t.alloc(hb.size() * 2);
      HIP_CHECK(hipMemcpy(src, hb.data(), hb.size() * 2, hipMemcpyHostToDevice));
      unsigned char* q8 = (unsigned char*)t.alloc(kv.size());
      float* sc = (float*)t.alloc((size_t)2 * H * B * 4);
      launch_quantize_crosskv_fp8(src, slab, 2 * H, dp, B, q8, sc, 0, nullptr);
      a.k_base = q8; a.v_base = q8 + half;
      a.k_scale = sc; a.v_scale = sc + (size_t)H * B; a.scale_ld = B;
      HIP_CHECK(hipDeviceSynchronize());
      if (d->kv8) HIP_CHECK(hipMemcpy(d->kv8, q8, kv.size(), hipMemcpyDeviceToHost));
      if (d->scale8) HIP_CHECK(hipMemcpy(d->scale8, sc, (size_t)2 * H * B * 4, hipMemcpyDeviceToHost));
    } else {
      T* dkv = up(kv.data(), kv.size());
      a.k_base = dkv; a.v_base = dkv + half;
    }
  }
  if (prompt) {
    PromptAttnArgs pa;
    pa.q = a.q; pa.ld_q = a.ld_q; pa.q_col0 = a.q_col0; pa.kv_new = a.kv_new; pa.ld_new = a.ld_new; pa.k_col0 = a.k_col0; pa.v_col0 = a.v_col0;
    pa.k_base = a.k_base; pa.v_base = a.v_base; pa.stride_b = a.stride_b; pa.stride_h = a.stride_h;
    pa.page_table = a.page_table; pa.pages_per_seq = a.pages_per_seq; pa.page_stride = a.page_stride; pa.plan = a.plan;
    pa.key_start = dks; pa.n = n; pa.n_heads = H; pa.out = a.out; pa.ld_out = a.ld_out;
    launch_prompt_attention<T>(pa, B, nullptr);
    snprintf(d->kernel, sizeof(d->kernel), "%s", d->cross ? "prompt_cross" : "prompt_self");
  } else {
    a.key_start = dks;
    launch_decode_attention<T>(a, nb, nullptr);
    snprintf(d->kernel, sizeof(d->kernel), "%s", decode_attn_last_kernel());
  }
  HIP_CHECK(hipDeviceSynchronize());
  std::vector<T> ho((size_t)B * n * D);
  HIP_CHECK(hipMemcpy(ho.data(), out, ho.size() * sizeof(T), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < ho.size(); ++i) d->out[i] = elem_to_f32(ho[i]);
  d->stray = 0;
  if (dcache) {
    std::vector<T> after(cache.size());
    HIP_CHECK(hipMemcpy(after.data(), dcache, after.size() * sizeof(T), hipMemcpyDeviceToHost));
    std::vector<unsigned char> seen(cache.size(), 0);
    for (size_t i = 0; i < kpos.size(); ++i)
      for (int e = 0; e < 64; ++e) {
        if (d->k_after) d->k_after[i * 64 + e] = elem_to_f32(after[kpos[i] + e]);
        if (d->v_after) d->v_after[i * 64 + e] = elem_to_f32(after[vpos[i] + e]);
        seen[kpos[i] + e] = seen[vpos[i] + e] = 1;
      }
    for (size_t i = 0; i < cache.size(); ++i) d->stray += (!seen[i] && !same_bits(cache[i], after[i])) ? 1 : 0;
  }
}
}  // namespace

namespace {
template <typename T>
void probe_decode_attention_beam(int rows, int beam, int H, int S, int p0, int hist, int hist_dev, const int32_t* src, int ld_src, const float* q,
                                 const float* kv_new, float* ext, float* out, int32_t* stray, char* kernel, const int32_t* key_start = nullptr) {
  Tmp t;
  const int D = H * 64;
  ASR_REQUIRE(rows > 0 && beam >= 1 && beam <= 8 && rows % beam == 0 && H > 0 && S > 0 && p0 >= 0 && p0 <= hist && hist < S && ld_src >= hist - p0 && ld_src > 0 &&
              src && q && kv_new && ext && out, "probe_decode_attention_beam: bad geometry");
  for (int r = 0; r < rows; ++r)
    for (int j = 0; j < hist - p0; ++j) {
      const int a = src[(size_t)r * ld_src + j];
      ASR_REQUIRE(a >= 0 && a < rows && a / beam == r / beam, "probe_decode_attention_beam: row %d slot %d names row %d outside its utterance", r, j, a);
    }
  auto up = [&](const float* h, size_t count) -> T* {
    std::vector<T> v(count);
    for (size_t i = 0; i < count; ++i) v[i] = elem_from_f32<T>(h[i]);
    T* p = (T*)t.alloc(count * sizeof(T));
    HIP_CHECK(hipMemcpy(p, v.data(), count * sizeof(T), hipMemcpyHostToDevice));
    return p;
  };
  const size_t ext_n = (size_t)rows * 2 * H * S * 64;
  std::vector<T> before(ext_n);
  for (size_t i = 0; i < ext_n; ++i) before[i] = elem_from_f32<T>(ext[i]);
  T* dext = up(ext, ext_n);
  int32_t* dsrc = (int32_t*)t.alloc((size_t)rows * ld_src * 4);
  HIP_CHECK(hipMemcpy(dsrc, src, (size_t)rows * ld_src * 4, hipMemcpyHostToDevice));
  DecAttnArgs a{};
  a.q = up(q, (size_t)rows * D); a.ld_q = D; a.q_col0 = 0;
  a.kv_new = up(kv_new, (size_t)rows * 2 * D); a.ld_new = 2 * D; a.k_col0 = 0; a.v_col0 = D;
  a.k_base = dext; a.v_base = dext + (size_t)H * S * 64; a.stride_b = (int64_t)2 * H * S * 64; a.stride_h = (int64_t)S * 64;
  a.beam_src = dsrc; a.ld_src = ld_src; a.beam_p0 = p0; a.beam = beam;
  a.n = 1; a.n_heads = H; a.causal = 1; a.max_keys = S; a.hist = hist;
  if (key_start) {                      // [rows / beam]: the utterances' left pads
    for (int u = 0; u < rows / beam; ++u) ASR_REQUIRE(key_start[u] >= 0 && key_start[u] <= hist, "probe_decode_attention_beam: key_start[%d] = %d outside 0..%d", u, key_start[u], hist);
    int32_t* dks = (int32_t*)t.alloc((size_t)(rows / beam) * 4);
    HIP_CHECK(hipMemcpy(dks, key_start, (size_t)(rows / beam) * 4, hipMemcpyHostToDevice));
    a.key_start = dks;
  }
  if (hist_dev) {                       // graph-replay form: the by-value history is deliberately wrong
    int32_t* hd = (int32_t*)t.alloc(4);
    HIP_CHECK(hipMemcpy(hd, &hist, 4, hipMemcpyHostToDevice));
    a.hist_dev = hd; a.hist = 0;
  }
  T* dout = (T*)t.alloc((size_t)rows * D * sizeof(T));
  a.out = dout; a.ld_out = D;
  launch_decode_attention<T>(a, rows, nullptr);
  snprintf(kernel, 32, "%s", decode_attn_last_kernel());
  HIP_CHECK(hipDeviceSynchronize());
  std::vector<T> ho((size_t)rows * D), after(ext_n);
  HIP_CHECK(hipMemcpy(ho.data(), dout, ho.size() * sizeof(T), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(after.data(), dext, ext_n * sizeof(T), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < ho.size(); ++i) out[i] = elem_to_f32(ho[i]);
  int n_stray = 0;
  for (size_t i = 0; i < ext_n; ++i) {
    ext[i] = elem_to_f32(after[i]);
    const bool own_slot = (int)((i / 64) % S) == hist;       // the one slot of every (row, K | V, head) the call writes
    n_stray += (!own_slot && !same_bits(before[i], after[i])) ? 1 : 0;
  }
  if (stray) *stray = n_stray;
}
}  // namespace

extern "C" int asr_probe_decode_attention_beam(int bf16, int rows, int beam, int H, int S, int p0, int hist, int hist_dev, const int32_t* src, int ld_src,
                                               const float* q, const float* kv_new, float* ext, float* out, int32_t* stray, char* kernel) {
  return asr_guard([&] {
    ASR_REQUIRE(kernel, "probe_decode_attention_beam: null kernel buffer");
    asr_require_device(0);
    gemm_reload_env();
    if (bf16) probe_decode_attention_beam<bf16_t>(rows, beam, H, S, p0, hist, hist_dev, src, ld_src, q, kv_new, ext, out, stray, kernel);
    else probe_decode_attention_beam<float>(rows, beam, H, S, p0, hist, hist_dev, src, ld_src, q, kv_new, ext, out, stray, kernel);
  });
}

extern "C" int asr_probe_decode_attention_beam_ks(int bf16, int rows, int beam, int H, int S, int p0, int hist, int hist_dev, const int32_t* src, int ld_src,
                                                  const float* q, const float* kv_new, float* ext, float* out, int32_t* stray, char* kernel, const int32_t* key_start) {
  return asr_guard([&] {
    ASR_REQUIRE(kernel, "probe_decode_attention_beam_ks: null kernel buffer");
    asr_require_device(0);
    gemm_reload_env();
    if (bf16) probe_decode_attention_beam<bf16_t>(rows, beam, H, S, p0, hist, hist_dev, src, ld_src, q, kv_new, ext, out, stray, kernel, key_start);
    else probe_decode_attention_beam<float>(rows, beam, H, S, p0, hist, hist_dev, src, ld_src, q, kv_new, ext, out, stray, kernel, key_start);
  });
}

extern "C" int asr_probe_beam_select(asr_probe_beam_select_desc* d) {
  return asr_guard([&] {
    ASR_REQUIRE(d && d->n_utt > 0 && d->beam >= 1 && d->beam <= 8 && d->K >= 1 && d->beam * d->K <= 64 && d->ld > 0 && d->n_slots >= 0 && d->n_slots <= d->ld &&
                d->n_stop >= 0 && d->topv && d->topi && d->cum && d->fin && d->len && d->next && d->done && d->src_in && d->tok_in && d->src_out && d->tok_out &&
                (d->n_stop == 0 || d->stop), "probe_beam_select: bad descriptor");
    asr_require_device(0);
    Tmp t;
    const int N = d->n_utt * d->beam;
    for (int r = 0; r < N; ++r) ASR_REQUIRE(d->len[r] >= 0 && d->len[r] <= d->ld, "probe_beam_select: row %d length %d outside the table", r, d->len[r]);
    auto up = [&](const void* h, size_t bytes) -> void* {
      void* p = t.alloc(std::max(bytes, (size_t)4));
      HIP_CHECK(hipMemcpy(p, h, bytes, hipMemcpyHostToDevice));
      return p;
    };
    const size_t tab = (size_t)N * d->ld * 4, rows4 = (size_t)N * 4;
    BeamArgs a{};
    a.beam = d->beam; a.K = d->K; a.ld = d->ld; a.first = d->first; a.n_slots = d->n_slots;
    a.topv = (const float*)up(d->topv, (size_t)(d->first ? d->n_utt : N) * d->K * 4);
    a.topi = (const int32_t*)up(d->topi, (size_t)(d->first ? d->n_utt : N) * d->K * 4);
    a.cum = (float*)up(d->cum, rows4); a.fin = (int32_t*)up(d->fin, rows4); a.len = (int32_t*)up(d->len, rows4); a.next = (int32_t*)up(d->next, rows4);
    a.done = (int32_t*)up(d->done, (size_t)d->n_utt * 4);
    a.stop = d->n_stop ? (const int32_t*)up(d->stop, (size_t)d->n_stop * 4) : nullptr; a.n_stop = d->n_stop;
    a.src_in = (const int32_t*)up(d->src_in, tab); a.tok_in = (const int32_t*)up(d->tok_in, tab);
    a.src_out = (int32_t*)up(d->src_out, tab); a.tok_out = (int32_t*)up(d->tok_out, tab);
    launch_beam_select(a, d->n_utt, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(d->cum, a.cum, rows4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d->fin, a.fin, rows4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d->len, a.len, rows4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d->next, a.next, rows4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d->done, a.done, (size_t)d->n_utt * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d->src_out, a.src_out, tab, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d->tok_out, a.tok_out, tab, hipMemcpyDeviceToHost));
  });
}

// ---- op 6 of asr_probe_token_head: a TokenHead driven as the sessions drive it -- restart, then enqueue + consumed per step on a fresh copy of the same rows
static void probe_head_steps(asr_probe_token_head_desc* d) {
  const char* who = "probe_token_head";
  const int rows = d->rows, ld = d->ld, steps = d->steps;
  ASR_REQUIRE(d->logits && d->picks && d->save_ids, "%s: head steps need logits, picks and save_ids", who);
  // (more steps than the table holds: only where nothing indexes the table by the raw counter -- the penalty window does)
  const bool may_overflow = d->scores && d->value == 1.0f && d->change_step <= 0 && d->logprob;
  ASR_REQUIRE(steps >= 1 && (d->ld_save >= steps || may_overflow) && d->ld_save >= 1 && d->ld_save <= 1024, "%s: %d steps do not fit the history table of %d", who, steps,
              d->ld_save);
  ASR_REQUIRE(!d->scores || d->logprob, "%s: scores without the logprob table", who);
  // timed: the rows are uploaded once (only a head that edits nothing in place may skip the fresh copy) and the steps' launches run back to back between two device events
  ASR_REQUIRE(!d->timed || (d->value == 1.0f && d->change_step <= 0 && !d->sampling && !d->timestamps), "%s: timed steps need the plain arg-max head", who);
  ASR_REQUIRE(d->range <= d->ld_save && (d->change_step <= 0 || d->range2 <= d->ld_save), "%s: penalty range past the history table of %d", who, d->ld_save);
  ASR_REQUIRE(!d->sampling || d->K <= d->n_valid, "%s: sampler top_k %d", who, d->K);
  ASR_REQUIRE(!d->noise || d->sampling, "%s: noise without the sampler", who);
  asr_require_device(0);
  Tmp t;
  const size_t lbytes = (size_t)rows * ld * 4;
  float* dlog = (float*)t.alloc(lbytes);
  int32_t* dpick = (int32_t*)t.alloc((size_t)steps * rows * 4);
  float* dvec = nullptr;
  if (d->vec) { dvec = (float*)t.alloc((size_t)ld * 4); HIP_CHECK(hipMemcpy(dvec, d->vec, (size_t)ld * 4, hipMemcpyHostToDevice)); }
  TokenHead h;
  h.init(d->ld_save, d->partial, d->range, 1024);
  h.set_penalty(d->value, d->range, who);
  h.set_track_history(d->track_history != 0);
  if (d->sampling) h.set_sampling(true, d->temperature, d->K, d->top_p, d->repetition_penalty, d->seed, who);
  if (d->timestamps) h.set_timestamps(true, d->ts_begin, d->no_timestamps_id, d->eot_id, d->max_initial, d->n_valid, who);
  h.set_scores(d->scores != 0);
  h.reserve(rows, nullptr);
  h.restart(nullptr);
  if (d->scores) HIP_CHECK(hipMemset(h.d_scores.ptr, 0xFF, (size_t)rows * d->ld_save * 4));      // NaN: a column no step wrote shows
  if (d->noise) h.arm_noise(d->noise, rows * d->K, nullptr);
  hipEvent_t ev[2] = {nullptr, nullptr};
  if (d->timed) { HIP_CHECK(hipEventCreate(&ev[0])); HIP_CHECK(hipEventCreate(&ev[1])); }
  d->head_ms = 0.0f;
  for (int i = 0; i < steps; ++i) {
    if (i > 0 && i == d->change_step) h.set_penalty(d->value2, d->range2, who);
    if (i == 0 || !d->timed) HIP_CHECK(hipMemcpy(dlog, d->logits, lbytes, hipMemcpyHostToDevice));
    if (d->timed && i == 0) HIP_CHECK(hipEventRecord(ev[0], nullptr));
    h.enqueue(dlog, ld, rows, d->n_valid, i == 0 ? dvec : nullptr, i > 0, dpick + (size_t)i * rows, nullptr);
    h.consumed();
  }
  if (d->timed) HIP_CHECK(hipEventRecord(ev[1], nullptr));
  HIP_CHECK(hipDeviceSynchronize());
  if (d->timed) {
    HIP_CHECK(hipEventElapsedTime(&d->head_ms, ev[0], ev[1]));
    HIP_CHECK(hipEventDestroy(ev[0])); HIP_CHECK(hipEventDestroy(ev[1]));
  }
  HIP_CHECK(hipMemcpy(d->picks, dpick, (size_t)steps * rows * 4, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(d->save_ids, h.d_save.ptr, (size_t)rows * d->ld_save * 4, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(&d->n_saved_after, h.d_nsaved.ptr, 4, hipMemcpyDeviceToHost));
  if (d->scores) HIP_CHECK(hipMemcpy(d->logprob, h.d_scores.ptr, (size_t)rows * d->ld_save * 4, hipMemcpyDeviceToHost));
}

// ---- the token-selection heads (kernels.h) on host arrays: one product launcher per call, unchanged. Every index a kernel will follow is checked here first.
extern "C" int asr_probe_token_head(asr_probe_token_head_desc* d) {
  return asr_guard([&] {
    ASR_REQUIRE(d && d->op >= 0 && d->op <= 9 && d->rows > 0 && d->n_valid >= 1 && d->ld >= d->n_valid && d->ld % 128 == 0, "probe_token_head: bad descriptor");
    if (d->op == 6) { probe_head_steps(d); return; }
    const int op = d->op, rows = d->rows, ld = d->ld;
    const bool uses_logits = op != 3, uses_save = op == 2 || op == 3 || op == 4 || op == 7;
    ASR_REQUIRE(!uses_logits || d->logits, "probe_token_head: logits missing");
    const bool scoring = op == 8 || op == 9;
    ASR_REQUIRE(!scoring || (d->logprob && d->ld_save >= 1 && d->n_saved >= 0 && (op == 8 || d->next_in)), "probe_token_head: score ops need the logprob table and a counter >= 0 (op 9: ids)");
    ASR_REQUIRE((op == 2 || op == 3 || op == 5 || op == 7 || op == 9 || d->out_i) && ((op != 1 && op != 5) || d->out_v), "probe_token_head: output array missing");
    ASR_REQUIRE(op != 2 || (d->range >= 1 && d->range <= 64 && d->range <= d->ld_save), "probe_token_head: apply_penalty range %d (1..64, within the table)", d->range);
    ASR_REQUIRE(op != 5 || (d->no_speech_id >= 0 && d->no_speech_id < d->n_valid), "probe_token_head: no_speech_id %d outside the vocabulary of %d", d->no_speech_id, d->n_valid);
    if (uses_save) {
      ASR_REQUIRE(d->save_ids && d->ld_save >= 1 && d->n_saved >= 0, "probe_token_head: history table missing");
      ASR_REQUIRE(op != 2 || d->n_saved <= d->ld_save, "probe_token_head: apply_penalty reads save_ids[n_saved - range, n_saved): n_saved %d past the table of %d", d->n_saved, d->ld_save);
      if (op == 7 && d->n_saved_rows)
        for (int r = 0; r < rows; ++r) ASR_REQUIRE(d->n_saved_rows[r] >= 0, "probe_token_head: timestamp_rules counter %d of row %d", d->n_saved_rows[r], r);
      const int used = op == 3 ? 0 : std::min(d->n_saved, d->ld_save);       // the columns whose ids index the logits row
      for (int r = 0; r < rows; ++r)
        for (int j = 0; j < (op == 7 ? d->ld_save : used); ++j) {      // (the rules only compare ids, but a whole table of valid ids is what a session holds)
          const int32_t id = d->save_ids[(size_t)r * d->ld_save + j];
          ASR_REQUIRE(id >= 0 && id < d->n_valid, "probe_token_head: saved id %d of row %d outside the vocabulary of %d", id, r, d->n_valid);
        }
    }
    asr_require_device(0);
    Tmp t;
    auto up = [&](const void* h, size_t bytes) -> void* {
      void* p = t.alloc(bytes);
      HIP_CHECK(hipMemcpy(p, h, bytes, hipMemcpyHostToDevice));
      return p;
    };
    const size_t lbytes = (size_t)rows * ld * 4, sbytes = uses_save ? (size_t)rows * d->ld_save * 4 : 0;
    float* dlog = uses_logits ? (float*)up(d->logits, lbytes) : nullptr;
    const float* dvec = d->vec ? (const float*)up(d->vec, (size_t)ld * 4) : nullptr;
    int32_t* dsave = uses_save ? (int32_t*)up(d->save_ids, sbytes) : nullptr;
    int32_t* dn = uses_save ? (int32_t*)up(&d->n_saved, 4) : nullptr;
    float* dv = nullptr; int32_t* di = nullptr;
    size_t nv = 0, ni = 0;
    switch (op) {
      case 0:
        ni = rows; di = (int32_t*)t.alloc(ni * 4);
        launch_argmax_rows(dlog, ld, rows, d->n_valid, dvec, di, nullptr);
        break;
      case 1:
        ASR_REQUIRE(d->K >= 1 && d->K <= BEAM_MAX, "probe_token_head: beam_topk K %d", d->K);
        nv = ni = (size_t)rows * d->K; dv = (float*)t.alloc(nv * 4); di = (int32_t*)t.alloc(ni * 4);
        launch_beam_topk(dlog, ld, rows, d->n_valid, dvec, d->K, dv, di, nullptr);
        break;
      case 2:
        launch_apply_penalty(dlog, ld, rows, dsave, d->ld_save, dn, d->range, d->value, nullptr, d->partial);
        break;
      case 3:
        ASR_REQUIRE(d->next_in, "probe_token_head: append_ids without ids");
        launch_append_ids((const int32_t*)up(d->next_in, (size_t)rows * 4), rows, dsave, d->ld_save, dn, nullptr);
        break;
      case 4: {
        ASR_REQUIRE(d->K >= 1 && d->K <= 64 && d->K <= d->n_valid, "probe_token_head: sampler top_k %d", d->K);
        ni = rows; di = (int32_t*)t.alloc(ni * 4);
        SampleArgs a{};
        a.logits = dlog; a.ld = ld; a.rows = rows; a.n_valid = d->n_valid; a.extra = dvec;
        a.save_ids = dsave; a.ld_save = d->ld_save; a.n_saved = dn;
        a.temperature = d->temperature; a.top_p = d->top_p; a.repetition_penalty = d->repetition_penalty; a.top_k = d->K;
        a.noise = d->noise ? (const float*)up(d->noise, (size_t)rows * d->K * 4) : nullptr; a.seed = d->seed;
        a.next = di;
        launch_sample_topk_topp(a, nullptr);
        break;
      }
      case 8:
      case 9: {             // ids outside the vocabulary are the kernel's to refuse (score -inf): it checks before it reads
        const size_t tbytes = (size_t)rows * d->ld_save * 4;
        float* dlp = (float*)up(d->logprob, tbytes);
        const int32_t* dcnt = (const int32_t*)up(&d->n_saved, 4);
        if (op == 8) {
          ni = rows; di = (int32_t*)up(d->out_i, ni * 4);
          launch_argmax_logprob_rows(dlog, ld, rows, d->n_valid, dvec, di, dlp, d->ld_save, dcnt, nullptr);
        } else {
          launch_logprob_at_rows(dlog, ld, rows, d->n_valid, dvec, (const int32_t*)up(d->next_in, (size_t)rows * 4), dlp, d->ld_save, dcnt, nullptr);
        }
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(d->logprob, dlp, tbytes, hipMemcpyDeviceToHost));
        break;
      }
      case 7: {             // the launcher checks the four parameters itself
        const int32_t* dnr = d->n_saved_rows ? (const int32_t*)up(d->n_saved_rows, (size_t)rows * 4) : dn;
        launch_timestamp_rules(dlog, ld, rows, d->n_valid, dsave, d->ld_save, dnr, d->n_saved_rows ? 1 : 0, d->ts_begin, d->no_timestamps_id, d->eot_id,
                               d->max_initial, nullptr);
        break;
      }
      default:
        ASR_REQUIRE(dvec, "probe_token_head: no_speech_prob without the penalty vector");
        nv = rows; dv = (float*)t.alloc(nv * 4);
        launch_no_speech_prob(dlog, ld, rows, d->n_valid, dvec, d->no_speech_id, dv, nullptr);
        break;
    }
    HIP_CHECK(hipDeviceSynchronize());
    if (nv) HIP_CHECK(hipMemcpy(d->out_v, dv, nv * 4, hipMemcpyDeviceToHost));
    if (ni) HIP_CHECK(hipMemcpy(d->out_i, di, ni * 4, hipMemcpyDeviceToHost));
    if (uses_logits) HIP_CHECK(hipMemcpy(d->logits, dlog, lbytes, hipMemcpyDeviceToHost));
    if (uses_save) {
      HIP_CHECK(hipMemcpy(d->save_ids, dsave, sbytes, hipMemcpyDeviceToHost));
      HIP_CHECK(hipMemcpy(&d->n_saved_after, dn, 4, hipMemcpyDeviceToHost));
    }
  });
}

// ---- the kernels of the Whisper token-timestamp path (csrc/whisper_align.hip) on host arrays, one product launcher per call
extern "C" int asr_probe_whisper_align(asr_probe_whisper_align_desc* d) {
  return asr_guard([&] {
    ASR_REQUIRE(d && d->op >= 0 && d->op <= 4, "probe_whisper_align: bad descriptor");
    const int op = d->op, B = d->B, P = d->n_pairs, R = d->max_rows, ld = d->ld;
    ASR_REQUIRE(B >= 1 && B <= 64 && P >= 1 && P <= 64 && R >= 1 && R <= 1536 && ld >= 1 && ld <= 4096, "probe_whisper_align: extents B %d pairs %d rows %d ld %d", B, P, R, ld);
    const size_t n_scores = (size_t)B * P * R * ld, n_cost = (size_t)B * R * ld, n_stats = (size_t)B * P * 2 * ld;
    int rows_max = 0, frames_max = 0;
    if (op >= 1) {
      ASR_REQUIRE(d->n_rows && d->n_frames, "probe_whisper_align: n_rows / n_frames missing");
      for (int b = 0; b < B; ++b) {
        ASR_REQUIRE(d->n_rows[b] >= 0 && d->n_rows[b] <= R && d->n_frames[b] >= 1 && d->n_frames[b] <= ld, "probe_whisper_align: utterance %d: %d rows, %d frames", b,
                    d->n_rows[b], d->n_frames[b]);
        rows_max = std::max(rows_max, d->n_rows[b]); frames_max = std::max(frames_max, d->n_frames[b]);
      }
      ASR_REQUIRE(rows_max >= 1, "probe_whisper_align: no utterance has rows");
    }
    asr_require_device(0);
    Tmp t;
    auto up = [&](const void* h, size_t bytes) -> void* {
      void* p = t.alloc(bytes);
      HIP_CHECK(hipMemcpy(p, h, bytes, hipMemcpyHostToDevice));
      return p;
    };
    const int32_t* dn = op >= 1 ? (const int32_t*)up(d->n_rows, (size_t)B * 4) : nullptr;
    const int32_t* df = op >= 1 ? (const int32_t*)up(d->n_frames, (size_t)B * 4) : nullptr;
    if (op == 0) {
      const int H = d->H, n = d->n;
      ASR_REQUIRE(d->q && d->k_slab && d->row_off && d->n_lfr && d->sel && d->scores, "probe_whisper_align: scores: array missing");
      ASR_REQUIRE(H >= 1 && H <= 64 && n >= 1 && n <= 8 && d->n_sel >= 1 && d->n_sel <= P && d->slab_rows >= 1, "probe_whisper_align: scores: H %d n %d n_sel %d", H, n, d->n_sel);
      int max_keys = 0;
      std::vector<UttPlan> plan(B);
      for (int b = 0; b < B; ++b) {
        ASR_REQUIRE(d->n_lfr[b] >= 1 && d->n_lfr[b] <= ld && d->row_off[b] >= 0 && d->row_off[b] + d->n_lfr[b] <= d->slab_rows, "probe_whisper_align: utterance %d outside the slab", b);
        plan[b] = UttPlan{}; plan[b].n_lfr = d->n_lfr[b]; plan[b].row_off = d->row_off[b];
        max_keys = std::max(max_keys, d->n_lfr[b]);
      }
      for (int i = 0; i < d->n_sel; ++i)
        ASR_REQUIRE(d->sel[2 * i] >= 0 && d->sel[2 * i] < H && d->sel[2 * i + 1] >= 0 && d->sel[2 * i + 1] < P, "probe_whisper_align: sel[%d] = (%d, %d)", i, d->sel[2 * i], d->sel[2 * i + 1]);
      const size_t nq = (size_t)B * n * H * 64, nk = (size_t)H * d->slab_rows * 64;
      AlignScoresArgs a;
      if (d->bf16) {
        std::vector<bf16_t> hq(nq), hk(nk);
        for (size_t i = 0; i < nq; ++i) hq[i] = f32_to_bf16(d->q[i]);
        for (size_t i = 0; i < nk; ++i) hk[i] = f32_to_bf16(d->k_slab[i]);
        a.q = up(hq.data(), nq * 2); a.k_base = up(hk.data(), nk * 2);
      } else {
        a.q = up(d->q, nq * 4); a.k_base = up(d->k_slab, nk * 4);
      }
      a.ld_q = H * 64; a.n = n; a.stride_h = (int64_t)d->slab_rows * 64;
      a.plan = (const UttPlan*)up(plan.data(), sizeof(UttPlan) * B);
      a.sel = (const int32_t*)up(d->sel, (size_t)d->n_sel * 8); a.n_sel = d->n_sel;
      a.pos_dev = (const int32_t*)up(&d->position, 4); a.row_bias = n - 1 - d->p0;
      float* ds = (float*)up(d->scores, n_scores * 4);
      a.out = ds; a.n_pairs = P; a.max_rows = R; a.ld = ld; a.max_keys = max_keys;
      if (d->bf16) launch_align_scores<bf16_t>(a, B, nullptr);
      else launch_align_scores<float>(a, B, nullptr);
      HIP_CHECK(hipDeviceSynchronize());
      HIP_CHECK(hipMemcpy(d->scores, ds, n_scores * 4, hipMemcpyDeviceToHost));
      return;
    }
    if (op == 1) {
      ASR_REQUIRE(d->scores, "probe_whisper_align: scores missing");
      float* ds = (float*)up(d->scores, n_scores * 4);
      launch_align_softmax(ds, B, P, R, ld, dn, df, rows_max, nullptr);
      HIP_CHECK(hipDeviceSynchronize());
      HIP_CHECK(hipMemcpy(d->scores, ds, n_scores * 4, hipMemcpyDeviceToHost));
    } else if (op == 2) {
      ASR_REQUIRE(d->scores && d->stats, "probe_whisper_align: scores / stats missing");
      float* dst = (float*)up(d->stats, n_stats * 4);
      launch_align_colstats((const float*)up(d->scores, n_scores * 4), B, P, R, ld, dn, df, frames_max, dst, nullptr);
      HIP_CHECK(hipDeviceSynchronize());
      HIP_CHECK(hipMemcpy(d->stats, dst, n_stats * 4, hipMemcpyDeviceToHost));
    } else if (op == 3) {
      ASR_REQUIRE(d->scores && d->stats && d->cost, "probe_whisper_align: scores / stats / cost missing");
      float* dc = (float*)up(d->cost, n_cost * 4);
      launch_align_cost((const float*)up(d->scores, n_scores * 4), (const float*)up(d->stats, n_stats * 4), B, P, R, ld, dn, df, rows_max, frames_max, d->width, dc, nullptr);
      HIP_CHECK(hipDeviceSynchronize());
      HIP_CHECK(hipMemcpy(d->cost, dc, n_cost * 4, hipMemcpyDeviceToHost));
    } else {
      ASR_REQUIRE(d->cost && d->frames && d->path && d->path_len && d->path_stride >= R + ld, "probe_whisper_align: dtw: array missing or path_stride below rows + frames");
      const size_t trace_stride = (size_t)(R + 1) * (ld + 1);
      int32_t* dfr = (int32_t*)up(d->frames, (size_t)B * R * 4);
      int32_t* dp = (int32_t*)up(d->path, (size_t)B * d->path_stride * 8);
      int32_t* dl = (int32_t*)t.alloc((size_t)B * 4);
      launch_align_dtw((const float*)up(d->cost, n_cost * 4), B, R, ld, dn, df, rows_max, (unsigned char*)t.alloc((size_t)B * trace_stride), trace_stride, dfr, R, dp,
                       d->path_stride, dl, nullptr);
      HIP_CHECK(hipDeviceSynchronize());
      HIP_CHECK(hipMemcpy(d->frames, dfr, (size_t)B * R * 4, hipMemcpyDeviceToHost));
      HIP_CHECK(hipMemcpy(d->path, dp, (size_t)B * d->path_stride * 8, hipMemcpyDeviceToHost));
      HIP_CHECK(hipMemcpy(d->path_len, dl, (size_t)B * 4, hipMemcpyDeviceToHost));
    }
  });
}

extern "C" int asr_probe_decode_attention(asr_probe_decode_attn_desc* d) {
  return asr_guard([&] {
    ASR_REQUIRE(d, "probe_decode_attention: null descriptor");
    asr_require_device(0);
    gemm_reload_env();
    if (d->bf16) probe_decode_attention<bf16_t>(d);
    else probe_decode_attention<float>(d);
  });
}

extern "C" int asr_probe_decode_attention_ks(asr_probe_decode_attn_desc* d, const int32_t* key_start) {
  return asr_guard([&] {
    ASR_REQUIRE(d, "probe_decode_attention_ks: null descriptor");
    asr_require_device(0);
    gemm_reload_env();
    if (d->bf16) probe_decode_attention<bf16_t>(d, key_start);
    else probe_decode_attention<float>(d, key_start);
  });
}

extern "C" int asr_probe_prompt_attention(asr_probe_decode_attn_desc* d, const int32_t* key_start) {
  return asr_guard([&] {
    ASR_REQUIRE(d, "probe_prompt_attention: null descriptor");
    asr_require_device(0);
    if (d->bf16) probe_decode_attention<bf16_t>(d, key_start, true);
    else probe_decode_attention<float>(d, key_start, true);
  });
}

// ---- the attention stage of a Qwen3 decoder layer (launch_qwen_attention, csrc/qwen_attn.h) on host arrays. The device state is what a session has at that
// point and no more: zeros where the session guarantees zeros (the q|k|v rows of gap rows -- the packed layout starts every sequence at a multiple of 16 rows and
// the gather writes zeros between them, so the V^T columns past a sequence are zero too), NaN everywhere else (cache slots at and past hist, pages and layers the
// table does not name, operand / key / context rows nobody wrote).
namespace {
inline size_t qw_pad_rows(size_t r) { return (r + 127) / 128 * 128 + 144; }       // QwSession's row padding

template <typename T>
void probe_qwen_attention(asr_probe_qwen_attn_desc* d) {
  Tmp t;
  constexpr int HD = 128, LAYERS = 2, LAYER = 1;          // the paged pool is page-major over two layers and the call works on the second: page_stride matters
  const int B = d->B, H = d->H, KV = d->KV, rows = d->rows, heads = H + 2 * KV;
  const bool beam = d->beam > 0;
  ASR_REQUIRE(B > 0 && H > 0 && KV > 0 && H % KV == 0 && rows > 0 && d->rope_rows > 0 && d->S_max > 0 && d->S_max <= 16000, "probe_qwen_attention: bad geometry");
  ASR_REQUIRE(d->qkv && d->qn && d->kn && d->rope && d->hist && d->T && d->row_off && d->row_seq && d->row_t && d->ctx, "probe_qwen_attention: null operand");
  const int G = H / KV;
  const int n_seq = beam ? B / d->beam : B;               // sequences of the session's own cache
  const int cap = d->paged ? d->pps * 16 : d->S_max;      // positions the session cache can address per sequence
  if (d->paged) {
    ASR_REQUIRE(d->table && d->n_pages > 0 && d->pps > 0, "probe_qwen_attention: paged cache without a table");
    for (int i = 0; i < n_seq * d->pps; ++i)
      ASR_REQUIRE(d->table[i] >= 0 && d->table[i] < d->n_pages, "probe_qwen_attention: page id %d outside the pool of %d", d->table[i], d->n_pages);
  }
  if (d->step) ASR_REQUIRE(rows == B, "probe_qwen_attention: a step has one row per sequence");
  int max_len = 0;
  for (int b = 0; b < B; ++b) {
    const int hb = d->hist[b], Tb = d->T[b], r0 = d->row_off[b];
    ASR_REQUIRE(Tb >= 1 && hb >= 0 && hb + Tb <= d->rope_rows && (beam || hb + Tb <= std::min(cap, d->S_max)), "probe_qwen_attention: sequence %d positions [%d, %d) outside the cache / rope table", b, hb, hb + Tb);
    ASR_REQUIRE(r0 >= 0 && r0 + Tb <= rows && (d->step ? (Tb == 1 && r0 == b) : r0 % 16 == 0), "probe_qwen_attention: sequence %d rows [%d, %d) of %d", b, r0, r0 + Tb, rows);
    max_len = std::max(max_len, Tb);
  }
  for (int r = 0; r < rows; ++r) {
    const int b = d->row_seq[r];
    ASR_REQUIRE(b >= -1 && b < B && (b < 0 || (d->row_t[r] >= 0 && d->row_t[r] < d->T[b] && r == d->row_off[b] + d->row_t[r])), "probe_qwen_attention: row %d does not match the plan", r);
  }
  if (beam) {
    ASR_REQUIRE(d->beam <= 8 && B % d->beam == 0 && d->step && !d->no_fuse && (G == 1 || G == 2 || G == 4), "probe_qwen_attention: beam rows need the fused step (G in 1, 2, 4)");
    ASR_REQUIRE(d->src && d->p0 && d->ext_k && d->ext_v && d->S_hyp > 0 && d->ld_src > 0, "probe_qwen_attention: beam mode without its tables");
    for (int b = 0; b < B; ++b) {
      const int p0 = d->p0[b], gen = d->hist[b] - p0;
      ASR_REQUIRE(p0 == d->p0[b / d->beam * d->beam] && p0 >= 0 && p0 <= std::min(cap, d->S_max) && gen >= 0 && gen < d->S_hyp && gen <= d->ld_src, "probe_qwen_attention: row %d prompt %d, %d generated", b, p0, gen);
      for (int j = 0; j < gen; ++j) {
        const int a = d->src[(size_t)b * d->ld_src + j];
        ASR_REQUIRE(a >= 0 && a < B && a / d->beam == b / d->beam, "probe_qwen_attention: row %d slot %d names row %d outside its utterance", b, j, a);
      }
    }
  }
  auto up_raw = [&](const void* h, size_t bytes) -> void* {
    void* p = t.alloc(bytes);
    HIP_CHECK(hipMemcpy(p, h, bytes, hipMemcpyHostToDevice));
    return p;
  };
  auto up_t = [&](const std::vector<T>& h) -> T* { return (T*)up_raw(h.data(), h.size() * sizeof(T)); };
  // ---- operands
  const size_t Md = qw_pad_rows(rows);
  std::vector<float> hqkv(Md * heads * HD, 0.0f);
  std::memcpy(hqkv.data(), d->qkv, (size_t)rows * heads * HD * 4);
  QwAttnArgs a;
  a.bf16 = sizeof(T) == 2; a.step = d->step != 0; a.no_fuse = d->no_fuse != 0;
  a.qkv = (const float*)up_raw(hqkv.data(), hqkv.size() * 4);
  a.rows = rows; a.B = B; a.H = H; a.KV = KV; a.eps = d->eps;
  a.qn = (const float*)up_raw(d->qn, HD * 4); a.kn = (const float*)up_raw(d->kn, HD * 4);
  a.rope = (const float*)up_raw(d->rope, (size_t)d->rope_rows * HD * 4);
  a.hist = (const int32_t*)up_raw(d->hist, (size_t)B * 4);
  a.row_seq = (const int32_t*)up_raw(d->row_seq, (size_t)rows * 4);
  a.row_t = (const int32_t*)up_raw(d->row_t, (size_t)rows * 4);
  std::vector<UttPlan> plan(B);
  std::memset(plan.data(), 0, plan.size() * sizeof(UttPlan));
  for (int b = 0; b < B; ++b) { plan[b].T = d->T[b]; plan[b].n_lfr = d->T[b]; plan[b].row_off = d->row_off[b]; }
  a.plan = (const UttPlan*)up_raw(plan.data(), plan.size() * sizeof(UttPlan));
  const std::vector<T> nan_rows(Md * H * HD, elem_nan<T>());
  T* dq = up_t(nan_rows);
  T* dctx = up_t(nan_rows);
  a.q = dq; a.ctx = dctx; a.S = d->S_max;
  // ---- bf16 prefill: the MFMA form's inputs, as QwSession::prefill_impl makes them
  T* dkrows = nullptr;
  d->qt = d->nw = 0;
  if (a.bf16 && !a.step) {
    int qt = 0, nw = 4, n_qb = 0;
    attention_geometry(max_len, HD, &qt, &nw);
    const int dq_rows = 16 * qt * nw;
    std::vector<int32_t> qb_utt, qb_q0;
    for (int b = 0; b < B; ++b)
      for (int q0 = 0; q0 < d->T[b]; q0 += dq_rows) { qb_utt.push_back(b); qb_q0.push_back(q0); ++n_qb; }
    a.qb_utt = (const int32_t*)up_raw(qb_utt.data(), qb_utt.size() * 4);
    a.qb_q0 = (const int32_t*)up_raw(qb_q0.data(), qb_q0.size() * 4);
    a.n_qb = a.no_fuse ? 0 : n_qb; a.qt = qt; a.nw = nw; a.max_T = max_len; a.ld_vt = (int)Md;
    d->qt = qt; d->nw = nw;
    dkrows = up_t(std::vector<T>(Md * KV * HD, elem_nan<T>()));
    a.k_rows = dkrows;
    std::vector<T> vt((size_t)KV * HD * Md, elem_from_f32<T>(0.0f));          // V^T of the q|k|v rows; gap rows are zero rows of the GEMM's input
    for (int r = 0; r < rows; ++r)
      if (d->row_seq[r] >= 0)
        for (int c = 0; c < KV * HD; ++c) vt[(size_t)c * Md + r] = elem_from_f32<T>(d->qkv[(size_t)r * heads * HD + (H + KV) * HD + c]);
    a.vt = up_t(vt);
  }
  // ---- the session's own cache (beam: the utterances' prompt cache): host image, NaN wherever no cached row was placed
  const size_t page_stride = (size_t)LAYERS * KV * 16 * HD;
  const size_t own_n = d->paged ? (size_t)d->n_pages * page_stride : (size_t)n_seq * KV * d->S_max * HD;
  auto own_off = [&](int b, int kvh, int s) -> size_t {
    if (d->paged) return (size_t)d->table[(size_t)b * d->pps + (s >> 4)] * page_stride + (size_t)LAYER * KV * 16 * HD + ((size_t)kvh * 16 + (s & 15)) * HD;
    return (((size_t)b * KV + kvh) * d->S_max + s) * HD;
  };
  std::vector<T> hk(own_n, elem_nan<T>()), hv(own_n, elem_nan<T>());
  std::vector<unsigned char> may_k(own_n, 0);             // elements the call is entitled to write (same set for K and V)
  for (int b = 0; b < n_seq; ++b) {
    const int have = beam ? d->p0[b * d->beam] : d->hist[b];
    ASR_REQUIRE(have == 0 || (d->k_hist && d->v_hist && have <= d->hist_ld), "probe_qwen_attention: sequence %d has %d cached positions, hist_ld %d", b, have, d->hist_ld);
    for (int kvh = 0; kvh < KV; ++kvh) {
      for (int s = 0; s < have; ++s)
        for (int e = 0; e < HD; ++e) {
          const size_t src = (((size_t)b * KV + kvh) * d->hist_ld + s) * HD + e;
          hk[own_off(b, kvh, s) + e] = elem_from_f32<T>(d->k_hist[src]);
          hv[own_off(b, kvh, s) + e] = elem_from_f32<T>(d->v_hist[src]);
        }
      if (!beam)
        for (int s = have; s < have + d->T[b]; ++s)
          for (int e = 0; e < HD; ++e) may_k[own_off(b, kvh, s) + e] = 1;
    }
  }
  T* dk = up_t(hk);
  T* dv = up_t(hv);
  KvAddr own{nullptr, 0, 0, d->S_max};
  if (d->paged) own = KvAddr{(const int32_t*)up_raw(d->table, (size_t)n_seq * d->pps * 4), d->pps, page_stride, d->S_max};
  const size_t layer_off = d->paged ? (size_t)LAYER * KV * 16 * HD : 0;
  // ---- beam search: hypothesis extents [B][KV][S_hyp][128], uploaded as given
  const size_t ext_n = beam ? (size_t)B * KV * d->S_hyp * HD : 0;
  std::vector<T> ek(ext_n), ev(ext_n);
  T *dek = nullptr, *dev = nullptr;
  if (beam) {
    for (size_t i = 0; i < ext_n; ++i) { ek[i] = elem_from_f32<T>(d->ext_k[i]); ev[i] = elem_from_f32<T>(d->ext_v[i]); }
    dek = up_t(ek); dev = up_t(ev);
    a.kc = dek; a.vc = dev; a.ka = KvAddr{nullptr, 0, 0, d->S_hyp};
    a.kc_p = dk + layer_off; a.vc_p = dv + layer_off; a.kap = own;
    a.beam_src = (const int32_t*)up_raw(d->src, (size_t)B * d->ld_src * 4); a.ld_src = d->ld_src; a.beam = d->beam;
    a.beam_p0 = (const int32_t*)up_raw(d->p0, (size_t)B * 4);
  } else {
    a.kc = dk + layer_off; a.vc = dv + layer_off; a.ka = own;
  }
  Profiler prof;                                          // (disabled: a ProfScope over it does nothing)
  const char* form = launch_qwen_attention<T>(a, prof, nullptr);
  HIP_CHECK(hipGetLastError());
  snprintf(d->kernel, sizeof(d->kernel), "%s", form);
  HIP_CHECK(hipDeviceSynchronize());
  // ---- results
  auto down = [&](const T* dev_p, size_t count, float* out) {
    std::vector<T> h(count);
    HIP_CHECK(hipMemcpy(h.data(), dev_p, count * sizeof(T), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < count; ++i) out[i] = elem_to_f32(h[i]);
  };
  down(dctx, (size_t)rows * H * HD, d->ctx);
  if (d->q_out) down(dq, (size_t)rows * H * HD, d->q_out);
  if (d->k_rows_out) {
    if (dkrows) down(dkrows, (size_t)rows * KV * HD, d->k_rows_out);
    else for (size_t i = 0; i < (size_t)rows * KV * HD; ++i) d->k_rows_out[i] = std::nanf("");
  }
  int64_t stray = 0;
  std::vector<T> ak(own_n), av(own_n);
  HIP_CHECK(hipMemcpy(ak.data(), dk, own_n * sizeof(T), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(av.data(), dv, own_n * sizeof(T), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < own_n; ++i)
    if (!may_k[i]) stray += (same_bits(hk[i], ak[i]) ? 0 : 1) + (same_bits(hv[i], av[i]) ? 0 : 1);
  if (!beam && d->k_after && d->v_after)
    for (int b = 0; b < B; ++b)
      for (int kvh = 0; kvh < KV; ++kvh)
        for (int s = 0; s < d->hist[b] + d->T[b] && s < d->after_ld; ++s)
          for (int e = 0; e < HD; ++e) {
            const size_t o = (((size_t)b * KV + kvh) * d->after_ld + s) * HD + e;
            d->k_after[o] = elem_to_f32(ak[own_off(b, kvh, s) + e]);
            d->v_after[o] = elem_to_f32(av[own_off(b, kvh, s) + e]);
          }
  if (beam) {
    std::vector<T> bk(ext_n), bv(ext_n);
    HIP_CHECK(hipMemcpy(bk.data(), dek, ext_n * sizeof(T), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(bv.data(), dev, ext_n * sizeof(T), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < ext_n; ++i) {
      const int b = (int)(i / ((size_t)KV * d->S_hyp * HD)), slot = (int)((i / HD) % d->S_hyp);
      if (slot != d->hist[b] - d->p0[b]) stray += (same_bits(ek[i], bk[i]) ? 0 : 1) + (same_bits(ev[i], bv[i]) ? 0 : 1);
      d->ext_k[i] = elem_to_f32(bk[i]); d->ext_v[i] = elem_to_f32(bv[i]);
    }
  }
  d->stray = (int32_t)std::min<int64_t>(stray, 0x7fffffff);
}
}  // namespace

extern "C" int asr_probe_qwen_attention(asr_probe_qwen_attn_desc* d) {
  return asr_guard([&] {
    ASR_REQUIRE(d, "probe_qwen_attention: null descriptor");
    asr_require_device(0);
    if (d->bf16) probe_qwen_attention<bf16_t>(d);
    else probe_qwen_attention<float>(d);
  });
}

// ---- grid-barrier latency probe (tuning hook): a cooperative launch of one workgroup per CU crossing `iters` barriers.
namespace {
__device__ __forceinline__ bool grid_barrier_probe_step(unsigned int* counter, unsigned int target) {
  __syncthreads();
  bool ok = true;
  if (threadIdx.x == 0) {
    __threadfence();
    atomicAdd(counter, 1u);
    int spins = 0;
    while (__hip_atomic_load(counter, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < target) {
      __builtin_amdgcn_s_sleep(1);
      if (++spins > (1 << 22)) { ok = false; break; }       // never hang the box: give up after ~1 s
    }
    __threadfence();
  }
  __syncthreads();
  return ok;
}
__global__ __launch_bounds__(512) void grid_barrier_probe_kernel(unsigned int* counter, int iters, float* sink, int* failed) {
  float acc = 0.0f;
  for (int it = 0; it < iters; ++it) {
    acc += sink[(blockIdx.x * 64 + (it & 63)) & 4095];          // a little cross-workgroup traffic between barriers
    if (threadIdx.x == 0) sink[(blockIdx.x * 64 + ((it + 1) & 63)) & 4095] = acc * 0.5f;
    if (!grid_barrier_probe_step(counter, (unsigned int)(it + 1) * gridDim.x)) { if (threadIdx.x == 0) *failed = 1; return; }
  }
  if (acc == 123.456f) sink[0] = acc;
}
}  // namespace

namespace {
// hierarchical barrier probe: arrivals are counted per XCD (workgroup b runs on XCD b % 8), the last arrival of an XCD counts
// itself on the chip counter, the last XCD publishes the generation. Relaxed agent-scope atomics only -- no fence, i.e. no L2
// write-back / invalidate; payload that must cross XCDs would travel through sc1 accesses.
struct HBar { unsigned int* xcd; unsigned int* chip; unsigned int* flag; };   // xcd[8 * 32], flag[8 * 32] (128-byte spacing)
__device__ __forceinline__ bool hbar_step(const HBar& hb, unsigned int gen, int mode) {
  __syncthreads();
  bool ok = true;
  if (threadIdx.x == 0) {
    const int x = blockIdx.x & 7;
    const unsigned int in_xcd = (gridDim.x + 7 - x) >> 3;
    const unsigned int old = __hip_atomic_fetch_add(hb.xcd + x * 32, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old + 1 == gen * in_xcd) {
      const unsigned int n_xcd = gridDim.x < 8 ? gridDim.x : 8;
      const unsigned int o2 = __hip_atomic_fetch_add(hb.chip, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (o2 + 1 == gen * n_xcd) {
        if (mode == 2) { for (int q = 0; q < 8; ++q) __hip_atomic_store(hb.flag + q * 32, gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
        else __hip_atomic_store(hb.flag, gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    const unsigned int* f = mode == 2 ? hb.flag + x * 32 : hb.flag;
    int spins = 0;
    while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < gen) {
      __builtin_amdgcn_s_sleep(1);
      if (++spins > (1 << 22)) { ok = false; break; }
    }
  }
  __syncthreads();
  return ok;
}
__global__ __launch_bounds__(512) void hbar_probe_kernel(HBar hb, int iters, int mode, float* sink, int* failed, const unsigned long long* bulk,
                                                         int bulk_words, int bulk_sc1) {
  float acc = 0.0f;
  for (int it = 0; it < iters; ++it) {
    // bulk activation read every workgroup does per phase: `bulk_words` 8-byte words of ONE shared buffer, through sc1 (relaxed
    // agent-scope atomic loads: what a persistent kernel must use for data produced by other XCDs) or through plain cached loads
    unsigned long long bsum = 0;
    if (bulk_sc1) { for (int w = threadIdx.x; w < bulk_words; w += 512) bsum += __hip_atomic_load(bulk + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    else { for (int w = threadIdx.x; w < bulk_words; w += 512) bsum += bulk[w]; }
    if (bsum == 0x123456789abcdefull) acc += 1.0f;
    // payload through sc1 accesses: one value written by this workgroup, one read from the neighbour's slot of the previous round
    const float v = __hip_atomic_load(sink + ((blockIdx.x + 1) % gridDim.x) * 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (it > 0 && v != (float)it) { if (threadIdx.x == 0) *failed = 2; }      // stale payload => visibility bug
    acc += v;
    if (!hbar_step(hb, 2u * it + 1u, mode)) { if (threadIdx.x == 0) *failed = 1; return; }
    if (threadIdx.x == 0) __hip_atomic_store(sink + blockIdx.x * 32, (float)(it + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (!hbar_step(hb, 2u * it + 2u, mode)) { if (threadIdx.x == 0) *failed = 1; return; }
  }
  if (acc == 123.456f) sink[0] = acc;
}
}  // namespace

extern "C" int asr_probe_grid_barrier2(int n_workgroups, int iters, int mode, float* us_per_barrier) {
  return asr_guard([&] {
    // mode = (1 | 2) + 16 * bulk KiB read per workgroup per round + 8 if that read goes through plain cached loads instead of sc1
    int bulk_kib = mode >> 4, bulk_sc1 = (mode & 8) ? 0 : 1;
    mode &= 7;
    ASR_REQUIRE(us_per_barrier && iters > 0 && n_workgroups > 0 && n_workgroups <= 1024 && (mode == 1 || mode == 2) && bulk_kib <= 1024, "probe_grid_barrier2: bad argument");
    asr_require_device(0);
    Tmp t;
    unsigned int* ctr = (unsigned int*)t.alloc(3 * 8 * 32 * 4);
    float* sink = (float*)t.alloc(1024 * 32 * 4);
    int* failed = (int*)t.alloc(256);
    HIP_CHECK(hipMemset(ctr, 0, 3 * 8 * 32 * 4));
    HIP_CHECK(hipMemset(sink, 0, 1024 * 32 * 4));
    HIP_CHECK(hipMemset(failed, 0, 256));
    HBar hb{ctr, ctr + 8 * 32, ctr + 2 * 8 * 32};
    const unsigned long long* bulk = (const unsigned long long*)t.alloc((size_t)std::max(bulk_kib, 1) * 1024);
    HIP_CHECK(hipMemset((void*)bulk, 1, (size_t)std::max(bulk_kib, 1) * 1024));
    int bulk_words = bulk_kib * 128;
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    void* args[] = {&hb, &iters, &mode, &sink, &failed, &bulk, &bulk_words, &bulk_sc1};
    HIP_CHECK(hipEventRecord(e0, nullptr));
    HIP_CHECK(hipLaunchCooperativeKernel(reinterpret_cast<const void*>(hbar_probe_kernel), dim3(n_workgroups), dim3(512), args, 0, nullptr));
    HIP_CHECK(hipEventRecord(e1, nullptr));
    HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    int hf = 0;
    HIP_CHECK(hipMemcpy(&hf, failed, 4, hipMemcpyDeviceToHost));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    ASR_REQUIRE(hf != 1, "probe_grid_barrier2: a workgroup gave up waiting (grid not co-resident?)");
    ASR_REQUIRE(hf != 2, "probe_grid_barrier2: a payload written before the barrier was not visible after it");
    *us_per_barrier = ms * 1e3f / (2.0f * iters);
  });
}

extern "C" int asr_probe_grid_barrier(int n_workgroups, int iters, float* us_per_barrier) {
  return asr_guard([&] {
    ASR_REQUIRE(us_per_barrier && iters > 0 && n_workgroups > 0, "probe_grid_barrier: bad argument");
    asr_require_device(0);
    Tmp t;
    unsigned int* counter = (unsigned int*)t.alloc(256);
    float* sink = (float*)t.alloc(4096 * 4);
    int* failed = (int*)t.alloc(256);
    HIP_CHECK(hipMemset(counter, 0, 256));
    HIP_CHECK(hipMemset(sink, 0, 4096 * 4));
    HIP_CHECK(hipMemset(failed, 0, 256));
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    void* args[] = {&counter, &iters, &sink, &failed};
    HIP_CHECK(hipEventRecord(e0, nullptr));
    HIP_CHECK(hipLaunchCooperativeKernel(reinterpret_cast<const void*>(grid_barrier_probe_kernel), dim3(n_workgroups), dim3(512), args, 0, nullptr));
    HIP_CHECK(hipEventRecord(e1, nullptr));
    HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    int hf = 0;
    HIP_CHECK(hipMemcpy(&hf, failed, 4, hipMemcpyDeviceToHost));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    ASR_REQUIRE(!hf, "probe_grid_barrier: a workgroup gave up waiting (grid not co-resident?)");
    *us_per_barrier = ms * 1e3f / iters;
  });
}

// ---- hotword boosting of the autoregressive decoders (kernels.h: launch_hotword_*; asr_mi355x_probe.h)
namespace {
struct ProbeTrie {
  HotTrie view;
  int n_nodes = 0, n_root = 0;
  // phrases -> the product's trie image on the device (build_hot_trie + hot_trie_view, as TokenHead::set_hotwords does); ids are checked against n_valid first
  ProbeTrie(Tmp& t, const int32_t* ids, const int32_t* offsets, int n_phrases, float boost, int n_valid, const char* who, bool optional = false) {
    if (optional && n_phrases == 0) return;                // (the LM hooks: no phrases, no trie -- the view stays empty)
    ASR_REQUIRE(n_phrases >= 1 && ids && offsets && offsets[0] >= 0 && std::isfinite(boost), "%s: hotword phrases missing", who);
    for (int p = 0; p < n_phrases; ++p) {
      ASR_REQUIRE(offsets[p + 1] > offsets[p], "%s: phrase %d is empty", who, p);
      for (int32_t i = offsets[p]; i < offsets[p + 1]; ++i) ASR_REQUIRE(ids[i] >= 0 && ids[i] < n_valid, "%s: phrase %d holds token %d (vocabulary %d)", who, p, ids[i], n_valid);
    }
    const std::vector<int32_t> words = build_hot_trie(ids, offsets, n_phrases, &n_nodes);
    int32_t* dw = (int32_t*)t.alloc(words.size() * 4);
    HIP_CHECK(hipMemcpy(dw, words.data(), words.size() * 4, hipMemcpyHostToDevice));
    view = hot_trie_view(dw, n_nodes, boost);
    n_root = words[(size_t)2 * n_nodes + 1];
  }
};

// the model of the LM hooks on the device: checked as TokenHead::set_lm checks it, uploaded, viewed
struct ProbeLm {
  LmView view;
  ProbeLm(Tmp& t, const asr_probe_lm_model* m, int vocab, const char* who) {
    ASR_REQUIRE(m && m->image && m->n_words > 0 && m->topk >= 1 && m->topk <= LM_TOPK_MAX && m->n_end >= 0 && m->n_end <= LM_ENDS_MAX && (m->n_end == 0 || m->end_ids),
                "%s: bad model descriptor", who);
    for (int i = 0; i < m->n_end; ++i) ASR_REQUIRE(m->end_ids[i] >= 0 && m->end_ids[i] < vocab, "%s: end id %d outside the vocabulary of %d", who, m->end_ids[i], vocab);
    ngram_lm_validate(m->image, m->n_words, vocab, -1, m->alpha, m->beta, m->oov_logprob, who);
    int32_t* dw = (int32_t*)t.alloc((size_t)m->n_words * 4);
    HIP_CHECK(hipMemcpy(dw, m->image, (size_t)m->n_words * 4, hipMemcpyHostToDevice));
    view.lm = ngram_lm_view(dw, m->image, m->alpha, m->beta, m->oov_logprob);
    view.topk = m->topk; view.ends.n = m->n_end;
    for (int i = 0; i < m->n_end; ++i) view.ends.id[i] = m->end_ids[i];
  }
};
}  // namespace

extern "C" int asr_probe_hotword(asr_probe_hotword_desc* d) {
  return asr_guard([&] {
    const char* who = "probe_hotword";
    ASR_REQUIRE(d && d->op >= 0 && d->op <= 2 && d->rows > 0 && d->node, "%s: bad descriptor", who);
    ASR_REQUIRE(d->op == 1 || (d->logits && d->n_valid >= 1 && d->ld >= d->n_valid && d->ld % 128 == 0), "%s: logits missing", who);
    asr_require_device(0);
    Tmp t;
    const int rows = d->rows;
    ProbeTrie tr(t, d->ids, d->offsets, d->n_phrases, d->boost, d->op == 1 ? INT32_MAX : d->n_valid, who);
    for (int r = 0; r < rows; ++r) ASR_REQUIRE(d->node[r] >= 0 && d->node[r] < tr.n_nodes, "%s: node %d of row %d outside the trie of %d", who, d->node[r], r, tr.n_nodes);
    auto up = [&](const void* h, size_t bytes) -> void* {
      void* p = t.alloc(std::max(bytes, (size_t)4));
      HIP_CHECK(hipMemcpy(p, h, bytes, hipMemcpyHostToDevice));
      return p;
    };
    int32_t* dnode = (int32_t*)up(d->node, (size_t)rows * 4);
    const int32_t* dn = (const int32_t*)up(&d->n_saved, 4);
    const size_t lbytes = d->op == 1 ? 0 : (size_t)rows * d->ld * 4;
    float* dlog = lbytes ? (float*)up(d->logits, lbytes) : nullptr;
    if (d->op == 0) {
      float* dsave = nullptr;
      if (d->root_save) { ASR_REQUIRE(d->n_root == tr.n_root, "%s: root_save is %d wide, the root has %d children", who, d->n_root, tr.n_root); dsave = (float*)up(d->root_save, (size_t)rows * d->n_root * 4); }
      launch_hotword_bias(dlog, d->ld, rows, d->n_valid, tr.view, dnode, dn, dsave, nullptr);
      HIP_CHECK(hipDeviceSynchronize());
      HIP_CHECK(hipMemcpy(d->logits, dlog, lbytes, hipMemcpyDeviceToHost));
      if (dsave) HIP_CHECK(hipMemcpy(d->root_save, dsave, (size_t)rows * d->n_root * 4, hipMemcpyDeviceToHost));
    } else if (d->op == 1) {
      ASR_REQUIRE(d->next_in, "%s: advance without picks", who);
      launch_hotword_advance((const int32_t*)up(d->next_in, (size_t)rows * 4), rows, tr.view, dnode, dn, nullptr);
      HIP_CHECK(hipDeviceSynchronize());
      HIP_CHECK(hipMemcpy(d->node, dnode, (size_t)rows * 4, hipMemcpyDeviceToHost));
    } else {
      ASR_REQUIRE(d->K >= 1 && d->K <= BEAM_MAX && d->topv && d->topi, "%s: rerank K %d", who, d->K);
      const float* dvec = d->vec ? (const float*)up(d->vec, (size_t)d->ld * 4) : nullptr;
      const size_t kb = (size_t)rows * d->K * 4;
      float* dv = (float*)t.alloc(kb); int32_t* di = (int32_t*)t.alloc(kb); float* dl = (float*)t.alloc((size_t)rows * 4);
      launch_beam_topk(dlog, d->ld, rows, d->n_valid, dvec, d->K, dv, di, nullptr, dl);
      launch_hotword_rerank(dlog, d->ld, rows, d->n_valid, dvec, dl, tr.view, dnode, 1, d->K, dv, di, nullptr);
      HIP_CHECK(hipDeviceSynchronize());
      HIP_CHECK(hipMemcpy(d->topv, dv, kb, hipMemcpyDeviceToHost));
      HIP_CHECK(hipMemcpy(d->topi, di, kb, hipMemcpyDeviceToHost));
      if (d->lse) HIP_CHECK(hipMemcpy(d->lse, dl, (size_t)rows * 4, hipMemcpyDeviceToHost));
    }
  });
}

// the body of asr_probe_hotword_head_steps; with a model (asr_probe_lm_head_steps) it is set after the hotwords and `states` gets the state table per step
static int probe_head_steps(asr_probe_hotword_head_desc* d, const asr_probe_lm_model* m, int32_t* states, const char* who) {
  return asr_guard([&] {
    ASR_REQUIRE(!m || states, "%s: the state table is missing", who);
    ASR_REQUIRE(d && d->rows > 0 && d->steps >= 1 && d->n_valid >= 1 && d->ld >= d->n_valid && d->ld % 128 == 0 && d->logits && d->picks && d->save_ids && d->nodes,
                "%s: bad descriptor", who);
    ASR_REQUIRE(d->ld_save >= d->steps && d->ld_save <= 1024 && d->range >= 1 && d->range <= d->ld_save, "%s: %d steps / range %d and a history table of %d", who, d->steps,
                d->range, d->ld_save);
    ASR_REQUIRE(!d->scores || d->logprob, "%s: scores without the logprob table", who);
    ASR_REQUIRE(!d->sampling || (d->K >= 1 && d->K <= d->n_valid), "%s: sampler top_k %d", who, d->K);
    ASR_REQUIRE(!d->noise || d->sampling, "%s: noise without the sampler", who);
    ASR_REQUIRE(!d->timed || (d->value == 1.0f && !d->sampling && !d->timestamps), "%s: timed steps need the arg-max head", who);
    asr_require_device(0);
    Tmp t;
    const int rows = d->rows, ld = d->ld, steps = d->steps;
    const size_t lbytes = (size_t)rows * ld * 4;
    // timed: logits holds ONE step's rows, uploaded once and reused by every step (the bias accumulates in them: a timing, not a result), and the launches
    // run back to back between two events; else one row buffer, uploaded before every step
    float* dlog = (float*)t.alloc(lbytes);
    if (d->timed) HIP_CHECK(hipMemcpy(dlog, d->logits, lbytes, hipMemcpyHostToDevice));
    int32_t* dpick = (int32_t*)t.alloc((size_t)steps * rows * 4);
    int32_t* dnodes = (int32_t*)t.alloc((size_t)steps * rows * 4);
    float* dvec = nullptr;
    if (d->vec) { dvec = (float*)t.alloc((size_t)ld * 4); HIP_CHECK(hipMemcpy(dvec, d->vec, (size_t)ld * 4, hipMemcpyHostToDevice)); }
    TokenHead h;
    h.init(d->ld_save, d->partial, d->range, 1024);
    h.set_penalty(d->value, d->range, who);
    if (d->sampling) h.set_sampling(true, d->temperature, d->K, d->top_p, d->repetition_penalty, d->seed, who);
    if (d->timestamps) h.set_timestamps(true, d->ts_begin, d->no_timestamps_id, d->eot_id, d->max_initial, d->n_valid, who);
    h.set_scores(d->scores != 0);
    h.set_hotwords(d->ids, d->offsets, d->n_phrases, d->boost, d->n_valid, nullptr, who);
    if (m) {
      ASR_REQUIRE(m->image && m->n_words > 0, "%s: the model's image is missing", who);
      h.set_lm(m->image, m->n_words, m->alpha, m->beta, m->oov_logprob, m->topk, m->end_ids, m->n_end, d->n_valid, nullptr, who);
    }
    int32_t* dstates = m ? (int32_t*)t.alloc((size_t)steps * rows * 4) : nullptr;
    h.reserve(rows, nullptr);
    h.restart(nullptr);
    if (d->scores) HIP_CHECK(hipMemset(h.d_scores.ptr, 0xFF, (size_t)rows * d->ld_save * 4));
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (d->timed) { HIP_CHECK(hipEventCreate(&ev[0])); HIP_CHECK(hipEventCreate(&ev[1])); HIP_CHECK(hipEventRecord(ev[0], nullptr)); }
    d->head_ms = 0.0f;
    for (int i = 0; i < steps; ++i) {
      float* row = dlog;
      if (!d->timed) HIP_CHECK(hipMemcpy(row, d->logits + (size_t)i * rows * ld, lbytes, hipMemcpyHostToDevice));
      if (d->noise) h.arm_noise(d->noise + (size_t)i * rows * d->K, rows * d->K, nullptr);
      h.enqueue(row, ld, rows, d->n_valid, i == 0 ? dvec : nullptr, i > 0, dpick + (size_t)i * rows, nullptr);
      h.consumed();
      if (h.hot() && !d->timed) HIP_CHECK(hipMemcpyAsync(dnodes + (size_t)i * rows, h.d_node.ptr, (size_t)rows * 4, hipMemcpyDeviceToDevice, nullptr));
      if (m && !d->timed) HIP_CHECK(hipMemcpyAsync(dstates + (size_t)i * rows, h.d_lmstate.ptr, (size_t)rows * 4, hipMemcpyDeviceToDevice, nullptr));
      if (d->logits_out && !d->timed) {
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(d->logits_out + (size_t)i * rows * ld, row, lbytes, hipMemcpyDeviceToHost));
      }
    }
    if (d->timed) HIP_CHECK(hipEventRecord(ev[1], nullptr));
    HIP_CHECK(hipDeviceSynchronize());
    if (d->timed) {
      HIP_CHECK(hipEventElapsedTime(&d->head_ms, ev[0], ev[1]));
      HIP_CHECK(hipEventDestroy(ev[0])); HIP_CHECK(hipEventDestroy(ev[1]));
    }
    HIP_CHECK(hipMemcpy(d->picks, dpick, (size_t)steps * rows * 4, hipMemcpyDeviceToHost));
    if (h.hot() && !d->timed) HIP_CHECK(hipMemcpy(d->nodes, dnodes, (size_t)steps * rows * 4, hipMemcpyDeviceToHost));
    if (m && !d->timed) HIP_CHECK(hipMemcpy(states, dstates, (size_t)steps * rows * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d->save_ids, h.d_save.ptr, (size_t)rows * d->ld_save * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(&d->n_saved_after, h.d_nsaved.ptr, 4, hipMemcpyDeviceToHost));
    if (d->scores) HIP_CHECK(hipMemcpy(d->logprob, h.d_scores.ptr, (size_t)rows * d->ld_save * 4, hipMemcpyDeviceToHost));
  });
}

extern "C" int asr_probe_hotword_head_steps(asr_probe_hotword_head_desc* d) { return probe_head_steps(d, nullptr, nullptr, "probe_hotword_head_steps"); }
extern "C" int asr_probe_lm_head_steps(const asr_probe_lm_model* m, asr_probe_hotword_head_desc* d, int32_t* states) {
  if (!m) return asr_guard([&] { ASR_REQUIRE(false, "probe_lm_head_steps: the model is missing"); });
  return probe_head_steps(d, m, states, "probe_lm_head_steps");
}

// the body of asr_probe_hotword_rank; with a model (asr_probe_lm_rank) the pass is BeamRanker's with the LM on and the trie is optional
static int probe_rank(asr_probe_hotword_rank_desc* d, const asr_probe_lm_model* m, const int32_t* state_in, int32_t* state_out, const char* who) {
  return asr_guard([&] {
    ASR_REQUIRE(d && d->n_utt > 0 && d->beam >= 1 && d->beam <= BEAM_MAX && d->beam * d->beam <= 64 && d->tab_ld > 0 && d->n_slots >= 0 && d->n_slots <= d->tab_ld &&
                d->n_stop >= 0 && (d->n_stop == 0 || d->stop) && d->logits && d->n_valid >= d->beam && d->ld >= d->n_valid && d->ld % 128 == 0 && d->cum && d->fin && d->len &&
                d->next && d->done && d->src_in && d->tok_in && d->src_out && d->tok_out && d->node_in && d->node_out && d->topv && d->topi, "%s: bad descriptor", who);
    ASR_REQUIRE(!m || (state_out && (d->first || state_in)), "%s: the state tables are missing", who);
    asr_require_device(0);
    Tmp t;
    const int N = d->n_utt * d->beam, R = d->first ? d->n_utt : N, K = d->beam;
    ProbeTrie tr(t, d->ids, d->offsets, d->n_phrases, d->boost, d->n_valid, who, m != nullptr);
    const bool hot = tr.view.n_nodes > 1;
    for (int r = 0; r < N; ++r) {
      ASR_REQUIRE(d->len[r] >= 0 && d->len[r] <= d->tab_ld, "%s: row %d length %d outside the table", who, r, d->len[r]);
      ASR_REQUIRE(!hot || (d->node_in[r] >= 0 && d->node_in[r] < tr.n_nodes), "%s: node %d of row %d outside the trie", who, d->node_in[r], r);
    }
    auto up = [&](const void* h, size_t bytes) -> void* {
      void* p = t.alloc(std::max(bytes, (size_t)4));
      HIP_CHECK(hipMemcpy(p, h, bytes, hipMemcpyHostToDevice));
      return p;
    };
    const size_t tab = (size_t)N * d->tab_ld * 4, rows4 = (size_t)N * 4, kb = (size_t)R * K * 4;
    float* dlog = (float*)up(d->logits, (size_t)R * d->ld * 4);
    const float* dvec = d->vec ? (const float*)up(d->vec, (size_t)d->ld * 4) : nullptr;
    float* dv = (float*)t.alloc(kb); int32_t* di = (int32_t*)t.alloc(kb); float* dl = (float*)t.alloc((size_t)R * 4);
    BeamArgs a{};
    a.beam = d->beam; a.K = K; a.ld = d->tab_ld; a.first = d->first; a.n_slots = d->n_slots;
    a.topv = dv; a.topi = di;
    a.cum = (float*)up(d->cum, rows4); a.fin = (int32_t*)up(d->fin, rows4); a.len = (int32_t*)up(d->len, rows4); a.next = (int32_t*)up(d->next, rows4);
    a.done = (int32_t*)up(d->done, (size_t)d->n_utt * 4);
    a.stop = d->n_stop ? (const int32_t*)up(d->stop, (size_t)d->n_stop * 4) : nullptr; a.n_stop = d->n_stop;
    a.src_in = (const int32_t*)up(d->src_in, tab); a.tok_in = (const int32_t*)up(d->tok_in, tab);
    a.src_out = (int32_t*)up(d->src_out, tab); a.tok_out = (int32_t*)up(d->tok_out, tab);
    const int32_t* dnode_in = (const int32_t*)up(d->node_in, rows4);
    int32_t* dnode_out = (int32_t*)up(d->node_out, rows4);
    if (hot) { a.node_in = dnode_in; a.node_out = dnode_out; a.trie = tr.view; }
    const int stride = d->first ? d->beam : 1;
    float* cv = nullptr; int32_t* ci = nullptr;
    LmView lmv;
    if (m) {
      ProbeLm pl(t, m, d->n_valid, who);
      lmv = pl.view;
      ASR_REQUIRE(lmv.topk >= K, "%s: the language model's topk %d is below the beam width %d", who, lmv.topk, K);
      for (int r = 0; r < N && !d->first; ++r) ASR_REQUIRE(state_in[r] >= 0 && state_in[r] < lmv.lm.n_nodes, "%s: state %d of row %d outside the image", who, state_in[r], r);
      cv = (float*)t.alloc((size_t)R * lmv.topk * 4); ci = (int32_t*)t.alloc((size_t)R * lmv.topk * 4);
      a.lm = lmv.lm; a.ends = lmv.ends;
      a.state_in = d->first ? nullptr : (const int32_t*)up(state_in, rows4);
      a.state_out = (int32_t*)up(state_out, rows4);
    }
    // the ranker's sequence (decode_head.h: BeamRanker::rank_first / enqueue_rank with hotwords on, or with a model)
    auto rank_lm = [&] {
      launch_lm_topk(dlog, d->ld, R, d->n_valid, dvec, lmv.topk, cv, ci, dl, nullptr);
      launch_lm_rerank(dlog, d->ld, R, d->n_valid, dvec, cv, ci, dl, lmv.topk, tr.view, hot ? a.node_in : nullptr, lmv.lm, lmv.ends, a.state_in, stride, K, dv, di, nullptr);
    };
    auto rank_plain = [&](bool with_lse) {
      launch_beam_topk(dlog, d->ld, R, d->n_valid, dvec, K, dv, di, nullptr, with_lse ? dl : nullptr);
      if (with_lse && hot) launch_hotword_rerank(dlog, d->ld, R, d->n_valid, dvec, dl, tr.view, a.node_in, stride, K, dv, di, nullptr);
    };
    if (m) rank_lm(); else rank_plain(true);
    launch_beam_select(a, d->n_utt, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(d->topv, dv, kb, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d->topi, di, kb, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d->cum, a.cum, rows4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d->fin, a.fin, rows4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d->len, a.len, rows4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d->next, a.next, rows4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d->done, a.done, (size_t)d->n_utt * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d->src_out, a.src_out, tab, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d->tok_out, a.tok_out, tab, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d->node_out, dnode_out, rows4, hipMemcpyDeviceToHost));
    if (m) HIP_CHECK(hipMemcpy(state_out, a.state_out, rows4, hipMemcpyDeviceToHost));
    d->ms_topk = d->ms_rerank = 0.0f;
    if (d->iters > 0) {                  // timing: beam_topk alone against beam_topk (lse_out) + re-rank, `iters` launches back to back (the pairs go to scratch)
      hipEvent_t ev[2];
      HIP_CHECK(hipEventCreate(&ev[0])); HIP_CHECK(hipEventCreate(&ev[1]));
      for (int mode = 0; mode < 2; ++mode) {
        HIP_CHECK(hipEventRecord(ev[0], nullptr));
        for (int i = 0; i < d->iters; ++i) {
          if (!m) rank_plain(mode != 0);                   // beam_topk alone against beam_topk (lse_out) + re-rank
          else if (mode) rank_lm();                        // with a model: the pass without it (the re-rank only with a trie) against lm_topk + lm_rerank
          else rank_plain(hot);
        }
        HIP_CHECK(hipEventRecord(ev[1], nullptr));
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipEventElapsedTime(mode ? &d->ms_rerank : &d->ms_topk, ev[0], ev[1]));
      }
      HIP_CHECK(hipEventDestroy(ev[0])); HIP_CHECK(hipEventDestroy(ev[1]));
    }
  });
}

extern "C" int asr_probe_hotword_rank(asr_probe_hotword_rank_desc* d) { return probe_rank(d, nullptr, nullptr, nullptr, "probe_hotword_rank"); }
extern "C" int asr_probe_lm_rank(const asr_probe_lm_model* m, asr_probe_hotword_rank_desc* d, const int32_t* state_in, int32_t* state_out) {
  if (!m) return asr_guard([&] { ASR_REQUIRE(false, "probe_lm_rank: the model is missing"); });
  return probe_rank(d, m, state_in, state_out, "probe_lm_rank");
}

extern "C" int asr_probe_lm_topk(asr_probe_lm_topk_desc* d) {
  return asr_guard([&] {
    const char* who = "probe_lm_topk";
    ASR_REQUIRE(d && d->rows > 0 && d->n_valid >= 1 && d->ld >= d->n_valid && d->ld % 128 == 0 && d->M >= 1 && d->M <= LM_TOPK_MAX && d->logits && d->cand_v && d->cand_i &&
                d->lse && d->iters >= 0, "%s: bad descriptor", who);
    asr_require_device(0);
    Tmp t;
    const int rows = d->rows, M = d->M;
    const size_t lbytes = (size_t)rows * d->ld * 4, cb = (size_t)rows * M * 4;
    float* dlog = (float*)t.alloc(lbytes);
    HIP_CHECK(hipMemcpy(dlog, d->logits, lbytes, hipMemcpyHostToDevice));
    float* dvec = nullptr;
    if (d->vec) { dvec = (float*)t.alloc((size_t)d->ld * 4); HIP_CHECK(hipMemcpy(dvec, d->vec, (size_t)d->ld * 4, hipMemcpyHostToDevice)); }
    float* cv = (float*)t.alloc(cb); int32_t* ci = (int32_t*)t.alloc(cb); float* dl = (float*)t.alloc((size_t)rows * 4);
    int32_t* slow = (int32_t*)t.alloc(256);
    HIP_CHECK(hipMemset(slow, 0, 4));
    launch_lm_topk(dlog, d->ld, rows, d->n_valid, dvec, M, cv, ci, dl, nullptr, slow);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(d->cand_v, cv, cb, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d->cand_i, ci, cb, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d->lse, dl, (size_t)rows * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(&d->slow_rows, slow, 4, hipMemcpyDeviceToHost));
    d->ms_lm_topk = d->ms_beam_topk = 0.0f;
    if (d->iters > 0) {
      const int K = std::min(M, (int)BEAM_MAX);
      float* dv = (float*)t.alloc((size_t)rows * K * 4); int32_t* di = (int32_t*)t.alloc((size_t)rows * K * 4);
      hipEvent_t ev[2];
      HIP_CHECK(hipEventCreate(&ev[0])); HIP_CHECK(hipEventCreate(&ev[1]));
      for (int mode = 0; mode < 2; ++mode) {
        HIP_CHECK(hipEventRecord(ev[0], nullptr));
        for (int i = 0; i < d->iters; ++i) {
          if (mode) launch_lm_topk(dlog, d->ld, rows, d->n_valid, dvec, M, cv, ci, dl, nullptr, nullptr);
          else launch_beam_topk(dlog, d->ld, rows, d->n_valid, dvec, K, dv, di, nullptr, dl);
        }
        HIP_CHECK(hipEventRecord(ev[1], nullptr));
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipEventElapsedTime(mode ? &d->ms_lm_topk : &d->ms_beam_topk, ev[0], ev[1]));
      }
      HIP_CHECK(hipEventDestroy(ev[0])); HIP_CHECK(hipEventDestroy(ev[1]));
    }
  });
}

extern "C" int asr_probe_lm_pick(const asr_probe_lm_model* m, asr_probe_lm_pick_desc* d) {
  return asr_guard([&] {
    const char* who = "probe_lm_pick";
    ASR_REQUIRE(m && d && d->rows > 0 && d->cand_v && d->cand_i && d->lse && d->state && d->next && (!d->logprob || d->ld_save >= 1) && d->n_saved >= 0, "%s: bad descriptor", who);
    ASR_REQUIRE(m->image && m->n_words >= NGRAM_LM_HEADER, "%s: the model's image is missing", who);
    asr_require_device(0);
    Tmp t;
    const int rows = d->rows, vocab = m->image[3];
    ProbeLm pl(t, m, vocab, who);
    const int M = pl.view.topk;
    for (int i = 0; i < rows * M; ++i) ASR_REQUIRE(d->cand_i[i] >= 0 && d->cand_i[i] < vocab, "%s: candidate id %d outside the image's vocabulary of %d", who, d->cand_i[i], vocab);
    for (int r = 0; r < rows; ++r) ASR_REQUIRE(d->state[r] >= 0 && d->state[r] < pl.view.lm.n_nodes, "%s: state %d of row %d outside the image", who, d->state[r], r);
    auto up = [&](const void* h, size_t bytes) -> void* {
      void* p = t.alloc(std::max(bytes, (size_t)4));
      HIP_CHECK(hipMemcpy(p, h, bytes, hipMemcpyHostToDevice));
      return p;
    };
    const size_t cb = (size_t)rows * M * 4, sb = (size_t)rows * std::max(d->ld_save, 1) * 4;
    int32_t* dstate = (int32_t*)up(d->state, (size_t)rows * 4);
    int32_t* dnext = (int32_t*)t.alloc((size_t)rows * 4);
    float* dlp = d->logprob ? (float*)up(d->logprob, sb) : nullptr;
    launch_lm_pick((const float*)up(d->cand_v, cb), (const int32_t*)up(d->cand_i, cb), (const float*)up(d->lse, (size_t)rows * 4), rows, M, pl.view.lm, pl.view.ends, dstate,
                   (const int32_t*)up(&d->n_saved, 4), dnext, dlp, d->ld_save, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(d->state, dstate, (size_t)rows * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d->next, dnext, (size_t)rows * 4, hipMemcpyDeviceToHost));
    if (dlp) HIP_CHECK(hipMemcpy(d->logprob, dlp, sb, hipMemcpyDeviceToHost));
  });
}

// =========================================================================================== encoder attention / FSMN on poisoned buffers
namespace {

// A logical buffer of n elements inside a larger allocation: `guard` elements in front of it and behind it, every element of the allocation `fill` before
// the rows are placed. A read that strays off the logical buffer then finds a finite number, not an unmapped page.
template <typename T>
struct Poisoned {
  std::vector<T> host;
  size_t guard = 0, n = 0;
  T* dev = nullptr;
  Poisoned(size_t n_, size_t guard_, float fill) : host(n_ + 2 * guard_, elem_from_f32<T>(fill)), guard(guard_), n(n_) {}
  T& at(size_t i) { return host[guard + i]; }
  T* upload(Tmp& t) {
    T* base = (T*)t.alloc(host.size() * sizeof(T));
    HIP_CHECK(hipMemcpy(base, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    dev = base + guard;
    return dev;
  }
  // after the launch: the logical buffer -> out; returns the guard elements whose bits changed
  int64_t download(std::vector<T>& out) {
    std::vector<T> all(host.size());
    HIP_CHECK(hipMemcpy(all.data(), dev - guard, all.size() * sizeof(T), hipMemcpyDeviceToHost));
    int64_t bad = 0;
    for (size_t i = 0; i < guard; ++i) bad += (same_bits(all[i], host[i]) ? 0 : 1) + (same_bits(all[guard + n + i], host[guard + n + i]) ? 0 : 1);
    out.assign(all.begin() + guard, all.begin() + guard + n);
    return bad;
  }
};

template <typename T>
void probe_encoder_attention(asr_probe_enc_attn_desc* d) {
  const int B = d->batch, H = d->n_heads, G = d->kv_group, HD = d->head_dim;
  const bool bf = sizeof(T) == 2, cross = d->q_lens != nullptr;
  ASR_REQUIRE(B > 0 && H > 0 && G >= 1 && H % G == 0 && d->key_lens && d->q && d->k && d->v && d->ctx, "probe_encoder_attention: bad argument");
  ASR_REQUIRE(HD == 64 || HD == 128, "probe_encoder_attention: head_dim %d (64 or 128)", HD);
  ASR_REQUIRE(bf || (G == 1 && !d->causal), "probe_encoder_attention: the f32 kernel has no causal / grouped-query form");
  ASR_REQUIRE(!d->packed_qk || (!cross && G == 1), "probe_encoder_attention: the packed q|k layout is the self form with one k head per q head");
  ASR_REQUIRE(d->slack_rows >= 0 && d->slack_rows % 8 == 0, "probe_encoder_attention: slack_rows %d (0 or a multiple of 8)", d->slack_rows);
  ASR_REQUIRE(std::isfinite(d->pad_fill_k) && std::isfinite(d->pad_fill_v), "probe_encoder_attention: the poison must be finite");
  const int KV = H / G, dq = H * HD, dk = KV * HD;
  std::vector<UttPlan> kp(B), qp(B);
  std::memset(kp.data(), 0, kp.size() * sizeof(UttPlan));
  std::memset(qp.data(), 0, qp.size() * sizeof(UttPlan));
  int max_T = 0, rows_k = 0, rows_q = 0;
  for (int b = 0; b < B; ++b) {
    const int Tk = d->key_lens[b], Tq = cross ? d->q_lens[b] : Tk;
    // (a session lays the query blocks of the cross form over the KEY rows -- csrc/sensevoice.hip, the Paraformer decoder -- so it has Tq <= T)
    ASR_REQUIRE(Tk >= 1 && Tq >= 1 && Tq <= Tk, "probe_encoder_attention: utterance %d has %d keys, %d queries", b, Tk, Tq);
    kp[b].T = kp[b].n_lfr = Tk; kp[b].row_off = rows_k;
    qp[b].T = qp[b].n_lfr = Tq; qp[b].row_off = rows_q;
    rows_k += round_up(Tk, 16); rows_q += round_up(Tq, 16);
    max_T = std::max(max_T, Tk);
  }
  int qt = 0, nw = 4, q_rows = 64;
  if (bf) { attention_geometry(max_T, HD, &qt, &nw); q_rows = 16 * qt * nw; }
  std::vector<int32_t> qb_utt, qb_q0;
  for (int b = 0; b < B; ++b)
    for (int q0 = 0; q0 < d->key_lens[b]; q0 += q_rows) { qb_utt.push_back(b); qb_q0.push_back(q0); }
  const int alloc_k = rows_k + d->slack_rows, alloc_q = rows_q + d->slack_rows;
  const int ld_k = d->packed_qk ? 2 * dq : dk, ld_q = d->packed_qk ? 2 * dq : dq;
  const size_t guard = (size_t)64 * 2 * dq;
  // ---- operands: poison everywhere, then the rows of the utterances
  Poisoned<T> hk((size_t)alloc_k * ld_k, guard, d->pad_fill_k), hv((size_t)dk * alloc_k, guard, d->pad_fill_v);
  Poisoned<T> hq(d->packed_qk ? 0 : (size_t)alloc_q * ld_q, guard, d->pad_fill_k), hc((size_t)alloc_q * dq, guard, d->pad_fill_v);
  Poisoned<T>& hq_in = d->packed_qk ? hk : hq;
  size_t rk = 0, rq = 0;
  for (int b = 0; b < B; ++b) {
    for (int t = 0; t < kp[b].T; ++t, ++rk) {
      const size_t row = (size_t)kp[b].row_off + t;
      for (int c = 0; c < dk; ++c) {
        hk.at(row * ld_k + (d->packed_qk ? dq : 0) + c) = elem_from_f32<T>(d->k[rk * dk + c]);
        hv.at((size_t)c * alloc_k + row) = elem_from_f32<T>(d->v[rk * dk + c]);
      }
    }
    for (int t = 0; t < qp[b].T; ++t, ++rq) {
      const size_t row = (size_t)qp[b].row_off + t;
      for (int c = 0; c < dq; ++c) hq_in.at(row * ld_q + c) = elem_from_f32<T>(d->q[rq * dq + c]);
    }
  }
  Tmp t;
  auto up_raw = [&](const void* h, size_t bytes) -> void* {
    void* p = t.alloc(bytes);
    HIP_CHECK(hipMemcpy(p, h, bytes, hipMemcpyHostToDevice));
    return p;
  };
  T* dkb = hk.upload(t);
  T* dqb = d->packed_qk ? dkb : hq.upload(t);
  AttnArgs aa;
  aa.q = dqb; aa.k = dkb + (d->packed_qk ? dq : 0); aa.ld_qk = ld_k;
  aa.ld_q = (cross || G > 1) ? ld_q : 0;                  // (the self form leaves ld_q to the launcher, as the sessions do)
  aa.vt = hv.upload(t); aa.ld_vt = alloc_k;
  aa.ctx = hc.upload(t); aa.ld_ctx = dq;
  aa.plan = (const UttPlan*)up_raw(kp.data(), kp.size() * sizeof(UttPlan));
  if (cross) aa.q_plan = (const UttPlan*)up_raw(qp.data(), qp.size() * sizeof(UttPlan));
  aa.qb_utt = (const int32_t*)up_raw(qb_utt.data(), qb_utt.size() * 4);
  aa.qb_q0 = (const int32_t*)up_raw(qb_q0.data(), qb_q0.size() * 4);
  aa.n_qblocks = (int)qb_utt.size(); aa.n_heads = H; aa.qt = qt; aa.n_waves = nw; aa.max_T = max_T;
  aa.causal = d->causal ? 1 : 0; aa.kv_group = G;
  d->n_qblocks = aa.n_qblocks;
  d->hd = d->chunk = d->qt = d->waves = d->grid_z = 0;
  if (!bf) launch_attention_f32(aa, HD, nullptr);
  else if (HD == 128) launch_attention_bf16_hd128(aa, nullptr);
  else launch_attention_bf16_hd64(aa, nullptr);
  const AttnLaunchInfo ran = attention_last_launch();
  d->hd = ran.hd; d->chunk = ran.chunk; d->qt = ran.qt; d->waves = ran.waves; d->grid_z = ran.grid_z;
  HIP_CHECK(hipDeviceSynchronize());
  // ---- results: the query rows; stray = context elements outside them (pad rows, slack, guards) whose bits changed
  std::vector<T> ctx;
  int64_t stray = hc.download(ctx);
  std::vector<unsigned char> valid((size_t)alloc_q, 0);
  rq = 0;
  for (int b = 0; b < B; ++b)
    for (int tq = 0; tq < qp[b].T; ++tq, ++rq) {
      const size_t row = (size_t)qp[b].row_off + tq;
      valid[row] = 1;
      for (int c = 0; c < dq; ++c) d->ctx[rq * dq + c] = elem_to_f32(ctx[row * dq + c]);
    }
  for (int r = 0; r < alloc_q; ++r)
    if (!valid[r])
      for (int c = 0; c < dq; ++c) stray += same_bits(ctx[(size_t)r * dq + c], hc.at((size_t)r * dq + c)) ? 0 : 1;
  d->stray = (int32_t)std::min<int64_t>(stray, 0x7fffffff);
}

template <typename T>
void probe_fsmn(asr_probe_fsmn_desc* d) {
  const int B = d->batch, C = d->channels;
  ASR_REQUIRE(B > 0 && C > 0 && d->lens && d->v && d->w && d->b && d->out, "probe_fsmn: bad argument");
  ASR_REQUIRE(std::isfinite(d->pad_fill), "probe_fsmn: the poison must be finite");
  std::vector<UttPlan> plan(B);
  std::memset(plan.data(), 0, plan.size() * sizeof(UttPlan));
  int rows = 0;
  for (int b = 0; b < B; ++b) {
    ASR_REQUIRE(d->lens[b] >= 1, "probe_fsmn: empty utterance %d", b);
    plan[b].T = plan[b].n_lfr = d->lens[b]; plan[b].row_off = rows;
    rows += round_up(d->lens[b], 16);
  }
  const int Mpad = round_up(rows, 128);                   // the sessions' packed row count: V^T's leading dimension and the launch's row bound
  std::vector<int32_t> row_utt(Mpad, -1);
  for (int b = 0; b < B; ++b)
    for (int r = 0; r < round_up(d->lens[b], 16); ++r) row_utt[plan[b].row_off + r] = b;
  Poisoned<T> hv((size_t)C * Mpad, 4096, d->pad_fill);
  Poisoned<float> ho((size_t)Mpad * C, 4096, d->pad_fill);
  size_t r = 0;
  for (int b = 0; b < B; ++b)
    for (int tt = 0; tt < plan[b].T; ++tt, ++r)
      for (int c = 0; c < C; ++c) hv.at((size_t)c * Mpad + plan[b].row_off + tt) = elem_from_f32<T>(d->v[r * C + c]);
  Tmp t;
  auto up_raw = [&](const void* h, size_t bytes) -> void* {
    void* p = t.alloc(bytes);
    HIP_CHECK(hipMemcpy(p, h, bytes, hipMemcpyHostToDevice));
    return p;
  };
  const T* dvt = hv.upload(t);
  float* dout = ho.upload(t);
  launch_fsmn<T>(dvt, Mpad, (const float*)up_raw(d->w, (size_t)C * 11 * 4), (const float*)up_raw(d->b, (size_t)C * 4), C, 11,
                 (const UttPlan*)up_raw(plan.data(), plan.size() * sizeof(UttPlan)), (const int32_t*)up_raw(row_utt.data(), row_utt.size() * 4), Mpad, dout, C,
                 nullptr);
  HIP_CHECK(hipDeviceSynchronize());
  // ---- results: the utterances' rows; stray = guard elements whose bits changed + pad rows (an utterance's T .. its 16-row boundary, rows of no
  // utterance) that are not the zeros the out-projection adds
  std::vector<float> out;
  int64_t stray = ho.download(out);
  std::vector<unsigned char> valid((size_t)Mpad, 0);
  r = 0;
  for (int b = 0; b < B; ++b)
    for (int tt = 0; tt < plan[b].T; ++tt, ++r) {
      valid[plan[b].row_off + tt] = 1;
      std::memcpy(d->out + r * C, &out[(size_t)(plan[b].row_off + tt) * C], (size_t)C * 4);
    }
  for (int m = 0; m < Mpad; ++m)
    if (!valid[m])
      for (int c = 0; c < C; ++c) stray += out[(size_t)m * C + c] == 0.0f ? 0 : 1;
  d->stray = (int32_t)std::min<int64_t>(stray, 0x7fffffff);
}

}  // namespace

extern "C" int asr_probe_encoder_attention(asr_probe_enc_attn_desc* d) {
  return asr_guard([&] {
    ASR_REQUIRE(d, "probe_encoder_attention: null descriptor");
    asr_require_device(0);
    if (d->bf16) probe_encoder_attention<bf16_t>(d); else probe_encoder_attention<float>(d);
  });
}

extern "C" int asr_probe_fsmn(asr_probe_fsmn_desc* d) {
  return asr_guard([&] {
    ASR_REQUIRE(d, "probe_fsmn: null descriptor");
    asr_require_device(0);
    if (d->bf16) probe_fsmn<bf16_t>(d); else probe_fsmn<float>(d);
  });
}
