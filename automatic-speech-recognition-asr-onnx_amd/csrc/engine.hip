// Session plumbing: error channel, arena parsing, workspace, profiler, taps.
#include "engine.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>

#include "../../include/asr_mi355x.h"

static thread_local std::string g_last_error;
void asr_set_error(const std::string& msg) { g_last_error = msg; }
const std::string& asr_get_error() { return g_last_error; }

void asr_require_device(int device_id) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    throw AsrError{ASR_ERR_NO_DEVICE, "no HIP device visible: the MI355X engine has no CPU fallback"};
  if (device_id < 0 || device_id >= n)
    throw AsrError{ASR_ERR_INVALID, "device_id " + std::to_string(device_id) + " out of range (" + std::to_string(n) + " devices)"};
  HIP_CHECK(hipSetDevice(device_id));
}

static std::atomic<int64_t> g_live_bytes{0};
int64_t asr_live_device_bytes() { return g_live_bytes.load(); }

// ---------------------------------------------------------------------------------------- Arena
namespace {
struct ArenaHeader {
  char magic[8];
  uint32_t version, n_tensors;
  uint64_t data_offset, total_bytes;
};
struct ArenaRecord {
  char name[80];
  uint32_t dtype, ndim;
  int64_t shape[4];
  uint64_t offset;
};
static_assert(sizeof(ArenaHeader) == 32, "arena header layout");
static_assert(sizeof(ArenaRecord) == 128, "arena record layout");
}  // namespace

void Arena::load(const void* src, size_t nbytes, int mem, hipStream_t s) {
  ASR_REQUIRE(src && nbytes >= sizeof(ArenaHeader), "arena: empty");
  ArenaHeader hdr;
  if (mem == 0) {
    memcpy(&hdr, src, sizeof(hdr));
  } else {
    HIP_CHECK(hipMemcpy(&hdr, src, sizeof(hdr), hipMemcpyDeviceToHost));
  }
  ASR_REQUIRE(memcmp(hdr.magic, "ASRARENA", 8) == 0, "arena: bad magic");
  ASR_REQUIRE(hdr.version == 1, "arena: unsupported version %u", hdr.version);
  ASR_REQUIRE(hdr.total_bytes == nbytes, "arena: size mismatch (header %llu, given %llu)",
              (unsigned long long)hdr.total_bytes, (unsigned long long)nbytes);
  const size_t table = (size_t)hdr.n_tensors * sizeof(ArenaRecord);
  ASR_REQUIRE(sizeof(hdr) + table <= hdr.data_offset && hdr.data_offset <= nbytes, "arena: corrupt manifest");
  std::vector<ArenaRecord> recs(hdr.n_tensors);
  if (mem == 0) {
    memcpy(recs.data(), (const unsigned char*)src + sizeof(hdr), table);
    HIP_CHECK(hipMalloc((void**)&base, nbytes));
    owned = true;
    g_live_bytes += (int64_t)nbytes;
    HIP_CHECK(hipMemcpyAsync(base, src, nbytes, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
  } else {
    HIP_CHECK(hipMemcpy(recs.data(), (const unsigned char*)src + sizeof(hdr), table, hipMemcpyDeviceToHost));
    base = (unsigned char*)const_cast<void*>(src);
    owned = false;
  }
  bytes = nbytes;
  static const int elt[4] = {4, 2, 4, 2};
  for (const auto& r : recs) {
    ASR_REQUIRE(r.dtype < 4 && r.ndim <= 4, "arena: bad record");
    TensorRef t;
    t.dtype = (int)r.dtype;
    t.ndim = (int)r.ndim;
    for (int i = 0; i < 4; ++i) t.shape[i] = r.shape[i];
    ASR_REQUIRE(r.offset % 256 == 0 && r.offset + (uint64_t)t.numel() * elt[r.dtype] <= nbytes, "arena: tensor out of range");
    t.ptr = base + r.offset;
    char nm[81];
    memcpy(nm, r.name, 80);
    nm[80] = 0;
    tensors[nm] = t;
  }
}

Arena::~Arena() {
  if (owned && base) { (void)hipFree(base); g_live_bytes -= (int64_t)bytes; }
}

const TensorRef& Arena::get(const std::string& name) const {
  auto it = tensors.find(name);
  if (it == tensors.end()) throw AsrError{ASR_ERR_NOT_FOUND, "arena: tensor '" + name + "' missing"};
  return it->second;
}

const TensorRef& Arena::get(const std::string& name, int dtype, std::initializer_list<int64_t> shape) const {
  const TensorRef& t = get(name);
  bool ok = t.dtype == dtype && t.ndim == (int)shape.size();
  int i = 0;
  for (int64_t d : shape) { if (ok && t.shape[i] != d) ok = false; ++i; }
  if (!ok) {
    std::string want, got;
    for (int64_t d : shape) want += std::to_string(d) + ",";
    for (int j = 0; j < t.ndim; ++j) got += std::to_string(t.shape[j]) + ",";
    throw AsrError{ASR_ERR_INVALID, "arena: tensor '" + name + "' has dtype " + std::to_string(t.dtype) + " shape (" + got +
                                        "), expected dtype " + std::to_string(dtype) + " shape (" + want + ")"};
  }
  return t;
}

// ---------------------------------------------------------------------------------------- DeviceBuffer, PinnedBuffer, StepGraph
DeviceBuffer& DeviceBuffer::operator=(DeviceBuffer&& o) noexcept {
  if (this != &o) {
    release();
    ptr = o.ptr; cap = o.cap;
    o.ptr = nullptr; o.cap = 0;
  }
  return *this;
}

void DeviceBuffer::reserve(size_t bytes, hipStream_t s) {
  if (bytes <= cap) return;
  if (ptr) {
    HIP_CHECK(hipStreamSynchronize(s));
    release();
  }
  const size_t want = (bytes + 255) & ~(size_t)255;
  HIP_CHECK(hipMalloc(&ptr, want));
  cap = want;
  g_live_bytes += (int64_t)want;
  HIP_CHECK(hipMemsetAsync(ptr, 0, want, s));
}

void DeviceBuffer::release() {
  if (ptr) { (void)hipFree(ptr); g_live_bytes -= (int64_t)cap; }
  ptr = nullptr;
  cap = 0;
}

PinnedBuffer::~PinnedBuffer() {
  if (ptr) (void)hipHostFree(ptr);
}

bool PinnedBuffer::reserve(size_t bytes) {
  if (bytes <= cap) return false;
  if (ptr) HIP_CHECK(hipHostFree(ptr));
  ptr = nullptr;
  cap = 0;
  HIP_CHECK(hipHostMalloc(&ptr, bytes * 2, hipHostMallocDefault));
  cap = bytes * 2;
  return true;
}

void PlanBlob::commit(hipStream_t s, size_t round_to) {
  lay.round_total(round_to);
  host_moved = h.reserve(lay.total);
  void* before = d.ptr;
  d.reserve(lay.total, s);
  dev_moved = d.ptr != before;
}

void PlanBlob::upload(hipStream_t s) const { HIP_CHECK(hipMemcpyAsync(d.ptr, h.ptr, lay.total, hipMemcpyHostToDevice, s)); }

void StepGraph::drop() {
  if (exec) (void)hipGraphExecDestroy(exec);
  exec = nullptr;
}

void StepGraph::capture(hipStream_t s, uint64_t k, const std::function<void()>& enqueue) {
  drop();
  hipGraph_t graph = nullptr;
  HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  try {
    enqueue();
  } catch (...) {
    (void)hipStreamEndCapture(s, &graph);
    if (graph) (void)hipGraphDestroy(graph);
    throw;
  }
  HIP_CHECK(hipStreamEndCapture(s, &graph));
  const hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (e != hipSuccess) exec = nullptr;
  HIP_CHECK(e);
  key = k;
}

// ---------------------------------------------------------------------------------------- Profiler
int Profiler::cls(const char* name) {
  for (size_t i = 0; i < names.size(); ++i)
    if (names[i] == name) return (int)i;
  names.push_back(name);
  total_ms.push_back(0.0);
  launches.push_back(0);
  return (int)names.size() - 1;
}

hipEvent_t Profiler::get_event() {
  if (!pool.empty()) {
    hipEvent_t e = pool.back();
    pool.pop_back();
    return e;
  }
  hipEvent_t e;
  HIP_CHECK(hipEventCreate(&e));
  return e;
}

void Profiler::begin(int c, hipStream_t s) {
  Pending p{c, get_event(), get_event()};
  HIP_CHECK(hipEventRecord(p.a, s));
  open.push_back((int)pending.size());
  pending.push_back(p);
}

void Profiler::end(hipStream_t s) {          // scopes nest: the innermost open one ends
  HIP_CHECK(hipEventRecord(pending[open.back()].b, s));
  open.pop_back();
}

void Profiler::collect() {
  for (auto& p : pending) {
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, p.a, p.b));
    total_ms[p.cls] += ms;
    launches[p.cls] += 1;
    pool.push_back(p.a);
    pool.push_back(p.b);
  }
  pending.clear();
}

void Profiler::reset() {
  for (auto& v : total_ms) v = 0.0;
  for (auto& v : launches) v = 0;
}

Profiler::~Profiler() {
  for (auto& p : pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
  for (auto e : pool) (void)hipEventDestroy(e);
}

// ---------------------------------------------------------------------------------------- taps
void asr_session::save_tap(const char* name, const void* src, int64_t rows, int64_t cols, int64_t ld_src, int elt) {
  if (!taps_enabled) return;
  Tap& t = taps[name];
  t.rows = rows;
  t.cols = cols;
  t.elt = elt;
  t.buf.reserve((size_t)rows * cols * elt, stream);
  HIP_CHECK(hipMemcpy2DAsync(t.buf.ptr, (size_t)cols * elt, src, (size_t)ld_src * elt, (size_t)cols * elt, (size_t)rows,
                             hipMemcpyDeviceToDevice, stream));
}

// ---------------------------------------------------------------------------------------- front end, session GEMM, low-bit weights
void FrontEnd::init(int nfft, int win_, int hop_, int n_mels_, int whisper_, float log_floor_) {
  n_bin_tiles = (nfft / 2 + 1 + 15) / 16;
  n_kchunks = win_ / 16;
  n_mels = n_mels_; win = win_; hop = hop_; whisper = whisper_; log_floor = log_floor_;
}

void FrontEnd::plan_utt(const char* family, int b, const int64_t* offs, int max_audio_len, UttPlan& p, int& frames, int& n_fb) const {
  const int64_t n = offs[b + 1] - offs[b];
  ASR_REQUIRE(n >= win, whisper ? "%s: utterance %d has %lld samples (< n_fft %d)" : "%s: utterance %d has %lld samples (< one %d-sample frame)", family, b, (long long)n, win);
  ASR_REQUIRE(n <= max_audio_len, "%s: utterance %d has %lld samples (> max_audio_len %d)", family, b, (long long)n, max_audio_len);
  p.audio_off = offs[b] - offs[0];
  p.n_samples = (int)n;
  p.n_frames = whisper ? (int)n / hop : ((int)n - win) / hop + 1;      // Whisper: centred STFT with the last frame dropped
  p.frame_off = frames;
  p.blk0 = n_fb;
  frames += p.n_frames;
  n_fb += (p.n_frames + 63) / 64;
}

FbankArgs FrontEnd::args(const void* audio, int audio_dtype, const UttPlan* plan, const int32_t* blk_utt, const int32_t* blk_f0, float* mel_out,
                         float* blk_max) const {
  FbankArgs fa;
  fa.audio = audio; fa.audio_dtype = audio_dtype; fa.plan = plan; fa.blk_utt = blk_utt; fa.blk_f0 = blk_f0; fa.dft_packed = dft; fa.mel_packed = melp;
  fa.mel_out = mel_out; fa.n_bin_tiles = n_bin_tiles; fa.n_kchunks = n_kchunks; fa.n_mel_tiles = n_mels / 16; fa.n_mels = n_mels;
  fa.win = win; fa.hop = hop; fa.log_floor = log_floor; fa.whisper = whisper; fa.blk_max = blk_max; fa.dft_split = dft_split;
  fa.log_at_floor = (float)(whisper ? std::log10((double)log_floor) : std::log((double)log_floor));
  return fa;
}

void fill_fbank_blocks(const UttPlan* plan, int B, int32_t* blk_utt, int32_t* blk_f0) {
  for (int b = 0, i = 0; b < B; ++b)
    for (int f0 = 0; f0 < plan[b].n_frames; f0 += 64) { blk_utt[i] = b; blk_f0[i++] = f0; }
}
void fill_query_blocks(const UttPlan* plan, int n, int q_rows, int32_t* qb_utt, int32_t* qb_q0) {
  for (int u = 0, i = 0; u < n; ++u)
    for (int q0 = 0; q0 < plan[u].T; q0 += q_rows) { qb_utt[i] = u; qb_q0[i++] = q0; }
}

const Resampler::Table& Resampler::table(int rate_in, int rate_model, hipStream_t s) {
  auto it = tables.find({rate_in, rate_model});
  if (it != tables.end()) return it->second;
  const ResampleDesign d = resample_design(rate_in, rate_model);
  std::vector<float> c((size_t)d.L * d.T), ct(c.size());
  resample_table(d, c.data());
  for (int p = 0; p < d.L; ++p)
    for (int k = 0; k < d.T; ++k) ct[(size_t)k * d.L + p] = c[(size_t)p * d.T + k];
  Table& t = tables[{rate_in, rate_model}];
  t.d = d;
  t.tab_t.reserve(ct.size() * 4, s);
  HIP_CHECK(hipMemcpyAsync(t.tab_t.ptr, ct.data(), ct.size() * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipStreamSynchronize(s));                    // (ct is a local; once per format)
  return t;
}

const float* Resampler::run(const void* audio, int audio_mem, int audio_dtype, int rate_in, int rate_model, int channels, float scale, const int64_t* offsets_in,
                            int batch, hipStream_t s) {
  ASR_REQUIRE(audio && offsets_in && batch >= 1, "resample: null argument");
  ASR_REQUIRE(channels >= 1 && channels <= 8, "input format: %d channels (1..8)", channels);
  const Table& tb = table(rate_in, rate_model, s);
  const ResampleDesign& d = tb.d;
  // ---- host plan: per utterance its frames and its n_out = ceil(n_in L / M) outputs; one (utterance, first output) entry per tile
  offs.assign((size_t)batch + 1, 0);
  int64_t n_tiles = 0;
  for (int b = 0; b < batch; ++b) {
    const int64_t n_in = offsets_in[b + 1] - offsets_in[b];
    ASR_REQUIRE(n_in >= 0 && n_in <= INT32_MAX, "resample: utterance %d has %lld frames", b, (long long)n_in);
    const int64_t n_out = resample_n_out(n_in, d);
    ASR_REQUIRE(n_out <= INT32_MAX, "resample: utterance %d has %lld samples at the model rate", b, (long long)n_out);
    offs[b + 1] = offs[b] + n_out;
    n_tiles += (n_out + d.tile - 1) / d.tile;
  }
  ASR_REQUIRE(n_tiles <= INT32_MAX, "resample: %lld tiles", (long long)n_tiles);
  PlanBlob pb(h_plan, d_plan);
  const auto s_utt = pb.add<RsUtt>(batch);
  const auto s_tile_utt = pb.add<int32_t>(std::max<int64_t>(n_tiles, 1)), s_tile_n0 = pb.add<int32_t>(std::max<int64_t>(n_tiles, 1));
  pb.commit(s);
  RsUtt* hu = pb.host(s_utt);
  int32_t *tile_utt = pb.host(s_tile_utt), *tile_n0 = pb.host(s_tile_n0);
  const int64_t base0 = offsets_in[0];
  for (int b = 0, i = 0; b < batch; ++b) {
    hu[b].in_off = offsets_in[b] - base0; hu[b].out_off = offs[b];
    hu[b].n_in = (int32_t)(offsets_in[b + 1] - offsets_in[b]); hu[b].n_out = (int32_t)(offs[b + 1] - offs[b]);
    for (int n0 = 0; n0 < hu[b].n_out; n0 += d.tile) { tile_utt[i] = b; tile_n0[i++] = n0; }
  }
  pb.upload(s);
  // ---- the frames where the kernel can read them, the output buffer, the launch
  const size_t frame_bytes = (size_t)channels * audio_elt_bytes(audio_dtype), in_bytes = (size_t)(offsets_in[batch] - base0) * frame_bytes;
  const void* src = static_cast<const unsigned char*>(audio) + (size_t)base0 * frame_bytes;
  if (audio_mem == ASR_MEM_HOST) {
    d_in.reserve(std::max<size_t>(in_bytes, 16), s);
    if (in_bytes) HIP_CHECK(hipMemcpyAsync(d_in.ptr, src, in_bytes, hipMemcpyHostToDevice, s));
    src = d_in.ptr;
  }
  d_out.reserve(std::max<size_t>((size_t)offs[batch] * 4, 16), s);
  ResampleArgs a;
  a.audio = src; a.utt = pb.dev(s_utt); a.tile_utt = pb.dev(s_tile_utt); a.tile_n0 = pb.dev(s_tile_n0); a.tab_t = tb.tab_t.as<float>(); a.out = d_out.as<float>();
  a.d = d; a.channels = channels; a.scale = scale; a.audio_dtype = audio_dtype;
  launch_resample(a, (int)n_tiles, s);
  return d_out.as<float>();
}

AudioIn stage_input(asr_session& s, bool int16_unit_scale, const void* audio, int audio_mem, const int64_t* offs, int batch) {
  if (!s.in_rate) return AudioIn{audio, audio_mem, offs, s.audio_dtype, false};
  ProfScope ps(s.prof, "resample", s.stream);
  const float scale = s.audio_dtype == AUDIO_I16 && int16_unit_scale ? 0x1p-15f : 1.0f;
  const float* out = s.resampler.run(audio, audio_mem, s.audio_dtype, s.in_rate, s.model_rate, s.in_channels, scale, offs, batch, s.stream);
  if (s.resampler.offs[batch] > 0) s.save_tap("resampled", out, 1, s.resampler.offs[batch], s.resampler.offs[batch], 4);
  return AudioIn{out, ASR_MEM_DEVICE, s.resampler.offs.data(), AUDIO_F32, true};
}

const void* stage_audio(asr_session& s, DeviceBuffer& d_audio, const AudioIn& in, int64_t first_sample, int64_t n_samples, bool* moved) {
  const size_t eA = audio_elt_bytes(in.dtype);           // the sample type of the call: offsets are samples, bytes step in eA
  const void* audio = in.audio;
  const int audio_mem = in.mem;
  const void* src = static_cast<const unsigned char*>(audio) + (size_t)first_sample * eA;
  void* before = d_audio.ptr;
  if (audio_mem == ASR_MEM_HOST) {
    d_audio.reserve((size_t)n_samples * eA, s.stream);
    HIP_CHECK(hipMemcpyAsync(d_audio.ptr, src, (size_t)n_samples * eA, hipMemcpyHostToDevice, s.stream));
    src = d_audio.ptr;
  }
  if (moved) *moved = d_audio.ptr != before;
  return src;
}

GemmArgs SplitKGemm::attach(const GemmArgs& g0, hipStream_t s) {
  ensure(s);
  GemmArgs g = g0;
  g.sk_ws = ws.as<float>(); g.sk_ws_bytes = WS_BYTES; g.sk_cnt = cnt.as<int32_t>();
  return g;
}

void SplitKGemm::run(const GemmArgs& g0, int precision, hipStream_t s) {
  if (precision != ASR_PRECISION_BF16) { launch_gemm_f32(g0, s); return; }
  launch_gemm_bf16(attach(g0, s), s);
}

void LowBitWeights::build(int n_layers, bool fp4_, const std::function<std::vector<Slot>(int)>& layer_slots, hipStream_t s) {
  fp4 = fp4_;
  size_t w_elems = 0, n_scales = 0;                      // per layer
  for (const Slot& t : layer_slots(0)) { w_elems += (size_t)t.N * t.K; n_scales += t.N; ++per_layer; }
  // MXFP4W: d_w8 holds the nibbles (half a byte per element), d_wscale the e8m0 block scales (one byte per 32 elements)
  d_w8.reserve(fp4 ? n_layers * w_elems / 2 : n_layers * w_elems, s);
  d_wscale.reserve(fp4 ? n_layers * w_elems / 32 : n_layers * n_scales * 4, s);
  d_wdq.reserve(n_layers * w_elems * 2, s);
  for (int i = 0; i < n_layers; ++i) {
    unsigned char* w8 = d_w8.as<unsigned char>() + (fp4 ? i * w_elems / 2 : i * w_elems);
    bf16_t* dq = d_wdq.as<bf16_t>() + i * w_elems;
    float* sc = d_wscale.as<float>() + i * n_scales;
    unsigned char* sc4 = d_wscale.as<unsigned char>() + i * w_elems / 32;
    for (const Slot& t : layer_slots(i)) {
      const size_t ne = (size_t)t.N * t.K;
      if (fp4) launch_quantize_rows_mxfp4((const bf16_t*)*t.w, t.K, t.N, t.K, w8, sc4, dq, s);
      else launch_quantize_rows_fp8((const bf16_t*)*t.w, t.K, t.N, t.K, w8, sc, dq, s);
      e.push_back(Entry{w8, sc, sc4});
      *t.w = dq;                                         // from here on "the weights" are the dequantised copies
      w8 += fp4 ? ne / 2 : ne; dq += ne; sc += t.N; sc4 += ne / 32;
    }
  }
}

// ---- tenancy table (engine.h)
#include <chrono>
namespace {
constexpr int TENANT_SLOTS = 512;
struct TenantSlot { std::atomic<int> used{0}, device{-1}, busy{0}; std::atomic<int64_t> last_ns{0}; };
TenantSlot g_tenants[TENANT_SLOTS];
int64_t tenant_now_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}  // namespace

void asr_tenant_attach(asr_session* s) {
  if (!s || s->tenant_slot >= 0) return;
  for (int i = 0; i < TENANT_SLOTS; ++i) {
    int expect = 0;
    if (g_tenants[i].used.compare_exchange_strong(expect, 1)) {
      g_tenants[i].device.store(s->device); g_tenants[i].busy.store(0); g_tenants[i].last_ns.store(0);
      s->tenant_slot = i;
      return;
    }
  }          // (table full: the session stays anonymous -- it is then never counted, which only ever errs towards the faster path)
}
asr_session::~asr_session() {
  if (own_stream && stream) (void)hipStreamDestroy(stream);
  if (tenant_slot >= 0) { g_tenants[tenant_slot].device.store(-1); g_tenants[tenant_slot].used.store(0); tenant_slot = -1; }
}
TenantScope::TenantScope(asr_session* s_) : s(s_) {
  if (s && s->tenant_slot >= 0) { g_tenants[s->tenant_slot].device.store(s->device); g_tenants[s->tenant_slot].busy.fetch_add(1); }
}
TenantScope::~TenantScope() {
  if (s && s->tenant_slot >= 0) { g_tenants[s->tenant_slot].last_ns.store(tenant_now_ns()); g_tenants[s->tenant_slot].busy.fetch_sub(1); }
}
int asr_tenant_live_others(const asr_session* s) {
  int n = 0;
  for (int i = 0; i < TENANT_SLOTS; ++i)
    if (i != s->tenant_slot && g_tenants[i].used.load() && g_tenants[i].device.load() == s->device) ++n;
  return n;
}
int asr_tenant_busy_others(const asr_session* s, double window_ms) {
  const int64_t now = tenant_now_ns(), win = (int64_t)(window_ms * 1e6);
  int n = 0;
  for (int i = 0; i < TENANT_SLOTS; ++i) {
    if (i == s->tenant_slot || !g_tenants[i].used.load() || g_tenants[i].device.load() != s->device) continue;
    const int64_t last = g_tenants[i].last_ns.load();
    if (g_tenants[i].busy.load() > 0 || (last != 0 && now - last < win)) ++n;
  }
  return n;
}

// ---- foreign-kernel gate (engine.h)
#include <condition_variable>
#include <mutex>
namespace {
constexpr int GATE_DEVS = 64;
std::mutex g_gate_mu;
std::condition_variable g_gate_cv;
int g_foreign[GATE_DEVS], g_cluster[GATE_DEVS];
int64_t g_gate_stats[GATE_DEVS][4];              // foreign sections opened, cluster passes diverted, sections that had to wait, cluster passes admitted
inline int gate_slot(int device) { return device >= 0 && device < GATE_DEVS ? device : GATE_DEVS - 1; }
}  // namespace

ClusterScope::ClusterScope(int device) : dev(gate_slot(device)), ok(false) {
  std::lock_guard<std::mutex> lk(g_gate_mu);
  if (g_foreign[dev] > 0) { ++g_gate_stats[dev][1]; return; }
  ++g_cluster[dev]; ++g_gate_stats[dev][3];
  ok = true;
}
ClusterScope::~ClusterScope() {
  if (!ok) return;
  { std::lock_guard<std::mutex> lk(g_gate_mu); --g_cluster[dev]; }
  g_gate_cv.notify_all();
}

extern "C" int asr_device_foreign_begin(int device_id) {
  return asr_guard([&] {
    ASR_REQUIRE(device_id >= 0 && device_id < GATE_DEVS, "device_foreign_begin: device %d", device_id);
    std::unique_lock<std::mutex> lk(g_gate_mu);
    ++g_foreign[device_id]; ++g_gate_stats[device_id][0];
    if (g_cluster[device_id] > 0) ++g_gate_stats[device_id][2];
    g_gate_cv.wait(lk, [&] { return g_cluster[device_id] == 0; });
  });
}
extern "C" int asr_device_foreign_end(int device_id) {
  return asr_guard([&] {
    ASR_REQUIRE(device_id >= 0 && device_id < GATE_DEVS, "device_foreign_end: device %d", device_id);
    std::lock_guard<std::mutex> lk(g_gate_mu);
    ASR_REQUIRE(g_foreign[device_id] > 0, "device_foreign_end: no foreign section is open on device %d", device_id);
    --g_foreign[device_id];
  });
}
extern "C" int asr_device_foreign_stats(int device_id, int64_t* out4) {
  return asr_guard([&] {
    ASR_REQUIRE(device_id >= 0 && device_id < GATE_DEVS && out4, "device_foreign_stats: bad argument");
    std::lock_guard<std::mutex> lk(g_gate_mu);
    for (int i = 0; i < 4; ++i) out4[i] = g_gate_stats[device_id][i];
  });
}

// ---- phase clocks of a debugged cluster launch (engine.h)
void dump_phase_clocks(const DeviceBuffer& times, int n_workgroups, int first, int last, const char* const* names, const char* title, bool inside_a) {
  std::vector<unsigned long long> t((size_t)n_workgroups * 16);
  HIP_CHECK(hipMemcpy(t.data(), times.ptr, t.size() * 8, hipMemcpyDeviceToHost));
  auto us = [&](int w, int from, int to) { return (double)(t[(size_t)w * 16 + to] - t[(size_t)w * 16 + from]) * 0.01; };     // 100 MHz clock -> us
  unsigned long long t_first = ~0ull, t_last = 0;
  int n = 0, n_plain = 0;
  double sum[16] = {}, mx[16] = {};
  for (int w = 0; w < n_workgroups; ++w) {
    if (!t[(size_t)w * 16]) continue;
    ++n;
    t_first = std::min(t_first, t[(size_t)w * 16 + first - 1]); t_last = std::max(t_last, t[(size_t)w * 16 + last]); n_plain += (int)t[(size_t)w * 16 + 15];
    for (int k = first; k <= last; ++k) { sum[k] += us(w, k - 1, k); mx[k] = std::max(mx[k], us(w, k - 1, k)); }
  }
  if (!names) {
    fprintf(stderr, "%s (us, mean of %d workgroups):", title, n);
    for (int k = first; k <= last; ++k) fprintf(stderr, " %.2f", sum[k] / std::max(n, 1));
    fprintf(stderr, "\n");
    return;
  }
  if (!n) return;
  fprintf(stderr, "[%s] %d workgroups, first start -> last end %.1f us\n", title, n, (double)(t_last - t_first) * 0.01);
  for (int k = first; k <= last; ++k) fprintf(stderr, "  %-22s avg %6.2f us  max %6.2f us\n", names[k - first], sum[k] / n, mx[k]);
  if (inside_a) {                         // stamps 4..7 were taken inside phase A (the rows "B prologue .. B epilogue" above are then meaningless)
    static const char* const inside[5] = {"A: statistics", "A: q/k/v images", "A: own attention tile", "A: shared 9th tile", "A: closing barrier"};
    const int from[5] = {1, 4, 5, 6, 7}, to[5] = {4, 5, 6, 7, 2};
    for (int q = 0; q < 5; ++q) {
      double sm = 0.0, m2 = 0.0;
      for (int w = 0; w < n_workgroups; ++w) if (t[(size_t)w * 16]) { sm += us(w, from[q], to[q]); m2 = std::max(m2, us(w, from[q], to[q])); }
      fprintf(stderr, "  %-22s avg %6.2f us  max %6.2f us\n", inside[q], sm / n, m2);
    }
  }
  fprintf(stderr, "  (debug word 15: %d of %d workgroups)\n", n_plain, n);
}
