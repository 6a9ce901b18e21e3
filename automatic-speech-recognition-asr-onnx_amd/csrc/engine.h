// Session plumbing shared by the model families: weight arena, grow-only HBM workspace,
// HIP-event profiler, debug taps.
#pragma once
#include <algorithm>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "common.h"
#include "gemm.h"
#include "kernels.h"
#include "plan_layout.h"
#include "result_layout.h"

#define ASR_LOCAL __attribute__((visibility("hidden")))

// ---- weight arena (layout written by arena.py) -----------------------------------------
//   header  : "ASRARENA" | u32 version | u32 n_tensors | u64 data_offset | u64 total_bytes
//   records : n_tensors x 128 B  { char name[80]; u32 dtype; u32 ndim; i64 shape[4]; u64 offset }
//   data    : tensors, each 256-byte aligned, offsets relative to the start of the arena
enum { ARENA_F32 = 0, ARENA_BF16 = 1, ARENA_I32 = 2, ARENA_F16 = 3 };

struct TensorRef {
  void* ptr = nullptr;
  int dtype = 0;
  int ndim = 0;
  int64_t shape[4] = {0, 0, 0, 0};
  int64_t numel() const {
    int64_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= shape[i];
    return n;
  }
};

struct Arena {
  unsigned char* base = nullptr;   // device
  size_t bytes = 0;
  bool owned = false;
  std::map<std::string, TensorRef> tensors;

  Arena() = default;
  Arena(const Arena&) = delete;
  Arena& operator=(const Arena&) = delete;
  ~Arena();
  void load(const void* src, size_t nbytes, int mem, hipStream_t s);
  const TensorRef& get(const std::string& name) const;
  const TensorRef& get(const std::string& name, int dtype, std::initializer_list<int64_t> shape) const;
  bool has(const std::string& name) const { return tensors.count(name) != 0; }
};

// Device bytes held by DeviceBuffers and owned arenas, process-wide (the probe library reports it).
int64_t asr_live_device_bytes();

// HBM workspace. Owns its allocation: move-only, freed by the destructor (or early by release()).
// No DeviceBuffer or PinnedBuffer may have static storage duration: it would be freed after the HIP runtime has shut down.
struct DeviceBuffer {
  void* ptr = nullptr;
  size_t cap = 0;
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  DeviceBuffer(DeviceBuffer&& o) noexcept : ptr(o.ptr), cap(o.cap) { o.ptr = nullptr; o.cap = 0; }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept;
  ~DeviceBuffer() { release(); }
  // grow-only (the old buffer is freed after a synchronise of s); new memory is zero-filled so padded rows/columns are finite
  void reserve(size_t bytes, hipStream_t s);
  void release();
  template <typename T> T* as() const { return reinterpret_cast<T*>(ptr); }
};

// `buf` sized to `bytes`; true when its pointer moved (a captured step that holds it is stale)
ASR_LOCAL inline bool reserve_moved(DeviceBuffer& buf, size_t bytes, hipStream_t s) {
  void* before = buf.ptr;
  buf.reserve(bytes, s);
  return buf.ptr != before;
}

// Pinned host staging: grow-only with 2x headroom, freed by the destructor.
struct PinnedBuffer {
  void* ptr = nullptr;
  size_t cap = 0;
  PinnedBuffer() = default;
  PinnedBuffer(const PinnedBuffer&) = delete;
  PinnedBuffer& operator=(const PinnedBuffer&) = delete;
  ~PinnedBuffer();
  bool reserve(size_t bytes);      // true when the buffer was (re)allocated: a captured graph that copies into it is stale
  template <typename T> T* as() const { return reinterpret_cast<T*>(ptr); }
};

// One call's index tables: sections declared once (PlanLayout), then the pinned and the device buffer reserved for the total, then host(x) and
// dev(x) from the same stored offset, then one copy. The buffers stay the session's; a blob lives on the stack of the call that builds it.
template <typename T> struct PlanSection { int i; };
struct PlanBlob {
  PlanLayout lay;
  PinnedBuffer& h;
  DeviceBuffer& d;
  bool host_moved = false, dev_moved = false;       // set by commit(): a captured graph that bakes that buffer's address in is stale
  PlanBlob(PinnedBuffer& h_, DeviceBuffer& d_) : h(h_), d(d_) {}
  template <typename T> PlanSection<T> add(size_t count) { return PlanSection<T>{lay.add(sizeof(T), alignof(T), count)}; }
  void commit(hipStream_t s, size_t round_to = 1);  // total rounded up to a multiple of round_to
  template <typename T> T* host(PlanSection<T> x) const { return reinterpret_cast<T*>(h.as<unsigned char>() + lay.off[x.i]); }
  template <typename T> const T* dev(PlanSection<T> x) const { return reinterpret_cast<const T*>(d.as<unsigned char>() + lay.off[x.i]); }
  void upload(hipStream_t s) const;
};

// One call's results, the PlanBlob counterpart for the way home: the sections of a ResultLayout in the session's pinned result buffer. The D2H copies a step
// enqueues (inside or outside a capture) and the host reads after the sync take their addresses from the same handles.
struct ResultBlob {
  ResultLayout lay;
  PinnedBuffer& h;
  ResultBlob(PinnedBuffer& h_, const ResultLayout& lay_) : lay(lay_), h(h_) {}
  bool commit() { return h.reserve(lay.total()); }          // true when the host buffer moved: a captured graph that copies into it is stale
  template <typename T> T* host(ResultSection<T> x) const { return reinterpret_cast<T*>(h.as<unsigned char>() + lay.off(x)); }
  template <typename T> T* dev(ResultSection<T> x, const DeviceBuffer& beam_block) const { return reinterpret_cast<T*>(beam_block.as<unsigned char>() + lay.dev_off(x)); }
  template <typename T> void enqueue_copy(ResultSection<T> x, const void* src, hipStream_t s) const {
    HIP_CHECK(hipMemcpyAsync(host(x), src, lay.bytes(x), hipMemcpyDeviceToHost, s));
  }
  // row r of a [rows][max_tokens] section into row r of dst, min(counts[r], max_tokens) elements of it
  template <typename T> void scatter_rows(ResultSection<T> x, T* dst, const int32_t* counts, int max_tokens) const {
    const T* src = host(x);
    for (size_t r = 0, n = lay.rows(x); r < n; ++r)
      memcpy(dst + r * max_tokens, src + r * max_tokens, (size_t)std::min(counts[r], max_tokens) * sizeof(T));
  }
};

// FNV-1a over the values a captured step bakes in
struct GraphKey {
  uint64_t h = 1469598103934665603ull;
  GraphKey& mix(uint64_t v) { h = (h ^ v) * 1099511628211ull; return *this; }
  GraphKey& mix(const void* p) { return mix((uint64_t)(uintptr_t)p); }
};

// One captured step and the capture policy every session uses: the first run of a key is eager (lazily created workspaces and kernel
// attributes settle), the second is captured and launched, later runs with that key replay. A capture that throws is ended and discarded.
// Runs that are not graphable are eager and leave the keys alone.
struct StepGraph {
  hipGraphExec_t exec = nullptr;
  uint64_t key = 0, eager_key = 0;
  StepGraph() = default;
  StepGraph(const StepGraph&) = delete;
  StepGraph& operator=(const StepGraph&) = delete;
  ~StepGraph() { drop(); }
  template <typename F> void run(hipStream_t s, bool graphable, uint64_t k, F&& enqueue) {
    if (graphable && exec && k == key) {
      HIP_CHECK(hipGraphLaunch(exec, s));
    } else if (graphable && k == eager_key) {
      capture(s, k, enqueue);
      HIP_CHECK(hipGraphLaunch(exec, s));
    } else {
      enqueue();
      if (graphable) eager_key = k;
    }
  }
  void drop();

 private:
  void capture(hipStream_t s, uint64_t k, const std::function<void()>& enqueue);
};

struct Profiler {
  bool enabled = false;
  std::vector<std::string> names;
  std::vector<double> total_ms;
  std::vector<int64_t> launches;
  struct Pending { int cls; hipEvent_t a, b; };
  std::vector<Pending> pending;
  std::vector<int> open;   // indices into `pending` of the scopes begun and not yet ended
  std::vector<hipEvent_t> pool;

  Profiler() = default;
  Profiler(const Profiler&) = delete;
  Profiler& operator=(const Profiler&) = delete;
  ~Profiler();
  int cls(const char* name);
  void begin(int c, hipStream_t s);
  void end(hipStream_t s);
  void collect();          // after the stream is synchronised
  void reset();
  hipEvent_t get_event();
};

struct ProfScope {
  Profiler& p; hipStream_t s; bool on;
  ProfScope(Profiler& p_, const char* name, hipStream_t s_) : p(p_), s(s_), on(p_.enabled) { if (on) p.begin(p.cls(name), s); }
  ~ProfScope() { if (on) p.end(s); }
};

struct Tap {
  DeviceBuffer buf;
  int64_t rows = 0, cols = 0;
  int elt = 4;
};

// The device resampler of a session (or of asr_op_resample): the coefficient tables it has built, one per (rate_in, rate_model), and the buffers of a call.
// run() leaves model-rate mono f32 in d_out and the utterances' new offsets (from 0) in `offs`.
struct Resampler {
  struct Table { ResampleDesign d; DeviceBuffer tab_t; };
  std::map<std::pair<int, int>, Table> tables;
  DeviceBuffer d_in, d_out, d_plan;
  PinnedBuffer h_plan;
  std::vector<int64_t> offs;
  const Table& table(int rate_in, int rate_model, hipStream_t s);
  // audio / offsets_in in input frames of `channels` interleaved samples of audio_dtype; host audio is copied into d_in, device audio is read in place
  const float* run(const void* audio, int audio_mem, int audio_dtype, int rate_in, int rate_model, int channels, float scale, const int64_t* offsets_in, int batch,
                   hipStream_t s);
};

struct asr_session {
  int kind = 0;               // 1 = sensevoice, 2 = whisper
  int device = 0;
  int tenant_slot = -1;       // this session's entry in the process-wide tenancy table (asr_tenant_attach; released by the destructor)
  int precision = 0;
  int audio_dtype = 0;        // asr_audio_dtype: the sample type every audio entry of this session reads its `audio` pointer as (asr_session_set_audio_dtype)
  size_t audio_elt() const { return audio_dtype == 0 ? 4 : 2; }
  // asr_session_set_input_format: in_rate == 0 is the default format (model-rate mono: nothing is launched in front of the front end); otherwise every audio
  // entry's audio and offsets count frames of in_channels interleaved samples at in_rate Hz, and stage_input resamples them on the device
  int model_rate = 16000;     // the family's sample_rate, set by its constructor
  int in_rate = 0, in_channels = 1;
  Resampler resampler;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  Arena arena;
  Profiler prof;
  bool taps_enabled = false;
  std::map<std::string, Tap> taps;
  virtual ~asr_session();     // destroys an owned stream; a derived session's members are gone by then
  // asr_session_set_input_format, behind the rate checks and in front of the change: a session whose state belongs to the format in force throws here
  virtual void check_input_format_change(int /*sample_rate*/, int /*channels*/) {}
  void save_tap(const char* name, const void* src, int64_t rows, int64_t cols, int64_t ld_src, int elt);
};

// ---- front end of a call, shared by the model families
// The per-session constants of the fbank / STFT launch. whisper = 1: the Whisper STFT (frames = samples / hop, "n_fft" in messages); 0: Kaldi frames.
struct FrontEnd {
  const float *dft = nullptr, *melp = nullptr;
  const void* dft_split = nullptr;
  int n_bin_tiles = 0, n_kchunks = 0, n_mels = 0, win = 0, hop = 0, whisper = 0;
  float log_floor = 0.0f;
  void init(int nfft, int win_, int hop_, int n_mels_, int whisper_, float log_floor_);     // dft / melp / dft_split: set by the session from its arena
  // utterance b of a packed batch: the length checks (messages carry the family's name), then its samples, frames and fbank workgroups into p;
  // `frames` and `n_fb` are the batch's running totals
  void plan_utt(const char* family, int b, const int64_t* offs, int max_audio_len, UttPlan& p, int& frames, int& n_fb) const;
  FbankArgs args(const void* audio, int audio_dtype, const UttPlan* plan, const int32_t* blk_utt, const int32_t* blk_f0, float* mel_out, float* blk_max) const;
};
void fill_fbank_blocks(const UttPlan* plan, int B, int32_t* blk_utt, int32_t* blk_f0);                    // one entry per 64 frames
void fill_query_blocks(const UttPlan* plan, int n, int q_rows, int32_t* qb_utt, int32_t* qb_q0);         // one entry per q_rows of every plan's T
// What a call plans its front end from: packed model-rate mono samples of `dtype`, and the utterances' offsets into them.
struct AudioIn {
  const void* audio; int mem; const int64_t* offs; int dtype;
  bool resampled;             // the samples are the session's resampler output (device f32), not the caller's
};
// The first thing an audio entry does with its arguments. Default input format: they come back as they are (the session's audio_dtype) and nothing is launched.
// Otherwise the frames are resampled on the session's stream (profiler class "resample") and the result is the f32 buffer with offsets from 0, which the session
// owns until its next call; int16_unit_scale: the front end behind is the Whisper / Qwen one, so int16 PCM takes its 2^-15 here (Pcm<int16_t>::widen).
AudioIn stage_input(asr_session& s, bool int16_unit_scale, const void* audio, int audio_mem, const int64_t* offs, int batch);
// samples [first_sample, first_sample + n_samples) of `in` where the kernels can read them: host audio is copied into d_audio (grow-only; *moved
// reports a re-allocation), device audio is used in place
const void* stage_audio(asr_session& s, DeviceBuffer& d_audio, const AudioIn& in, int64_t first_sample, int64_t n_samples, bool* moved = nullptr);

// The split-K workspace (16 MiB) and tickets of the skinny / decode GEMMs. Per session (sessions may run concurrently), allocated at the first use.
struct SplitKGemm {
  static constexpr size_t WS_BYTES = (size_t)16 << 20;
  static constexpr int TICKETS = 4096;
  DeviceBuffer ws, cnt;
  void ensure(hipStream_t s) { if (!ws.ptr) { ws.reserve(WS_BYTES, s); cnt.reserve((size_t)TICKETS * 4, s); } }
  GemmArgs attach(const GemmArgs& g0, hipStream_t s);                  // g0 with the workspace in place
  void run(const GemmArgs& g0, int precision, hipStream_t s);          // bf16: with the workspace; f32: as given
};

// Decoder projections of an FP8W / MXFP4W session: e4m3 bytes + a power-of-two scale per output row (d_wscale as f32), or e2m1 nibbles + e8m0 block
// scales per 32 k (d_wscale as bytes), for the weight-streaming GEMMs of a decode step; the exact bf16 dequantisation (d_wdq) serves every other path.
struct LowBitWeights {
  struct Slot { const void** w; int N, K; };            // one projection: where the session keeps its pointer, output rows, row length
  struct Entry { const unsigned char* w; const float* s; const unsigned char* s4; };
  DeviceBuffer d_w8, d_wscale, d_wdq;
  std::vector<Entry> e;                                 // [n_layers][per_layer]
  int per_layer = 0;
  bool fp4 = false;
  // layer_slots(i): the projections of layer i, the same (N, K) list in every layer. Quantises them and points every slot at its dequantised copy.
  void build(int n_layers, bool fp4_, const std::function<std::vector<Slot>(int)>& layer_slots, hipStream_t s);
  template <typename G> void select(G& g, int layer, int wi) const {      // G: GemmArgs or DecGemmArgs
    const Entry& x = e[(size_t)layer * per_layer + wi];
    if (fp4) { g.W4 = x.w; g.w_scale4 = x.s4; }
    else { g.W8 = x.w; g.w_scale = x.s; }
  }
};

template <typename F>
int asr_guard(F&& f) {
  try {
    f();
    return ASR_OK;
  } catch (const AsrError& e) {
    asr_set_error(e.msg);
    return e.code;
  } catch (const std::exception& e) {
    asr_set_error(std::string("internal error: ") + e.what());
    return ASR_ERR_INVALID;
  }
}

void asr_require_device(int device_id);

// ---- who else uses this GPU (process-wide). The cluster kernels of the streaming path (and the block kernel) hold every CU for a whole launch and wait on
// sibling workgroups; next to another session's kernels that costs the other tenant its CUs (Qwen3-ASR 3 415 -> 319 audio-s/s beside 1 024 cluster
// workgroups) and can void the launch. Every session registers at creation; every compute entry point holds a TenantScope while it runs.
void asr_tenant_attach(asr_session* s);                                         // after s->device is set
struct TenantScope { asr_session* s; explicit TenantScope(asr_session* s_); ~TenantScope(); };
int asr_tenant_live_others(const asr_session* s);                              // other sessions that exist on s->device
int asr_tenant_busy_others(const asr_session* s, double window_ms);            // ... that are inside a compute call now, or left one less than window_ms ago

// ---- foreign kernels on this GPU: RCCL collectives (or anything else the host program launches outside this library) must never share the chip with a
// cluster kernel (sanm_block8 / sanm_tiles / stream_layers / stream_dec: every workgroup of the grid must be resident and they spin on each other's counters --
// an RCCL kernel parked on a few CUs is exactly the co-tenant that splits a cluster). The rule, process-wide and per device:
//   * asr_device_foreign_begin(dev) (C ABI) opens a foreign section and BLOCKS until no cluster pass is in flight on `dev`; asr_device_foreign_end(dev) closes it
//     (the caller makes sure its kernels have finished by then);
//   * a compute call that would launch cluster kernels asks ClusterScope first: while a foreign section is open it takes its cluster-free path instead
//     (four launches per SANM block, per-layer launches of the streaming step -- same results), it never waits, so the two sides cannot deadlock.
struct ClusterScope {
  int dev; bool ok;                 // ok: cluster kernels may be launched until this scope ends (the call returns with its stream drained)
  explicit ClusterScope(int device);
  ~ClusterScope();
};

// Tuning: the phase clocks a debugged cluster launch left in `times` ([workgroup][16] stamps of the 100 MHz clock; interval k = stamp k - stamp k - 1), over the
// workgroups that ran, to stderr. names == nullptr: one line "<title> (us, mean of N workgroups): ..." of the means of intervals first .. last. Otherwise a table
// "[<title>] ..." of mean and maximum per named interval, with the stamps taken inside phase A as rows of their own when inside_a is set.
void dump_phase_clocks(const DeviceBuffer& times, int n_workgroups, int first, int last, const char* const* names, const char* title, bool inside_a = false);
