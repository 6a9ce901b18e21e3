// C ABI: session utilities and operator-level entry points (see include/asr_mi355x.h).
#include <cstring>

#include "../../include/asr_mi355x.h"
#include "beam_dev.h"
#include "engine.h"
#include "gemm.h"
#include "kernels.h"
#include "nar_stream_state.h"
#include "ngram_lm.h"

const std::string& asr_get_error();

extern "C" int asr_abi_version(void) { return ASR_ABI_VERSION; }
extern "C" const char* asr_last_error(void) { return asr_get_error().c_str(); }

extern "C" int asr_device_count(int* count) {
  return asr_guard([&] {
    ASR_REQUIRE(count, "device_count: null argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
  });
}

extern "C" int asr_mem_alloc(int device_id, size_t bytes, void** out) {
  return asr_guard([&] {
    ASR_REQUIRE(out, "mem_alloc: null argument");
    asr_require_device(device_id);
    HIP_CHECK(hipMalloc(out, std::max<size_t>(bytes, 16)));
  });
}

extern "C" int asr_mem_free(int device_id, void* ptr) {
  return asr_guard([&] {
    if (!ptr) return;
    asr_require_device(device_id);
    HIP_CHECK(hipFree(ptr));
  });
}

extern "C" int asr_mem_copy(int device_id, void* dst, const void* src, size_t bytes, int kind) {
  return asr_guard([&] {
    ASR_REQUIRE(dst && src, "mem_copy: null argument");
    ASR_REQUIRE(kind >= 0 && kind <= 2, "mem_copy: bad kind %d", kind);
    asr_require_device(device_id);
    static const hipMemcpyKind kinds[3] = {hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice};
    HIP_CHECK(hipMemcpy(dst, src, bytes, kinds[kind]));
  });
}

extern "C" int asr_session_destroy(asr_session* s) {
  return asr_guard([&] {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    delete s;
  });
}

extern "C" int asr_session_set_stream(asr_session* s, void* hip_stream) {
  return asr_guard([&] {
    ASR_REQUIRE(s, "set_stream: null session");
    HIP_CHECK(hipStreamSynchronize(s->stream));
    if (s->own_stream && s->stream) (void)hipStreamDestroy(s->stream);
    s->stream = reinterpret_cast<hipStream_t>(hip_stream);
    s->own_stream = false;
  });
}

extern "C" int asr_session_device(asr_session* s, int* device_id) {
  return asr_guard([&] {
    ASR_REQUIRE(s && device_id, "session_device: null argument");
    *device_id = s->device;
  });
}

// The sample type is read at every audio entry (staging size, pointer step, fbank instantiation) and is part of the keys of the step graphs that hold the
// front end, so it may change between any two compute calls.
extern "C" int asr_session_set_audio_dtype(asr_session* s, int audio_dtype) {
  return asr_guard([&] {
    ASR_REQUIRE(s, "set_audio_dtype: null session");
    ASR_REQUIRE(audio_dtype == ASR_AUDIO_F32 || audio_dtype == ASR_AUDIO_I16 || audio_dtype == ASR_AUDIO_F16,
                "set_audio_dtype: unknown audio dtype %d (0 = f32, 1 = int16, 2 = f16)", audio_dtype);
    s->audio_dtype = audio_dtype;
  });
}

extern "C" int asr_session_audio_dtype(asr_session* s, int* audio_dtype_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && audio_dtype_out, "audio_dtype: null argument");
    *audio_dtype_out = s->audio_dtype;
  });
}

// The input format is read where an audio entry stages its audio (stage_input), in front of everything a step graph captures, so it may change between any
// two compute calls. A refused format leaves the one in force.
extern "C" int asr_session_set_input_format(asr_session* s, int sample_rate, int channels) {
  return asr_guard([&] {
    ASR_REQUIRE(s, "set_input_format: null session");
    ASR_REQUIRE(channels >= 1 && channels <= 8, "input format: %d channels (1..8)", channels);
    (void)resample_design(sample_rate, s->model_rate);   // the rate checks; the table itself is built by the first call that uses it
    s->check_input_format_change(sample_rate, channels);  // (a streaming session whose streams carry frames of the filter in force)
    const bool off = sample_rate == s->model_rate && channels == 1;
    s->in_rate = off ? 0 : sample_rate;
    s->in_channels = channels;
  });
}

extern "C" int asr_session_input_format(asr_session* s, int* sample_rate_out, int* channels_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && sample_rate_out && channels_out, "input_format: null argument");
    *sample_rate_out = s->in_rate ? s->in_rate : s->model_rate;
    *channels_out = s->in_channels;
  });
}

extern "C" int asr_session_profile_enable(asr_session* s, int enable) {
  return asr_guard([&] {
    ASR_REQUIRE(s, "profile_enable: null session");
    s->prof.enabled = enable != 0;
  });
}

extern "C" int asr_session_profile_reset(asr_session* s) {
  return asr_guard([&] {
    ASR_REQUIRE(s, "profile_reset: null session");
    s->prof.reset();
  });
}

extern "C" int asr_session_profile_read(asr_session* s, int cap, char* names, double* total_ms, int64_t* launches, int* n_out) {
  return asr_guard([&] {
    ASR_REQUIRE(s && names && total_ms && launches && n_out, "profile_read: null argument");
    const int n = std::min<int>(cap, (int)s->prof.names.size());
    for (int i = 0; i < n; ++i) {
      memset(names + i * 32, 0, 32);
      strncpy(names + i * 32, s->prof.names[i].c_str(), 31);
      total_ms[i] = s->prof.total_ms[i];
      launches[i] = s->prof.launches[i];
    }
    *n_out = n;
  });
}

extern "C" int asr_session_taps_enable(asr_session* s, int enable) {
  return asr_guard([&] {
    ASR_REQUIRE(s, "taps_enable: null session");
    s->taps_enabled = enable != 0;
  });
}

extern "C" int asr_session_tap_shape(asr_session* s, const char* name, int64_t* rows, int64_t* cols) {
  return asr_guard([&] {
    ASR_REQUIRE(s && name && rows && cols, "tap_shape: null argument");
    auto it = s->taps.find(name);
    if (it == s->taps.end()) throw AsrError{ASR_ERR_NOT_FOUND, std::string("tap '") + name + "' not recorded (enable taps, then run)"};
    *rows = it->second.rows;
    *cols = it->second.cols;
  });
}

extern "C" int asr_session_tap_read(asr_session* s, const char* name, void* host_out, size_t bytes) {
  return asr_guard([&] {
    ASR_REQUIRE(s && name && host_out, "tap_read: null argument");
    auto it = s->taps.find(name);
    if (it == s->taps.end()) throw AsrError{ASR_ERR_NOT_FOUND, std::string("tap '") + name + "' not recorded (enable taps, then run)"};
    const Tap& t = it->second;
    const size_t need = (size_t)t.rows * t.cols * t.elt;
    ASR_REQUIRE(bytes == need, "tap_read: '%s' is %zu bytes, buffer is %zu", name, need, bytes);
    HIP_CHECK(hipSetDevice(s->device));
    // on the session's own stream, not the legacy null stream: a synchronous null-stream copy next to captured graphs is what tools/probes/stream_taps_toggle.py
    // trips over on this runtime (taps read between steps, then the cached step graph replayed: a cluster of the fused launch never saw its siblings)
    HIP_CHECK(hipMemcpyAsync(host_out, t.buf.ptr, need, hipMemcpyDeviceToHost, s->stream));
    HIP_CHECK(hipStreamSynchronize(s->stream));
  });
}

// =========================================================================================== operator hooks
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

// upload a host f32 matrix [rows][cols] into a zero-padded device matrix [rows_pad][ld] of the operand dtype
void* upload_operand(Tmp& t, int precision, const float* src, int rows, int cols, int rows_pad, int ld) {
  if (precision == ASR_PRECISION_F32) {
    float* d = (float*)t.alloc((size_t)rows_pad * ld * 4);
    HIP_CHECK(hipMemcpy2D(d, (size_t)ld * 4, src, (size_t)cols * 4, (size_t)cols * 4, rows, hipMemcpyHostToDevice));
    return d;
  }
  std::vector<bf16_t> tmp((size_t)rows * ld, 0);
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) tmp[(size_t)r * ld + c] = f32_to_bf16(src[(size_t)r * cols + c]);
  bf16_t* d = (bf16_t*)t.alloc((size_t)rows_pad * ld * 2);
  HIP_CHECK(hipMemcpy(d, tmp.data(), tmp.size() * 2, hipMemcpyHostToDevice));
  return d;
}

void download_operand(int precision, const void* dsrc, int rows, int cols, int ld, float* out) {
  if (precision == ASR_PRECISION_F32) {
    HIP_CHECK(hipMemcpy2D(out, (size_t)cols * 4, dsrc, (size_t)ld * 4, (size_t)cols * 4, rows, hipMemcpyDeviceToHost));
    return;
  }
  std::vector<bf16_t> tmp((size_t)rows * ld);
  HIP_CHECK(hipMemcpy(tmp.data(), dsrc, tmp.size() * 2, hipMemcpyDeviceToHost));
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) {
      union { uint32_t u; float f; } cv;
      cv.u = ((uint32_t)tmp[(size_t)r * ld + c]) << 16;
      out[(size_t)r * cols + c] = cv.f;
    }
}

struct PackedPlan {
  std::vector<UttPlan> plan;
  std::vector<int32_t> qb_utt, qb_q0, row_utt;
  int rows = 0, Mpad = 0;
  PackedPlan(const int32_t* seq_lens, int batch, int q_rows = 64) {
    plan.resize(batch);
    for (int b = 0; b < batch; ++b) {
      ASR_REQUIRE(seq_lens[b] > 0, "op: empty sequence %d", b);
      memset(&plan[b], 0, sizeof(UttPlan));
      plan[b].T = seq_lens[b];
      plan[b].row_off = rows;
      for (int q0 = 0; q0 < seq_lens[b]; q0 += q_rows) { qb_utt.push_back(b); qb_q0.push_back(q0); }
      rows += round_up(seq_lens[b], 16);
    }
    Mpad = round_up(rows, 128);
    row_utt.assign(Mpad, -1);
    for (int b = 0; b < batch; ++b)
      for (int r = 0; r < round_up(seq_lens[b], 16); ++r) row_utt[plan[b].row_off + r] = b;
  }
};

// scatter dense-packed host rows [sum T][cols] into the 16-row-aligned packed layout (and back)
void to_aligned(const PackedPlan& pp, const int32_t* seq_lens, int batch, int cols, const float* src, std::vector<float>& dst) {
  dst.assign((size_t)pp.Mpad * cols, 0.0f);
  size_t r = 0;
  for (int b = 0; b < batch; ++b) {
    memcpy(&dst[(size_t)pp.plan[b].row_off * cols], src + r * cols, (size_t)seq_lens[b] * cols * 4);
    r += seq_lens[b];
  }
}
void from_aligned(const PackedPlan& pp, const int32_t* seq_lens, int batch, int cols, const std::vector<float>& src, float* dst) {
  size_t r = 0;
  for (int b = 0; b < batch; ++b) {
    memcpy(dst + r * cols, &src[(size_t)pp.plan[b].row_off * cols], (size_t)seq_lens[b] * cols * 4);
    r += seq_lens[b];
  }
}

}  // namespace

extern "C" int asr_op_gemm(int precision, const float* a, const float* w, const float* bias, int M, int N, int K, int act,
                           float* out) {
  return asr_guard([&] {
    ASR_REQUIRE(a && w && out, "op_gemm: null argument");
    asr_require_device(0);
    gemm_reload_env();
    Tmp t;
    const int Mp = round_up(M, 128), Np = round_up(N, 128), Kp = round_up(K, 64);
    void* da = upload_operand(t, precision, a, M, K, Mp, Kp);
    void* dw = upload_operand(t, precision, w, N, K, Np, Kp);
    float* db = nullptr;
    if (bias) {
      db = (float*)t.alloc((size_t)Np * 4);
      HIP_CHECK(hipMemcpy(db, bias, (size_t)N * 4, hipMemcpyHostToDevice));
    }
    float* dout = (float*)t.alloc((size_t)Mp * Np * 4);
    GemmArgs g;
    g.A = da; g.lda = Kp; g.W = dw; g.ldw = Kp; g.M = M; g.N = Np; g.K = Kp; g.bias = db; g.act = act;
    g.out_f32 = dout; g.ld_out_f32 = Np;
    g.sk_ws = (float*)t.alloc((size_t)8 << 20); g.sk_ws_bytes = (size_t)8 << 20;     // lets the launcher pick the split-K tiled path for small grids
    if (precision == ASR_PRECISION_BF16) launch_gemm_bf16(g, nullptr); else launch_gemm_f32(g, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy2D(out, (size_t)N * 4, dout, (size_t)Np * 4, (size_t)N * 4, M, hipMemcpyDeviceToHost));
  });
}

extern "C" int asr_op_layernorm(int precision, const float* x, int rows, int D, const float* gamma, const float* beta, float eps,
                                float* out) {
  return asr_guard([&] {
    ASR_REQUIRE(x && out, "op_layernorm: null argument");
    asr_require_device(0);
    Tmp t;
    float* dx = (float*)t.alloc((size_t)rows * D * 4);
    HIP_CHECK(hipMemcpy(dx, x, (size_t)rows * D * 4, hipMemcpyHostToDevice));
    float *dg = nullptr, *db = nullptr;
    if (gamma) {
      dg = (float*)t.alloc((size_t)D * 4);
      db = (float*)t.alloc((size_t)D * 4);
      HIP_CHECK(hipMemcpy(dg, gamma, (size_t)D * 4, hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(db, beta, (size_t)D * 4, hipMemcpyHostToDevice));
    }
    const int ld = round_up(D, 64);
    if (precision == ASR_PRECISION_F32) {
      float* dout = (float*)t.alloc((size_t)rows * ld * 4);
      launch_layernorm<float>(dx, D, rows, D, dg, db, eps, dout, ld, ld, nullptr);
      HIP_CHECK(hipDeviceSynchronize());
      download_operand(precision, dout, rows, D, ld, out);
    } else {
      bf16_t* dout = (bf16_t*)t.alloc((size_t)rows * ld * 2);
      launch_layernorm<bf16_t>(dx, D, rows, D, dg, db, eps, dout, ld, ld, nullptr);
      HIP_CHECK(hipDeviceSynchronize());
      download_operand(precision, dout, rows, D, ld, out);
    }
  });
}

extern "C" int asr_op_attention(int precision, const float* q, const float* k, const float* v, const int32_t* seq_lens,
                                int batch, int n_heads, int d_head, float* ctx) {
  return asr_guard([&] {
    ASR_REQUIRE(q && k && v && seq_lens && ctx && batch > 0, "op_attention: null argument");
    ASR_REQUIRE(precision == ASR_PRECISION_F32 || d_head == 128 || d_head == 64, "op_attention: bf16 kernel is built for head_dim 64/128");
    asr_require_device(0);
    Tmp t;
    int max_T = 0, att_qt = 0, att_nw = 4, q_rows = 64;
    for (int b = 0; b < batch; ++b) max_T = std::max(max_T, seq_lens[b]);
    if (precision == ASR_PRECISION_BF16) { attention_geometry(max_T, d_head, &att_qt, &att_nw); q_rows = 16 * att_qt * att_nw; }
    PackedPlan pp(seq_lens, batch, q_rows);
    const int d = n_heads * d_head;
    std::vector<float> qa, ka, va;
    to_aligned(pp, seq_lens, batch, d, q, qa);
    to_aligned(pp, seq_lens, batch, d, k, ka);
    to_aligned(pp, seq_lens, batch, d, v, va);
    std::vector<float> vt((size_t)d * pp.Mpad);
    for (int r = 0; r < pp.Mpad; ++r)
      for (int c = 0; c < d; ++c) vt[(size_t)c * pp.Mpad + r] = va[(size_t)r * d + c];
    void* dq = upload_operand(t, precision, qa.data(), pp.Mpad, d, pp.Mpad, d);
    void* dk = upload_operand(t, precision, ka.data(), pp.Mpad, d, pp.Mpad, d);
    void* dvt = upload_operand(t, precision, vt.data(), d, pp.Mpad, d, pp.Mpad);
    const size_t e = precision == ASR_PRECISION_F32 ? 4 : 2;
    void* dctx = t.alloc((size_t)pp.Mpad * d * e);
    UttPlan* dplan = (UttPlan*)t.alloc(sizeof(UttPlan) * batch);
    int32_t* dqu = (int32_t*)t.alloc(pp.qb_utt.size() * 4);
    int32_t* dq0 = (int32_t*)t.alloc(pp.qb_q0.size() * 4);
    HIP_CHECK(hipMemcpy(dplan, pp.plan.data(), sizeof(UttPlan) * batch, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dqu, pp.qb_utt.data(), pp.qb_utt.size() * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dq0, pp.qb_q0.data(), pp.qb_q0.size() * 4, hipMemcpyHostToDevice));
    AttnArgs aa;
    aa.q = dq; aa.k = dk; aa.ld_qk = d; aa.vt = dvt; aa.ld_vt = pp.Mpad; aa.ctx = dctx; aa.ld_ctx = d;
    aa.plan = dplan; aa.qb_utt = dqu; aa.qb_q0 = dq0; aa.n_qblocks = (int)pp.qb_utt.size(); aa.n_heads = n_heads;
    aa.qt = att_qt; aa.n_waves = att_nw; aa.max_T = max_T;
    if (precision == ASR_PRECISION_F32) launch_attention_f32(aa, d_head, nullptr);
    else if (d_head == 128) launch_attention_bf16_hd128(aa, nullptr);
    else launch_attention_bf16_hd64(aa, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    std::vector<float> ca((size_t)pp.Mpad * d);
    download_operand(precision, dctx, pp.Mpad, d, d, ca.data());
    from_aligned(pp, seq_lens, batch, d, ca, ctx);
  });
}

extern "C" int asr_op_fsmn(int precision, const float* v, const float* w, const float* b, const int32_t* seq_lens, int batch,
                           int channels, int ktaps, float* out) {
  return asr_guard([&] {
    ASR_REQUIRE(v && w && b && seq_lens && out && batch > 0, "op_fsmn: null argument");
    asr_require_device(0);
    Tmp t;
    PackedPlan pp(seq_lens, batch);
    std::vector<float> va;
    to_aligned(pp, seq_lens, batch, channels, v, va);
    std::vector<float> vt((size_t)channels * pp.Mpad);
    for (int r = 0; r < pp.Mpad; ++r)
      for (int c = 0; c < channels; ++c) vt[(size_t)c * pp.Mpad + r] = va[(size_t)r * channels + c];
    void* dvt = upload_operand(t, precision, vt.data(), channels, pp.Mpad, channels, pp.Mpad);
    float* dw = (float*)t.alloc((size_t)channels * ktaps * 4);
    float* db = (float*)t.alloc((size_t)channels * 4);
    HIP_CHECK(hipMemcpy(dw, w, (size_t)channels * ktaps * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(db, b, (size_t)channels * 4, hipMemcpyHostToDevice));
    UttPlan* dplan = (UttPlan*)t.alloc(sizeof(UttPlan) * batch);
    int32_t* dru = (int32_t*)t.alloc((size_t)pp.Mpad * 4);
    HIP_CHECK(hipMemcpy(dplan, pp.plan.data(), sizeof(UttPlan) * batch, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dru, pp.row_utt.data(), (size_t)pp.Mpad * 4, hipMemcpyHostToDevice));
    float* dout = (float*)t.alloc((size_t)channels * pp.Mpad * 4);
    if (precision == ASR_PRECISION_F32)
      launch_fsmn<float>((const float*)dvt, pp.Mpad, dw, db, channels, ktaps, dplan, dru, pp.Mpad, dout, channels, nullptr);
    else
      launch_fsmn<bf16_t>((const bf16_t*)dvt, pp.Mpad, dw, db, channels, ktaps, dplan, dru, pp.Mpad, dout, channels, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    std::vector<float> oa((size_t)pp.Mpad * channels);
    HIP_CHECK(hipMemcpy(oa.data(), dout, oa.size() * 4, hipMemcpyDeviceToHost));
    from_aligned(pp, seq_lens, batch, channels, oa, out);
  });
}

extern "C" int asr_op_ctc_collapse(const int32_t* frame_ids, const int32_t* seq_lens, int batch, int blank_id,
                                   int32_t* token_ids, int max_tokens, int32_t* num_id) {
  return asr_guard([&] {
    ASR_REQUIRE(frame_ids && seq_lens && token_ids && num_id && batch > 0 && max_tokens > 0, "op_ctc_collapse: bad argument");
    asr_require_device(0);
    Tmp t;
    PackedPlan pp(seq_lens, batch);
    std::vector<int32_t> ids(pp.Mpad, 0);
    size_t r = 0;
    for (int b = 0; b < batch; ++b) {
      memcpy(&ids[pp.plan[b].row_off], frame_ids + r, (size_t)seq_lens[b] * 4);
      r += seq_lens[b];
    }
    int32_t* dids = (int32_t*)t.alloc((size_t)pp.Mpad * 4);
    UttPlan* dplan = (UttPlan*)t.alloc(sizeof(UttPlan) * batch);
    int32_t* dtok = (int32_t*)t.alloc((size_t)batch * max_tokens * 4);
    int32_t* dnum = (int32_t*)t.alloc((size_t)batch * 4);
    HIP_CHECK(hipMemcpy(dids, ids.data(), (size_t)pp.Mpad * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dplan, pp.plan.data(), sizeof(UttPlan) * batch, hipMemcpyHostToDevice));
    launch_ctc_collapse(dids, dplan, batch, blank_id, dtok, max_tokens, dnum, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(token_ids, dtok, (size_t)batch * max_tokens * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(num_id, dnum, (size_t)batch * 4, hipMemcpyDeviceToHost));
  });
}

extern "C" int asr_op_ctc_collapse_timed(const int32_t* frame_ids, const float* frame_logprob, const int32_t* seq_lens, int batch, int blank_id,
                                         int32_t* token_ids, int32_t* first_frame, int32_t* last_frame, float* token_logprob, int max_tokens,
                                         int32_t* num_id) {
  return asr_guard([&] {
    ASR_REQUIRE(frame_ids && frame_logprob && seq_lens && token_ids && first_frame && last_frame && token_logprob && num_id && batch > 0 && max_tokens > 0,
                "op_ctc_collapse_timed: bad argument");
    asr_require_device(0);
    Tmp t;
    PackedPlan pp(seq_lens, batch);
    std::vector<int32_t> ids(pp.Mpad, 0);
    std::vector<float> lp(pp.Mpad, 0.0f);
    size_t r = 0;
    for (int b = 0; b < batch; ++b) {
      memcpy(&ids[pp.plan[b].row_off], frame_ids + r, (size_t)seq_lens[b] * 4);
      memcpy(&lp[pp.plan[b].row_off], frame_logprob + r, (size_t)seq_lens[b] * 4);
      r += seq_lens[b];
    }
    const size_t out_bytes = (size_t)batch * max_tokens * 4;
    int32_t* dids = (int32_t*)t.alloc((size_t)pp.Mpad * 4);
    float* dlp = (float*)t.alloc((size_t)pp.Mpad * 4);
    UttPlan* dplan = (UttPlan*)t.alloc(sizeof(UttPlan) * batch);
    int32_t* dtok = (int32_t*)t.alloc(out_bytes);
    int32_t* dfirst = (int32_t*)t.alloc(out_bytes);
    int32_t* dlast = (int32_t*)t.alloc(out_bytes);
    float* dtlp = (float*)t.alloc(out_bytes);
    int32_t* dnum = (int32_t*)t.alloc((size_t)batch * 4);
    HIP_CHECK(hipMemcpy(dids, ids.data(), (size_t)pp.Mpad * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dlp, lp.data(), (size_t)pp.Mpad * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dplan, pp.plan.data(), sizeof(UttPlan) * batch, hipMemcpyHostToDevice));
    // the caller's arrays go up first, so that slots the kernel leaves alone come back as they were
    HIP_CHECK(hipMemcpy(dtok, token_ids, out_bytes, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dfirst, first_frame, out_bytes, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dlast, last_frame, out_bytes, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dtlp, token_logprob, out_bytes, hipMemcpyHostToDevice));
    launch_ctc_collapse_timed(dids, dlp, dplan, batch, blank_id, dtok, dfirst, dlast, dtlp, max_tokens, dnum, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(token_ids, dtok, out_bytes, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(first_frame, dfirst, out_bytes, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(last_frame, dlast, out_bytes, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(token_logprob, dtlp, out_bytes, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(num_id, dnum, (size_t)batch * 4, hipMemcpyDeviceToHost));
  });
}

namespace {
// the hotword trie arrays and the language model image of the host-array searches, as their entry points take them (lm words null: no model)
struct TrieArrays { const int32_t *depth, *is_end, *child_off, *child_tok, *child_node; int n_nodes; float boost; };
struct LmImage { const int32_t* words; int64_t n_words; float alpha, beta, oov; };

// a tree in the documented layout -- every node but the root is the child of exactly one node, one level below it
void require_trie(const char* who, const TrieArrays& tr, int blank_id) {
  const int n_nodes = tr.n_nodes;
  ASR_REQUIRE(n_nodes >= 0 && (n_nodes <= 1 || (tr.depth && tr.is_end && tr.child_off && tr.child_tok && tr.child_node)), "%s: trie arrays missing", who);
  if (n_nodes <= 1) return;
  ASR_REQUIRE(tr.child_off[0] == 0 && tr.child_off[n_nodes] == n_nodes - 1 && tr.depth[0] == 0, "%s: malformed trie", who);
  for (int n = 0; n < n_nodes; ++n) {
    ASR_REQUIRE(tr.child_off[n] <= tr.child_off[n + 1], "%s: malformed trie (child_off)", who);
    for (int e = tr.child_off[n]; e < tr.child_off[n + 1]; ++e) {
      const int ch = tr.child_node[e];
      ASR_REQUIRE(ch > 0 && ch < n_nodes && tr.depth[ch] == tr.depth[n] + 1 && tr.child_tok[e] != blank_id && (e == tr.child_off[n] || tr.child_tok[e - 1] < tr.child_tok[e]),
                  "%s: malformed trie (node %d, child entry %d)", who, n, e);
    }
  }
}
// ... and their device copy (t keeps it alive)
HotTrie upload_trie(Tmp& t, const TrieArrays& tr) {
  const int n_nodes = tr.n_nodes;
  if (n_nodes <= 1) return HotTrie{};
  std::vector<int32_t> img;
  img.insert(img.end(), tr.depth, tr.depth + n_nodes); img.insert(img.end(), tr.is_end, tr.is_end + n_nodes);
  img.insert(img.end(), tr.child_off, tr.child_off + n_nodes + 1); img.insert(img.end(), tr.child_tok, tr.child_tok + n_nodes - 1);
  img.insert(img.end(), tr.child_node, tr.child_node + n_nodes - 1);
  int32_t* dtrie = (int32_t*)t.alloc(img.size() * 4);
  HIP_CHECK(hipMemcpy(dtrie, img.data(), img.size() * 4, hipMemcpyHostToDevice));
  return hot_trie_view(dtrie, n_nodes, tr.boost);
}

// What the three host-array searches share on their way to the device. cand_id / cand_lp hold lens[i] rows of topk candidates per sequence i < n, densely; the
// rows go up by plan: PACKED is PackedPlan's layout (the CTC search), COMPACT the compact token plan's (16-row aligned per sequence, an empty sequence keeps one
// dummy row, the total row count on the device in m_dev, plan[i].lang = streams[i] when given), as the Paraformer sessions hand them to the kernels. Checked
// on the way, in this order: with a model the image (blank_id -1: "no blank") and every id the walk will look up, then the device, then distinct ids per row.
// who / lm_who / unit are the names the messages carry. t keeps everything alive; the entry point allocates its outputs from it.
struct BeamOpInput {
  enum Layout { PACKED, COMPACT };
  Tmp t;
  int32_t* ids = nullptr; float* lp = nullptr; UttPlan* plan = nullptr; int32_t* m_dev = nullptr;
  HotTrie trie;
  NgramLm lm;
  int max_len = 1;                    // the longest sequence's rows, at least 1
  BeamOpInput(const char* who, const char* lm_who, const char* unit, const int32_t* cand_id, const float* cand_lp, int topk, const int32_t* lens, int n, Layout layout,
              const int32_t* streams, int blank_id, const TrieArrays& tr, const LmImage& model) {
    if (model.words) {
      const int vocab = model.n_words >= NGRAM_LM_HEADER ? model.words[3] : 0;
      ngram_lm_validate(model.words, model.n_words, vocab, blank_id, model.alpha, model.beta, model.oov, lm_who);
      int64_t n_rows = 0;
      for (int i = 0; i < n; ++i) n_rows += lens[i];
      for (int64_t i = 0; i < n_rows * topk; ++i)
        ASR_REQUIRE(cand_lp[i] == -INFINITY || (cand_id[i] >= 0 && cand_id[i] < vocab), "%s: candidate %d outside the model's vocabulary of %d", lm_who, cand_id[i], vocab);
    }
    asr_require_device(0);
    std::vector<UttPlan> hplan;
    int rows = 0;
    if (layout == PACKED) {
      PackedPlan pp(lens, n);
      hplan = pp.plan; rows = pp.Mpad;
    } else {
      hplan.resize(n);
      for (int i = 0; i < n; ++i) {
        memset(&hplan[i], 0, sizeof(UttPlan));
        hplan[i].n_lfr = lens[i]; hplan[i].T = std::max(lens[i], 1); hplan[i].row_off = rows; hplan[i].lang = streams ? streams[i] : 0;
        rows += round_up(hplan[i].T, 16);
      }
    }
    std::vector<int32_t> hids((size_t)rows * topk, 0);
    std::vector<float> hlp((size_t)rows * topk, 0.0f);
    size_t r = 0;
    for (int i = 0; i < n; ++i) {
      for (int q = 0; q < lens[i]; ++q)
        for (int a = 0; a < topk; ++a)
          for (int c = 0; c < a; ++c)
            ASR_REQUIRE(cand_id[(r + q) * topk + a] != cand_id[(r + q) * topk + c], "%s: %s %d row %d lists token %d twice", who, unit, i, q, cand_id[(r + q) * topk + a]);
      memcpy(&hids[(size_t)hplan[i].row_off * topk], cand_id + r * topk, (size_t)lens[i] * topk * 4);
      memcpy(&hlp[(size_t)hplan[i].row_off * topk], cand_lp + r * topk, (size_t)lens[i] * topk * 4);
      r += lens[i];
      max_len = std::max(max_len, lens[i]);
    }
    ids = (int32_t*)t.alloc(hids.size() * 4);
    lp = (float*)t.alloc(hlp.size() * 4);
    plan = (UttPlan*)t.alloc(sizeof(UttPlan) * n);
    HIP_CHECK(hipMemcpy(ids, hids.data(), hids.size() * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(lp, hlp.data(), hlp.size() * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(plan, hplan.data(), sizeof(UttPlan) * n, hipMemcpyHostToDevice));
    if (layout == COMPACT) {
      m_dev = (int32_t*)t.alloc(4);
      HIP_CHECK(hipMemcpy(m_dev, &rows, 4, hipMemcpyHostToDevice));
    }
    trie = upload_trie(t, tr);
    if (model.words) {
      int32_t* dlm = (int32_t*)t.alloc((size_t)model.n_words * 4);
      HIP_CHECK(hipMemcpy(dlm, model.words, (size_t)model.n_words * 4, hipMemcpyHostToDevice));
      lm = ngram_lm_view(dlm, model.words, model.alpha, model.beta, model.oov);
    }
  }
};

// both host-array entries of the search; lm.words null: without a language model
int op_ctc_prefix_beam(const int32_t* cand_id, const float* cand_logprob, int topk, const int32_t* seq_lens, int batch, int blank_id, const TrieArrays& tr, int beam, int nbest,
                       int32_t* token_ids, int max_tokens, int32_t* num_id, float* score, float* ctc_score, const LmImage& lm) {
  return asr_guard([&] {
    ASR_REQUIRE(cand_id && cand_logprob && seq_lens && token_ids && num_id && score && ctc_score && batch > 0 && max_tokens > 0, "op_ctc_prefix_beam: bad argument");
    ASR_REQUIRE(topk >= 1 && topk <= TOKEN_BEAM_MAX && beam >= 1 && beam <= TOKEN_BEAM_MAX && nbest >= 1 && nbest <= beam,
                "op_ctc_prefix_beam: beam %d, topk %d, nbest %d (1..16, nbest <= beam)", beam, topk, nbest);
    require_trie("op_ctc_prefix_beam", tr, blank_id);
    BeamOpInput in("op_ctc_prefix_beam", "op_ctc_prefix_beam_lm", "utterance", cand_id, cand_logprob, topk, seq_lens, batch, BeamOpInput::PACKED, nullptr, blank_id, tr, lm);
    Tmp& t = in.t;
    const int pool_stride = in.max_len * beam;
    int2* dpool = (int2*)t.alloc((size_t)batch * pool_stride * sizeof(int2));
    const size_t hyps = (size_t)batch * nbest;
    int32_t* dtok = (int32_t*)t.alloc(hyps * max_tokens * 4);
    int32_t* dnum = (int32_t*)t.alloc(hyps * 4);
    float* dsc = (float*)t.alloc(hyps * 4);
    float* dctc = (float*)t.alloc(hyps * 4);
    launch_ctc_prefix_beam(in.ids, in.lp, topk, in.plan, batch, blank_id, beam, nbest, in.trie, dpool, pool_stride, dtok, max_tokens, dnum, dsc, dctc, nullptr, &in.lm);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(token_ids, dtok, hyps * max_tokens * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(num_id, dnum, hyps * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(score, dsc, hyps * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(ctc_score, dctc, hyps * 4, hipMemcpyDeviceToHost));
  });
}
}  // namespace

extern "C" int asr_op_ctc_prefix_beam(const int32_t* cand_id, const float* cand_logprob, int topk, const int32_t* seq_lens, int batch, int blank_id,
                                      const int32_t* trie_depth, const int32_t* trie_is_end, const int32_t* trie_child_off, const int32_t* trie_child_tok,
                                      const int32_t* trie_child_node, int n_nodes, float boost, int beam, int nbest, int32_t* token_ids, int max_tokens,
                                      int32_t* num_id, float* score, float* ctc_score) {
  return op_ctc_prefix_beam(cand_id, cand_logprob, topk, seq_lens, batch, blank_id, TrieArrays{trie_depth, trie_is_end, trie_child_off, trie_child_tok, trie_child_node, n_nodes, boost},
                            beam, nbest, token_ids, max_tokens, num_id, score, ctc_score, LmImage{nullptr, 0, 0.0f, 0.0f, 0.0f});
}

extern "C" int asr_op_ctc_prefix_beam_lm(const int32_t* cand_id, const float* cand_logprob, int topk, const int32_t* seq_lens, int batch, int blank_id,
                                         const int32_t* trie_depth, const int32_t* trie_is_end, const int32_t* trie_child_off, const int32_t* trie_child_tok,
                                         const int32_t* trie_child_node, int n_nodes, float boost, int beam, int nbest, int32_t* token_ids, int max_tokens,
                                         int32_t* num_id, float* score, float* ctc_score, const int32_t* lm_image, int64_t lm_words, float alpha, float beta,
                                         float oov_logprob) {
  if (!lm_image) return asr_guard([&] { ASR_REQUIRE(false, "op_ctc_prefix_beam_lm: no language model image"); });
  return op_ctc_prefix_beam(cand_id, cand_logprob, topk, seq_lens, batch, blank_id, TrieArrays{trie_depth, trie_is_end, trie_child_off, trie_child_tok, trie_child_node, n_nodes, boost},
                            beam, nbest, token_ids, max_tokens, num_id, score, ctc_score, LmImage{lm_image, lm_words, alpha, beta, oov_logprob});
}

// The beam search over token rows on host arrays (the rows in the compact token plan's layout: BeamOpInput).
extern "C" int asr_op_nar_beam(const int32_t* cand_id, const float* cand_logprob, int topk, const int32_t* seq_lens, int batch, const int32_t* trie_depth,
                               const int32_t* trie_is_end, const int32_t* trie_child_off, const int32_t* trie_child_tok, const int32_t* trie_child_node, int n_nodes,
                               float boost, const int32_t* lm_image, int64_t lm_words, float alpha, float beta, float oov_logprob, int beam, int nbest,
                               int32_t* token_ids, int max_tokens, int32_t* num_id, float* score, float* am_score, float* token_logprob) {
  return asr_guard([&] {
    ASR_REQUIRE(cand_id && cand_logprob && seq_lens && token_ids && num_id && score && am_score && batch > 0 && max_tokens > 0, "op_nar_beam: bad argument");
    ASR_REQUIRE(topk >= 1 && topk <= TOKEN_BEAM_MAX && beam >= 1 && beam <= TOKEN_BEAM_MAX && nbest >= 1 && nbest <= beam,
                "op_nar_beam: beam %d, topk %d, nbest %d (1..16, nbest <= beam)", beam, topk, nbest);
    const TrieArrays tr{trie_depth, trie_is_end, trie_child_off, trie_child_tok, trie_child_node, n_nodes, boost};
    require_trie("op_nar_beam", tr, -1);
    for (int b = 0; b < batch; ++b) ASR_REQUIRE(seq_lens[b] >= 0, "op_nar_beam: sequence %d has %d rows", b, seq_lens[b]);
    BeamOpInput in("op_nar_beam", "op_nar_beam", "sequence", cand_id, cand_logprob, topk, seq_lens, batch, BeamOpInput::COMPACT, nullptr, -1, tr,
                   LmImage{lm_image, lm_words, alpha, beta, oov_logprob});
    Tmp& t = in.t;
    const int pool_stride = in.max_len * beam;
    int2* dpool = (int2*)t.alloc((size_t)batch * pool_stride * sizeof(int2));
    const size_t hyps = (size_t)batch * nbest;
    int32_t* dtok = (int32_t*)t.alloc(hyps * max_tokens * 4);
    float* dtlp = (float*)t.alloc(hyps * max_tokens * 4);
    int32_t* dnum = (int32_t*)t.alloc(hyps * 4);
    float* dsc = (float*)t.alloc(hyps * 4);
    float* dam = (float*)t.alloc(hyps * 4);
    launch_nar_beam(in.ids, in.lp, topk, in.plan, in.m_dev, batch, beam, nbest, in.trie, dpool, pool_stride, dtok, max_tokens, dnum, dsc, dam, dtlp, nullptr, &in.lm);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(token_ids, dtok, hyps * max_tokens * 4, hipMemcpyDeviceToHost));
    if (token_logprob) HIP_CHECK(hipMemcpy(token_logprob, dtlp, hyps * max_tokens * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(num_id, dnum, hyps * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(score, dsc, hyps * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(am_score, dam, hyps * 4, hipMemcpyDeviceToHost));
  });
}

// The streaming search on host arrays: `n_steps` launches over state the call keeps between them. Step s has the slots step_off[s] .. step_off[s + 1]; slot i
// is stream slot_stream[i] with slot_rows[i] rows (in slot order in cand_id / cand_logprob) and the flag slot_final[i]. The rows go up in the compact token
// plan's layout, as asr_op_nar_beam sends them. state_io (nullable: every stream starts cleared) holds every stream's state before the call and after it.
extern "C" int asr_nar_stream_beam_state_words(int beam, int pend_cap) {
  if (beam < 1 || beam > TOKEN_BEAM_MAX || pend_cap < 1 || pend_cap > NAR_STREAM_PEND_MAX) return -1;
  return nar_stream_beam_state_words(beam, pend_cap);
}

extern "C" int asr_op_nar_stream_beam(const int32_t* cand_id, const float* cand_logprob, int topk, int n_streams, int n_steps, const int32_t* step_off,
                                      const int32_t* slot_stream, const int32_t* slot_rows, const int32_t* slot_final, const int32_t* trie_depth,
                                      const int32_t* trie_is_end, const int32_t* trie_child_off, const int32_t* trie_child_tok, const int32_t* trie_child_node,
                                      int n_nodes, float boost, const int32_t* lm_image, int64_t lm_words, float alpha, float beta, float oov_logprob, int beam,
                                      int nbest, int pend_cap, int32_t* state_io, int state_words, int32_t* commit_ids, float* commit_logprob, int commit_cap,
                                      int32_t* commit_num, int32_t* pend_ids, float* pend_logprob, int32_t* pend_num, float* pend_score, float* pend_am,
                                      int32_t* total) {
  return asr_guard([&] {
    namespace S = nar_stream_state;
    ASR_REQUIRE(cand_id && cand_logprob && step_off && slot_stream && slot_rows && slot_final && commit_ids && commit_logprob && commit_num && pend_ids && pend_logprob &&
                    pend_num && pend_score && pend_am && total && n_streams > 0 && n_steps > 0,
                "op_nar_stream_beam: bad argument");
    ASR_REQUIRE(topk >= 1 && topk <= TOKEN_BEAM_MAX && beam >= 1 && beam <= TOKEN_BEAM_MAX && nbest >= 1 && nbest <= beam && pend_cap >= 1 && pend_cap <= NAR_STREAM_PEND_MAX,
                "op_nar_stream_beam: beam %d, topk %d, nbest %d (1..16, nbest <= beam), pend_cap %d (1..%d)", beam, topk, nbest, pend_cap, NAR_STREAM_PEND_MAX);
    const TrieArrays tr{trie_depth, trie_is_end, trie_child_off, trie_child_tok, trie_child_node, n_nodes, boost};
    require_trie("op_nar_stream_beam", tr, -1);
    const int sw = nar_stream_beam_state_words(beam, pend_cap);
    ASR_REQUIRE(!state_io || state_words == sw, "op_nar_stream_beam: a state of %d words per stream, beam %d and pend_cap %d take %d", state_words, beam, pend_cap, sw);
    ASR_REQUIRE(step_off[0] == 0, "op_nar_stream_beam: step_off[0] = %d", step_off[0]);
    const int lm_nodes = lm_image && lm_words >= NGRAM_LM_HEADER ? lm_image[1] : 0;
    std::vector<int> seen(n_streams);
    int max_rows = 0;
    for (int s = 0; s < n_steps; ++s) {
      ASR_REQUIRE(step_off[s + 1] > step_off[s], "op_nar_stream_beam: step %d has no stream", s);
      std::fill(seen.begin(), seen.end(), 0);
      for (int i = step_off[s]; i < step_off[s + 1]; ++i) {
        const int sid = slot_stream[i];
        ASR_REQUIRE(sid >= 0 && sid < n_streams && !seen[sid], "op_nar_stream_beam: step %d names stream %d (of %d, once per step)", s, sid, n_streams);
        ASR_REQUIRE(slot_rows[i] >= 0, "op_nar_stream_beam: step %d, stream %d has %d rows", s, sid, slot_rows[i]);
        seen[sid] = 1;
        max_rows = std::max(max_rows, slot_rows[i]);
        if (state_io && state_io[(size_t)sid * sw + S::L] > 0) {         // a stream that comes with history: everything the kernel will index with
          const int32_t* st = state_io + (size_t)sid * sw;
          const int L = st[S::L], C = st[S::C], n_live = st[S::N_LIVE];
          ASR_REQUIRE(C >= 0 && C <= L && L - C <= pend_cap && n_live >= 1 && n_live <= beam, "op_nar_stream_beam: stream %d: L %d, C %d, %d live", sid, L, C, n_live);
          for (int r = 0; r < n_live; ++r)
            ASR_REQUIRE(st[S::NODE + r] >= 0 && st[S::NODE + r] < std::max(n_nodes, 1) && (!lm_nodes || (st[S::LMSTATE + r] >= 0 && st[S::LMSTATE + r] < lm_nodes)),
                        "op_nar_stream_beam: stream %d, hypothesis %d: a trie node or model state out of range", sid, r);
          const int32_t* parent = st + S::ring_parent(beam, pend_cap);
          for (int i2 = 0; i2 < pend_cap * beam; ++i2)
            ASR_REQUIRE(parent[i2] >= 0 && parent[i2] < beam, "op_nar_stream_beam: stream %d: ring parent %d", sid, parent[i2]);
        }
      }
    }
    const int n_slots = step_off[n_steps];
    ASR_REQUIRE(commit_cap >= pend_cap + max_rows, "op_nar_stream_beam: commit_cap %d, pend_cap + the longest step is %d", commit_cap, pend_cap + max_rows);
    BeamOpInput in("op_nar_stream_beam", "op_nar_stream_beam", "slot", cand_id, cand_logprob, topk, slot_rows, n_slots, BeamOpInput::COMPACT, slot_stream, -1, tr,
                   LmImage{lm_image, lm_words, alpha, beta, oov_logprob});
    Tmp& t = in.t;
    int32_t* dfinal = (int32_t*)t.alloc((size_t)n_slots * 4);
    const size_t state_bytes = (size_t)n_streams * sw * 4;
    int32_t* dstate = (int32_t*)t.alloc(state_bytes);
    HIP_CHECK(hipMemcpy(dfinal, slot_final, (size_t)n_slots * 4, hipMemcpyHostToDevice));
    if (state_io) HIP_CHECK(hipMemcpy(dstate, state_io, state_bytes, hipMemcpyHostToDevice));
    else HIP_CHECK(hipMemset(dstate, 0, state_bytes));
    const size_t hyps = (size_t)n_slots * nbest, n_commit = (size_t)n_slots * commit_cap;
    NarStreamOut o;
    o.commit_ids = (int32_t*)t.alloc(n_commit * 4); o.commit_lp = (float*)t.alloc(n_commit * 4); o.commit_cap = commit_cap;
    o.commit_num = (int32_t*)t.alloc((size_t)n_slots * 4);
    o.pend_ids = (int32_t*)t.alloc(hyps * pend_cap * 4); o.pend_lp = (float*)t.alloc(hyps * pend_cap * 4);
    o.pend_num = (int32_t*)t.alloc(hyps * 4); o.pend_score = (float*)t.alloc(hyps * 4); o.pend_am = (float*)t.alloc(hyps * 4);
    o.total = (int32_t*)t.alloc((size_t)n_slots * 4);
    // the caller's arrays go up first, so that slots the kernel leaves alone come back as they were
    HIP_CHECK(hipMemcpy(o.commit_ids, commit_ids, n_commit * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(o.commit_lp, commit_logprob, n_commit * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(o.pend_ids, pend_ids, hyps * pend_cap * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(o.pend_lp, pend_logprob, hyps * pend_cap * 4, hipMemcpyHostToDevice));
    for (int s = 0; s < n_steps; ++s) {
      const size_t at = step_off[s];
      NarStreamOut so = o;
      so.commit_ids += at * commit_cap; so.commit_lp += at * commit_cap; so.commit_num += at;
      so.pend_ids += at * nbest * pend_cap; so.pend_lp += at * nbest * pend_cap; so.pend_num += at * nbest; so.pend_score += at * nbest; so.pend_am += at * nbest;
      so.total += at;
      launch_nar_stream_beam(in.ids, in.lp, topk, in.plan + at, in.m_dev, dfinal + at, step_off[s + 1] - step_off[s], beam, nbest, pend_cap, in.trie, dstate, sw, so, nullptr,
                             &in.lm);
    }
    HIP_CHECK(hipDeviceSynchronize());
    if (state_io) HIP_CHECK(hipMemcpy(state_io, dstate, state_bytes, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(commit_ids, o.commit_ids, n_commit * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(commit_logprob, o.commit_lp, n_commit * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(commit_num, o.commit_num, (size_t)n_slots * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(pend_ids, o.pend_ids, hyps * pend_cap * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(pend_logprob, o.pend_lp, hyps * pend_cap * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(pend_num, o.pend_num, hyps * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(pend_score, o.pend_score, hyps * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(pend_am, o.pend_am, hyps * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(total, o.total, (size_t)n_slots * 4, hipMemcpyDeviceToHost));
  });
}

extern "C" int asr_op_ctc_align(const float* em, int ld_em, const int32_t* seq_lens, int batch, int row0, const int32_t* target_ids, const int32_t* target_offsets,
                                int32_t* first_frame, int32_t* last_frame, float* token_logprob, int max_tokens, float* path_score, float* loglik, int32_t* status) {
  return asr_guard([&] {
    ASR_REQUIRE(em && seq_lens && target_ids && target_offsets && first_frame && last_frame && token_logprob && path_score && loglik && status && batch > 0 && max_tokens > 0,
                "op_ctc_align: bad argument");
    ASR_REQUIRE(target_offsets[0] == 0 && row0 >= 0, "op_ctc_align: target_offsets[0] = %d, row0 = %d", target_offsets[0], row0);
    int max_L = 0, max_T = 1;
    for (int b = 0; b < batch; ++b) {
      const int L = target_offsets[b + 1] - target_offsets[b];
      ASR_REQUIRE(L >= 0, "op_ctc_align: target_offsets decrease at sequence %d", b);
      ASR_REQUIRE(seq_lens[b] > row0, "op_ctc_align: sequence %d has %d rows, row0 = %d", b, seq_lens[b], row0);
      max_L = std::max(max_L, L); max_T = std::max(max_T, seq_lens[b]);
    }
    ASR_REQUIRE(ld_em >= max_L + 1 && max_tokens >= max_L, "op_ctc_align: ld_em = %d, max_tokens = %d for a transcript of %d tokens", ld_em, max_tokens, max_L);
    asr_require_device(0);
    Tmp t;
    PackedPlan pp(seq_lens, batch);
    std::vector<float> ea;
    to_aligned(pp, seq_lens, batch, ld_em, em, ea);
    const size_t out_bytes = (size_t)batch * max_tokens * 4, n_tgt = (size_t)target_offsets[batch];
    float* dem = (float*)t.alloc(ea.size() * 4);
    UttPlan* dplan = (UttPlan*)t.alloc(sizeof(UttPlan) * batch);
    int32_t* dtgt = (int32_t*)t.alloc(n_tgt * 4);
    int32_t* doff = (int32_t*)t.alloc((size_t)(batch + 1) * 4);
    int32_t* dfirst = (int32_t*)t.alloc(out_bytes);
    int32_t* dlast = (int32_t*)t.alloc(out_bytes);
    float* dtlp = (float*)t.alloc(out_bytes);
    float* dpath = (float*)t.alloc((size_t)batch * 4);
    float* dlik = (float*)t.alloc((size_t)batch * 4);
    int32_t* dstat = (int32_t*)t.alloc((size_t)batch * 4);
    const size_t ws = ctc_align_ws_bytes(batch, max_T, row0, max_L);
    uint32_t* dbp = ws ? (uint32_t*)t.alloc(ws) : nullptr;
    HIP_CHECK(hipMemcpy(dem, ea.data(), ea.size() * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dplan, pp.plan.data(), sizeof(UttPlan) * batch, hipMemcpyHostToDevice));
    if (n_tgt) HIP_CHECK(hipMemcpy(dtgt, target_ids, n_tgt * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(doff, target_offsets, (size_t)(batch + 1) * 4, hipMemcpyHostToDevice));
    // the caller's arrays go up first, so that slots the kernel leaves alone come back as they were
    HIP_CHECK(hipMemcpy(dfirst, first_frame, out_bytes, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dlast, last_frame, out_bytes, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dtlp, token_logprob, out_bytes, hipMemcpyHostToDevice));
    launch_ctc_align(dem, ld_em, dplan, batch, row0, max_T, dtgt, doff, max_L, dbp, dfirst, dlast, dtlp, max_tokens, dpath, dlik, dstat, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(first_frame, dfirst, out_bytes, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(last_frame, dlast, out_bytes, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(token_logprob, dtlp, out_bytes, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(path_score, dpath, (size_t)batch * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(loglik, dlik, (size_t)batch * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(status, dstat, (size_t)batch * 4, hipMemcpyDeviceToHost));
  });
}

extern "C" int asr_op_cif_scan_timed(const float* alpha, const float* enc, int d, const int32_t* seq_lens, int batch, float tail_threshold,
                                     float* acoustic_out, int32_t* fire_frame_out, int max_tokens, int32_t* num_id_out) {
  return asr_guard([&] {
    ASR_REQUIRE(alpha && enc && seq_lens && acoustic_out && fire_frame_out && num_id_out && batch > 0 && d > 0 && max_tokens > 0, "op_cif_scan_timed: bad argument");
    asr_require_device(0);
    Tmp t;
    PackedPlan pp(seq_lens, batch);
    std::vector<float> aa, ea;
    to_aligned(pp, seq_lens, batch, 1, alpha, aa);
    to_aligned(pp, seq_lens, batch, d, enc, ea);
    const size_t fire_bytes = (size_t)batch * max_tokens * 4;
    float* dalpha = (float*)t.alloc((size_t)pp.Mpad * 4);
    float* denc = (float*)t.alloc((size_t)pp.Mpad * d * 4);
    float* dac = (float*)t.alloc((size_t)pp.Mpad * d * 4);
    UttPlan* dplan = (UttPlan*)t.alloc(sizeof(UttPlan) * batch);
    UttPlan* dtplan = (UttPlan*)t.alloc(sizeof(UttPlan) * batch);
    int32_t* dfire = (int32_t*)t.alloc(fire_bytes);
    int32_t* dnum = (int32_t*)t.alloc((size_t)batch * 4);
    HIP_CHECK(hipMemcpy(dalpha, aa.data(), (size_t)pp.Mpad * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(denc, ea.data(), (size_t)pp.Mpad * d * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dplan, pp.plan.data(), sizeof(UttPlan) * batch, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dfire, fire_frame_out, fire_bytes, hipMemcpyHostToDevice));      // slots the kernel leaves alone come back as they were
    launch_cif_scan_timed(dalpha, denc, d, dplan, batch, tail_threshold, dac, dtplan, dnum, dfire, max_tokens, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    std::vector<float> oa((size_t)pp.Mpad * d);
    HIP_CHECK(hipMemcpy(oa.data(), dac, oa.size() * 4, hipMemcpyDeviceToHost));
    from_aligned(pp, seq_lens, batch, d, oa, acoustic_out);
    HIP_CHECK(hipMemcpy(fire_frame_out, dfire, fire_bytes, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(num_id_out, dnum, (size_t)batch * 4, hipMemcpyDeviceToHost));
  });
}

extern "C" int asr_op_gemm_ln(const float* x, const float* w, const float* bias, const float* gamma, const float* beta, int M, int N,
                              int K, float* out) {
  return asr_guard([&] {
    ASR_REQUIRE(x && w && out && M >= 1 && M <= 64 && N % 16 == 0 && K % 256 == 0, "op_gemm_ln: bad argument");
    asr_require_device(0);
    Tmp t;
    float* dx = (float*)t.alloc((size_t)M * K * 4);
    HIP_CHECK(hipMemcpy(dx, x, (size_t)M * K * 4, hipMemcpyHostToDevice));
    void* dw = upload_operand(t, ASR_PRECISION_BF16, w, N, K, N, K);
    float *db = nullptr, *dg = nullptr, *dbe = nullptr;
    if (bias) { db = (float*)t.alloc((size_t)N * 4); HIP_CHECK(hipMemcpy(db, bias, (size_t)N * 4, hipMemcpyHostToDevice)); }
    if (gamma) {
      dg = (float*)t.alloc((size_t)K * 4); dbe = (float*)t.alloc((size_t)K * 4);
      HIP_CHECK(hipMemcpy(dg, gamma, (size_t)K * 4, hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(dbe, beta, (size_t)K * 4, hipMemcpyHostToDevice));
    }
    float* dout = (float*)t.alloc((size_t)M * N * 4);
    GemmArgs g;
    g.W = dw; g.ldw = K; g.M = M; g.N = N; g.K = K; g.bias = db; g.ln_x = dx; g.ld_ln_x = K; g.ln_gamma = dg; g.ln_beta = dbe;
    g.out_f32 = dout; g.ld_out_f32 = N;
    launch_gemm_bf16(g, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, dout, (size_t)M * N * 4, hipMemcpyDeviceToHost));
  });
}

extern "C" int asr_resample_table(int rate_in, int rate_model, int* L, int* M, int* W, float* coeffs) {
  return asr_guard([&] {
    ASR_REQUIRE(L && M && W, "resample_table: null argument");
    const ResampleDesign d = resample_design(rate_in, rate_model);
    *L = d.L; *M = d.M; *W = d.W;
    if (coeffs) resample_table(d, coeffs);
  });
}

extern "C" int asr_op_resample(const void* audio, const int64_t* offsets, int batch, int audio_dtype, int rate_in, int rate_model, int channels, int int16_scale,
                               float* out, int64_t out_cap, int64_t* offsets_out) {
  return asr_guard([&] {
    ASR_REQUIRE(audio && offsets && out && offsets_out && batch > 0, "op_resample: bad argument");
    ASR_REQUIRE(audio_dtype == ASR_AUDIO_F32 || audio_dtype == ASR_AUDIO_I16 || audio_dtype == ASR_AUDIO_F16, "op_resample: unknown audio dtype %d", audio_dtype);
    const ResampleDesign d = resample_design(rate_in, rate_model);
    int64_t total = 0;
    for (int b = 0; b < batch; ++b) {
      ASR_REQUIRE(offsets[b + 1] >= offsets[b], "op_resample: offsets decrease at utterance %d", b);
      total += resample_n_out(offsets[b + 1] - offsets[b], d);
    }
    ASR_REQUIRE(out_cap >= total, "op_resample: out holds %lld samples, the batch has %lld at the model rate", (long long)out_cap, (long long)total);
    asr_require_device(0);
    Resampler rs;                                        // (the session path's launcher on its own buffers, on the null stream)
    const float scale = audio_dtype == ASR_AUDIO_I16 && int16_scale ? 0x1p-15f : 1.0f;
    const float* dout = rs.run(audio, ASR_MEM_HOST, audio_dtype, rate_in, rate_model, channels, scale, offsets, batch, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    if (total) HIP_CHECK(hipMemcpy(out, dout, (size_t)total * 4, hipMemcpyDeviceToHost));
    memcpy(offsets_out, rs.offs.data(), (size_t)(batch + 1) * 8);
  });
}

extern "C" int asr_op_resample_stream(const void* audio, int audio_dtype, int rate_in, int rate_model, int channels, int int16_scale, int chunk, int n_streams, int n_steps,
                                      const int32_t* mode, float* out, int32_t* frames_out, int32_t* pitch_out) {
  return asr_guard([&] {
    ASR_REQUIRE(audio && mode && out && frames_out && pitch_out && chunk >= 1 && n_streams >= 1 && n_steps >= 1, "op_resample_stream: bad argument");
    ASR_REQUIRE(audio_dtype == ASR_AUDIO_F32 || audio_dtype == ASR_AUDIO_I16 || audio_dtype == ASR_AUDIO_F16, "op_resample_stream: unknown audio dtype %d", audio_dtype);
    ASR_REQUIRE(channels >= 1 && channels <= 8, "input format: %d channels (1..8)", channels);
    for (int i = 0; i < n_steps * n_streams; ++i) ASR_REQUIRE(mode[i] >= 0 && mode[i] <= 2, "op_resample_stream: mode %d (0, 1 or 2)", mode[i]);
    asr_require_device(0);
    Resampler rs;                                        // (the session path's table and launcher, on the null stream)
    const Resampler::Table& tb = rs.table(rate_in, rate_model, nullptr);
    const int pitch = resample_stream_pitch(tb.d, chunk), keep = resample_stream_keep(tb.d);
    *pitch_out = pitch;
    Tmp t;                                               // (zeroed: every stream starts reset)
    const size_t row_bytes = (size_t)pitch * channels * audio_elt_bytes(audio_dtype);
    int32_t* d_count = (int32_t*)t.alloc((size_t)n_streams * 4);
    float* d_hist = (float*)t.alloc((size_t)2 * n_streams * keep * 4);
    unsigned char* d_rows = (unsigned char*)t.alloc(row_bytes * n_streams);
    float* d_out = (float*)t.alloc((size_t)n_streams * chunk * 4);
    int32_t* d_sid = (int32_t*)t.alloc((size_t)n_streams * 4);
    int32_t* d_need = (int32_t*)t.alloc((size_t)n_streams * 4);
    std::vector<int32_t> sid, need;
    for (int k = 0; k < n_steps; ++k) {
      const int32_t* mk = mode + (size_t)k * n_streams;
      sid.clear();
      for (int u = 0; u < n_streams; ++u) {
        frames_out[(size_t)k * n_streams + u] = 0;
        if (mk[u] == 0) continue;
        if (mk[u] == 2) {                                // what asr_paraformer_stream_reset does to the stream's count and carried frames
          HIP_CHECK(hipMemset(d_count + u, 0, 4));
          for (int half = 0; half < 2 && keep > 0; ++half) HIP_CHECK(hipMemset(d_hist + ((size_t)half * n_streams + u) * keep, 0, (size_t)keep * 4));
        }
        HIP_CHECK(hipMemcpy(d_rows + row_bytes * sid.size(), static_cast<const unsigned char*>(audio) + row_bytes * ((size_t)k * n_streams + u), row_bytes,
                            hipMemcpyHostToDevice));
        sid.push_back(u);
      }
      const int n = (int)sid.size();
      if (n == 0) continue;
      HIP_CHECK(hipMemcpy(d_sid, sid.data(), (size_t)n * 4, hipMemcpyHostToDevice));
      ResampleStreamArgs a;
      a.audio = d_rows; a.sid = d_sid; a.sid_stride = 1; a.count = d_count; a.hist = d_hist; a.streams = n_streams; a.tab_t = tb.tab_t.as<float>(); a.out = d_out;
      a.need_out = d_need; a.d = tb.d; a.chunk = chunk; a.pitch = pitch; a.channels = channels;
      a.scale = audio_dtype == ASR_AUDIO_I16 && int16_scale ? 0x1p-15f : 1.0f; a.audio_dtype = audio_dtype;
      launch_resample_stream(a, n, nullptr);
      HIP_CHECK(hipDeviceSynchronize());
      need.resize(n);
      HIP_CHECK(hipMemcpy(need.data(), d_need, (size_t)n * 4, hipMemcpyDeviceToHost));
      for (int i = 0; i < n; ++i) {
        HIP_CHECK(hipMemcpy(out + ((size_t)k * n_streams + sid[i]) * chunk, d_out + (size_t)i * chunk, (size_t)chunk * 4, hipMemcpyDeviceToHost));
        frames_out[(size_t)k * n_streams + sid[i]] = need[i];
      }
    }
  });
}


static int vad_level_of(double a) { return vad_level((float)a); }

extern "C" int asr_vad_default_params(int rate, float full_scale, asr_vad_params* p) {
  return asr_guard([&] {
    ASR_REQUIRE(p, "vad_default_params: null argument");
    ASR_REQUIRE(rate >= 100, "vad: sample rate %d (at least 100 Hz)", rate);
    ASR_REQUIRE(full_scale > 0.f, "vad: full scale %g (positive)", (double)full_scale);
    memset(p, 0, sizeof(*p));
    p->p_floor = 0.10f; p->margin = 24; p->peak_drop = 16;
    const double amp = (double)full_scale * 1e-3;          // -60 dBFS
    p->abs_level = vad_level_of((double)vad_hop(rate) * amp * amp);
    p->min_speech = 10; p->min_pause = 50; p->pad = 10; p->max_frames = 3000;
  });
}

extern "C" int asr_op_vad(const void* audio, int mem, const int64_t* offsets, int batch, int audio_dtype, int rate, int channels, const asr_vad_params* params,
                          int64_t* seg_out, int64_t seg_cap, int32_t* seg_utt, int32_t* seg_count, float* energy_out, int32_t* level_out, int32_t* stats_out) {
  return asr_guard([&] {
    ASR_REQUIRE(audio && offsets && params && seg_count && batch > 0 && seg_cap >= 0 && (seg_out || seg_cap == 0), "op_vad: bad argument");
    ASR_REQUIRE(mem == ASR_MEM_HOST || mem == ASR_MEM_DEVICE, "op_vad: unknown memory kind %d", mem);
    ASR_REQUIRE(audio_dtype == ASR_AUDIO_F32 || audio_dtype == ASR_AUDIO_I16 || audio_dtype == ASR_AUDIO_F16, "op_vad: unknown audio dtype %d", audio_dtype);
    ASR_REQUIRE(rate >= 100, "vad: sample rate %d (at least 100 Hz)", rate);
    ASR_REQUIRE(channels >= 1 && channels <= 8, "vad: %d channels (1..8)", channels);
    ASR_REQUIRE(params->max_frames >= 2, "vad: max_frames %d (at least 2)", params->max_frames);
    ASR_REQUIRE(params->p_floor > 0.f && params->p_floor <= 1.f, "vad: p_floor %g (in (0, 1])", (double)params->p_floor);
    const int H = vad_hop(rate);
    // ---- host plan: per utterance its frames, F = ceil(n / H) and the floor's count; one (utterance, first frame) entry per stage-1 tile
    std::vector<VadUtt> hu((size_t)batch);
    std::vector<int32_t> tile_utt, tile_f0;
    int64_t total_F = 0;
    int max_F = 0;
    for (int b = 0; b < batch; ++b) {
      const int64_t n = offsets[b + 1] - offsets[b];
      ASR_REQUIRE(n >= 0 && n <= INT32_MAX, "op_vad: utterance %d has %lld frames", b, (long long)n);
      const int64_t F = (n + H - 1) / H;
      ASR_REQUIRE(F <= VAD_MAX_F, "vad: utterance %d has %lld analysis frames (at most %d, about 2.9 h)", b, (long long)F, VAD_MAX_F);
      VadUtt& u = hu[b];
      u.in_off = offsets[b] - offsets[0]; u.abs_off = offsets[b]; u.f_off = total_F; u.n = (int32_t)n; u.F = (int32_t)F; u.pad_ = 0;
      u.need = (int32_t)std::min<int64_t>(F, std::max<int64_t>(1, (int64_t)std::ceil((double)params->p_floor * (double)F)));
      for (int f0 = 0; f0 < F; f0 += VAD_TILE_F) { tile_utt.push_back(b); tile_f0.push_back(f0); }
      total_F += F;
      max_F = std::max(max_F, (int)F);
    }
    asr_require_device(0);
    Tmp t;
    const size_t frame_bytes = (size_t)channels * audio_elt_bytes(audio_dtype), in_bytes = (size_t)(offsets[batch] - offsets[0]) * frame_bytes;
    const void* src = static_cast<const unsigned char*>(audio) + (size_t)offsets[0] * frame_bytes;
    if (mem == ASR_MEM_HOST) {
      void* d_in = nullptr;                                // (no memset of a buffer the copy fills)
      HIP_CHECK(hipMalloc(&d_in, std::max<size_t>(in_bytes, 256)));
      t.ptrs.push_back(d_in);
      if (in_bytes) HIP_CHECK(hipMemcpy(d_in, src, in_bytes, hipMemcpyHostToDevice));
      src = d_in;
    }
    const size_t n_tiles = tile_utt.size(), nF = (size_t)std::max<int64_t>(total_F, 1);
    VadUtt* d_utt = (VadUtt*)t.alloc(sizeof(VadUtt) * batch);
    int32_t* d_tile_utt = (int32_t*)t.alloc(4 * std::max<size_t>(n_tiles, 1));
    int32_t* d_tile_f0 = (int32_t*)t.alloc(4 * std::max<size_t>(n_tiles, 1));
    HIP_CHECK(hipMemcpy(d_utt, hu.data(), sizeof(VadUtt) * batch, hipMemcpyHostToDevice));
    if (n_tiles) {
      HIP_CHECK(hipMemcpy(d_tile_utt, tile_utt.data(), 4 * n_tiles, hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(d_tile_f0, tile_f0.data(), 4 * n_tiles, hipMemcpyHostToDevice));
    }
    const size_t cap = (size_t)std::min<int64_t>(seg_cap, total_F);      // (an utterance has at most F segments)
    VadArgs a{};
    a.audio = src; a.utt = d_utt; a.tile_utt = d_tile_utt; a.tile_f0 = d_tile_f0;
    a.energy = (float*)t.alloc(4 * nF); a.level = (int32_t*)t.alloc(4 * nF); a.hist = (int32_t*)t.alloc((size_t)batch * VAD_LEVELS * 4);
    a.seg_tmp = (int32_t*)t.alloc(8 * nF); a.seg_count = (int32_t*)t.alloc((size_t)batch * 4); a.stats = (int32_t*)t.alloc((size_t)batch * 12);
    a.seg_out = (int64_t*)t.alloc(16 * std::max<size_t>(cap, 1)); a.seg_utt = (int32_t*)t.alloc(4 * std::max<size_t>(cap, 1)); a.seg_cap = (int64_t)cap;
    a.r = VadRules{params->margin, params->peak_drop, params->abs_level, params->min_speech, params->min_pause, params->pad, params->max_frames};
    a.H = H; a.channels = channels; a.batch = batch; a.max_F = max_F; a.audio_dtype = audio_dtype;
    launch_vad(a, (int)n_tiles, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(seg_count, a.seg_count, (size_t)batch * 4, hipMemcpyDeviceToHost));
    int64_t total = 0;
    for (int b = 0; b < batch; ++b) total += seg_count[b];
    const size_t n_out = (size_t)std::min<int64_t>(total, (int64_t)cap);
    if (n_out) {
      HIP_CHECK(hipMemcpy(seg_out, a.seg_out, n_out * 16, hipMemcpyDeviceToHost));
      if (seg_utt) HIP_CHECK(hipMemcpy(seg_utt, a.seg_utt, n_out * 4, hipMemcpyDeviceToHost));
    }
    if (energy_out && total_F) HIP_CHECK(hipMemcpy(energy_out, a.energy, (size_t)total_F * 4, hipMemcpyDeviceToHost));
    if (level_out && total_F) HIP_CHECK(hipMemcpy(level_out, a.level, (size_t)total_F * 4, hipMemcpyDeviceToHost));
    if (stats_out) HIP_CHECK(hipMemcpy(stats_out, a.stats, (size_t)batch * 12, hipMemcpyDeviceToHost));
  });
}
