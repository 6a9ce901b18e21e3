// The session's audio sample types as the kernels that read raw audio see them (the fbank kernels of kernels.hip, the resampler of resample.hip).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

// S is the session's audio sample type (asr_audio_dtype): float as is; int16_t raw PCM, widened at the load and -- for the Whisper / Qwen front end, whose
// reference folds 1/32768 into the STFT window (Whisper/STFT_Process.py:143) -- scaled by 2^-15, which is exact and commutes with every later f32 rounding;
// _Float16 widened as is. Loads are per lane and per sample (2-byte aligned only: utterances start at any sample offset). The load loop keeps the RAW samples
// (one register each) and the store loop widens them; hold() between the two keeps the compiler from moving the conversion up to its load, where it would put a
// wait behind every load (the round trip per sample that the load shape exists to avoid). The float instantiation has no hold and no conversion.
// After the LDS store nothing differs.
template <typename S> struct Pcm;
template <> struct Pcm<float> {
  typedef float raw_t;
  static __device__ __forceinline__ raw_t load(const float* p, int i) { return p[i]; }
  static __device__ __forceinline__ raw_t hold(raw_t r) { return r; }
  static __device__ __forceinline__ float widen(raw_t r, float) { return r; }
};
template <> struct Pcm<int16_t> {
  typedef int raw_t;                       // sign-extended by the load
  static __device__ __forceinline__ raw_t load(const int16_t* p, int i) { return p[i]; }
  static __device__ __forceinline__ raw_t hold(raw_t r) { asm volatile("" : "+v"(r)); return r; }
  static __device__ __forceinline__ float widen(raw_t r, float scale) { return (float)r * scale; }
};
template <> struct Pcm<_Float16> {
  typedef uint32_t raw_t;                  // the half's bits
  static __device__ __forceinline__ raw_t load(const _Float16* p, int i) { return reinterpret_cast<const uint16_t*>(p)[i]; }
  static __device__ __forceinline__ raw_t hold(raw_t r) { asm volatile("" : "+v"(r)); return r; }
  static __device__ __forceinline__ float widen(raw_t r, float) { return (float)__builtin_bit_cast(_Float16, (uint16_t)r); }
};
