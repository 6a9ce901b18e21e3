/* asr_mi355x.h -- C ABI of the MI355X-native ASR hot path (libasr_mi355x.so).
 *
 * This library replaces what the reference executes behind
 *   onnxruntime.InferenceSession.run_with_iobinding(binding, run_options)
 * (process->native boundary: SenseVoice/Inference_SenseVoice_ONNX.py:303,
 *  Whisper/Inference_Whisper_ONNX.py:247-248,640), i.e. the arithmetic that
 * Export_*.py freezes into the .onnx graphs: in-graph STFT/FBank front-end,
 * encoder, and CTC / autoregressive decoder. The reference has no native code of
 * its own; its FFI for this path is the onnxruntime Python binding, so the
 * reference-side stub that binds these symbols is a ctypes shim exposing the
 * onnxruntime API subset the Inference_*_ONNX.py scripts use.
 *
 * Conventions
 *  - plain pointers and sizes only; no C++/torch types cross this boundary;
 *  - every function returns ASR_OK (0) or an error code; asr_last_error() returns a
 *    thread-local message (the Python shim raises it, mirroring ORT's exceptions;
 *    nothing is swallowed);
 *  - a session owns one HIP stream (or borrows the caller's, asr_session_set_stream)
 *    and is re-entrant per session; runs are synchronous: outputs are complete when the
 *    call returns (RunOptions "disable_synchronize_execution_providers"="0",
 *    SenseVoice/Inference_SenseVoice_ONNX.py:142-147);
 *  - there is NO CPU fallback: every entry point fails with ASR_ERR_NO_DEVICE when no
 *    gfx950 device is visible.
 */
#ifndef ASR_MI355X_H
#define ASR_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASR_ABI_VERSION 1

enum asr_status {
  ASR_STATUS_OK = 0,
  ASR_STATUS_INVALID = 1,
  ASR_STATUS_HIP = 2,
  ASR_STATUS_NOT_FOUND = 3,
  ASR_STATUS_UNSUPPORTED = 4,
  ASR_STATUS_NO_DEVICE = 5
};

/* Arithmetic mode. BF16: bf16 MFMA operands, f32 accumulate, f32 residual stream / LayerNorm /
 * soft-max / front-end. F32: exact-f32 MFMA everywhere (verification mode for the
 * "logits within 1e-3" parity bar). The weight arena must be built for the same mode.
 *
 * FP8W (opt-in, Whisper and Qwen3-ASR sessions; the low-bit counterpart of the reference's quantised decoders, Whisper/Optimize_ONNX.py:81-96,
 * Optimize_ONNX_Common.py:27,55-60, README.md:70 q4f32): bf16 mode whose decoder projection weights (Whisper: and the cross-K/V cache) are stored as
 * OCP e4m3 bytes with power-of-two scales (per output column / per (sequence, head) slab) and widened to bf16 in registers -- activations, accumulation,
 * self-KV cache, encoder and vocabulary projection are unchanged. Takes a bf16 arena; quantisation happens at session creation. Qwen3-ASR: the four
 * projections of every decoder layer (q|k|v, o, gate|up, down); decode steps of <= 64 rows stream the bytes, every other pass (prefill, wider beam steps)
 * reads their exact bf16 dequantisation, so all passes of a session see the same effective weights. Needs d_model, d_ffn and heads x head_dim multiples of 256.
 *
 * FP8MM (opt-in, Whisper sessions only): FP8W plus the encoder's feed-forward pair on the FP8 MATRIX pipe -- fc1 / fc2 weights as e4m3 bytes with one
 * power-of-two scale per output column, their activation operands as e4m3 bytes: the second LayerNorm's output at unit scale (its affine pair is folded
 * into fc1, so |value| <= sqrt(d_model) < 448), the GELU output as value * 2^-shift (asr_whisper_set_fp8_act_shift, default 0) saturating at 448 -- every
 * element that meets the clamp is counted (asr_whisper_fp8_stats): a count that moves says the shift is too small for this checkpoint --, products on v_mfma_scale_f32_16x16x128_f8f6f4 at unit block scales with f32 accumulation; attention, the other projections,
 * the residual stream and the decoder are FP8W's. Needs d_model and d_ffn multiples of 256. The reference's counterpart: its MatMulNBits /
 * dynamic-int8 graphs (Optimize_ONNX_Common.py:55-60).
 *
 * MXFP4W (opt-in, Whisper and Qwen3-ASR sessions; round 6): FP8W with the decoder projection weights stored as OCP MXFP4 instead of e4m3 -- e2m1 elements, two per byte,
 * one e8m0 scale per 32 consecutive input channels (4.25 bits per weight; the 4-bit counterpart of the reference's MatMulNBits Q4 graphs, README.md:70 q4f32).
 * The block of the format is the K-step of the bf16 MFMA, so a decode-step fragment is widened -- exactly: 2 significant bits x a power of two -- by
 * v_cvt_scalef32_pk_bf16_fp4 with its block's scale; every other pass reads the exact bf16 dequantisation. Whisper's cross-K/V cache is FP8W's; Qwen3-ASR: the four
 * projections of every decoder layer (the reference's own headline for this family is a 4-bit decoder, README.md:70 q4f32). */
enum asr_precision { ASR_PRECISION_BF16 = 0, ASR_PRECISION_F32 = 1, ASR_PRECISION_FP8W = 2, ASR_PRECISION_FP8MM = 3, ASR_PRECISION_MXFP4W = 4 };

enum asr_mem { ASR_MEM_HOST = 0, ASR_MEM_DEVICE = 1 };

/* Sample type of the `audio` argument of every entry that takes audio (asr_sensevoice_run, asr_paraformer_run, asr_paraformer_stream_step,
 * asr_whisper_encode, asr_qwen_prefill, asr_qwen_align). The reference fixes it per exported graph (INPUT_AUDIO_DTYPE = "INT16" | "F32" | "F16"), so here
 * it is a property of the session (asr_session_set_audio_dtype, default F32). What a value means follows the family's export:
 *   SenseVoice / Paraformer / streaming Paraformer (SenseVoice/Export_SenseVoice.py:21,275,368; Paraformer/Non-Streaming/Export_Paraformer.py:88,359,594;
 *     Paraformer/Streaming/Export_Paraformer_Streaming.py:21,316,596): I16 = raw PCM used as is (audio.float()); F32 / F16 = int16-RANGE values;
 *   Whisper / Qwen3-ASR / ForcedAligner (Whisper/Export_Whisper.py:43,367,423,735,741; Qwen_ASR/Export_Qwen_ASR.py:80,710-731,854,1596): I16 = raw PCM, the
 *     1/32768 that the export folds into the STFT window (STFT_Process.py:143) is applied at the load; F32 / F16 = values already in [-1, 1].
 * Widening int16 / f16 to f32 is exact and 2^-15 commutes with every f32 rounding, so an I16 call equals the F32 call on the widened (and, for the second
 * group, scaled) samples bit for bit. audio_offsets always count samples (frames of interleaved samples once asr_session_set_input_format has set another
 * format); a 2-byte utterance needs 2-byte alignment only. */
enum asr_audio_dtype { ASR_AUDIO_F32 = 0, ASR_AUDIO_I16 = 1, ASR_AUDIO_F16 = 2 };

typedef struct asr_session asr_session;

int asr_abi_version(void);
const char* asr_last_error(void);
int asr_device_count(int* count);

/* Foreign kernels on a GPU this library computes on -- the RCCL collectives of the data-parallel path (weight-arena broadcast, hypothesis
 * gather; the reference has no counterpart, its runtime is one onnxruntime session per process) or any other kernel the host program launches itself.
 * The SANM block / tile kernels and the fused streaming step need every workgroup of their grid resident at once; a foreign kernel holding a few CUs can
 * split a cluster (the launch then gives up after a bounded spin and the batch is redone cluster-free). So bracket foreign work:
 *   asr_device_foreign_begin(dev)  blocks until no cluster pass is in flight on `dev`; until the matching _end every compute call on `dev` takes its
 *                                  cluster-free path (same results; the call never waits, so the two sides cannot deadlock);
 *   asr_device_foreign_end(dev)    after the foreign kernels have FINISHED on the device (synchronise their stream first).
 * Sections nest (a count per device, process-wide). _stats: out4 = {sections opened, cluster passes diverted to the cluster-free path, sections that had
 * to wait for a cluster pass, cluster passes admitted}. dist.py brackets every torch.distributed collective on a CUDA device with this pair. */
int asr_device_foreign_begin(int device_id);
int asr_device_foreign_end(int device_id);
int asr_device_foreign_stats(int device_id, int64_t* out4);

/* ------------------------------------------------------------------ SenseVoice (non-AR, CTC)
 * Replaces SenseVoiceSmall.onnx == SENSE_VOICE.forward (SenseVoice/Export_SenseVoice.py:271-296).
 * Graph I/O it mirrors (Export_SenseVoice.py:375-379): audio (1,1,audio_len) f32 int16-range,
 * language_idx (1,) i32  ->  token_ids (num_token,) i32, num_id (1,) i32.
 * Extension over the batch-1 reference: B independent utterances per call, ragged lengths. */
typedef struct asr_sensevoice_config {
  int32_t sample_rate, n_mels, nfft, win_length, hop_length;
  int32_t lfr_m, lfr_n;
  int32_t d_model, n_heads, d_head, d_ffn;
  int32_t n_blocks;       /* total SANM blocks (encoders0 + encoders + tp_encoders) */
  int32_t n_main;         /* blocks before after_norm (encoders0 + encoders)          */
  int32_t fsmn_kernel;
  int32_t vocab, blank_id;
  int32_t n_prompt;       /* prompt rows prepended to the speech rows (1 language + 3 system) */
  int32_t n_languages;    /* rows of the language embedding table */
  int32_t max_audio_len;
  int32_t reserved[8];
} asr_sensevoice_config;

/* `arena` is the flat weight arena built by arena.py (manifest + tensors). With
 * ASR_MEM_HOST it is copied to HBM; with ASR_MEM_DEVICE the pointer is borrowed and must outlive
 * the session (same ownership rule as SessionOptions.add_initializer,
 * Whisper/Inference_Whisper_ONNX.py:242-243) -- used after the RCCL weight broadcast. */
int asr_sensevoice_create(const asr_sensevoice_config* cfg, const void* arena, size_t arena_bytes, int arena_mem,
                          int device_id, int precision, asr_session** out);

/* audio: packed samples of the session's asr_audio_dtype -- F32 / F16: int16-range values; I16: raw PCM used as is (Export_SenseVoice.py:275,368);
 * utterance b spans samples [audio_offsets[b], audio_offsets[b+1]).
 * language_idx: B selector indices (host). token_ids_out: host [B][max_tokens] (row b holds num_id_out[b]
 * ids, rest untouched); num_id_out: host [B]. Fails if any utterance is shorter than one frame. */
int asr_sensevoice_run(asr_session* s, const void* audio, int audio_mem, const int64_t* audio_offsets, int batch,
                       const int32_t* language_idx, int32_t* token_ids_out, int max_tokens, int32_t* num_id_out);
/* The same forward pass with a time span and a confidence per token (no reference counterpart: the reference graph returns ids only). The CTC head also
 * yields log soft-max at the arg-max of every row (frame log-probability); the collapse keeps, for the token emitted on the last row of its run of equal
 * ids, first_frame_out = the first row of that run (runs do not wrap), last_frame_out = that last row, logprob_out = the mean frame log-probability over
 * first..last (<= 0). Rows are indices into the utterance's sequence, the n_prompt prompt rows included: row j >= n_prompt covers samples
 * [(j - n_prompt) lfr_n hop_length, (j - n_prompt + 1) lfr_n hop_length). The three arrays are host [B][max_tokens] with the row contract of token_ids_out.
 * Token ids and counts equal asr_sensevoice_run's. */
int asr_sensevoice_run_timed(asr_session* s, const void* audio, int audio_mem, const int64_t* audio_offsets, int batch,
                             const int32_t* language_idx, int32_t* token_ids_out, int max_tokens, int32_t* num_id_out,
                             int32_t* first_frame_out, int32_t* last_frame_out, float* logprob_out);

/* CTC prefix beam search instead of the frame-wise arg-max (no reference counterpart). The forward pass is asr_sensevoice_run's up to the head;
 * per row the `topk` (1..16) best tokens and their log soft-max are taken without storing the logits, and a standard (not circular) prefix beam search of width
 * `beam` (1..16) runs over every utterance's rows, prompt rows included. The `nbest` (1..beam) best hypotheses come back best first: token_ids_out host
 * [B][nbest][max_tokens] (each row holds min(num, max_tokens) ids, rest untouched), num_id_out [B][nbest] (the full length), score_out [B][nbest] = the
 * hypothesis' CTC log-probability over the candidates plus its hotword bonus, ctc_score_out [B][nbest] = without the bonus. Hypotheses beyond the number
 * found have num 0 and score -inf. Scores tie-break to the earlier entry of the documented enumeration; two calls on the same input return the same bytes.
 * With a language model set (asr_sensevoice_set_lm) the search ranks by CTC + bonus + LM and score_out includes the LM term (alpha * log P + beta per token,
 * alpha * log P(</s>) at the end when the model lists it); ctc_score_out stays the CTC figure. */
int asr_sensevoice_run_beam(asr_session* s, const void* audio, int audio_mem, const int64_t* audio_offsets, int batch,
                            const int32_t* language_idx, int beam, int topk, int nbest, int32_t* token_ids_out, int max_tokens,
                            int32_t* num_id_out, float* score_out, float* ctc_score_out);
/* Hotwords of asr_sensevoice_run_beam: n_phrases token-id lists, phrase p = ids[offsets[p] .. offsets[p + 1]) (host). A hypothesis gains `boost` per token
 * while it spells a phrase; a partial match that breaks off, or is still open at the end of the utterance, gives its part back. n_phrases == 0 clears the
 * list. Ids outside the vocabulary, empty phrases and phrases containing the blank id are rejected (the list in force stays). */
int asr_sensevoice_set_hotwords(asr_session* s, const int32_t* ids, const int32_t* offsets, int n_phrases, float boost);
/* Back-off n-gram language model of asr_sensevoice_run_beam, fused into the search (shallow fusion). image_words (host): one blob of n_words 32-bit
 * words over token ids, order N in 1..5 --
 *   [order, n_nodes, n_edges, vocab, start_node, eos_edge_token]
 *   depth i32 [n_nodes], backoff f32 [n_nodes], suffix i32 [n_nodes], child_off i32 [n_nodes + 1], tok i32 [n_edges], logp f32 [n_edges], next i32 [n_edges],
 *   uni i32 [vocab + 2]
 * Nodes are the contexts (node 0 the empty one, every listed n-gram of order 1..N-1 a node of that depth; suffix = its longest proper suffix that is a node);
 * edges [child_off[n], child_off[n + 1]) are node n's listed continuations sorted by token, logp / backoff natural logs, next = the node of the longest suffix
 * of the full n-gram that is a node. uni[c] is the root's edge for token c or -1; </s> and <s> take the ids vocab and vocab + 1. start_node is next of the <s>
 * unigram (0 without one), eos_edge_token is vocab when </s> is listed, else -1. A token without a unigram is out of vocabulary: it costs oov_logprob and
 * leaves the state alone. Every appended token adds alpha * log P(token | state) + beta to the hypothesis' ranking score.
 * n_words == 0 clears the model. The image is checked on the host before it replaces the one in force: sizes against n_words, vocab against the session's,
 * monotone offsets, children strictly sorted and none on the blank id, suffix links to smaller depths, next in range, logp finite and <= 0, backoff finite,
 * oov_logprob finite and <= 0, alpha finite and >= 0, beta finite. A rejected image leaves the previous one in force. */
int asr_sensevoice_set_lm(asr_session* s, const int32_t* image_words, int64_t n_words, float alpha, float beta, float oov_logprob);
/* CTC forced alignment of transcripts the caller supplies (no reference counterpart: the reference graph returns its own greedy ids and no times; DESIGN
 * 4.3c). The forward pass is asr_sensevoice_run's up to the head; per row the log soft-max at the blank and at the utterance's target columns is taken without
 * storing the logits, and a Viterbi and a forward trellis run over every utterance's speech rows (rows >= n_prompt). Targets are ragged: utterance b's are
 * target_ids[target_offsets[b] .. target_offsets[b + 1]) (host; target_offsets[0] = 0, at most 1023 per utterance, none is legal: the path is all blank).
 * Ids outside [0, vocab), the blank id and decreasing offsets are rejected. first_frame_out / last_frame_out / token_logprob_out are host arrays in the layout
 * of target_ids: the rows of the target's span on the best path, in the row convention of asr_sensevoice_run_timed, and the mean over the span of log soft-max
 * at the target. Ties go to the smaller move (stay, then one state, then two) and, at the end, to the last target over the final blank. path_score_out [B] =
 * the best path's log-probability, loglik_out [B] = the transcript's log-likelihood (all paths), status_out [B] = 0 aligned, 1 no alignment exists (fewer
 * speech rows than targets plus adjacent equal targets): the utterance's spans then keep the caller's fill, both scores are -inf, and the call succeeds. */
int asr_sensevoice_align(asr_session* s, const void* audio, int audio_mem, const int64_t* audio_offsets, int batch, const int32_t* language_idx,
                         const int32_t* target_ids, const int32_t* target_offsets, int32_t* first_frame_out, int32_t* last_frame_out,
                         float* token_logprob_out, float* path_score_out, float* loglik_out, int32_t* status_out);

/* sequence length (prompt + LFR rows) the graph produces for an utterance of n_samples */
int asr_sensevoice_seq_len(const asr_sensevoice_config* cfg, int n_samples, int* seq_len);
/* Counters of a SenseVoice / Paraformer session's cluster kernels: out8 = {forward passes redone cluster-free because a cluster gave up, batches left on the
 * cluster-free path after the last give-up, passes that took the cluster-free path because a foreign section was open (asr_device_foreign_begin),
 * block kernel enabled, 0, 0, 0, 0}. */
int asr_sanm_stats(asr_session* s, int32_t* out8);

/* ------------------------------------------------------------------ Paraformer (non-streaming, CIF + NAR decoder)
 * Replaces Paraformer.onnx == PARAFORMER.forward (Paraformer/Non-Streaming/Export_Paraformer.py:474-563).
 * Graph I/O it mirrors (:600-606): audio (1,1,audio_len) f32 int16-range -> token_ids (1,num_token) i32, num_id (1,) i32. */
typedef struct asr_paraformer_config {
  int32_t sample_rate, n_mels, nfft, win_length, hop_length, lfr_m, lfr_n;
  int32_t d_model, n_heads, d_head, d_ffn, n_blocks, fsmn_kernel;
  int32_t n_dec, n_dec3, d_dec_ffn, cif_kernel, vocab, max_audio_len;
  float tail_threshold;
  int32_t reserved[8];
} asr_paraformer_config;

int asr_paraformer_create(const asr_paraformer_config* cfg, const void* arena, size_t arena_bytes, int arena_mem, int device_id,
                          int precision, asr_session** out);
/* same calling convention as asr_sensevoice_run, the audio types included (Export_Paraformer.py:88,359,594), no language input: token_ids_out host [B][max_tokens], num_id_out host [B]
 * (num_id is the CIF fire count; an utterance can legitimately yield zero tokens). */
int asr_paraformer_run(asr_session* s, const void* audio, int audio_mem, const int64_t* audio_offsets, int batch,
                       int32_t* token_ids_out, int max_tokens, int32_t* num_id_out);
/* The same forward pass with the row at which the CIF predictor fired each token and the token's log-probability (no reference counterpart: the reference
 * graph returns ids only, Export_Paraformer.py:600-606). Fire rule (:505-507): the alphas of the utterance's T rows, then the tail threshold as row T, are
 * summed in float64; after each row the running sum is rounded ONCE to f32 and floored, and a token fires at the row t where that floor rises.
 * fire_frame_out[b][k] = t of token k, in [0, T] and strictly increasing; t == T means the tail threshold fired the token behind the last row (the value is
 * kept: the caller clips). Rows are the utterance's LFR rows, there are no prompt rows: row j covers samples [j lfr_n hop_length, (j + 1) lfr_n hop_length).
 * logprob_out[b][k] = natural-log soft-max of the decoder head's logits row of token k at its arg-max (<= 0). Both arrays are host [B][max_tokens] with the
 * row contract of token_ids_out (row b holds min(num_id_out[b], max_tokens) entries, the rest untouched). Token ids and counts equal asr_paraformer_run's. */
int asr_paraformer_run_timed(asr_session* s, const void* audio, int audio_mem, const int64_t* audio_offsets, int batch,
                             int32_t* token_ids_out, int max_tokens, int32_t* num_id_out, int32_t* fire_frame_out, float* logprob_out);

/* The same forward pass with a beam search over the decoder's token rows in place of the per-row arg-max (no reference counterpart). Per token
 * row the `topk` (1..16) best tokens and their log soft-max are taken from the head without storing the logits. Every hypothesis picks one candidate per row,
 * so all hypotheses of utterance b have its CIF fire count N_b as their length: there is no blank, no collapse and no merging. A hypothesis ranks by the sum
 * of its candidates' log-probabilities + its hotword bonus (asr_paraformer_set_hotwords) + its language-model term (asr_paraformer_set_lm: alpha * log P(token |
 * history) + beta per token, alpha * log P(</s> | history) at the end when the model lists </s>); `beam` (1..16) hypotheses stay live from row to row, ties go
 * to the earlier entry of the enumeration (live hypothesis in rank order, then candidate column), and the `nbest` (1..beam) best come back, best first.
 * token_ids_out host [B][nbest][max_tokens] and num_id_out host [B][nbest] follow the row contract of asr_sensevoice_run_beam; score_out [B][nbest] is
 * acoustic + bonus + LM, am_score_out [B][nbest] the acoustic sum alone. Hypotheses beyond the number found (early rows offer fewer than `beam`) have num 0 and
 * both scores -inf; an utterance without tokens yields one empty hypothesis of score 0 (+ the </s> term) and am_score 0. fire_frame_out (nullable, host
 * [B][max_tokens]) holds the CIF fire rows of asr_paraformer_run_timed, N_b entries in row b: every hypothesis of the utterance shares them. token_logprob_out
 * (nullable, host [B][nbest][max_tokens]) holds each hypothesis' per-token log soft-max, rows as token_ids_out. Without hotwords and without a model,
 * hypothesis 0 holds asr_paraformer_run's ids. Two calls on the same input return the same bytes. */
int asr_paraformer_run_beam(asr_session* s, const void* audio, int audio_mem, const int64_t* audio_offsets, int batch, int beam, int topk, int nbest,
                            int32_t* token_ids_out, int max_tokens, int32_t* num_id_out, float* score_out, float* am_score_out, int32_t* fire_frame_out,
                            float* token_logprob_out);
/* Hotwords and language model of asr_paraformer_run_beam: arguments, rules and rejections as asr_sensevoice_set_hotwords / asr_sensevoice_set_lm, except that
 * this family has no blank id -- every id in [0, vocab) is legal in a phrase or an image. A rejected list or image leaves the one in force. Offline sessions
 * only: a streaming chunk step commits its tokens when it returns. */
int asr_paraformer_set_hotwords(asr_session* s, const int32_t* ids, const int32_t* offsets, int n_phrases, float boost);
int asr_paraformer_set_lm(asr_session* s, const int32_t* image_words, int64_t n_words, float alpha, float beta, float oov_logprob);

/* Streaming Paraformer: replaces Paraformer_Streaming_Encoder.onnx + Paraformer_Streaming_Decoder.onnx (PARAFORMER_ENCODER /
 * PARAFORMER_DECODER, Paraformer/Streaming/Export_Paraformer_Streaming.py:330-553) and the state shuttling of
 * Inference_Paraformer_Streaming_ONNX.py:309-449. The 100 in_en_key/value tensors, in_previous_mel_features, in_cif_hidden,
 * in_cif_alphas, start_idx, in_de_fsmn / in_de_key / in_de_value of a stream live in HBM inside the session, indexed by a
 * stream id in [0, max_streams); one step advances n_streams DIFFERENT streams by one chunk_samples-sample chunk each
 * (audio: [n_streams][chunk_samples] of the session's asr_audio_dtype, int16-range values or raw PCM: Export_Paraformer_Streaming.py:21,316,596) and runs the decoder for the streams whose CIF fired -- streams
 * without a fired frame keep their decoder state, exactly like the host loop (:420-447). token_ids_out: host
 * [n_streams][max_tokens] (max_tokens >= LFR rows per chunk + 1), num_id_out: host [n_streams]. The arena is the
 * non-streaming Paraformer arena built for streaming (position table up to MAX_CONTINUE_STREAMING, causal decoder FSMN). */
int asr_paraformer_stream_create(const asr_paraformer_config* cfg, const void* arena, size_t arena_bytes, int arena_mem, int device_id,
                                 int precision, int chunk_samples, int look_back_encoder, int look_back_decoder, int max_streams,
                                 asr_session** out);
int asr_paraformer_stream_reset(asr_session* s, int stream_id);      /* -1 = every stream: empty histories, zero CIF state, no carried input frames, step count 0 */
/* Per listed stream the frames its next step reads; *pitch_out: the row pitch in frames. Default format: chunk_samples and chunk_samples. */
int asr_paraformer_stream_input_frames(asr_session* s, const int32_t* stream_ids, int n_streams, int32_t* frames_out, int32_t* pitch_out);
int asr_paraformer_stream_step(asr_session* s, const void* audio, int audio_mem, const int32_t* stream_ids, int n_streams,
                               int32_t* token_ids_out, int max_tokens, int32_t* num_id_out);
/* The same step with the integration step at which each token fired and the token's log-probability (the build's own mode, as asr_paraformer_run_timed).
 * A step integrates B rows -- the C rows carried from the previous chunk, then the first B - C of its B new rows (B, C = LFR rows per chunk and its half:
 * 9 and 4 at the reference's chunk; Export_Paraformer_Streaming.py:398-399, 447-458) -- in f32, firing where the carried weight plus the row's alpha reaches 1.
 * fire_step_out[i][k] = that step t in [0, B), or -1 for a token fired in front of the loop because the weight carried in had already reached 1 (:440-446):
 * it belongs to the previous chunk's last integrated row. For the stream's c-th chunk since its reset (c = 0, 1, ..) step t is the absolute LFR row
 * c B + t - C of the stream (negative for the zero rows in front of the first chunk); absolute row j covers samples [j lfr_n hop_length, (j + 1) lfr_n hop_length)
 * up to the front end's window centring. logprob_out[i][k] = natural-log soft-max of the token's logits row at its arg-max. Both arrays are host
 * [n_streams][max_tokens], row i holds num_id_out[i] entries, the rest untouched. Ids and counts equal asr_paraformer_stream_step's; the two forms may be mixed
 * freely on one session. */
int asr_paraformer_stream_step_timed(asr_session* s, const void* audio, int audio_mem, const int32_t* stream_ids, int n_streams,
                                     int32_t* token_ids_out, int max_tokens, int32_t* num_id_out, int32_t* fire_step_out, float* logprob_out);
/* Beam search for the streaming session, with hotwords and an n-gram language model: the build's own mode (the reference graph returns the per-row arg-max;
 * Export_Paraformer_Streaming.py). The search of asr_paraformer_run_beam cannot keep hypotheses open across chunk steps whose tokens are final when they
 * return, so this one carries its state per stream and per hypothesis in HBM and commits with a fixed lag: a stream holds at most pend_cap uncommitted
 * tokens; before a further token row is searched the oldest of them is committed with the token of the best live hypothesis, and the hypotheses that
 * disagree there are dropped. A committed token is final and never revised; the pending tokens are reported as pending. The result depends on the sequence
 * of a stream's token rows, not on how the chunks cut it; a stream of at most pend_cap tokens followed by a finish is the offline search bit for bit.
 * set_beam switches the mode on (beam 1..16, topk 1..8, nbest 1..beam, pend_cap 1..64; the search state of every stream is allocated and cleared) or, with
 * beam = 0, off (the state is freed). This entry, the hotword list and the language model -- the build's own too, taken and checked as
 * asr_paraformer_set_hotwords / asr_paraformer_set_lm take theirs, which keep refusing a streaming session -- fail while any stream holds search history
 * (tokens searched since its last finish or reset): the carried trie nodes and model states belong to the list and the image in force. */
int asr_paraformer_stream_set_beam(asr_session* s, int beam, int topk, int nbest, int pend_cap);
int asr_paraformer_stream_set_hotwords(asr_session* s, const int32_t* ids, const int32_t* offsets, int n_phrases, float boost);
int asr_paraformer_stream_set_lm(asr_session* s, const int32_t* image_words, int64_t n_words, float alpha, float beta, float oov_logprob);
/* asr_paraformer_stream_step_timed (same arguments, same outputs, bit for bit), then the topk candidates of the step's token rows and the search (the build's
 * own mode). Per stream i of the call, host arrays: commit_ids_out / commit_logprob_out [n_streams][pend_cap + max_tokens] and commit_num_out [n_streams]: the
 * tokens this step committed, with their log-probabilities; pend_ids_out / pend_logprob_out [n_streams][nbest][pend_cap] and pend_num_out / pend_score_out /
 * pend_am_out [n_streams][nbest]: the uncommitted tails of the best nbest live hypotheses, best first (score = acoustic + hotword bonus + lm and am = the sum
 * of the picked log-probabilities since the stream's search was cleared, both without the end terms; hypotheses beyond the live ones: num 0, both scores
 * -inf); total_out [n_streams]: the token rows searched since the clear. Rows hold their counts' worth of entries, the rest is untouched. The greedy ids of
 * the step are not the search's tokens: a caller shows the committed tokens followed by the best pending tail. The step costs a second synchronisation. */
int asr_paraformer_stream_step_beam(asr_session* s, const void* audio, int audio_mem, const int32_t* stream_ids, int n_streams, int32_t* token_ids_out,
                                    int max_tokens, int32_t* num_id_out, int32_t* fire_step_out, float* logprob_out, int32_t* commit_ids_out,
                                    float* commit_logprob_out, int32_t* commit_num_out, int32_t* pend_ids_out, float* pend_logprob_out, int32_t* pend_num_out,
                                    float* pend_score_out, float* pend_am_out, int32_t* total_out);
/* The end of the named streams' searches (the build's own mode); takes no audio. The end terms of asr_paraformer_run_beam -- an open phrase gives its bonus
 * back, a model that lists </s> adds alpha log P(</s> | state) -- the hypotheses ranked again, the best nbest tails with their final scores in the pend_*
 * arrays, the best one's tail committed (commit_* arrays [n_streams][pend_cap]) and the search state cleared. The acoustic state stays the caller's to
 * asr_paraformer_stream_reset (which clears the stream's search state too). A stream that was never stepped gives the one empty hypothesis. */
int asr_paraformer_stream_finish_beam(asr_session* s, const int32_t* stream_ids, int n_streams, int32_t* commit_ids_out, float* commit_logprob_out,
                                      int32_t* commit_num_out, int32_t* pend_ids_out, float* pend_logprob_out, int32_t* pend_num_out, float* pend_score_out,
                                      float* pend_am_out, int32_t* total_out);
/* Which path the chunk steps of a streaming session took (no reference counterpart: the reference runs one stream per InferenceSession and has no
 * co-tenancy to manage). A bf16 step runs the encoder / decoder layer loops as two cluster launches when (i) no more than fused_max streams are active,
 * (ii) no other session of this process is computing on the same GPU (otherwise the per-launch path, which leaves CUs to the other tenant and waits on nobody);
 * when other sessions merely exist on the GPU the step first snapshots the active streams' recurrent state, so that a cluster launch that gave up is restored and
 * redone on the per-launch path instead of costing the streams their history. out8 = {give-ups recovered, steps that took the per-launch path because the GPU
 * was shared, snapshots taken, fused_max, steps left of the per-launch cool-down after a give-up, 1 if the session can fuse at all, 0, 0}. */
int asr_paraformer_stream_stats(asr_session* s, int32_t* out8);

/* ------------------------------------------------------------------ Whisper (encoder + KV-cache decoder)
 * Replaces the merged graphs Whisper_ProbePrefillGreedy / Whisper_PrefillGreedy / Whisper_DecodeGreedy
 * (Whisper/Shared_Merged.py:864-888; I/O planner Whisper/Inference_Whisper_ONNX.py:323-392), i.e.
 * STFT_Process + WHISPER_ENCODER.forward (Export_Whisper.py:422-447), WHISPER_DECODER_EMBED / _PREFILL / _DECODE /
 * WHISPER_DECODER.forward (:450-497,614-667) and the BEGIN_SUPPRESS / ARGMAX heads (:228-260).
 * The reference passes 2 x n_layers self-KV and 2 x n_layers cross-KV tensors through Python on every call; here
 * they are session state: `encode` fills the cross-KV slabs, `prefill` resets and fills the self-KV cache (paged: 16-position
 * pages from a per-session pool behind a block table that grows with the sequences; ASR_KV_PAGED=0 keeps contiguous extents), `decode`
 * appends one position in place. Batch B = independent utterances (the reference is batch 1). */
typedef struct asr_whisper_config {
  int32_t sample_rate, n_mels, nfft, hop_length;
  int32_t d_model, n_heads, d_head, d_ffn, n_enc_layers, n_dec_layers;
  int32_t vocab, max_source_positions, max_target_positions, max_audio_len;
  int32_t gelu_tanh;      /* 0 = erf GELU as exported (:428); 1 = tanh GELU, what ORT runs with
                             optimization.enable_gelu_approximation=1 (Inference_Whisper_ONNX.py:166) */
  int32_t reserved[9];
} asr_whisper_config;

int asr_whisper_create(const asr_whisper_config* cfg, const void* arena, size_t arena_bytes, int arena_mem, int device_id,
                       int precision, asr_session** out);
/* audio: packed samples of the session's asr_audio_dtype -- F32 / F16 in [-1, 1] (audio_pcm_scale 32768, Export_Whisper.py:1068), I16 raw PCM scaled by
 * 2^-15 at the load (Export_Whisper.py:43,367,423; STFT_Process.py:143); n_positions_out (host, B,
 * nullable) receives the encoder length (n_samples / 160 + 1) / 2 of each utterance. */
int asr_whisper_encode(asr_session* s, const void* audio, int audio_mem, const int64_t* audio_offsets, int batch,
                       int32_t* n_positions_out);
/* ids: host [B][n] prompt tokens (n <= 8), history is reset to 0 like the reference's prefill. next_ids_out (host B,
 * nullable): arg-max(logits + begin_suppress); logits_out (host [B][vocab], nullable): raw logits incl. the -128
 * suppress penalty -- what language detection and NO_SPEECH_DETECTION read (Inference_Whisper_ONNX.py:780-805). */
int asr_whisper_prefill(asr_session* s, const int32_t* ids, int n, int32_t* next_ids_out, float* logits_out);
/* prefill with one text prompt per sequence -- OpenAI Whisper's initial_prompt / condition_on_previous_text ([<|startofprev|>, previous text ...,
 * <|startoftranscript|>, language, task, ...]; decoding.py:_get_initial_tokens). The reference always decodes [SOT, language, task, <|notimestamps|>], so this
 * is the build's own mode; the truth for parity is oracle/whisper_oracle.py (WhisperOracle.decoder / .greedy take a prompt of any length per utterance).
 * ids: host, sequence b's prompt = ids[offsets[b] .. offsets[b+1]) (1 .. max_target_positions ids each), offsets: host [B + 1], ascending. Outputs and head
 * behaviour are those of asr_whisper_prefill (BEGIN_SUPPRESS, penalty, sampler, timestamp rules, token scores, hotwords: the hotword node starts at the
 * root, prompt ids do not move it). Equal lengths of at most 8 ids forward to asr_whisper_prefill and give identical results. Otherwise the batch is
 * prefilled as n = max(len) slots per sequence, sequence b left-padded by n - len[b] slots (slot s is position s - pad; the keys of the pad slots do not
 * exist for it), so the session keeps one history counter and asr_whisper_decode / _generate / _beam_search / _token_scores / _align and word-timestamp
 * capture work as after a prefill, with n as the prompt length: the LONGEST prompt bounds the whole batch -- n + new positions <= max_target_positions
 * (asr_whisper_beam_search refuses more, asr_whisper_generate stops there). F32 and BF16 sessions; FP8W / FP8MM / MXFP4W sessions refuse ragged lengths
 * and prompts of more than 8 ids (their cross-K/V slabs are e4m3, the prompt-attention kernel reads bf16 / f32 slabs). Errors: a prompt of 0 ids or of more
 * than max_target_positions, offsets that do not ascend, an id outside the vocabulary. */
int asr_whisper_prefill_prompts(asr_session* s, const int32_t* ids, const int32_t* offsets, int32_t* next_ids_out, float* logits_out);
/* one position per sequence. ids: host [B], or NULL to feed the device-resident arg-max of the previous step (no
 * host round trip); next_ids_out / logits_out nullable (NULL, NULL => fully asynchronous step). */
int asr_whisper_decode(asr_session* s, const int32_t* ids, int32_t* next_ids_out, float* logits_out);
/* greedy continuation after a prefill: tokens_out host [B][max_new], n_out host [B]; stops per sequence at eos_id
 * (not emitted) -- the loop of _decode_tokens (Inference_Whisper_ONNX.py:584-663); the head is the one selected by
 * asr_whisper_set_penalty (plain arg-max by default). */
int asr_whisper_generate(asr_session* s, int max_new, int eos_id, int32_t* tokens_out, int32_t* n_out);
/* beam search after asr_whisper_prefill (the reference has no Whisper beam search; the rule is this build's own, the one written down in
 * oracle/qwen_asr_oracle.py:beam_search_core, stop set {eos_id}; eos_id < 0: no stop id): width-`beam` (1..8) search over summed log-soft-max scores of
 * the logits the greedy head sees (the -128 suppress penalty included; the first ranking adds BEGIN_SUPPRESS, as the arg-max after a prefill does), no
 * length normalisation. A hypothesis ends at eos_id (not emitted) and then stands with its score; an utterance is finished when its best hypothesis has
 * ended or after max_new ids. Every step is one decoder pass over the B * beam hypothesis rows: self-K/V in per-row extents of prompt + max_new - 1
 * positions followed through each row's ancestry (device memory: layers x rows x 2 x d_model x slots x element size -- large-v3 bf16, 32 x 30 s at
 * width 5 with 444 new ids: 11.7 GB, kept for the next search), cross-attention reading each utterance's slabs once for all of its rows. Host outputs,
 * hypotheses best-first: tokens_out [B][beam][max_new], n_out [B][beam], scores_out [B][beam] (nullable). Errors: not right after a prefill ("prefill
 * first"), width outside 1..8, a repeat penalty or sampling head set ("do not combine"; asr_whisper_set_timestamps does combine), prompt + max_new > max_target_positions. The session's greedy
 * state (pages, block table, history, ids, logits) is left as the prefill left it: asr_whisper_generate afterwards continues the same prefill. */
int asr_whisper_beam_search(asr_session* s, int beam, int max_new, int eos_id, int32_t* tokens_out, int32_t* n_out, float* scores_out);
/* decode head: repeat_penalty == 1 => ARGMAX (Export_Whisper.py:254-260); otherwise penalty-greedy = APPLY_PENALTY (:312-325)
 * + GREEDY_SEARCH (:243-251): the logits of the last penalty_range generated ids (1..64) are multiplied by repeat_penalty
 * once penalty_range ids exist (REPEAT_PENALTY / PENALTY_RANGE, Inference_Whisper_ONNX.py:78-79,630-632). The id history is kept
 * on the device and restarts at every prefill. Applies to prefill / decode / generate; logits_out then holds the
 * penalised logits. */
int asr_whisper_set_penalty(asr_session* s, float repeat_penalty, int penalty_range);
/* FP8MM sessions: the GELU operand of fc2 is stored as value * 2^-shift (0 .. 16; also ASR_FP8MM_ACT_SHIFT at creation); takes effect at the next encode.
 * asr_whisper_fp8_stats: stats[0] = activation elements that met the e4m3 clamp (|value * 2^-shift| > 448, or NaN) since the session was created,
 * stats[1] = the shift in use. Zero / the shift on sessions of other precisions. No reference counterpart (its low-bit graphs quantise activations
 * dynamically per tensor, Optimize_ONNX_Common.py:55-60); here the scale is static and the counter is what makes a wrong one loud. */
int asr_whisper_set_fp8_act_shift(asr_session* s, int shift);
int asr_whisper_fp8_stats(asr_session* s, uint64_t stats[2]);

/* The *PenaltyGreedy graphs run GREEDY_SEARCH (:243-251) on every step, so save_id grows even while the host still feeds
 * penalty_penalty_value = 1.0 (before PENALTY_RANGE ids exist, Inference_Whisper_ONNX.py:630-632): enable = 1 keeps appending the
 * picks to the device-side history whatever the penalty value is (the onnxruntime shim drives the value per step). */
int asr_whisper_track_history(asr_session* s, int enable);
/* NO_SPEECH_DETECTION head (Export_Whisper.py:334-348; graph Whisper_No_Speech_Detection.onnx, host :799-805) on the logits of the last
 * prefill (the probe with [SOT]): prob_out host [B] = softmax(logits + 128 on the permanently suppressed ids)[no_speech_id]. */
int asr_whisper_no_speech_prob(asr_session* s, int no_speech_id, float* prob_out);
/* decode head TOPK_TOPP_SAMPLING (Export_Whisper.py:263-308; USE_SAMPLING / TEMPERATURE / TOP_K / TOP_P /
 * SAMPLING_REPETITION_PENALTY, Inference_Whisper_ONNX.py:71-75): repetition penalty over every previously sampled id,
 * temperature, top-k (1..64), top-p, Gumbel-max. enable = 0 returns to the arg-max / penalty-greedy head. The reference draws
 * torch.rand_like inside the graph; here the uniforms come from a counter-based generator keyed by (seed, step, sequence, rank)
 * -- reproducible run to run, but a different stream than torch's. */
int asr_whisper_set_sampling(asr_session* s, int enable, float temperature, int top_k, float top_p, float repetition_penalty,
                             uint64_t seed);
/* parity hook: the uniforms of the NEXT prefill / decode step, host [batch][top_k] (count = batch * top_k); consumed once. */
int asr_whisper_set_sampling_noise(asr_session* s, const float* uniforms, int count);
/* Token scores: the log-probability of every pick of the arg-max, penalty-greedy and sampling heads (the beam search keeps its hypothesis score). The
 * reference reports none; the definition is the build's own, after OpenAI Whisper's `logprobs`: the natural-log soft-max, at the picked id, of the f32 logits
 * row as the selection sees it over the vocabulary -- after the repeat penalty, the timestamp rules and the sampler's repetition penalty, plus BEGIN_SUPPRESS
 * on the prefill step; temperature, top-k and top-p are not part of it. It is the log-soft-max of what logits_out of that step holds (+ BEGIN_SUPPRESS after a
 * prefill). Logits are finite or -inf (masks); a row that holds +inf or NaN is outside the contract. A -inf column has zero weight; a pick whose own column is -inf, or a row without a column above -inf, scores -inf; never NaN. With enable != 0
 * every pick also joins the device-side id history (as in timestamp mode), and the greedy pick and its score come out of one kernel; with enable = 0 no step
 * launches anything new. Switch it before the prefill whose picks are wanted.
 * asr_whisper_token_scores drains the stream and copies the scores of the picks since the last prefill, oldest first (column 0: the prefill's pick), to
 * logprob_out host [batch][out_stride] -- min(count, out_stride) per sequence, slots past the count keep the caller's fill; *n_out = count. It works after
 * asr_whisper_generate (count = 1 + decode steps run: the stop pick and whatever a finished sequence picked while others went on are included) and after
 * hand-driven prefill / decode loops. Errors: the mode is off, or no prefill has run since it was switched on. */
int asr_whisper_set_token_scores(asr_session* s, int enable);
/* Hotword boosting of the decoder (the build's own mode, the reference has none): n_phrases token-id lists, phrase p = ids[offsets[p] ..
 * offsets[p + 1]) (host), in the shape of asr_sensevoice_set_hotwords and with its context graph. Every sequence (in asr_whisper_beam_search every hypothesis)
 * carries a node of the graph that follows its own picks -- the root after a prefill; prompt tokens and ids the host feeds to asr_whisper_decode do not move it.
 * A token that continues the match gains `boost`; the node returns to the root when a phrase ends (the bonus stays); a token that breaks a partial match of
 * depth d gives d * boost back, and the root's child is tried by the same rule. No fail links: a phrase that continues another complete phrase is unreachable.
 * Selection head (arg-max, penalty-greedy, sampler): before every selection the logits row is biased in place -- children of the node + (d + 1) * boost, the
 * root's other children + boost -- after the repeat penalty and before the timestamp rules; that is the bonus change plus the row constant d * boost, which
 * no selection and no log-soft-max sees. logits_out of a step shows the biased row, and a token score (asr_whisper_set_token_scores) is the log-soft-max of
 * the biased row. Every pick joins the device-side id history, as in timestamp mode. Beam search: a hypothesis score is log-soft-max(model)(c) + the bonus
 * change of c, the refund included; scores_out reports these sums. A stop id picked inside a partial match pays the refund; a hypothesis cut off at max_new
 * keeps the bonus of a match still open. The mode combines with the penalty, the sampler, the timestamp rules, token scores and beam search; word-timestamp
 * capture and asr_whisper_align are unaffected. n_phrases == 0 clears the list: no step launches anything new and results are what they were without the mode.
 * Every call returns all nodes to the root. Ids outside the vocabulary, empty phrases and a boost that is not finite are rejected (the list in force stays).
 * Set the list before the prefill; asr_whisper_beam_search refuses a list that changed between the prefill and the search. */
int asr_whisper_set_hotwords(asr_session* s, const int32_t* ids, const int32_t* offsets, int n_phrases, float boost);
/* Back-off n-gram language model fused into the decoder's selection (shallow fusion; the build's own mode). image_words / n_words / alpha / beta /
 * oov_logprob as asr_sensevoice_set_lm takes them, the image checked the same way against the session's vocabulary (this family has no blank id); a null image
 * or n_words == 0 clears the model. Every sequence (in asr_whisper_beam_search every hypothesis) carries a state of the model that follows its own picks from
 * start_node after a prefill; prompt tokens and ids the host feeds to asr_whisper_decode do not move it. The LM term of a token is alpha * log P(token | state)
 * + beta; a token without a unigram (timestamps, specials) costs oov_logprob and keeps the state; one of the n_end_ids (at most 8, inside the vocabulary)
 * end_ids costs alpha * log P(</s> | state) when the image lists </s>, no beta, and keeps the state. Only the `topk` (1..32) best columns of the row the
 * selection sees -- after the penalty, the hotword bias, the timestamp rules and BEGIN_SUPPRESS, by value then id -- are candidates (a -inf column never is):
 * the arg-max, penalty-greedy, timestamp and token-score heads pick the candidate with the largest logit + LM term (ties to the lower id); a token score stays
 * the model's log-soft-max of the row at the pick. The sampling head ignores the model. asr_whisper_beam_search ranks a row's extensions by log-soft-max +
 * hotword bonus change + LM term over the topk columns and the hotword columns, scores_out includes the LM terms, and topk below the beam width is refused
 * there. Setting or clearing returns every state to start_node. A refused call leaves the model in force. */
int asr_whisper_set_lm(asr_session* s, const int32_t* image_words, int64_t n_words, float alpha, float beta, float oov_logprob, int topk,
                       const int32_t* end_ids, int n_end_ids);
int asr_whisper_token_scores(asr_session* s, float* logprob_out, int out_stride, int32_t* n_out);
/* Segment timestamps: OpenAI Whisper's ApplyTimestampRules inside the decode head. The reference has no timestamp mode (it defines NO_TIMESTAMPS_TOKEN and
 * always puts it in the prompt), so -- like the beam search -- this mode is the build's own. With enable != 0 the prompt carries no <|notimestamps|> and,
 * before every selection (arg-max, penalty-greedy after its penalty, sampling, every ranking of asr_whisper_beam_search), the f32 logits row of a sequence
 * with h generated ids since the prefill is masked with -inf, in this order. Columns: [0, eot_id) text, eot_id, (eot_id, timestamp_begin_id) specials,
 * [timestamp_begin_id, vocab) timestamps; timestamp_begin_id = no_timestamps_id + 1 in every released vocabulary.
 *   1. no_timestamps_id.
 *   2. last_ts = h >= 1 and id[h-1] >= timestamp_begin_id; penult_ts = h < 2 or id[h-2] >= timestamp_begin_id. After a pair (last_ts and penult_ts) all
 *      timestamps: text follows. After a lone timestamp (last_ts and not penult_ts) [0, eot_id): the segment closes or the stream ends.
 *   3. m = the largest generated id >= timestamp_begin_id, if any: [timestamp_begin_id, m + 1) -- after a lone timestamp [timestamp_begin_id, m): the next
 *      segment may open where the last one closed, every other timestamp is strictly later (no segment of zero length).
 *   4. h == 0: [0, timestamp_begin_id), and with max_initial_index >= 0 also (timestamp_begin_id + max_initial_index, vocab). -1: no limit.
 *   5. Over the columns left, L = log-sum-exp of the timestamps and T = max of [0, timestamp_begin_id): if L > T, [0, timestamp_begin_id) (OpenAI's comparison of
 *      log-probabilities; the soft-max normaliser is common to both sides. An empty side counts as -inf).
 * Every pick is appended to the device-side history, which restarts at a prefill: a prefill in this mode selects by rule 4, so switch the mode off for the
 * [SOT] probe that asr_whisper_no_speech_prob and the language detection read. logits_out of prefill / decode then holds the masked logits, as it holds
 * the penalised ones under asr_whisper_set_penalty; beam scores are log-soft-max values of the masked rows, as OpenAI's are. Ids are checked:
 * 0 <= eot_id < no_timestamps_id < timestamp_begin_id < vocab. enable = 0 ignores the other arguments; no kernel is added to any step then. */
int asr_whisper_set_timestamps(asr_session* s, int enable, int timestamp_begin_id, int no_timestamps_id, int eot_id, int max_initial_index);
/* Token / word timestamps: OpenAI Whisper's cross-attention DTW (openai-whisper timing.py). Like the beam search and the timestamp rules this is the build's own
 * mode: the reference always decodes behind <|notimestamps|> and aligns nothing. With enable != 0 the last position of every prefill and the position of every
 * single-token decode step (host-fed or fed from the device inside the captured graph) write one row of raw cross-attention scores q . k -- f32 accumulate, no
 * extra scale: the folded projections carry it -- of every selected (layer, head) pair over all encoder positions of the sequence, into session memory
 * f32 [B][n_pairs][max_rows][ld], ld >= the longest encoder length (B * n_pairs * max_rows * ld * 4 bytes: 32 x 10 x 225 x 1504 x 4 = 0.43 GB). Row index =
 * position - (prompt length - 1); rows >= max_rows are not written. The scores are taken against the bf16 (f32 sessions: f32) cross-K slabs in every precision
 * mode, FP8W / FP8MM / MXFP4W included. layer_head_pairs: host [n_pairs][2], in range, distinct, 1 <= n_pairs <= n_dec_layers * n_heads; 1 <= max_rows <=
 * max_target_positions. While the mode is on asr_whisper_beam_search is refused (align a hypothesis with a forced pass over its ids: prefill + host-fed decode
 * steps) and a decode step takes one position. enable = 0 ignores the other arguments; no kernel is added to any step then. */
int asr_whisper_set_word_timestamps(asr_session* s, int enable, const int32_t* layer_head_pairs, int n_pairs, int max_rows);
/* The alignment of the rows captured since the last prefill, four launches on the session's stream: soft-max over the first n_frames[b] scores of each row
 * (crop, then soft-max, in place); mean and population variance over the n_rows[b] rows per (pair, frame) -- a column of variance 0 standardises to 0, where
 * OpenAI divides by zero --; median filter of medfilt_width (odd, 1..9; OpenAI: 7) along frames with reflect padding (skipped when n_frames <= width / 2), mean
 * over the pairs, negated; DTW with OpenAI's recurrence and tie rule in f32. n_rows[b] (host): 0 = skip, else 2 .. rows captured -- the text tokens plus one:
 * the row of the <|notimestamps|> input predicts the first text token, the row of the last text token predicts eot. n_frames[b]: 1 .. encoder length of b, the
 * part of the window that holds audio (OpenAI's num_frames / 2). token_frames_out host [B][out_stride]: for r < n_rows[b] the first encoder frame (0.02 s each)
 * of row r on the path, OpenAI's jump_times before the division. One align per capture: the soft-max is in place. */
int asr_whisper_align(asr_session* s, const int32_t* n_rows, const int32_t* n_frames, int medfilt_width, int32_t* token_frames_out, int out_stride);
/* Tests / debugging: what = 0 the captured scores of utterance b, f32 [n_pairs][rows captured][encoder length of b] (after an align the aligned part holds the
 * soft-max); what = 1 its cost matrix of the last align, f32 [1][n_rows[b]][n_frames[b]]. shape_out (host [3], nullable) receives the extents: the number of
 * rows captured is the session's knowledge (asr_whisper_generate decides how many steps run), so a caller asks for it -- host_out NULL reports the extents
 * only -- before it sizes host_out; else bytes must be their product times 4. */
int asr_whisper_align_read(asr_session* s, int what, int b, void* host_out, size_t bytes, int32_t* shape_out);

/* ------------------------------------------------------------------ Qwen3-ASR (audio encoder + Qwen3 decoder with KV cache)
 * Replaces the merged graphs Qwen_ASR prefill_greedy / decode_greedy and the Embed graph (Qwen_ASR/Shared_Merged.py; I/O planner
 * Qwen_ASR/Inference_Qwen_ASR_ONNX.py:330-366), i.e. STFT_Process + QWEN3_ASR_ENCODER.forward (Export_Qwen_ASR.py:850-927),
 * CONCAT_EMBED (:1428-1435), ROTARY_MASK_PREFILL / _DECODE (:933-1028), DECODER_MAIN.forward (:1265-1336) and the ARGMAX head.
 * The reference hands 2 x n_layers KV tensors through Python per token (Inference_Qwen_ASR_ONNX.py:700-712); here the cache is
 * session state appended in place, and the prompt embeddings (query_embed / language_tail_embed inputs) are gathered on the
 * device from token ids. Batch B = independent utterances with their own prompts (the reference is batch 1). */
typedef struct asr_qwen_config {
  int32_t sample_rate, n_mels, nfft, hop_length;
  int32_t enc_d, enc_heads, enc_ffn, n_enc_layers, conv_channels, n_window, n_window_infer, max_source_positions;
  int32_t d_model, n_heads, n_kv_heads, d_head, d_ffn, n_layers, vocab, max_seq_len, max_audio_len;
  float rms_eps, rope_theta;
  /* 0: Qwen3-ASR (vocabulary LM head). > 0: Qwen3-ForcedAligner -- dec.lm_head holds classify_num timestamp-bucket rows (padded to a
   * multiple of 128, like the vocabulary), Qwen_ForcedAligner/Export_Qwen_ForcedAligner.py:531-586; the session then serves
   * asr_qwen_align only. */
  int32_t classify_num;
  int32_t reserved[8];
} asr_qwen_config;

int asr_qwen_create(const asr_qwen_config* cfg, const void* arena, size_t arena_bytes, int arena_mem, int device_id, int precision,
                    asr_session** out);
/* One call = the reference's prefill launch (:640-668): audio encoding, prompt assembly, rotary / causal mask, decoder prefill,
 * first-token selection. Sequence b's prompt is [pre_ids[pre_offsets[b] : pre_offsets[b+1]] | audio embeddings of utterance b |
 * post_ids[post_offsets[b] : post_offsets[b+1]]] -- pre = head + query + suffix ids, post = tail (+ language tail) ids
 * (:923-927, CONCAT_EMBED). next_ids_out (host B, nullable) = arg-max of the last position; logits_out (host [B][vocab],
 * nullable); ids_len_out (host B, nullable) = prompt length = the reference's kv_seq_len output (:672). Resets the KV cache.
 * audio: the session's asr_audio_dtype with Whisper's meaning (Export_Qwen_ASR.py:80,710-731,854,1596): F32 / F16 in [-1, 1], I16 raw PCM x 2^-15. */
int asr_qwen_prefill(asr_session* s, const void* audio, int audio_mem, const int64_t* audio_offsets, int batch, const int32_t* pre_ids,
                     const int32_t* pre_offsets, const int32_t* post_ids, const int32_t* post_offsets, int32_t* next_ids_out, float* logits_out,
                     int32_t* ids_len_out);
/* one position per sequence (Embed + decode_greedy, :690-716). ids: host [B], or NULL to feed the device-resident arg-max of the
 * previous call; next_ids_out / logits_out nullable (ids NULL and both outputs NULL => asynchronous step). */
int asr_qwen_decode(asr_session* s, const int32_t* ids, int32_t* next_ids_out, float* logits_out);
/* decode heads (strategy selection Inference_Qwen_ASR_ONNX.py:369-376; graphs Shared_Merged.py merge_prefill_* / merge_decode_*):
 * repeat_penalty == 1 => ARGMAX (Export_Qwen_ASR.py:1418-1420); otherwise penalty-greedy = APPLY_PENALTY (:1403-1415, the logits of
 * save_id[:, -penalty_range:] -- fewer ids while the history is shorter -- multiplied by repeat_penalty, decode steps only) +
 * GREEDY_SEARCH (:1342-1345). set_sampling selects TOPK_TOPP_SAMPLING (:1348-1400) for prefill and decode, with the counter-based
 * uniforms of asr_whisper_set_sampling; set_sampling_noise supplies the next step's uniforms [batch][top_k] (parity hook). The id
 * history lives on the device and restarts at every prefill. */
int asr_qwen_set_penalty(asr_session* s, float repeat_penalty, int penalty_range);
int asr_qwen_track_history(asr_session* s, int enable);   /* like asr_whisper_track_history: the *_Penalty_Greedy graphs append every pick */
int asr_qwen_set_sampling(asr_session* s, int enable, float temperature, int top_k, float top_p, float repetition_penalty, uint64_t seed);
int asr_qwen_set_sampling_noise(asr_session* s, const float* uniforms, int count);
/* token scores, as asr_whisper_set_token_scores / asr_whisper_token_scores (no bias on the prefill step here) */
int asr_qwen_set_token_scores(asr_session* s, int enable);
/* hotword boosting, as asr_whisper_set_hotwords (no timestamp rules here; in asr_qwen_beam_search every hypothesis carries its node) */
int asr_qwen_set_hotwords(asr_session* s, const int32_t* ids, const int32_t* offsets, int n_phrases, float boost);
/* n-gram language model fusion, as asr_whisper_set_lm (no timestamp rules or BEGIN_SUPPRESS here; a forced-aligner session refuses the call) */
int asr_qwen_set_lm(asr_session* s, const int32_t* image_words, int64_t n_words, float alpha, float beta, float oov_logprob, int topk, const int32_t* end_ids,
                    int n_end_ids);
int asr_qwen_token_scores(asr_session* s, float* logprob_out, int out_stride, int32_t* n_out);
/* continuation after a prefill with the selected head (:687-745): tokens_out host [B][max_new], n_out host [B]; a sequence ends at
 * the first id in stop_ids (not emitted) or when the cache is full. */
int asr_qwen_generate(asr_session* s, int max_new, const int32_t* stop_ids, int n_stop, int32_t* tokens_out, int32_t* n_out);
/* The session's KV cache (Qwen_ASR/Export_Qwen_ASR.py:1265-1336 keeps `in_key_i / in_value_i` tensors of the whole history per sequence; the north-star's paged
 * cache): 16-position pages behind one block table for all layers, a free list on the host -- a sequence holds pages for the positions it has, and a sequence that
 * asr_qwen_generate finished gives its pages back while its neighbours go on. out4 = {1 if paged (0: extents of max_seq_len positions, ASR_QWEN_KV_PAGED=0),
 * pages in the pool, pages held by sequences now, high-water mark of pages in use since the last prefill}. */
int asr_qwen_kv_stats(asr_session* s, int32_t* out4);
/* beam search after a prefill (the README's "greedy / beam search" for Qwen3-ASR, README.md:38; the reference ships no code for it, the
 * semantics are written down in oracle/qwen_asr_oracle.py:beam_search_core): width-`beam` (1..8) search over summed log-soft-max scores,
 * no length normalisation. A hypothesis ends at the first id in stop_ids (not emitted) and then stands with its score; an utterance is
 * finished when its best hypothesis has ended (no live one can overtake it: log-probabilities are <= 0) or after max_new ids. Every
 * step is one decoder pass over all B * beam rows; the KV cache is never re-ordered (the attention kernel follows each row's
 * ancestry). Host outputs, hypotheses best-first: tokens_out [B][beam][max_new], n_out [B][beam], scores_out [B][beam] (nullable).
 * Plain arg-max head only (no penalty / sampling). The session's greedy state (asr_qwen_decode / _generate) is left untouched. */
int asr_qwen_beam_search(asr_session* s, int beam, int max_new, const int32_t* stop_ids, int n_stop, int32_t* tokens_out, int32_t* n_out,
                         float* scores_out);

/* Forced alignment (aligner sessions only, classify_num > 0): the reference's one non-autoregressive pass of the merged
 * ForcedAligner graph (Qwen_ForcedAligner/Inference_Qwen_ForcedAligner_ONNX.py:540-575) = FORCED_ALIGNER_ENCODER (Export_Qwen_ForcedAligner.py:678-836,
 * the Qwen3-ASR audio path) + FORCED_ALIGNER_EMBED (:843) + FORCED_ALIGNER_ROTARY_MASK (:855-880, the f16-rounded cos / sin table lives
 * in the arena) + FORCED_ALIGNER_DECODER_MAIN (:921-1110) whose final RMSNorm -> classify head -> arg-max (:1104-1109) runs on the
 * selected rows only. Prompts as in asr_qwen_prefill: sequence b = [pre | audio embeddings | post] (the reference: pre = <|audio_start|>,
 * post = <|audio_end|> + the word / <timestamp> ids). Rows selected on the device: positions whose prompt id == timestamp_id, or
 * every position when timestamp_id < 0 (the graph's output_ids (1, L)). Host outputs, packed utterance-major in position order:
 * slot_offsets_out [B + 1] (utterance b's rows are [off[b], off[b+1])), buckets_out [buckets_cap >= off[B]] = arg-max bucket per row,
 * logits_out [off[B]][classify_num] (nullable), ids_len_out [B] (nullable). The KV cache is written as in a prefill, and nothing reads it.
 * audio: as in asr_qwen_prefill (the aligner shares the Qwen3-ASR audio path and its INPUT_AUDIO_DTYPE, Export_Qwen_ASR.py:80,710-731). */
int asr_qwen_align(asr_session* s, const void* audio, int audio_mem, const int64_t* audio_offsets, int batch, const int32_t* pre_ids,
                   const int32_t* pre_offsets, const int32_t* post_ids, const int32_t* post_offsets, int32_t timestamp_id, int32_t* slot_offsets_out,
                   int32_t* buckets_out, int64_t buckets_cap, float* logits_out, int32_t* ids_len_out);

/* ------------------------------------------------------------------ device buffers
 * Backing store of the shim's OrtValue (OrtValue.ortvalue_from_numpy / update_inplace / numpy,
 * SenseVoice/Inference_SenseVoice_ONNX.py:280-299): update_inplace is an H2D copy into the same
 * allocation, numpy() a blocking D2H copy. kind: 0 = host->device, 1 = device->host, 2 = device->device. */
int asr_mem_alloc(int device_id, size_t bytes, void** out);
int asr_mem_free(int device_id, void* ptr);
int asr_mem_copy(int device_id, void* dst, const void* src, size_t bytes, int kind);

/* ------------------------------------------------------------------ session utilities */
int asr_session_destroy(asr_session* s);
int asr_session_set_stream(asr_session* s, void* hip_stream);       /* borrow a caller stream (e.g. torch's) */
int asr_session_device(asr_session* s, int* device_id);
/* asr_audio_dtype of the session's audio entries (default ASR_AUDIO_F32). May be set between any two compute calls; the step graphs that hold the front
 * end are keyed by it. INVALID for a null session or an unknown value. */
int asr_session_set_audio_dtype(asr_session* s, int audio_dtype);
int asr_session_audio_dtype(asr_session* s, int* audio_dtype_out);
/* Sample rate (Hz) and interleaved channel count of the session's audio entries; the default is the model's own rate (the config's sample_rate) and one channel,
 * and with it nothing changes and nothing is launched. With any other format every audio entry's `audio` and `audio_offsets` count FRAMES -- one frame is
 * `channels` interleaved samples of the session's audio dtype, host or device memory alike -- and the library turns them into model-rate mono f32 on the device in
 * front of the front end: channel mean, then a polyphase Kaiser-windowed sinc (cutoff 0.945 of the narrower Nyquist; the table is asr_resample_table's). An
 * utterance of n frames becomes ceil(n * rate_model / sample_rate) samples, and frame counts, length limits (max_audio_len) and result frames all refer to those.
 * This is the build's own mode (the reference resamples on the host with audioop, no low-pass): sample parity with the reference holds for the default format only.
 * May be set between any two compute calls. INVALID (the format in force stays) for a null session, a rate < 1, channels outside 1..8, rates whose reduced ratio
 * needs more than 1024 filter phases (16001 Hz), or a rate beyond ~40 x the model's.
 *
 * The streaming input format (asr_paraformer_stream_create sessions, chunk_samples = S; filter (L, M, W, T = 2 W + 1) of asr_resample_table). The model-rate
 * signal of a stream is the one the offline resampler defines: output n reads the stream's input frames floor(n M / L) - W .. + W against phase (n M) mod L,
 * frames before the stream's first are zeros, widening and the channel mean are the offline kernel's. The stream's c-th step since its reset (c = 0, 1, ..)
 * produces outputs [c S, (c + 1) S) and feeds them to the unchanged chunk step. With hi(c) = floor(((c + 1) S - 1) M / L) + W, A(0) = 0 and A(c) = hi(c - 1) + 1,
 * step c consumes the stream's frames [A(c), A(c + 1)): need(c) = hi(c) + 1 - A(c) of them. The first step takes W frames more than the later ones (the
 * look-ahead: 2.1 ms at 48 kHz, 4.25 ms at 8 kHz; S = 8000: 24100 then 24000 at 48 kHz, 22142 then 22050 at 44.1 kHz, 5546 then 5512 or 5513 at 11.025 kHz, 4034
 * then 4000 at 8 kHz). A step reaches back at most 2 W frames before A(c); the session keeps them per stream in HBM as mono f32. The `audio` of the three step
 * entries is then [n_streams][pitch][channels] samples of the session's audio dtype, host or device memory, pitch = max(need(0), floor(S M / L) + 1); the library
 * reads the first need(c_i) frames of row i, c_i that stream's own step count, and ignores the rest of the row (asr_paraformer_stream_input_frames reports both).
 * The end of a stream is the caller's to pad: to A(C) frames for a whole number C of chunks. For any input x of A(C) frames the C S samples the steps produce
 * equal asr_op_resample(x)[: C S] bit for bit, however the streams' steps interleave. int16 audio is widened with the offline Paraformer session's scale (1).
 * A stream's state belongs to one format from reset to reset: a streaming session refuses asr_session_set_input_format (INVALID, the format in force stays)
 * while a stream holds audio history -- it was stepped with a non-default format in force and not reset since (the carried frames belong to that filter) -- and a
 * formatted step refuses (INVALID) a stream that was stepped at the default format and not reset since: until its reset such a stream takes model-rate mono. */
int asr_session_set_input_format(asr_session* s, int sample_rate, int channels);
int asr_session_input_format(asr_session* s, int* sample_rate_out, int* channels_out);

/* Per-kernel-class timing with HIP events on the session stream (bench.py roofline leg).
 * read: up to `cap` classes; names are NUL-terminated, 32 bytes apart in `names`. */
int asr_session_profile_enable(asr_session* s, int enable);
int asr_session_profile_reset(asr_session* s);
int asr_session_profile_read(asr_session* s, int cap, char* names, double* total_ms, int64_t* launches, int* n_out);

/* Debug taps (the reference's decode graphs expose no logits; the 1e-3 logit check needs one).
 * enable before a run; read copies the named f32 tensor of the LAST run to host.
 * names: "mel" "enc_in" "block0" "enc_out" "logits" "frame_ids"(i32); timed Paraformer runs add "fire_frames"(i32) "token_logprob" ([utterances][max_tokens]);
 * offline Paraformer runs add "alphas" and, on the packed token rows like "logits" (rows at or past the device-side count hold nothing defined),
 * "acoustic" (the CIF output) and "dec0" .. (the rows behind each decoder layer, full layers first, then the decoders3 ones); every family with a
 * non-default input format adds "resampled" ([1][samples]: the packed model-rate mono samples the front end read; a streaming step: [n_streams][chunk_samples]) */
int asr_session_taps_enable(asr_session* s, int enable);
int asr_session_tap_shape(asr_session* s, const char* name, int64_t* rows, int64_t* cols);
int asr_session_tap_read(asr_session* s, const char* name, void* host_out, size_t bytes);

/* ------------------------------------------------------------------ operator-level entry points
 * Single kernels on host arrays (device temporaries are internal). Used by the parity tests to pin
 * each HIP kernel against the oracle separately; not part of the reference-facing surface. */
int asr_op_gemm(int precision, const float* a, const float* w, const float* bias, int M, int N, int K, int act,
                float* out);                                        /* out[M][N] = act(a[M][K] w[N][K]^T + bias) */
int asr_op_layernorm(int precision, const float* x, int rows, int D, const float* gamma, const float* beta, float eps,
                     float* out);
int asr_op_attention(int precision, const float* q, const float* k, const float* v, const int32_t* seq_lens, int batch,
                     int n_heads, int d_head, float* ctx);          /* packed rows, row-major [sum T][H*D] */
int asr_op_fsmn(int precision, const float* v, const float* w, const float* b, const int32_t* seq_lens, int batch,
                int channels, int ktaps, float* out);               /* v,out: [sum T][C] row-major */
/* out[M<=64][N] = LayerNorm(x[M][K]; gamma, beta) w[N][K]^T + bias  (bf16 skinny GEMM with the fused LayerNorm prologue) */
int asr_op_gemm_ln(const float* x, const float* w, const float* bias, const float* gamma, const float* beta, int M, int N, int K,
                   float* out);
int asr_op_ctc_collapse(const int32_t* frame_ids, const int32_t* seq_lens, int batch, int blank_id, int32_t* token_ids,
                        int max_tokens, int32_t* num_id);
/* the collapse of asr_sensevoice_run_timed on host arrays: frame_logprob [sum T] beside frame_ids; first_frame / last_frame / token_logprob host
 * [batch][max_tokens] (slots at or past the token count, or past max_tokens, are not written) */
int asr_op_ctc_collapse_timed(const int32_t* frame_ids, const float* frame_logprob, const int32_t* seq_lens, int batch, int blank_id,
                              int32_t* token_ids, int32_t* first_frame, int32_t* last_frame, float* token_logprob, int max_tokens, int32_t* num_id);
/* the search of asr_sensevoice_run_beam on host arrays: cand_id / cand_logprob [sum T][topk] (ids distinct inside a row, -inf log-probabilities ignored),
 * seq_lens [batch] (each >= 1). The hotword trie: node 0 the root, per node depth / is_end [n_nodes], children of node n = child_tok / child_node
 * [child_off[n], child_off[n + 1]) sorted by token (child_off [n_nodes + 1]); n_nodes <= 1: no hotwords, the arrays may be null. Outputs as above
 * ([batch][nbest]...; token slots the search does not write come back 0). */
int asr_op_ctc_prefix_beam(const int32_t* cand_id, const float* cand_logprob, int topk, const int32_t* seq_lens, int batch, int blank_id,
                           const int32_t* trie_depth, const int32_t* trie_is_end, const int32_t* trie_child_off, const int32_t* trie_child_tok,
                           const int32_t* trie_child_node, int n_nodes, float boost, int beam, int nbest, int32_t* token_ids, int max_tokens,
                           int32_t* num_id, float* score, float* ctc_score);
/* the same with a language model image as asr_sensevoice_set_lm takes it (lm_words 32-bit words, checked the same way against blank_id; its header's vocab
 * bounds the candidate ids with a finite log-probability) */
int asr_op_ctc_prefix_beam_lm(const int32_t* cand_id, const float* cand_logprob, int topk, const int32_t* seq_lens, int batch, int blank_id,
                              const int32_t* trie_depth, const int32_t* trie_is_end, const int32_t* trie_child_off, const int32_t* trie_child_tok,
                              const int32_t* trie_child_node, int n_nodes, float boost, int beam, int nbest, int32_t* token_ids, int max_tokens,
                              int32_t* num_id, float* score, float* ctc_score, const int32_t* lm_image, int64_t lm_words, float alpha, float beta,
                              float oov_logprob);
/* the search of asr_paraformer_run_beam on host arrays: cand_id / cand_logprob [sum N][topk] (ids distinct inside a row, a -inf log-probability makes no
 * entry), seq_lens [batch] = the token counts N (0 is legal: one empty hypothesis). The hotword trie as above; the language model image as
 * asr_paraformer_set_lm takes it, or null for none (its header's vocab then bounds the candidate ids with a finite log-probability). Outputs [batch][nbest],
 * best first: token_ids / token_logprob (nullable) [batch][nbest][max_tokens] (slots the search does not write come back 0), num_id, score (acoustic + bonus +
 * lm) and am_score (the sum of the picked candidates' log-probabilities); hypotheses beyond the number found have num_id 0 and both scores -inf. */
int asr_op_nar_beam(const int32_t* cand_id, const float* cand_logprob, int topk, const int32_t* seq_lens, int batch, const int32_t* trie_depth,
                    const int32_t* trie_is_end, const int32_t* trie_child_off, const int32_t* trie_child_tok, const int32_t* trie_child_node, int n_nodes,
                    float boost, const int32_t* lm_image, int64_t lm_words, float alpha, float beta, float oov_logprob, int beam, int nbest,
                    int32_t* token_ids, int max_tokens, int32_t* num_id, float* score, float* am_score, float* token_logprob);
/* The search of asr_op_nar_beam for streams that arrive in chunks, on host arrays: the build's own mode (the reference graph returns the per-row arg-max).
 * Search state is carried per stream and per hypothesis, and tokens are committed with a fixed lag: before the row at position L of a stream is searched, a
 * stream with pend_cap (1..64) uncommitted positions commits the oldest one with the token of its best live hypothesis and drops the hypotheses that disagree
 * there. A committed token is final. The row rule is asr_op_nar_beam's, bit for bit, so a stream of at most pend_cap rows followed by a finish is that search
 * however it was cut. One call runs n_steps launches over state it keeps between them: step s has the slots step_off[s] .. step_off[s + 1] - 1 (step_off
 * [n_steps + 1], step_off[0] = 0, no empty step); slot i is stream slot_stream[i] (0 .. n_streams - 1, once per step, any order, any subset) with slot_rows[i]
 * candidate rows (0 is legal) and, where slot_final[i] != 0, the end of the stream behind them. cand_id / cand_logprob [sum of slot_rows][topk] in slot order.
 * Trie and language model as asr_op_nar_beam takes them. state_io: null (every stream starts cleared) or host [n_streams][state_words], state_words =
 * asr_nar_stream_beam_state_words of (beam, pend_cap): the streams' states before the call and after it; a stream whose first word is 0 is cleared, and the
 * words of a stream that no step names come back as they went in. Outputs per slot: commit_ids / commit_logprob [slots][commit_cap] (commit_cap >= pend_cap +
 * the longest slot_rows) and commit_num: the tokens the step committed; pend_ids / pend_logprob [slots][nbest][pend_cap], pend_num / pend_score / pend_am
 * [slots][nbest]: the uncommitted tails of the best nbest live hypotheses, best first, score (acoustic + bonus + lm) and am without the end terms --
 * hypotheses beyond the live ones have num 0 and both scores -inf; total [slots] = L, the rows searched since the stream was cleared. A finished slot applies
 * the end terms of asr_op_nar_beam, ranks again, reports the tails with their final scores, commits the best one's tail and clears the stream. Array slots the
 * search does not write come back as they went in. */
int asr_nar_stream_beam_state_words(int beam, int pend_cap); /* words of one stream's state; -1 for a beam outside 1..16 or a pend_cap outside 1..64 */
int asr_op_nar_stream_beam(const int32_t* cand_id, const float* cand_logprob, int topk, int n_streams, int n_steps, const int32_t* step_off,
                           const int32_t* slot_stream, const int32_t* slot_rows, const int32_t* slot_final, const int32_t* trie_depth,
                           const int32_t* trie_is_end, const int32_t* trie_child_off, const int32_t* trie_child_tok, const int32_t* trie_child_node,
                           int n_nodes, float boost, const int32_t* lm_image, int64_t lm_words, float alpha, float beta, float oov_logprob, int beam,
                           int nbest, int pend_cap, int32_t* state_io, int state_words, int32_t* commit_ids, float* commit_logprob, int commit_cap,
                           int32_t* commit_num, int32_t* pend_ids, float* pend_logprob, int32_t* pend_num, float* pend_score, float* pend_am,
                           int32_t* total);
/* the trellis of asr_sensevoice_align on host arrays: em [sum T][ld_em] log-probabilities, slot 0 the blank and slot j the sequence's target j - 1 (ld_em >
 * the longest transcript); each sequence is aligned against its rows row0 .. seq_lens[b] - 1 (seq_lens[b] > row0; earlier rows are never read). Targets ragged as
 * above (any ids: only the equality of neighbours matters). first_frame / last_frame / token_logprob host [batch][max_tokens], max_tokens >= the longest
 * transcript: slots past a sequence's length, and every slot of a sequence with status 1, are not written. path_score / loglik / status host [batch]. */
int asr_op_ctc_align(const float* em, int ld_em, const int32_t* seq_lens, int batch, int row0, const int32_t* target_ids, const int32_t* target_offsets,
                     int32_t* first_frame, int32_t* last_frame, float* token_logprob, int max_tokens, float* path_score, float* loglik, int32_t* status);
/* the CIF scan of asr_paraformer_run_timed on host arrays: alpha [sum T], enc [sum T][d], seq_lens [batch] (each >= 1); acoustic_out [sum T][d] receives, per
 * utterance, its token embeddings in its first rows and zeros behind them (tokens past row T - 1 of a 16-row-padded range are not returned);
 * fire_frame_out host [batch][max_tokens] (slots at or past the token count, or past max_tokens, are not written); num_id_out [batch] holds the full count */
int asr_op_cif_scan_timed(const float* alpha, const float* enc, int d, const int32_t* seq_lens, int batch, float tail_threshold, float* acoustic_out,
                          int32_t* fire_frame_out, int max_tokens, int32_t* num_id_out);
/* The resampler of asr_session_set_input_format on host arrays (the same launch): audio = packed frames of `channels` interleaved samples of audio_dtype at rate_in,
 * offsets [batch + 1] in frames (any first offset). out [out_cap] receives the packed model-rate mono f32 samples, offsets_out [batch + 1] their offsets from 0:
 * utterance b has ceil(n_b * rate_model / rate_in) samples. int16_scale != 0: int16 samples are scaled by 2^-15, as in front of the Whisper / Qwen front end. */
int asr_op_resample(const void* audio, const int64_t* offsets, int batch, int audio_dtype, int rate_in, int rate_model, int channels, int int16_scale,
                    float* out, int64_t out_cap, int64_t* offsets_out);
/* The streaming input format's launches on host arrays (every stream starts reset): n_steps steps over n_streams streams. audio [n_steps][n_streams][pitch][channels];
 * mode [n_steps][n_streams]: 0 = not in this step, 1 = stepped, 2 = reset, then stepped.
 * out [n_steps][n_streams][chunk] f32 (rows of streams not in a step untouched); frames_out [n_steps][n_streams]: frames the step read (0 if not in it). */
int asr_op_resample_stream(const void* audio, int audio_dtype, int rate_in, int rate_model, int channels, int int16_scale, int chunk, int n_streams, int n_steps,
                           const int32_t* mode, float* out, int32_t* frames_out, int32_t* pitch_out);
/* The filter the library uses for rate_in -> rate_model: with g their greatest common divisor L = rate_model / g phases, M = rate_in / g, half width W input
 * frames, T = 2 W + 1 taps per phase; output n reads input frames floor(n M / L) - W .. + W against row (n M) mod L. coeffs: null, or [L][T] f32 (computed in
 * double, rounded once). Equal rates give L = M = 1, W = 0 and the single coefficient 1. INVALID as asr_session_set_input_format refuses rates. */
int asr_resample_table(int rate_in, int rate_model, int* L, int* M, int* W, float* coeffs);

/* ------------------------------------------------------------------ voice activity: pause-aware segmentation of long audio (csrc/vad.hip)
 * An energy detector over analysis frames of H = max(1, (rate + 50) / 100) input frames (about 10 ms). An utterance of n frames has F = ceil(n / H) analysis
 * frames; e[f] is the f32 sum of x^2 over frame f with x the widened channel mean (int16 as is, never scaled: full_scale says what the values mean), and its level
 * q[f] = min(1023, (bits(max(e[f], 2^-40)) >> 20) - (bits(2^-40) >> 20)): the f32 exponent and three mantissa bits, 8 steps per octave. Everything after e[] is
 * integer work on q[]: floor = the lowest level whose cumulative count reaches ceil(p_floor F), peak = max q, thr = max(abs_level, min(floor + margin,
 * peak - peak_drop)), mask q >= thr; then speech runs shorter than min_speech are cleared, pauses shorter than min_pause between two speech runs are set, every run
 * grows by pad on both sides (touching runs are one), and a run longer than max_frames is cut -- while end - start > max_frames -- at the frame of lowest level in
 * [start + max_frames / 2, start + max_frames], the latest on a tie. All fields but p_floor count analysis frames or level steps. */
typedef struct {
  float p_floor;          /* (0, 1] */
  int32_t margin, peak_drop, abs_level;
  int32_t min_speech, min_pause, pad;
  int32_t max_frames;     /* >= 2 */
  int32_t reserved[8];
} asr_vad_params;
/* The defaults: p_floor 0.10, margin 24 (9 dB), peak_drop 16 (6 dB), abs_level = the level of H (full_scale 10^(-60/20))^2 (-60 dBFS), min_speech 10, min_pause 50,
 * pad 10, max_frames 3000. full_scale: 32768 for int16-range samples, 1 for unit-range ones. INVALID for rate < 100 or full_scale <= 0. */
int asr_vad_default_params(int rate, float full_scale, asr_vad_params* params);
/* The detector on a ragged batch: audio = packed frames of `channels` interleaved samples of audio_dtype at `rate` Hz, in host (ASR_MEM_HOST) or device memory;
 * offsets host [batch + 1] in frames (any first offset). The detector works at the input's own rate and never resamples. seg_out host [seg_cap][2] receives the
 * segments of all utterances in order as (start, end) input-frame offsets in the coordinates of `offsets`; seg_utt (nullable) host [seg_cap] the utterance of
 * each; seg_count host [batch] the FULL count of every utterance, even where the segments past seg_cap were not written. energy_out / level_out (nullable): host,
 * packed [sum F]; stats_out (nullable): host [batch][3] = floor, peak, thr. The op owns its device buffers for the call and touches no session.
 * INVALID (nothing written): an utterance of more than 2^20 analysis frames, rate < 100, channels outside 1..8, max_frames < 2, p_floor outside (0, 1]. */
int asr_op_vad(const void* audio, int mem, const int64_t* offsets, int batch, int audio_dtype, int rate, int channels, const asr_vad_params* params,
               int64_t* seg_out, int64_t seg_cap, int32_t* seg_utt, int32_t* seg_count, float* energy_out, int32_t* level_out, int32_t* stats_out);

#ifdef __cplusplus
}
#endif
#endif /* ASR_MI355X_H */
