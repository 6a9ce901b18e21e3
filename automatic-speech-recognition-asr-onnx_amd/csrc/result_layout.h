// The result sections of one SenseVoice / Paraformer call, offline or streaming: what the call's D2H copies write into the pinned result buffer and what
// the host reads after the sync, declared once as a function of (n_rows, max_tokens, form, nbest). Every result offset is computed here and nowhere else.
// Plain C++ without HIP types (ResultBlob in engine.h adds the buffer): tests/test_plan_blob_cpu.py compiles it on the CPU.
//   plain              [tokens n x max_tokens][counts n][status: error word + 3 reserved words]
//   SenseVoice timed   ... [first][last][logprob]      (n x max_tokens each)
//   Paraformer timed   ... [first][logprob]            (offline: fire rows, streaming: fire steps; one layout for both)
//   SenseVoice beam    ... [beam block: hyp_tokens n nbest x max_tokens][hyp_counts n nbest][hyp_scores n nbest][hyp_ctc n nbest]
//   Paraformer beam    ... [first: the fire rows][beam block: the four sections above, hyp_ctc holding the acoustic score, then hyp_logprob n nbest x max_tokens]
//   Paraformer stream beam  ... [first][logprob] as the Paraformer-timed form, then [stream-beam block: commit_ids n x commit_cap][commit_logprob n x commit_cap]
//                      [commit_num n][pend_ids n nbest x pend_cap][pend_logprob n nbest x pend_cap][pend_num n nbest][pend_score n nbest][pend_am n nbest][total n]
//                      (commit_cap = pend_cap + max_tokens; the finish takes it with max_tokens = 0)
//   SenseVoice align   ... [first][last][logprob][path_score n][loglik n][align_status n]      (max_tokens = the longest transcript, at least 1)
// The beam block is a layout of its own: the device-side block the beam kernel writes has the same sections from offset 0 and comes home in one copy.
#pragma once
#include <cstdint>

#include "plan_layout.h"

enum class ResultForm { PLAIN, SV_TIMED, PF_TIMED, SV_BEAM, SV_ALIGN, PF_BEAM, PF_STREAM_BEAM };

template <typename T> struct ResultSection { int i = -1; bool in_beam = false; };      // i < 0: the form has no such section

struct ResultLayout {
  PlanLayout lay, beam_lay;
  size_t n_rows, max_tokens, commit_cap = 0;
  ResultSection<int32_t> tokens, counts, first, last, hyp_tokens, hyp_counts, align_status, commit_ids, commit_num, pend_ids, pend_num, total_rows;
  ResultSection<uint32_t> status;
  ResultSection<float> logprob, hyp_scores, hyp_ctc, hyp_logprob, path_score, loglik, commit_logprob, pend_logprob, pend_score, pend_am;
  ResultSection<unsigned char> beam;                     // the hyp_* (stream beam: the commit_* / pend_* / total_rows) sections as one
  ResultLayout(size_t n, size_t max_tok, ResultForm form, size_t nbest = 1, size_t pend_cap = 0) : n_rows(n), max_tokens(max_tok) {
    const size_t toks = n * max_tok, hyps = n * nbest;
    tokens.i = lay.add(4, 4, toks);
    counts.i = lay.add(4, 4, n);
    status.i = lay.add(4, 4, 1);
    lay.add(4, 4, 3);
    const bool spans = form == ResultForm::SV_TIMED || form == ResultForm::SV_ALIGN;
    const bool pf_timed = form == ResultForm::PF_TIMED || form == ResultForm::PF_STREAM_BEAM;
    if (spans || pf_timed) first.i = lay.add(4, 4, toks);
    if (spans) last.i = lay.add(4, 4, toks);
    if (spans || pf_timed) logprob.i = lay.add(4, 4, toks);
    if (form == ResultForm::SV_ALIGN) { path_score.i = lay.add(4, 4, n); loglik.i = lay.add(4, 4, n); align_status.i = lay.add(4, 4, n); }
    if (form == ResultForm::PF_BEAM) first.i = lay.add(4, 4, toks);
    if (form == ResultForm::PF_STREAM_BEAM) {
      commit_cap = pend_cap + max_tok;
      commit_ids = {beam_lay.add(4, 4, n * commit_cap), true};
      commit_logprob = {beam_lay.add(4, 4, n * commit_cap), true};
      commit_num = {beam_lay.add(4, 4, n), true};
      pend_ids = {beam_lay.add(4, 4, hyps * pend_cap), true};
      pend_logprob = {beam_lay.add(4, 4, hyps * pend_cap), true};
      pend_num = {beam_lay.add(4, 4, hyps), true};
      pend_score = {beam_lay.add(4, 4, hyps), true};
      pend_am = {beam_lay.add(4, 4, hyps), true};
      total_rows = {beam_lay.add(4, 4, n), true};
      beam.i = lay.add(1, 4, beam_lay.total);
      return;
    }
    if (form != ResultForm::SV_BEAM && form != ResultForm::PF_BEAM) return;
    hyp_tokens = {beam_lay.add(4, 4, hyps * max_tok), true};
    hyp_counts = {beam_lay.add(4, 4, hyps), true};
    hyp_scores = {beam_lay.add(4, 4, hyps), true};
    hyp_ctc = {beam_lay.add(4, 4, hyps), true};
    if (form == ResultForm::PF_BEAM) hyp_logprob = {beam_lay.add(4, 4, hyps * max_tok), true};
    beam.i = lay.add(1, 4, beam_lay.total);
  }
  size_t total() const { return lay.total; }             // what the pinned buffer is reserved for
  template <typename T> bool has(ResultSection<T> s) const { return s.i >= 0; }
  template <typename T> size_t bytes(ResultSection<T> s) const { assert(has(s)); return (s.in_beam ? beam_lay : lay).bytes[s.i]; }
  template <typename T> size_t off(ResultSection<T> s) const { assert(has(s)); return s.in_beam ? lay.off[beam.i] + beam_lay.off[s.i] : lay.off[s.i]; }
  template <typename T> size_t dev_off(ResultSection<T> s) const { assert(has(s) && s.in_beam); return beam_lay.off[s.i]; }      // inside the device-side beam block
  template <typename T> size_t rows(ResultSection<T> s) const { return bytes(s) / (sizeof(T) * max_tokens); }                     // of a [rows][max_tokens] section
};
