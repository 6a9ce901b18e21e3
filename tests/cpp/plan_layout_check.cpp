// Stand-alone check of csrc/plan_layout.h (built and run by tests/test_plan_blob_cpu.py under AddressSanitizer + UBSan).
// For the section lists of the four call sites that build a plan blob -- WhSession::encode, QwSession::prefill (+ its step plan), SvSession::run and
// SvSession::stream_step -- it checks every section's alignment, bounds and order, the total, and that the offsets are those of the hand-written layout
// these sites used before PlanLayout: the expected numbers below are written out from those formulas, none comes from PlanLayout.
// The same for csrc/result_layout.h, the result blob of the SenseVoice / Paraformer session, in every form (result_blob below), and for
// csrc/nar_stream_state.h, the carried state of the streaming beam search (stream_state below).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "nar_stream_state.h"
#include "plan_layout.h"
#include "result_layout.h"

struct Utt { int64_t audio_off; int32_t v[8]; };      // the shape of UttPlan (kernels.h): one int64 + eight int32
static_assert(sizeof(Utt) == 40 && alignof(Utt) == 8, "UttPlan is 40 bytes, 8-aligned");
constexpr size_t U = 40;

struct Sec { size_t elt, align, count; };
static const Sec utt(size_t n) { return Sec{U, 8, n}; }
static const Sec i32(size_t n) { return Sec{4, 4, n}; }

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL %s: ", name); printf(__VA_ARGS__); printf("\n"); } } while (0)

static void check(const char* name, const std::vector<Sec>& secs, size_t round_to, const std::vector<size_t>& want_off, size_t want_total) {
  PlanLayout lay;
  std::vector<int> id;
  for (const Sec& s : secs) id.push_back(lay.add(s.elt, s.align, s.count));
  lay.round_total(round_to);
  size_t end = 0, payload = 0, padding = 0;
  for (size_t k = 0; k < secs.size(); ++k) {
    const size_t off = lay.off[id[k]], bytes = lay.bytes[id[k]];
    CHECK(id[k] == (int)k, "section %zu got index %d", k, id[k]);
    CHECK(off % secs[k].align == 0, "section %zu at %zu is not %zu-aligned", k, off, secs[k].align);
    CHECK(bytes == secs[k].elt * secs[k].count, "section %zu holds %zu bytes", k, bytes);
    CHECK(off >= end, "section %zu at %zu overlaps its predecessor (ends at %zu)", k, off, end);
    CHECK(off - end < secs[k].align, "section %zu: %zu bytes of padding for alignment %zu", k, off - end, secs[k].align);
    CHECK(off + bytes <= lay.total, "section %zu ends at %zu, past the total %zu", k, off + bytes, lay.total);
    CHECK(off == want_off[k], "section %zu at %zu, hand layout %zu", k, off, want_off[k]);
    padding += off - end; payload += bytes; end = off + bytes;
  }
  padding += lay.total - end;
  CHECK(lay.total - end < round_to, "total %zu is more than one rounding step past the last section (%zu)", lay.total, end);
  CHECK(lay.total % round_to == 0, "total %zu is no multiple of %zu", lay.total, round_to);
  CHECK(lay.total == payload + padding, "total %zu != %zu + %zu", lay.total, payload, padding);
  CHECK(lay.total == want_total, "total %zu, hand layout %zu", lay.total, want_total);
}

static size_t up(size_t v, size_t m) { return (v + m - 1) / m * m; }

// ---- the four sites: section lists in declaration order, expected offsets from the hand layouts
static void whisper(const char* name, size_t B, size_t n_fb, size_t n_qb, size_t Mpad, size_t Mg) {
  const size_t R = 2 * Mg, t0 = 2 * U * B;      // [UttPlan B][UttPlan B][blk_utt][blk_f0][qb_utt][qb_q0][row_utt Mpad][pos_rows Mg][grow_utt R]
  check(name, {utt(B), utt(B), i32(n_fb), i32(n_fb), i32(n_qb), i32(n_qb), i32(Mpad), i32(Mg), i32(R)}, 1,
        {0, U * B, t0, t0 + 4 * n_fb, t0 + 4 * (2 * n_fb), t0 + 4 * (2 * n_fb + n_qb), t0 + 4 * (2 * n_fb + 2 * n_qb), t0 + 4 * (2 * n_fb + 2 * n_qb + Mpad),
         t0 + 4 * (2 * n_fb + 2 * n_qb + Mpad + Mg)},
        2 * U * B + 4 * (2 * n_fb + 2 * n_qb + Mpad + Mg + R));
}
static void qwen(const char* name, size_t B, size_t wins, size_t n_fb, size_t n_qb, size_t slots, size_t Me, size_t Md, size_t n_dqb) {
  // [UttPlan B][win plans][dec plans B][blk_utt][blk_f0][qb_utt][qb_q0][slot_utt][slot_local][pos_rows Me][src Md][row_seq Md][row_t Md][last B][dqb_utt][dqb_q0]
  const size_t t0 = U * (2 * B + wins);
  std::vector<size_t> off = {0, U * B, U * (B + wins)};
  size_t words = 0;
  for (size_t n : {n_fb, n_fb, n_qb, n_qb, slots, slots, Me, Md, Md, Md, B, n_dqb, n_dqb}) { off.push_back(t0 + 4 * words); words += n; }
  check(name, {utt(B), utt(wins), utt(B), i32(n_fb), i32(n_fb), i32(n_qb), i32(n_qb), i32(slots), i32(slots), i32(Me), i32(Md), i32(Md), i32(Md), i32(B),
               i32(n_dqb), i32(n_dqb)}, 16, off,
        (U * (2 * B + wins) + 4 * (2 * n_fb + 2 * n_qb + 2 * slots + Me + 3 * Md + B + 2 * n_dqb) + 15) / 16 * 16);
}
static void qwen_step(const char* name, size_t rows) {      // [UttPlan rows][row_seq Mb][row_t Mb][last Mb], Mb = rows rounded up to 128
  const size_t Mb = up(rows, 128);
  check(name, {utt(rows), i32(Mb), i32(Mb), i32(Mb)}, 1, {0, U * rows, U * rows + 4 * Mb, U * rows + 8 * Mb}, U * rows + 4 * 3 * Mb);
}
static void sensevoice(const char* name, size_t B, size_t n_fb, size_t n_qb, size_t rows) {
  const size_t Mpad = up(rows, 128), n_tiles = rows / 16, t0 = U * B;      // [UttPlan B][blk_utt][blk_f0][qb_utt][qb_q0][row_utt Mpad][tile_win][tile_idx]
  check(name, {utt(B), i32(n_fb), i32(n_fb), i32(n_qb), i32(n_qb), i32(Mpad), i32(n_tiles), i32(n_tiles)}, 1,
        {0, t0, t0 + 4 * n_fb, t0 + 8 * n_fb, t0 + 4 * (2 * n_fb + n_qb), t0 + 4 * (2 * n_fb + 2 * n_qb), t0 + 4 * (2 * n_fb + 2 * n_qb + Mpad),
         t0 + 4 * (2 * n_fb + 2 * n_qb + Mpad + n_tiles)},
        U * B + 4 * (2 * n_fb + 2 * n_qb + Mpad + 2 * n_tiles));
}
static void stream_step(const char* name, size_t n) {       // [UttPlan n][blk_utt n][blk_f0 n][row_utt Mpad], 16 rows per stream
  const size_t Mpad = up(16 * n, 128);
  check(name, {utt(n), i32(n), i32(n), i32(Mpad)}, 1, {0, U * n, U * n + 4 * n, U * n + 8 * n}, U * n + 4 * (2 * n + Mpad));
}

// ---- the result blob of the SenseVoice / Paraformer session (csrc/result_layout.h): every form against the byte arithmetic SvSession::enqueue, ::run and
// ::stream_step spelled out by hand before ResultLayout. Offline Paraformer timed had a gap the size of `last` in front of `logprob`; it now has the streaming
// step's compact layout, which is what is asserted for it.
struct Span { const char* what; size_t off, bytes; };
static void result_sections(const char* name, const ResultLayout& L, const std::vector<Span>& got, const std::vector<size_t>& want_off, size_t want_total) {
  CHECK(got.size() == want_off.size(), "%zu sections, %zu expected", got.size(), want_off.size());
  for (size_t k = 0; k < got.size() && k < want_off.size(); ++k) {
    CHECK(got[k].off == want_off[k], "%s at %zu, hand layout %zu", got[k].what, got[k].off, want_off[k]);
    CHECK(got[k].off % 4 == 0 && got[k].bytes % 4 == 0, "%s at %zu (%zu bytes) is not 4-byte aligned", got[k].what, got[k].off, got[k].bytes);
    CHECK(got[k].off + got[k].bytes <= L.total(), "%s ends at %zu, past the total %zu", got[k].what, got[k].off + got[k].bytes, L.total());
    for (size_t j = 0; j < k; ++j)
      CHECK(got[j].off + got[j].bytes <= got[k].off || got[k].off + got[k].bytes <= got[j].off, "%s overlaps %s", got[k].what, got[j].what);
  }
  CHECK(L.total() == want_total, "total %zu, the hand-written reserve() argument %zu", L.total(), want_total);
}
#define SPAN(L, s) Span{#s, (L).off((L).s), (L).bytes((L).s)}
static void result_blob(size_t n, size_t mt, size_t nbest) {
  char name[96];
  const size_t tok_bytes = n * mt * 4;
  {
    snprintf(name, sizeof name, "result plain n=%zu max_tokens=%zu", n, mt);
    const ResultLayout L(n, mt, ResultForm::PLAIN);
    result_sections(name, L, {SPAN(L, tokens), SPAN(L, counts), Span{"status (16 bytes)", L.off(L.status), 16}}, {0, n * mt * 4, n * mt * 4 + n * 4}, n * mt * 4 + n * 4 + 16);
    CHECK(L.bytes(L.tokens) == tok_bytes && L.bytes(L.counts) == n * 4 && L.bytes(L.status) == 4, "section sizes");
    CHECK(!L.has(L.first) && !L.has(L.last) && !L.has(L.logprob) && !L.has(L.beam), "the plain form has three sections");
    CHECK(L.rows(L.tokens) == n, "%zu token rows", L.rows(L.tokens));
  }
  {
    snprintf(name, sizeof name, "result sensevoice timed n=%zu max_tokens=%zu", n, mt);
    const ResultLayout L(n, mt, ResultForm::SV_TIMED);
    const size_t ext = tok_bytes + n * 4 + 16;          // SvSession::enqueue: unsigned char* ext = h_out + tok_bytes + batch * 4 + 16
    result_sections(name, L, {SPAN(L, tokens), SPAN(L, counts), Span{"status (16 bytes)", L.off(L.status), 16}, SPAN(L, first), SPAN(L, last), SPAN(L, logprob)},
                    {0, tok_bytes, tok_bytes + n * 4, ext, ext + tok_bytes, ext + 2 * tok_bytes}, n * mt * 4 + n * 4 + 16 + n * mt * 12);
    CHECK(L.bytes(L.first) == tok_bytes && L.bytes(L.last) == tok_bytes && L.bytes(L.logprob) == tok_bytes, "span sections hold n x max_tokens words");
  }
  for (int offline = 0; offline < 2; ++offline) {       // streaming timed as it was; offline Paraformer timed: the same, compact
    snprintf(name, sizeof name, "result paraformer timed (%s) n=%zu max_tokens=%zu", offline ? "offline" : "streaming", n, mt);
    const ResultLayout L(n, mt, ResultForm::PF_TIMED);
    const size_t out_bytes = tok_bytes + n * 4;         // SvSession::stream_step: h_out.reserve(out_bytes + 16 + 2 * tok_bytes), fire steps at out_bytes + 16
    result_sections(name, L, {SPAN(L, tokens), SPAN(L, counts), Span{"status (16 bytes)", L.off(L.status), 16}, SPAN(L, first), SPAN(L, logprob)},
                    {0, tok_bytes, out_bytes, out_bytes + 16, out_bytes + 16 + tok_bytes}, out_bytes + 16 + 2 * tok_bytes);
    CHECK(!L.has(L.last), "Paraformer has no last-frame section");
  }
  {
    snprintf(name, sizeof name, "result sensevoice beam n=%zu max_tokens=%zu nbest=%zu", n, mt, nbest);
    const ResultLayout L(n, mt, ResultForm::SV_BEAM, nbest);
    const size_t hyps = n * nbest, tokb = hyps * mt * 4, bo = n * mt * 4 + n * 4 + 16;
    result_sections(name, L, {SPAN(L, tokens), SPAN(L, counts), Span{"status (16 bytes)", L.off(L.status), 16}, SPAN(L, hyp_tokens), SPAN(L, hyp_counts), SPAN(L, hyp_scores),
                              SPAN(L, hyp_ctc)},
                    {0, n * mt * 4, n * mt * 4 + n * 4, bo, bo + tokb, bo + tokb + hyps * 4, bo + tokb + hyps * 8}, n * mt * 4 + n * 4 + 16 + n * nbest * (mt * 4 + 12));
    // the device-side block: launch_ctc_prefix_beam's four outputs at bo, bo + tokb, bo + tokb + hyps * 4, bo + tokb + hyps * 8 of d_bout, copied home as tokb + hyps * 12 bytes
    CHECK(L.dev_off(L.hyp_tokens) == 0 && L.dev_off(L.hyp_counts) == tokb && L.dev_off(L.hyp_scores) == tokb + hyps * 4 && L.dev_off(L.hyp_ctc) == tokb + hyps * 8, "device beam block");
    CHECK(L.off(L.beam) == bo && L.bytes(L.beam) == tokb + hyps * 12 && L.bytes(L.beam) == n * nbest * (mt * 4 + 12), "beam block at %zu, %zu bytes", L.off(L.beam), L.bytes(L.beam));
    CHECK(L.bytes(L.hyp_tokens) == tokb && L.bytes(L.hyp_counts) == hyps * 4 && L.bytes(L.hyp_scores) == hyps * 4 && L.bytes(L.hyp_ctc) == hyps * 4, "beam section sizes");
    CHECK(L.rows(L.hyp_tokens) == hyps, "%zu hypothesis rows", L.rows(L.hyp_tokens));
  }
}

// ---- the carried state of one stream of the streaming beam search (csrc/nar_stream_state.h) against the documented layout, written out in words: the
// header [L, C, live, unused], five live planes of 16 (am, bonus, node, lm, lmstate), three ring planes [pend_cap][beam] (parent, token, log-probability)
static void stream_state_planes() {                       // what does not depend on (beam, pend_cap)
  namespace S = nar_stream_state;
  const char* name = "stream state header and live planes";
  CHECK(S::L == 0 && S::C == 1 && S::N_LIVE == 2 && S::UNUSED == 3 && S::HEADER == 4, "header words %d %d %d %d, %d in all", S::L, S::C, S::N_LIVE, S::UNUSED, S::HEADER);
  CHECK(S::AM == 4 && S::BONUS == 4 + 16 && S::NODE == 4 + 32 && S::LM == 4 + 48 && S::LMSTATE == 4 + 64, "live planes at %d %d %d %d %d", S::AM, S::BONUS, S::NODE,
        S::LM, S::LMSTATE);
}
static void stream_state(int beam, int pend_cap) {
  namespace S = nar_stream_state;
  char name[64];
  snprintf(name, sizeof name, "stream state beam=%d pend_cap=%d", beam, pend_cap);
  const int ring = pend_cap * beam;
  CHECK(S::ring_parent(beam, pend_cap) == 4 + 5 * 16 && S::ring_token(beam, pend_cap) == 4 + 5 * 16 + ring && S::ring_logprob(beam, pend_cap) == 4 + 5 * 16 + 2 * ring,
        "ring planes at %d %d %d", S::ring_parent(beam, pend_cap), S::ring_token(beam, pend_cap), S::ring_logprob(beam, pend_cap));
  CHECK(S::words(beam, pend_cap) == 4 + 5 * 16 + 3 * pend_cap * beam, "%d words", S::words(beam, pend_cap));
}

int main() {
  stream_state_planes();
  stream_state(4, 16);
  stream_state(16, 64);                                         // the widest beam at the longest lag
  result_blob(1, 1, 1);
  result_blob(1, 5, 1);
  result_blob(3, 7, 2);
  result_blob(64, 213, 16);
  for (size_t n : {1, 3, 64}) result_blob(n, 11 + 1, 1);       // the streaming step's minimum, max_tokens = st_B + 1 (600 ms chunks: st_B = 11)
  result_blob(1, 1 + 1, 1);                                     // ... of the smallest chunk (st_B = 1)
  // Whisper (hop 160; T = (frames + 1) / 2; encoder rows round16(T), stem rows round16(T + 1); f32 query blocks of 64 rows)
  whisper("whisper B=1 (26240 samples)", 1, 3, 2, 128, 128);                      // 164 frames, T 82: 96 rows
  whisper("whisper ragged B=3 (26240, 12640, 48000)", 3, 3 + 2 + 5, 2 + 1 + 3, 384, 384);   // T 82, 40, 150: rows 96 + 48 + 160, stem 96 + 48 + 160
  whisper("whisper rows == Mpad (40000 samples)", 1, 4, 2, 128, 128);             // 250 frames, T 125: 128 rows, stem round16(126) = 128
  whisper("whisper no query blocks", 2, 5, 0, 256, 256);
  // Qwen3 (B, windows, fbank blocks, encoder query blocks, chunk slots, Me, Md, decoder query blocks)
  qwen("qwen B=1", 1, 1, 3, 1, 8, 128, 128, 1);
  qwen("qwen ragged B=3", 3, 4, 11, 5, 32, 512, 256, 4);
  qwen("qwen f32: n_qb = 0, n_dqb = 0", 2, 2, 5, 0, 16, 256, 128, 0);
  qwen("qwen total needs rounding", 1, 1, 1, 1, 8, 128, 128, 0);                 // 40 * 3 + 4 * (2 + 2 + 16 + 128 + 384 + 1) = 2252 -> 2256
  qwen("qwen rows == Mpad", 2, 2, 6, 2, 16, 208, 128, 2);
  for (size_t rows : {1, 3, 128, 129, 640}) qwen_step("qwen step plan", rows);
  // SenseVoice (B, fbank blocks, query blocks, rows)
  sensevoice("sensevoice B=1 (16000 samples)", 1, 2, 1, 32);
  sensevoice("sensevoice ragged B=3", 3, 2 + 2 + 4, 3, 32 + 32 + 64);             // rows == Mpad == 128
  sensevoice("sensevoice n_qb = 0", 2, 4, 0, 80);
  sensevoice("sensevoice 12 utterances", 12, 30, 12, 12 * 48);
  for (size_t n : {1, 3, 8, 9, 64}) stream_step("paraformer stream step", n);      // n = 8: rows == Mpad
  // alignment: an odd run of 4-byte words in front of 8-aligned plans is padded (no site does this today; a new section order may)
  check("padding before an 8-aligned section", {i32(3), utt(2), i32(1)}, 16, {0, 16, 96}, 112);
  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("plan layout ok\n");
  return 0;
}
