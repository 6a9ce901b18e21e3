// The carried state of one stream of the streaming beam search (nar_stream_beam.hip): the layout, once, for the kernel that reads and writes it
// and for the host code that checks a caller's copy (api.hip). Plain C++, host and device. int32 words:
//   [L]       rows searched since the stream's search was last cleared; L == 0 IS the cleared state (nothing else is read then: zeroed memory is a cleared stream)
//   [C]       how many of them are committed (L - C <= pend_cap)
//   [N_LIVE]  the number of live hypotheses; [UNUSED] is written as 0
//   AM, BONUS (f32), NODE, LM (f32), LMSTATE: planes of PLANE words each, the live hypotheses in rank order (LM / LMSTATE only with a model)
//   ring: parent rank, token id, token log-probability (f32): three planes [pend_cap][beam] from RING on; row (pos % pend_cap) holds position pos, entry r of
//   the row at L - 1 is live hypothesis r, and `parent` indexes the row below
// 4 + 5 * 16 + 3 * pend_cap * beam words in all.
#pragma once

namespace nar_stream_state {
constexpr int PLANE = 16;             // the widest beam (beam_dev.h asserts that it is TOKEN_BEAM_MAX)
constexpr int L = 0, C = 1, N_LIVE = 2, UNUSED = 3, HEADER = 4;
constexpr int AM = HEADER, BONUS = AM + PLANE, NODE = BONUS + PLANE, LM = NODE + PLANE, LMSTATE = LM + PLANE, RING = LMSTATE + PLANE;
constexpr int RING_PARENT = 0, RING_TOKEN = 1, RING_LOGPROB = 2, RING_PLANES = 3;        // the ring planes in their order
constexpr int ring_plane_words(int beam, int pend_cap) { return pend_cap * beam; }
constexpr int ring_parent(int beam, int pend_cap) { return RING + RING_PARENT * ring_plane_words(beam, pend_cap); }
constexpr int ring_token(int beam, int pend_cap) { return RING + RING_TOKEN * ring_plane_words(beam, pend_cap); }
constexpr int ring_logprob(int beam, int pend_cap) { return RING + RING_LOGPROB * ring_plane_words(beam, pend_cap); }
constexpr int words(int beam, int pend_cap) { return RING + RING_PLANES * ring_plane_words(beam, pend_cap); }
}  // namespace nar_stream_state
