// Device-side walk of the hotword context graph (kernels.h: HotTrie), shared by the three token-synchronous beam searches through beam_dev.h (ctc_beam.hip,
// nar_beam.hip, nar_stream_beam.hip), the hotword kernels of the autoregressive decoders (hotword.hip), their LM re-rank (decoder_lm.hip) and the beam ranker's
// node hand-over (kernels.hip). The float64 statement is tests/ctc_beam_ref.py: trie_step.
#pragma once
#include "kernels.h"

__device__ __forceinline__ int trie_child(const HotTrie& tr, int node, int c) {
  int lo = tr.child_off[node], hi = tr.child_off[node + 1];
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const int t = tr.child_tok[mid];
    if (t == c) return tr.child_node[mid];
    if (t < c) lo = mid + 1; else hi = mid;
  }
  return -1;
}

// (node, bonus) after appending the non-blank token c: a child c -> there, + boost, back to the root when it ends a phrase (the bonus stays); no child and
// not at the root -> the partial match is taken back, then the root's child c by the same rule. No fail links.
__device__ __forceinline__ void trie_step(const HotTrie& tr, int& node, float& bonus, int c) {
  if (tr.n_nodes <= 1) return;
  int ch = trie_child(tr, node, c);
  if (ch < 0 && node != 0) {
    bonus -= (float)tr.depth[node] * tr.boost;
    node = 0;
    ch = trie_child(tr, 0, c);
  }
  if (ch >= 0) { bonus += tr.boost; node = tr.is_end[ch] ? 0 : ch; }
  else node = 0;
}
