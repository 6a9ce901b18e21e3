"""Back-off n-gram language models for the CTC prefix beam search (SenseVoiceSession.set_lm, asr_sensevoice_set_lm): the ARPA reader, the
in-memory image the search walks on the device, and a float64 walk of that image on the host.

The image is one int32 blob (include/asr_mi355x.h states the layout): a header [order, n_nodes, n_edges, vocab, start_node, eos_edge_token], then depth,
backoff (f32), suffix, child_off, tok, logp (f32), next, uni. Nodes are the contexts, edges the listed n-grams; </s> and <s> take the ids vocab and vocab + 1."""
from __future__ import annotations

import math
import os

import numpy as np

EOS, BOS = -1, -2                      # </s> and <s> inside NgramLM.ngrams (the image gives them vocab and vocab + 1)
_SPECIAL = {"</s>": EOS, "<s>": BOS}
_LN10 = math.log(10.0)
MAX_ORDER = 5
HEADER = 6


class NgramLM:
    """ngrams: {tuple of token ids (EOS / BOS for the sentence marks): (logp, backoff)}, natural logs. unk_logprob: the <unk> unigram of the file (None
    without one): the default cost of a token the model has no unigram for."""

    def __init__(self, ngrams, unk_logprob=None):
        if not ngrams:
            raise ValueError("a language model needs at least one n-gram")
        self.ngrams = {tuple(int(t) for t in g): (float(lp), float(bo)) for g, (lp, bo) in ngrams.items()}
        self.order = max(len(g) for g in self.ngrams)
        if not 1 <= self.order <= MAX_ORDER:
            raise ValueError(f"order {self.order}: orders 1..{MAX_ORDER} are supported")
        for g, (lp, bo) in self.ngrams.items():
            if len(g) > 1 and g[:-1] not in self.ngrams:
                raise ValueError(f"the context of the n-gram {g} is not listed")
            if not (math.isfinite(lp) and lp <= 0.0 and math.isfinite(bo)):
                raise ValueError(f"n-gram {g}: log-probability {lp}, back-off {bo}")
        self.unk_logprob = None if unk_logprob is None else float(unk_logprob)
        self._images = {}

    @property
    def default_oov_logprob(self) -> float:
        return 0.0 if self.unk_logprob is None else self.unk_logprob

    @classmethod
    def from_arpa(cls, path_or_lines, token_to_id=None):
        """An ARPA file (a path) or its lines. Words are decimal token ids when every word other than <s>, </s> and <unk> parses as an integer; otherwise
        they are pieces resolved through token_to_id (a mapping or a callable returning None for an unknown piece). log10 becomes the natural log; <unk>'s
        unigram becomes the default oov_logprob and n-grams through <unk> are dropped. Errors name the line."""
        if isinstance(path_or_lines, (str, os.PathLike)):
            with open(path_or_lines, "r", encoding="utf-8") as f:
                lines = f.read().splitlines()
        else:
            lines = [str(x).rstrip("\n") for x in path_or_lines]
        entries, section = [], 0                                       # (line number, order, words, log10 p, log10 backoff)
        for no, raw in enumerate(lines, 1):
            line = raw.strip()
            if not line or line == "\\data\\" or line.startswith("ngram "):
                continue
            if line == "\\end\\":
                break
            if line.startswith("\\") and line.endswith("-grams:"):
                try:
                    section = int(line[1:-len("-grams:")])
                except ValueError:
                    raise ValueError(f"line {no}: unreadable section header {line!r}") from None
                continue
            if section < 1:
                raise ValueError(f"line {no}: an n-gram before any \\n-grams: section")
            f = line.split()
            if len(f) not in (section + 1, section + 2):
                raise ValueError(f"line {no}: a {section}-gram line has {section + 1} or {section + 2} fields, this one {len(f)}")
            try:
                lp, bo = float(f[0]), (float(f[section + 1]) if len(f) == section + 2 else 0.0)
            except ValueError:
                raise ValueError(f"line {no}: unreadable number in {line!r}") from None
            if not (math.isfinite(lp) and math.isfinite(bo)):
                raise ValueError(f"line {no}: log-probability {lp}, back-off {bo}")
            if lp > 0.0:
                raise ValueError(f"line {no}: positive log-probability {lp}")
            entries.append((no, section, f[1:section + 1], lp, bo))
        if not entries:
            raise ValueError("no n-gram in the ARPA text")

        def is_int(w):
            try:
                int(w)
                return True
            except ValueError:
                return False
        as_ids = all(is_int(w) for _, _, ws, _, _ in entries for w in ws if w not in _SPECIAL and w != "<unk>")
        if not as_ids and token_to_id is None:
            raise ValueError("the model's words are pieces: token_to_id is needed")
        lookup = (lambda w: int(w)) if as_ids else (token_to_id if callable(token_to_id) else token_to_id.get)
        ngrams, unk = {}, None
        for no, n, ws, lp, bo in entries:
            if "<unk>" in ws:
                if n == 1:
                    unk = lp * _LN10
                continue
            g = []
            for w in ws:
                t = _SPECIAL[w] if w in _SPECIAL else lookup(w)
                if t is None or (w not in _SPECIAL and int(t) < 0):
                    raise ValueError(f"line {no}: the word {w!r} is not in the vocabulary")
                g.append(int(t))
            g = tuple(g)
            if n > 1 and g[:-1] not in ngrams:
                raise ValueError(f"line {no}: the context of {' '.join(ws)!r} is not listed")
            ngrams[g] = (lp * _LN10, bo * _LN10)
        return cls(ngrams, unk)

    def image(self, vocab: int) -> np.ndarray:
        """The int32 blob for a vocabulary of `vocab` ids. A token id outside [0, vocab) is an error."""
        vocab = int(vocab)
        if vocab in self._images:
            return self._images[vocab]
        ident = lambda t: vocab if t == EOS else vocab + 1 if t == BOS else t
        grams = {}
        for g, val in self.ngrams.items():
            for t in g:
                if t not in (EOS, BOS) and not 0 <= t < vocab:
                    raise ValueError(f"the n-gram {g} holds token {t}, outside the vocabulary of {vocab}")
            grams[tuple(ident(t) for t in g)] = val
        nodes = [()] + sorted((g for g in grams if len(g) < self.order), key=lambda g: (len(g), g))
        index = {g: i for i, g in enumerate(nodes)}

        def longest(g):                                    # the node of the longest suffix of g that is one
            while g not in index:
                g = g[1:]
            return index[g]
        kids = [[] for _ in nodes]
        for g, (lp, _) in grams.items():
            kids[index[g[:-1]]].append((g[-1], lp, longest(g)))
        child_off, tok, logp, nxt = [0], [], [], []
        for ks in kids:
            for t, lp, nx in sorted(ks):
                tok.append(t); logp.append(lp); nxt.append(nx)
            child_off.append(len(tok))
        uni = np.full(vocab + 2, -1, dtype=np.int32)
        uni[tok[:child_off[1]]] = np.arange(child_off[1], dtype=np.int32)
        start = nxt[uni[vocab + 1]] if uni[vocab + 1] >= 0 else 0
        header = [self.order, len(nodes), len(tok), vocab, start, vocab if uni[vocab] >= 0 else -1]
        i32 = lambda a: np.asarray(a, dtype=np.int32)
        f32 = lambda a: np.asarray(a, dtype=np.float32).view(np.int32)
        img = np.concatenate([i32(header), i32([len(g) for g in nodes]), f32([0.0] + [grams[g][1] for g in nodes[1:]]),
                              i32([0] + [longest(g[1:]) for g in nodes[1:]]), i32(child_off), i32(tok), f32(logp), i32(nxt), uni])
        self._images[vocab] = img
        return img

    def score(self, tokens, vocab: int | None = None, alpha: float = 1.0, beta: float = 0.0, oov_logprob: float | None = None) -> float:
        """What the search adds to a hypothesis with these tokens: the sum of alpha * log P(token | history) + beta, plus alpha * log P(</s> | history) when
        the model lists </s> -- a float64 walk of the image, from the <s> state. score - this is the hypothesis' CTC figure plus its hotword bonus."""
        tokens = [int(t) for t in tokens]
        if vocab is None:
            vocab = 1 + max([t for g in self.ngrams for t in g] + tokens + [0])
        img = self.image(vocab)
        n, m = int(img[1]), int(img[2])
        at = HEADER + n
        backoff = img[at:at + n].view(np.float32); at += n
        suffix = img[at:at + n]; at += n
        off = img[at:at + n + 1]; at += n + 1
        tok = img[at:at + m]; at += m
        logp = img[at:at + m].view(np.float32); at += m
        nxt = img[at:at + m]; at += m
        uni = img[at:]
        oov = self.default_oov_logprob if oov_logprob is None else float(oov_logprob)

        def step(state, c):
            if uni[c] < 0:
                return oov, state
            acc, node = 0.0, state
            while True:
                if node == 0:
                    e = int(uni[c])
                else:
                    lo, hi = int(off[node]), int(off[node + 1])
                    i = lo + int(np.searchsorted(tok[lo:hi], c))
                    e = i if i < hi and tok[i] == c else -1
                if e >= 0:
                    return acc + float(logp[e]), int(nxt[e])
                acc += float(backoff[node])
                node = int(suffix[node])
        total, state = 0.0, int(img[4])
        for c in tokens:
            if not 0 <= c < vocab:
                raise ValueError(f"token {c} outside the vocabulary of {vocab}")
            lp, state = step(state, c)
            total += alpha * lp + beta
        if img[5] >= 0:
            total += alpha * step(state, int(img[5]))[0]
        return total
