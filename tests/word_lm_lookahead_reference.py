"""An independent restatement of the word n-gram scorer **with look-ahead** (include/ctcasr.h, K26):
`word_lm_reference.Scorer` with K26's `edge` and `end` and the table rule, over the reference's
dicts and its recursive trie - nothing of the product's arrays.  `word_lm_reference.dense_automaton`
works on it unchanged, so the existing dense kernels and tests/lm_beam_reference.py decode it.

The table: for a node n >= 2, la[n] is the best ``weight * ln P(w | ())`` of a word w at or below
n; with OOV on never below ``unk = oov_score + weight * ln P(<unk> | ())``, which is la[1]; what is
not finite becomes 0.0, and la[0] = 0.0."""

import math

import numpy as np

from tests import word_lm_reference as ref

NEG_INF = ref.NEG_INF


class LookaheadScorer(ref.Scorer):
    """The pinned edge and end rules of K26 over states (trie node, context tuple).  ``table``
    replaces the rule's table (any finite values: the sums telescope for every one)."""

    def __init__(self, model, weight=1.0, bonus=0.0, oov_score=NEG_INF, table=None):
        super().__init__(model, weight, bonus, oov_score)
        self.la = self.table() if table is None else [float(v) for v in table]

    def unigram(self, w):
        return self.weight * self.model.stored((), w)       # the empty context stores every word

    def table(self):
        best = [NEG_INF] * len(self.trie.edges)

        def below(n):
            found = self.unigram(self.trie.word[n]) if self.trie.word[n] >= 0 else NEG_INF
            for m in self.trie.edges[n].values():
                found = max(found, below(m))
            best[n] = found
            return found

        below(0)
        best[0] = best[1] = NEG_INF
        unk = self.oov_score + self.unigram(ref.UNK)
        if self.oov and math.isfinite(unk):
            best = best[:2] + [max(v, unk) for v in best[2:]]
            best[1] = unk
        best = [v if math.isfinite(v) else 0.0 for v in best]
        best[0] = 0.0
        return best

    def full(self, n, h):
        """(what the word that n closes costs in full, context after, back-offs) or None."""
        if n == 0:
            return None
        w = -1 if n == 1 else self.trie.word[n]
        if w >= 0:
            return self.model.wd(h, w, self.weight)
        if not self.oov:
            return None
        score, after, steps = self.model.wd(h, ref.UNK, self.weight)
        return score + self.oov_score, after, steps

    def edge(self, n, h, c):
        la = self.la
        if c != self.model.space:
            if n == 1:
                return (1, h), np.float32(self.bonus), None
            if c in self.trie.edges[n]:
                m = self.trie.edges[n][c]
                return (m, h), np.float32((la[m] - la[n]) + self.bonus), None
            if self.oov:
                return (1, h), np.float32((la[1] - la[n]) + self.bonus), None
            return None, np.float32(NEG_INF), None
        closed = self.full(n, h)
        if closed is None:
            return None, np.float32(NEG_INF), None
        return (0, closed[1]), np.float32((closed[0] - la[n]) + self.bonus), closed[2]

    def end(self, n, h):
        if n == 0:
            return np.float32(self.model.wd(h, ref.EOS, self.weight)[0])
        closed = self.full(n, h)
        if closed is None:
            return np.float32(NEG_INF)
        return np.float32((closed[0] - self.la[n]) +
                          self.model.wd(closed[1], ref.EOS, self.weight)[0])


# ---- the effect of the rule on pruning: the utterances both the host and the device test use ------
EFFECT_CLASSES, EFFECT_BLANK, EFFECT_ORDER, EFFECT_STEPS = 6, 5, 2, 28
EFFECT_TEXTS = ['ab cab d a', 'dd acbd bb ca', 'c', 'bad ba ab', 'acbd acbd', 'cab ca c d']
EFFECT_SEEDS = (100, 101, 102, 103, 104, 105)
EFFECT_WIDTHS, EFFECT_WIDE = (4, 8), 512


def effect_batches(seeds=EFFECT_SEEDS):
    """One batch per seed of the six texts: (logits float32 [28, 6, 6], seq_len)."""
    from tests.test_gpu_word_lm import _logits
    seq_len = np.full(len(EFFECT_TEXTS), EFFECT_STEPS, dtype=np.int32)
    return [(_logits(np.random.default_rng(seed), EFFECT_STEPS, EFFECT_CLASSES, EFFECT_BLANK,
                     EFFECT_TEXTS, noise=1.5, peak=2.5), seq_len) for seed in seeds]


def effect_counts(decode, seeds=EFFECT_SEEDS):
    """``decode(logits, seq_len, width, lookahead)`` -> one label list per utterance.  Returns
    ({width: (plain, look-ahead)}, decodes): how many of the utterances (six per seed) decode, at
    that width, to what the plain search of width 512 decodes; and every decode, keyed (seed,
    width, lookahead)."""
    counts = {width: [0, 0] for width in EFFECT_WIDTHS}
    decodes = {}
    for seed, (logits, seq_len) in zip(seeds, effect_batches(seeds)):
        wide = decodes[(seed, EFFECT_WIDE, False)] = decode(logits, seq_len, EFFECT_WIDE, False)
        for width in EFFECT_WIDTHS:
            for ahead in (False, True):
                got = decodes[(seed, width, ahead)] = decode(logits, seq_len, width, ahead)
                counts[width][ahead] += sum(list(a) == list(b) for a, b in zip(got, wide))
    return {width: tuple(pair) for width, pair in counts.items()}, decodes
