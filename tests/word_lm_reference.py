"""An independent restatement of the word n-gram scorer (include/ctcasr.h, K24) that shares nothing
with the product's arrays: n-grams in dicts, ``Wd`` by dict lookup with the pinned order of adds,
and `dense_automaton`, which materialises the **dense** ``(next, score, final)`` automaton over the
reachable (trie node, context) pairs of a *small* model.  That automaton is the oracle: the
existing `hip.ctc_beam_decode_lm` / `ctc_beam_decode_nbest` on the GPU and
tests/lm_beam_reference.py on the CPU already decode it.

Word ids: 0 ``<unk>``, 1 ``</s>``, real words from 2 in ascending order of their label rows.
Contexts are tuples of word ids; their ids are their rank in (length, tuple) order."""

import math

import numpy as np

UNK, EOS = 0, 1
NEG_INF = float('-inf')


def words_of(row, space):
    words, word = [], []
    for c in list(row) + [space]:
        if c != space:
            word.append(int(c))
        elif word:
            words.append(tuple(word))
            word = []
    return words


class WordNgram:
    """Interpolated Witten-Bell over words, counts and probabilities in dicts."""

    def __init__(self, rows, order, space, vocab_size=0):
        self.order, self.space = order, space
        sentences = [words_of(row, space) for row in rows]
        frequency = {}
        for sentence in sentences:
            for word in sentence:
                frequency[word] = frequency.get(word, 0) + 1
        ranked = sorted(frequency, key=lambda word: (-frequency[word], word))
        self.vocab = sorted(ranked[:vocab_size] if vocab_size > 0 else ranked)
        self.word_id = {word: 2 + i for i, word in enumerate(self.vocab)}
        self.events = len(self.vocab) + 2
        self.counts = {(): {}}
        for sentence in sentences:
            ids = [self.word_id.get(word, UNK) for word in sentence] + [EOS]
            for i, event in enumerate(ids):
                for m in range(min(order - 1, i) + 1):
                    seen = self.counts.setdefault(tuple(ids[i - m:i]), {})
                    seen[event] = seen.get(event, 0) + 1
        self.contexts = sorted(self.counts, key=lambda h: (len(h), h))
        self.context_id = {h: i for i, h in enumerate(self.contexts)}

    def prob(self, h, w):
        """P(w | h) by the interpolated formula, evaluated directly (h any tuple of word ids)."""
        if h not in self.counts:
            return self.prob(h[1:], w)
        lower = self.prob(h[1:], w) if h else 1.0 / self.events
        seen, total = float(len(self.counts[h])), float(sum(self.counts[h].values()))
        if total == 0:
            return lower
        return (self.counts[h].get(w, 0) + seen * lower) / (total + seen)

    def stored(self, h, w):
        """ln P(w | h) of a pair the back-off form stores (seen, or any w at the empty context),
        else None."""
        if h and w not in self.counts[h]:
            return None
        return float(np.log(self.prob(h, w)))

    def backoff(self, h):
        seen, total = float(len(self.counts[h])), float(sum(self.counts[h].values()))
        return float(np.log(seen / (total + seen))) if total > 0 else 0.0

    def after(self, h, w):
        target = (h + (w,))[-(self.order - 1):] if self.order > 1 else ()
        while target not in self.counts:
            target = target[1:]
        return target

    def wd(self, h, w, weight=1.0):
        """(Wd(h, w) in float64, context after, number of back-offs): acc = 0; found: acc +=
        weight * ln P, stop; else acc += weight * ln bo(h), h = h less its oldest word."""
        acc, steps, first = 0.0, 0, h
        for _ in range(self.order):
            value = self.stored(h, w)
            if value is not None:
                return acc + weight * value, self.after(h, w), steps
            acc += weight * self.backoff(h)
            h, steps = h[1:], steps + 1
        raise AssertionError('the empty context stores every word: {} {}'.format(first, w))


def wd_tables(entries, backoff, parent, order, h, w):
    """``Wd`` over hand-built tables held in dicts: ``entries[(h, w)] = (lp, next context)``.
    Returns (float64 score, next context); a chain longer than ``order`` gives (-inf, 0)."""
    acc = 0.0
    for _ in range(order):
        if (h, w) in entries:
            return acc + entries[(h, w)][0], entries[(h, w)][1]
        acc += backoff[h]
        h = parent[h]
    return NEG_INF, 0


class Trie:
    """Node 0 the root, node 1 the out-of-vocabulary sink; ``edges[n]`` label -> node."""

    def __init__(self, model):
        self.edges, self.word = [{}, {}], [-1, -1]
        for word in model.vocab:
            node = 0
            for c in word:
                if c not in self.edges[node]:
                    self.edges[node][c] = len(self.edges)
                    self.edges.append({})
                    self.word.append(-1)
                node = self.edges[node][c]
            self.word[node] = model.word_id[word]


class Scorer:
    """The pinned edge and end rules over states (trie node, context tuple)."""

    def __init__(self, model, weight=1.0, bonus=0.0, oov_score=NEG_INF):
        self.model, self.trie = model, Trie(model)
        self.weight, self.bonus, self.oov_score = float(weight), float(bonus), float(oov_score)
        self.oov = math.isfinite(self.oov_score)

    def close(self, n, h):
        """(word score without bonus, context after, back-offs) or None where nothing closes."""
        if n == 0:
            return None
        w = -1 if n == 1 else self.trie.word[n]
        if w >= 0:
            return self.model.wd(h, w, self.weight)
        if not self.oov:
            return None
        score, after, steps = self.model.wd(h, UNK, self.weight)
        return (score if n == 1 else score + self.oov_score), after, steps

    def edge(self, n, h, c):
        """(next state or None, float32 score, back-offs of the lookup or None)."""
        if c != self.model.space:
            if n == 1:
                return (1, h), np.float32(self.bonus), None
            if c in self.trie.edges[n]:
                return (self.trie.edges[n][c], h), np.float32(self.bonus), None
            if self.oov:
                return (1, h), np.float32(self.oov_score + self.bonus), None
            return None, np.float32(NEG_INF), None
        closed = self.close(n, h)
        if closed is None:
            return None, np.float32(NEG_INF), None
        return (0, closed[1]), np.float32(closed[0] + self.bonus), closed[2]

    def end(self, n, h):
        if n == 0:
            return np.float32(self.model.wd(h, EOS, self.weight)[0])
        closed = self.close(n, h)
        if closed is None:
            return np.float32(NEG_INF)
        return np.float32(closed[0] + self.model.wd(closed[1], EOS, self.weight)[0])


def dense_automaton(scorer, classes, blank):
    """(next int32 [S, C], score float32 [S, C], final float32 [S], states, backoffs) over the
    (node, context) pairs reachable from (0, ()), which is state 0.  The blank's column and every
    forbidden edge are -inf and lead to state 0; ``backoffs[s]`` is the number of back-offs the
    space edge out of state s took (None: no lookup)."""
    index, states = {(0, ()): 0}, [(0, ())]
    rows_next, rows_score, backoffs = [], [], []
    at = 0
    while at < len(states):
        n, h = states[at]
        row_next, row_score = np.zeros(classes, dtype=np.int32), \
            np.full(classes, NEG_INF, dtype=np.float32)
        steps = None
        for c in range(classes):
            if c == blank:
                continue
            target, score, took = scorer.edge(n, h, c)
            if c == scorer.model.space:
                steps = took
            if target is None or score == NEG_INF:
                continue
            if target not in index:
                index[target] = len(states)
                states.append(target)
            row_next[c], row_score[c] = index[target], score
        rows_next.append(row_next)
        rows_score.append(row_score)
        backoffs.append(steps)
        at += 1
    final = np.array([scorer.end(n, h) for n, h in states], dtype=np.float32)
    return np.stack(rows_next), np.stack(rows_score), final, states, backoffs
