"""Sentence-level truth of the word-model beam searches (include/ctcasr.h, K24 and K26), written
on WORDS: what a whole labelling is worth under the fused model, from `WordNgram.wd` and
`WordNgram.word_id` of tests/word_lm_reference.py and nothing else - no trie, no edge rules, no
automaton, nothing of ctc_asr_amd.lm.  The pinned rules are stated per edge; summed along a
labelling they say:

  - the labelling is split at the spaces; a leading or a doubled space has no edge: -inf;
  - every word costs Wd(h, w); a word outside the vocabulary costs Wd(h, <unk>) + oov_score - the
    same whether it is a proper prefix of a vocabulary word ("other n": one charge at the space) or
    leaves the trie (oov_score on the edge into the sink, Wd(h, <unk>) at the space) -, and -inf
    with a closed vocabulary (oov_score = -inf);
  - the context advances as Wd returns it;
  - a word still open at the end is closed by the same rule, and Wd(h, </s>) is added, without a
    bonus;
  - every label, the spaces included, adds `bonus` ("bonus is added per label": each edge rule of
    the header ends in "+ bonus", the end rule says "without a bonus").

With look-ahead (K26) the sums telescope to the same value for every finite table, so this is the
truth of both rules.  `ranked` adds ln p_ctc from the exhaustive enumeration of all C^T paths."""

import functools
import math

import numpy as np

from oracle import ctc as octc
from tests.word_lm_reference import EOS, UNK, WordNgram

NEG_INF = float('-inf')
SEEDS = 10
# (classes, frames, blank, space): at most 1023 prefixes exist, so width 1024 prunes nothing
CASES = [(3, 9, 2, 0), (3, 9, 0, 1), (3, 9, 1, 2),
         (4, 5, 3, 0), (4, 5, 0, 3), (4, 5, 1, 2),
         (5, 4, 2, 4), (5, 4, 0, 1)]
# (order, weight, bonus)
SETTINGS = [(1, 1.0, 0.0), (2, 0.7, 0.4), (3, 1.0, 0.0)]
# The finite oov_score.  A trial at -4 never put an out-of-vocabulary word into a best labelling
# where every letter is in the lexicon; -1 costs an unknown word about what a rare known one costs.
OOV_ON = -1.0
# Lexicons and corpora in letters; a letter is a label that is neither the blank nor the space, in
# ascending order.  C = 3 has one letter.  Where there are more, the last one is in no word: a
# labelling that holds it holds an out-of-vocabulary word that leaves the trie at once.  'aa' (C
# <= 4) and 'b', 'ba' (C = 5) are proper prefixes of vocabulary words and no words themselves.
CORPORA = {
    1: ['a aaa', 'aaa a', 'a', 'aaa', 'aaa a aaa', 'aa a', 'a aa', 'aa', 'aaaa', 'a aaaa', 'aaaa aa'],
    2: ['a aaa', 'aaa a', 'a', 'aaa', 'aaa a aaa', 'aa a', 'a aa', 'aa', 'aaaa', 'a aaaa', 'aaaa aa'],
    3: ['a ab', 'ab bab a', 'bab a', 'a a ab', 'ab', 'bab ab a a', 'b a', 'ab b'],
}
# the vocabulary keeps the most frequent words; the rest of the corpus counts as <unk>
VOCAB_SIZE = {1: 2, 2: 2, 3: 3}


def letters_of(classes, blank, space):
    return [c for c in range(classes) if c not in (blank, space)]


def spell(text, classes, blank, space):
    letters = letters_of(classes, blank, space)
    return tuple(space if ch == ' ' else letters['abc'.index(ch)] for ch in text)


@functools.lru_cache(maxsize=None)
def corpus(classes, blank, space):
    texts = CORPORA[classes - 2]
    return tuple(spell(text, classes, blank, space) for text in texts)


@functools.lru_cache(maxsize=None)
def model(classes, blank, space, order):
    return WordNgram(corpus(classes, blank, space), order, space, VOCAB_SIZE[classes - 2])


def sentence_score(ngram, labelling, weight=1.0, bonus=0.0, oov_score=NEG_INF):
    """(score in float64, facts): what the fused search adds to ln p_ctc(labelling).  ``facts`` is
    a dict: ``words``, ``oov`` (out-of-vocabulary words), ``backoffs`` (the most back-off steps
    of one lookup) and ``largest`` (the largest magnitude among the word scores and the running
    sum)."""
    space = ngram.space
    facts = {'words': 0, 'oov': 0, 'backoffs': 0, 'largest': 0.0}
    words, word = [], []
    for c in labelling:
        if c != space:
            word.append(int(c))
            continue
        if not word:                       # a leading or a doubled space
            return NEG_INF, facts
        words.append(tuple(word))
        word = []
    if word:                               # still open at the end: it closes
        words.append(tuple(word))
    total, h = 0.0, ()
    for w in words + [None]:
        if w is None:
            cost, h, steps = ngram.wd(h, EOS, weight)
        elif w in ngram.word_id:
            cost, h, steps = ngram.wd(h, ngram.word_id[w], weight)
            facts['words'] += 1
        else:
            if not math.isfinite(oov_score):
                return NEG_INF, facts
            cost, h, steps = ngram.wd(h, UNK, weight)
            cost += oov_score
            facts['words'] += 1
            facts['oov'] += 1
        total += cost
        facts['backoffs'] = max(facts['backoffs'], steps)
        facts['largest'] = max(facts['largest'], abs(cost), abs(total))
    total += bonus * len(labelling)
    facts['largest'] = max(facts['largest'], abs(total))
    return total, facts


@functools.lru_cache(maxsize=None)
def inputs(classes, num_steps, blank):
    """(logits float32 [T, SEEDS, C], one dict labelling -> ln p_ctc per utterance)."""
    rng = np.random.default_rng(30000 * classes + 100 * num_steps + blank)
    logits = (rng.normal(size=(num_steps, SEEDS, classes)) * 2).astype(np.float32)
    logits.setflags(write=False)
    tables = []
    for b in range(SEEDS):
        post = octc.brute_force_posteriors(logits[:, b].astype(np.float64), blank)
        assert abs(sum(post.values()) - 1.0) < 1e-12
        tables.append({label: math.log(p) for label, p in post.items() if p > 0})
    return logits, tuple(tables)


@functools.lru_cache(maxsize=None)
def ranked(classes, num_steps, blank, space, order, weight, bonus, oov_score, keep=2):
    """Per utterance the ``keep`` best labellings by ln p_ctc + sentence score, best first:
    (labelling, value, facts of its sentence score).  Labellings worth -inf are left out."""
    ngram = model(classes, blank, space, order)
    _, tables = inputs(classes, num_steps, blank)
    result = []
    for table in tables:
        fused = []
        for label, logp in table.items():
            score, facts = sentence_score(ngram, label, weight, bonus, oov_score)
            if score > NEG_INF:
                fused.append((label, logp + score, facts))
        fused.sort(key=lambda entry: -entry[1])
        result.append(tuple(fused[:keep]))
    return tuple(result)


def near_tie(value, runner_up):
    """check_truth's rule: the two fused posteriors are within 1e-4 relative."""
    return math.exp(runner_up - value) > 1 - 1e-4


def bar(value, largest=32.0):
    """check_truth's bar, 1e-5 relative + 5e-5 absolute.  The absolute term is the float32 worst
    case of about 3 T <= 30 rounded operations on intermediates below 32 in magnitude; it grows
    in proportion where ``largest`` exceeds 32."""
    return 1e-5 * abs(value) + 5e-5 * max(1.0, largest / 32.0)
