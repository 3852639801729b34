"""The sentence-level truth of tests/word_lm_truth_reference.py against the CPU reference of the
fused search, no GPU: tests/lm_beam_reference.py at width 1024 (which prunes nothing here) on the
dense automaton of `word_lm_reference.Scorer` and of `word_lm_lookahead_reference.LookaheadScorer`
must return the argmax over ALL labellings of ln p_ctc + the sentence score.  The edge rules of
those two scorers are what every other word-model test leans on; the truth shares nothing with
them but `WordNgram`.  Protocol and bar are `check_truth`'s of tests/test_lm_host.py.

The bar's absolute term, 5e-5, is check_truth's: about 3 T <= 30 rounded float32 operations on
intermediates below 32 in magnitude, each off by at most 2^-24 * 32 = 1.9e-6.  `largest_
intermediate` measures that magnitude for the best labelling - every finite cell of its search
lattice (prefix totals ending in a blank and in a label, the model's prefix sums included), the
frame values, the edge scores of the rule in use (so look-ahead's la differences) and the end
score - and where it exceeds 32 the absolute term grows in proportion, 5e-5 * largest / 32
(`truth.bar`).  It is printed per case."""

import functools

import numpy as np
import pytest

from oracle import ctc as octc
from tests import lm_beam_reference as lref
from tests import word_lm_lookahead_reference as laref
from tests import word_lm_reference as ref
from tests import word_lm_truth_reference as truth

NEG_INF = float('-inf')


@functools.lru_cache(maxsize=None)
def dense_tables(classes, blank, space, order, weight, bonus, oov, ahead):
    """(next, score, final) of the dense automaton of the restated scorer, plain or look-ahead."""
    ngram = truth.model(classes, blank, space, order)
    kind = laref.LookaheadScorer if ahead else ref.Scorer
    nxt, score, final, _, _ = ref.dense_automaton(kind(ngram, weight, bonus, oov), classes, blank)
    return nxt, score, final


def _lse(a, b):
    if a == NEG_INF:
        return b
    if b == NEG_INF:
        return a
    return max(a, b) + np.log1p(np.exp(-abs(a - b)))


def largest_intermediate(logits, blank, labelling, tables):
    """The largest finite magnitude the fused search meets on its way to ``labelling``'s total, in
    float64: frame values, edge and end scores of ``tables``, and every cell (blank, label, total)
    of the lattice over the labelling's prefixes, each with its prefix's model score."""
    nxt, score, final = tables
    x = octc.log_softmax(np.asarray(logits, dtype=np.float64))
    y = list(labelling)
    state, prefix, seen = 0, [0.0], []
    for c in y:
        seen.append(float(score[state, c]))
        prefix.append(prefix[-1] + seen[-1])
        state = int(nxt[state, c])
    seen.append(float(final[state]))
    seen += [float(v) for v in x[:, sorted(set(y) | {blank})].ravel()]
    pb = [0.0] + [NEG_INF] * len(y)
    pl = [NEG_INF] * (len(y) + 1)
    for t in range(x.shape[0]):
        new_b = [_lse(pb[k], pl[k]) + x[t, blank] for k in range(len(y) + 1)]
        new_l = [NEG_INF]
        for k in range(1, len(y) + 1):
            repeat = k >= 2 and y[k - 1] == y[k - 2]
            enter = pb[k - 1] if repeat else _lse(pb[k - 1], pl[k - 1])
            new_l.append(_lse(pl[k], enter) + x[t, y[k - 1]])
        pb, pl = new_b, new_l
        for k in range(len(y) + 1):
            seen += [pb[k] + prefix[k], pl[k] + prefix[k], _lse(pb[k], pl[k]) + prefix[k]]
    seen.append(_lse(pb[-1], pl[-1]) + prefix[-1] + float(final[state]))
    return max(abs(v) for v in seen if np.isfinite(v))


def check_word_truth(decode, classes, num_steps, blank, space, tables_of=dense_tables):
    """``decode(logits, order, weight, bonus, oov, ahead)`` -> (paths, logp) of an unpruned
    `log_softmax` search, for every setting, vocabulary and rule of the case.  Returns the facts of
    the best labellings that were compared."""
    assert sum((classes - 1) ** k for k in range(num_steps + 1)) <= 1023
    logits, _ = truth.inputs(classes, num_steps, blank)
    seen = {'words': 0, 'backoffs': 0, 'oov seeds': {}}
    for order, weight, bonus in truth.SETTINGS:
        for oov in (NEG_INF, truth.OOV_ON):
            ranked = truth.ranked(classes, num_steps, blank, space, order, weight, bonus, oov)
            for ahead in (False, True):
                paths, logp = decode(logits, order, weight, bonus, oov, ahead)
                tables = tables_of(classes, blank, space, order, weight, bonus, oov, ahead)
                skipped, worst, largest, with_oov = 0, 0.0, 0.0, 0
                for b, ((best, value, facts), (_, runner_up, _)) in enumerate(ranked):
                    if truth.near_tie(value, runner_up):
                        skipped += 1
                        continue
                    assert tuple(paths[b]) == best, (order, oov, ahead, b)
                    size = max(largest_intermediate(logits[:, b], blank, best, tables),
                               facts['largest'])
                    err = abs(float(logp[b]) - value)
                    assert err <= truth.bar(value, size), (order, oov, ahead, b, float(logp[b]),
                                                           value)
                    worst, largest = max(worst, err / truth.bar(value, size)), max(largest, size)
                    with_oov += facts['oov'] > 0
                    seen['words'] = max(seen['words'], facts['words'])
                    if order > 1:
                        seen['backoffs'] = max(seen['backoffs'], facts['backoffs'])
                print('word truth C {} T {} blank {} space {} order {} weight {} bonus {} oov {} '
                      '{}: skipped {} of {}, largest error {:.2%} of the bar, largest '
                      'intermediate {:.1f}, best labellings with an OOV word {}'
                      .format(classes, num_steps, blank, space, order, weight, bonus, oov,
                              'look-ahead' if ahead else 'plain', skipped, truth.SEEDS, worst,
                              largest, with_oov))
                assert skipped * 10 <= truth.SEEDS, skipped
                if oov > NEG_INF:
                    seen['oov seeds'][(order, ahead)] = with_oov
    # the paths the case is there for, so that another generator or seed cannot empty it
    # (per case and rule, as the OOV rules ask: a one-letter alphabet at order 1 may hold none)
    for ahead in (False, True):
        assert sum(n for (_, rule), n in seen['oov seeds'].items() if rule == ahead) >= 1, seen
    assert seen['backoffs'] >= 1, seen
    assert seen['words'] >= 2 or num_steps < 5, seen     # two words and a space need 3 frames
    return seen


def test_sentence_score_by_hand():
    """The restatement itself on a model small enough to add up by hand."""
    space, a, b = 0, 1, 2
    ngram = ref.WordNgram([(a, space, a, a), (a,)], 2, space)
    ids = ngram.word_id
    assert ids == {(a,): 2, (a, a): 3}
    one = ngram.wd((), 2)[0]
    end_after_a = ngram.wd((2,), ref.EOS)[0]
    score, facts = truth.sentence_score(ngram, (a,))
    assert score == one + end_after_a and facts['words'] == 1 and facts['oov'] == 0
    # a trailing space closes the word; the end is then that of the root: the same sentence
    assert truth.sentence_score(ngram, (a, space))[0] == score
    assert truth.sentence_score(ngram, (a, space), bonus=0.5)[0] == score + 1.0
    assert truth.sentence_score(ngram, (a,), bonus=0.5)[0] == score + 0.5
    assert truth.sentence_score(ngram, ())[0] == ngram.wd((), ref.EOS)[0]
    for bad in ((space,), (space, a), (a, space, space), (a, space, space, a)):
        assert truth.sentence_score(ngram, bad, oov_score=-1.0)[0] == NEG_INF
    # 'b' leaves the trie, 'aaa' too (beyond 'aa'); both cost Wd(h, <unk>) + oov
    unk, after_unk, _ = ngram.wd((), ref.UNK)
    for word in ((b,), (a, a, a), (a, b)):
        assert truth.sentence_score(ngram, word)[0] == NEG_INF
        got, facts = truth.sentence_score(ngram, word, oov_score=-3.0)
        assert got == (unk - 3.0) + ngram.wd(after_unk, ref.EOS)[0] and facts['oov'] == 1
    # the weight scales the model's part only
    got = truth.sentence_score(ngram, (a, space, b), 0.5, 0.25, -3.0)[0]
    first, h, _ = ngram.wd((), 2, 0.5)
    second, h, _ = ngram.wd(h, ref.UNK, 0.5)
    assert got == first + (second - 3.0) + ngram.wd(h, ref.EOS, 0.5)[0] + 0.75


@pytest.mark.parametrize('classes,num_steps,blank,space', truth.CASES)
def test_reference_unpruned_search_finds_the_best_sentence(classes, num_steps, blank, space):
    if classes > 3:     # a letter that no word of the lexicon holds
        letters = truth.letters_of(classes, blank, space)
        assert letters[-1] not in {c for row in truth.corpus(classes, blank, space) for c in row}

    def decode(logits, order, weight, bonus, oov, ahead):
        tables = dense_tables(classes, blank, space, order, weight, bonus, oov, ahead)
        return lref.beam_search_decode(logits, [num_steps] * truth.SEEDS, 1024, *tables,
                                       blank=blank, normalization='log_softmax')
    check_word_truth(decode, classes, num_steps, blank, space)
