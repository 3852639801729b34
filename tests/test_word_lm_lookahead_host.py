"""Look-ahead scores inside a word (include/ctcasr.h, K26) on the host: `WordLmScorer.lookahead_table`,
`scaled(..., lookahead=True)`, `step` / `end_score` / `sequence_scores` under the table, the flag -
against tests/word_lm_lookahead_reference.py, and the effect of the rule on pruning, measured on
the Python references alone.  No GPU."""

import functools

import numpy as np
import pytest

from ctc_asr_amd import lm
from ctc_asr_amd.params import FLAGS
from tests import lm_beam_reference as lref
from tests import word_lm_lookahead_reference as laref
from tests import word_lm_reference as ref
from tests.test_gpu_word_lm import ALPHABETS, LEXICON, _models

CLASSES, BLANK = 6, 5
SPACE = ALPHABETS[(CLASSES, BLANK)][0]
SETTINGS = [(order, oov) for order in (1, 2, 3) for oov in (-np.inf, -4.0)]


@functools.lru_cache(maxsize=None)
def _pair(order, weight, bonus, oov):
    """(scaled WordLmScorer with its table, the reference's look-ahead scorer)."""
    model, restated = _models(CLASSES, BLANK, order)
    return (model.scaled(weight, bonus, oov, lookahead=True),
            laref.LookaheadScorer(restated, weight, bonus, oov))


def _prefixes(model):
    """The label row that leads to each trie node (None for the sink), by walking the vocabulary."""
    rows = {0: ()}
    for word in model.vocab:
        node = 0
        for i, c in enumerate(word):
            node = int(model.trie_next[node, c])
            rows[node] = tuple(word[:i + 1])
    return rows


# ------------------------------------------------------------------------------------------------
# 1. The table
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('order,oov', SETTINGS)
def test_table_is_the_brute_force_maximum_and_the_references(order, oov):
    for weight in (1.0, 0.7):
        scorer, restated = _pair(order, weight, 0.0, oov)
        table = scorer.lookahead
        assert table.dtype == np.float64 and table.shape == (scorer.num_nodes,)
        assert np.array_equal(table, scorer.lookahead_table())
        unigram = scorer.succ_lp[:scorer.num_words]
        unk = oov + unigram[lm.UNK]
        rows = _prefixes(scorer)
        assert sorted(rows) == [0] + list(range(2, scorer.num_nodes))
        assert len(LEXICON) == len(scorer.vocab)
        for node in range(2, scorer.num_nodes):
            below = [unigram[2 + i] for i, word in enumerate(scorer.vocab)
                     if tuple(word[:len(rows[node])]) == rows[node]]
            assert below, node
            want = max(below) if np.isneginf(oov) else max(max(below), unk)
            assert table[node] == want, node
        assert table[0] == 0.0
        assert table[1] == (0.0 if np.isneginf(oov) else unk)
        # the reference's trie numbers its nodes as the product's does: the same table, to the bit
        assert [dict(e) for e in restated.trie.edges] == \
            [{c: int(m) for c, m in enumerate(row) if m >= 0} for row in scorer.trie_next]
        assert table.tolist() == restated.la
    # a child is never above its parent (the bound only tightens on the way down) - unless the
    # parent is the root, where nothing is paid ahead
    for node in range(2, scorer.num_nodes):
        for child in scorer.trie_next[node][scorer.trie_next[node] >= 0]:
            assert table[child] <= table[node]


def _tiny(trie_next, trie_word, succ_lp, oov=-np.inf):
    """Three words (ids 2, 3, 4) over a hand-built trie; one context."""
    return lm.WordLmScorer(np.asarray(trie_next, dtype=np.int32), trie_word, [0, 5],
                           [0, 1, 2, 3, 4], succ_lp, [0] * 5, [0.0], [0], 1, 2, oov_score=oov)


#     0 -a-> 2 -a-> 3 (word 2)      0 -b-> 4 (word 3) -a-> 5 (word 4)
TINY_NEXT = [[2, 4, -1], [-1, -1, -1], [3, -1, -1], [-1, -1, -1], [5, -1, -1], [-1, -1, -1]]
TINY_WORD = [-1, -1, -1, 2, 3, 4]


def test_entries_that_are_not_finite_do_not_count():
    scorer = _tiny(TINY_NEXT, TINY_WORD, [-3.0, -1.0, -np.inf, -np.inf, -2.0])
    # word 2 (-inf) alone below nodes 2 and 3: nothing finite, 0.0; word 3 (-inf) at node 4 does
    # not count against word 4 (-2) below it
    assert scorer.lookahead_table().tolist() == [0.0, 0.0, 0.0, 0.0, -2.0, -2.0]
    # OOV on: unk = -1.5 + -3 joins every node >= 2 and is the sink's entry
    opened = _tiny(TINY_NEXT, TINY_WORD, [-3.0, -1.0, -np.inf, -np.inf, -2.0], oov=-1.5)
    assert opened.lookahead_table().tolist() == [0.0, -4.5, -4.5, -4.5, -2.0, -2.0]
    # ... unless <unk> itself is -inf: then as with OOV off, and the sink gets 0.0
    dead = _tiny(TINY_NEXT, TINY_WORD, [-np.inf, -1.0, -0.5, -np.inf, -2.0], oov=-1.5)
    assert dead.lookahead_table().tolist() == [0.0, 0.0, -0.5, -0.5, -2.0, -2.0]
    # scaled carries it; weight 0: 0 everywhere (-inf stays -inf and does not count)
    assert scorer.scaled(0.0, 0.3, lookahead=True).lookahead.tolist() == [0.0] * 6
    assert scorer.scaled(2.0, 0.0, lookahead=True).lookahead.tolist() == [0, 0, 0, 0, -4.0, -4.0]
    assert scorer.scaled(2.0, 0.0).lookahead is None and scorer.lookahead is None


def test_a_trie_that_is_no_tree_is_refused_by_name():
    lps = [-3.0, -1.0, -1.0, -1.5, -2.0]
    twice = [row[:] for row in TINY_NEXT]
    twice[4][1] = 3                                   # node 3 reached from 2 and from 4
    into_root = [row[:] for row in TINY_NEXT]
    into_root[5][2] = 0
    into_sink = [row[:] for row in TINY_NEXT]
    into_sink[3][1] = 1
    orphan = [row[:] for row in TINY_NEXT]
    orphan[4][0] = -1                                 # nothing leads to node 5
    loop = [row[:] for row in TINY_NEXT]
    loop[4][0] = -1
    loop[5][0] = 5                                    # node 5 reached once - from itself
    for bad in (twice, into_root, into_sink, orphan, loop):
        scorer = _tiny(bad, TINY_WORD, lps)           # loads as before ...
        plain = scorer.scaled(0.5, 0.1)
        assert plain.lookahead is None
        assert np.isfinite(plain.sequence_scores([[1]])[0])       # ... and scores as before
        with pytest.raises(ValueError, match='trie_next'):
            scorer.lookahead_table()
        with pytest.raises(ValueError, match='trie_next'):
            scorer.scaled(0.5, 0.1, lookahead=True)
    assert _tiny(TINY_NEXT, TINY_WORD, lps).scaled(0.5, 0.1, lookahead=True).lookahead is not None


def test_a_large_lexicon_builds_without_recursion():
    """20 000 random words of up to 40 labels: a trie far deeper than Python would recurse into
    comfortably, built level by level; the table of a few nodes is checked by hand."""
    rng = np.random.default_rng(3)
    words = sorted({tuple(rng.integers(0, 27, size=int(rng.integers(1, 41))).tolist())
                    for _ in range(20000)})
    rows = [list(word) + [27] for word in words]
    model = lm.build_word_ngram([sum(rows[i:i + 50], []) for i in range(0, len(rows), 50)], 1, 29,
                                27)
    table = model.scaled(1.0, 0.0, lookahead=True).lookahead
    assert model.num_nodes > 100000 and table.shape == (model.num_nodes,)
    unigram = model.succ_lp[:model.num_words]
    for first in range(3):
        node = int(model.trie_next[0, first])
        below = [unigram[2 + i] for i, word in enumerate(model.vocab) if word[0] == first]
        assert table[node] == max(below)


# ------------------------------------------------------------------------------------------------
# 2. The scores
# ------------------------------------------------------------------------------------------------
def _bits(value):
    return np.float32(value).view(np.int32)


@pytest.mark.parametrize('order,oov', SETTINGS)
def test_step_and_end_score_give_the_references_bits_on_every_reachable_state(order, oov):
    for weight, bonus in ((1.0, 0.0), (0.7, 0.4)):
        scorer, restated = _pair(order, weight, bonus, oov)
        _, _, _, states, _ = ref.dense_automaton(restated, CLASSES, BLANK)
        ids = restated.model.context_id
        edges = 0
        for n, h in states:
            for c in range(CLASSES):
                if c == BLANK:
                    continue
                target, score, _ = restated.edge(n, h, c)
                got_target, got = scorer.step(n, ids[h], c)
                assert _bits(got) == _bits(score), (n, h, c)
                if target is None or np.isneginf(score):
                    assert got_target is None
                else:
                    assert got_target == (target[0], ids[target[1]])
                    edges += 1
            assert _bits(scorer.end_score(n, ids[h])) == _bits(restated.end(n, h)), (n, h)
        assert edges > len(states)


def _random_rows(rng, count, oov):
    """Label rows of 1 - 12 labels: lexicon words with spaces, some with a letter changed (a word
    outside the lexicon), some cut short inside a word, some plain noise."""
    space, letters = ALPHABETS[(CLASSES, BLANK)]
    rows = []
    for _ in range(count):
        kind = int(rng.integers(0, 4))
        if kind == 3:
            row = rng.integers(0, CLASSES - 1, size=int(rng.integers(1, 13))).tolist()
        else:
            row = []
            while len(row) < 12:
                word = LEXICON[int(rng.integers(0, len(LEXICON)))]
                row += ([space] if row else []) + [letters['abcde'.index(ch)] for ch in word]
                if rng.random() < 0.3:
                    break
            row = row[:int(rng.integers(1, 13))]
            if kind == 1 and oov > -np.inf:
                row[int(rng.integers(0, len(row)))] = int(rng.integers(0, 4))
        rows.append(row)
    return rows


def _sum_of_magnitudes(scorer, row):
    """sum of |edge score| and |end score| along ``row`` (finite rows only)."""
    state, total = (0, 0), 0.0
    for c in row:
        state, score = scorer.step(state[0], state[1], int(c))
        total += abs(float(score))
    return total + abs(float(scorer.end_score(*state)))


@pytest.mark.parametrize('oov', [-np.inf, -4.0])
def test_the_sums_telescope(oov):
    """`sequence_scores` with and without the table: both -inf, or apart by no more than the
    roundings allow.  Every edge score is one float64 expression rounded once to float32 - a
    relative error of 2^-24 - and the float64 sums of either form are exact beside that; in exact
    arithmetic the two sums are equal.  So |difference| <= 2^-24 * (sum of |score| over both
    sums), plus the float64 roundings inside the expressions (16 per row at 2^-53 relative to
    magnitudes below 2^6: under 1e-13)."""
    rng = np.random.default_rng(17 if oov == -4.0 else 18)
    rows = _random_rows(rng, 1000, oov)
    finite, worst = 0, 0.0
    for order, weight, bonus in ((2, 1.0, 0.0), (3, 0.7, 0.4)):
        model, _ = _models(CLASSES, BLANK, order)
        plain, ahead = model.scaled(weight, bonus, oov), \
            model.scaled(weight, bonus, oov, lookahead=True)
        a, b = plain.sequence_scores(rows), ahead.sequence_scores(rows)
        for row, x, y in zip(rows, a, b):
            if np.isneginf(x) or np.isneginf(y):
                assert np.isneginf(x) and np.isneginf(y), row
                continue
            finite += 1
            bound = 2.0 ** -24 * (_sum_of_magnitudes(plain, row) +
                                  _sum_of_magnitudes(ahead, row)) + 1e-13
            assert abs(x - y) <= bound, (row, x, y, bound)
            worst = max(worst, abs(x - y))
    print('telescoping: {} finite rows of 2000, largest difference {:.3g}'.format(finite, worst))
    assert finite >= 400


@pytest.mark.parametrize('oov', [-np.inf, -4.0])
def test_weight_zero_is_the_plain_scorer_edge_by_edge(oov):
    for order in (1, 2, 3):
        model, restated = _models(CLASSES, BLANK, order)
        for bonus in (0.0, 0.4):
            plain, ahead = model.scaled(0.0, bonus, oov), \
                model.scaled(0.0, bonus, oov, lookahead=True)
            assert not ahead.lookahead[[0] + list(range(2, ahead.num_nodes))].any()
            _, _, _, states, _ = ref.dense_automaton(ref.Scorer(restated, 0.0, bonus, oov),
                                                     CLASSES, BLANK)
            for n, h in states:
                ctx = restated.context_id[h]
                for c in range(CLASSES - 1):
                    want, got = plain.step(n, ctx, c), ahead.step(n, ctx, c)
                    assert want[0] == got[0] and _bits(want[1]) == _bits(got[1]), (n, h, c)
                assert _bits(plain.end_score(n, ctx)) == _bits(ahead.end_score(n, ctx))


# ------------------------------------------------------------------------------------------------
# 3. The flag
# ------------------------------------------------------------------------------------------------
def test_the_flag_needs_a_word_model(tmp_path):
    from ctc_asr_amd.labels import ctoi
    FLAGS.reset()
    try:
        assert FLAGS.lm_lookahead is False
        words, chars = str(tmp_path / 'w.npz'), str(tmp_path / 'c.npz')
        rows = [[ctoi(ch) for ch in text] for text in ('ab cab a', 'a cab', 'ab ab')]
        lm.build_word_ngram(rows, 2, 29, ctoi(' ')).save(words)
        lm.build_char_ngram(rows, 2, 29).save(chars)
        with pytest.raises(ValueError, match='lm_lookahead'):
            FLAGS.parse(['--lm_lookahead'])
        FLAGS.reset()
        with pytest.raises(ValueError, match='lm_lookahead'):
            FLAGS.parse(['--lm_lookahead', '--lm_path', chars])
        FLAGS.reset()
        with pytest.raises(ValueError, match='lm_lookahead'):
            FLAGS.parse(['--nbest', '2', '--rescore_lm_path', words, '--lm_lookahead'])
        FLAGS.reset()
        assert FLAGS.parse(['--lm_path', words, '--lm_lookahead', '--lm_oov_score=-5',
                            '--lm_weight', '0.5']) == []
        scorer = lm.from_flags(29)
        assert isinstance(scorer.lookahead, np.ndarray) and scorer.oov_score == -5.0
        assert np.array_equal(scorer.lookahead,
                              lm.load(words, 29).scaled(0.5, 0.0, -5.0).lookahead_table())
        # the host re-ranker's totals do not depend on it: never a table there
        FLAGS.reset()
        assert FLAGS.parse(['--lm_path', words, '--lm_lookahead', '--nbest', '2',
                            '--rescore_lm_path', words]) == []
        assert lm.rescorer_from_flags(29).lookahead is None
        # without the flag: what there was
        FLAGS.reset()
        assert FLAGS.parse(['--lm_path', words]) == []
        assert lm.from_flags(29).lookahead is None
        # the file holds no table, with or without one on the scorer
        lm.load(words, 29).scaled(1.0, 0.0, lookahead=True).save(str(tmp_path / 'again.npz'))
        with np.load(str(tmp_path / 'again.npz')) as data:
            assert not any('look' in name for name in data.files)
    finally:
        FLAGS.reset()


# ------------------------------------------------------------------------------------------------
# 4. The effect, on the references
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference_decoder():
    """``decode(logits, seq_len, width, lookahead)`` under tests/lm_beam_reference.py, on the dense
    automata of the two reference scorers (built once; the device test decodes with it too)."""
    _, restated = _models(laref.EFFECT_CLASSES, laref.EFFECT_BLANK, laref.EFFECT_ORDER)
    dense = {ahead: ref.dense_automaton(scorer, laref.EFFECT_CLASSES, laref.EFFECT_BLANK)[:3]
             for ahead, scorer in ((False, ref.Scorer(restated, 1.0, 0.0)),
                                   (True, laref.LookaheadScorer(restated, 1.0, 0.0)))}

    def decode(logits, seq_len, width, ahead):
        nxt, score, final = dense[ahead]
        return lref.beam_search_decode(logits, seq_len, width, nxt, score, final,
                                       blank=laref.EFFECT_BLANK)[0]
    return decode


def test_a_narrow_beam_with_look_ahead_agrees_with_the_wide_plain_beam_more_often():
    """Closed vocabulary, order 2, weight 1, bonus 0, the utterances of `laref.effect_batches`.  At
    widths 4 and 8 the look-ahead decode equals the width-512 plain decode on strictly more
    utterances than the plain decode of that width does.  Over all six seeds (36 utterances) the
    reference counts 12 against 6 at width 4 and 19 against 10 at width 8, in 40 s of Python, nearly
    all of it in the six width-512 decodes; the host suite keeps seeds 103 and 104 (12 utterances:
    5 against 1, and 6 against 1), and the device test counts all 36 against the device's own
    width-512 decode."""
    counts, _ = laref.effect_counts(reference_decoder(), seeds=(103, 104))
    print('utterances of 12 equal to the width-512 plain decode (plain, look-ahead):', counts)
    for width in laref.EFFECT_WIDTHS:
        assert counts[width][1] > counts[width][0], (width, counts)
