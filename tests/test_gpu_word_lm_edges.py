"""The three fused forms of the beam search (csrc/beam.hip `LM == 1` dense automaton, `LM == 2` word
n-gram, `LM == 3` the same with look-ahead) against exhaustive truth and at their edges.

Oracles, in order of strength:
  1. tests/word_lm_truth_reference.py: the best labellings of the exhaustive enumeration, scored on
     words - it shares nothing with the edge rules the other two lean on;
  2. tests/lm_beam_reference.py on the dense automaton of the restated scorers, at the bars of
     test_gpu_word_lm.py: path and length equal, row zero beyond out_len, logp rtol 1e-5 /
     atol 1e-3;
  3. bit equality with the dense GPU kernels (`ctc_beam_decode_nbest(scorer=dense)` and
     `ctc_beam_decode_lm`) on that automaton, where the CPU reference is too slow.
Every case that is there to reach a particular path asserts that it does."""

import ctypes
import functools

import numpy as np
import pytest
import torch

from ctc_asr_amd import lm
from oracle import ctc as octc
from tests import lm_beam_reference as lref
from tests import nbest_reference
from tests import word_lm_lookahead_reference as laref
from tests import word_lm_reference as ref
from tests import word_lm_truth_reference as truth
from tests.test_gpu_word_lm import LEXICON, NORMS, _dense_nbest, _facts, _same_bits, _t, _word
from tests.test_gpu_word_lm_lookahead import _raw
from tests.test_word_lm_truth_host import check_word_truth, dense_tables, largest_intermediate

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NEG_INF = float('-inf')
BAD_ARGUMENT = -1
MAIN = (29, 28, 1)          # (classes, blank, space) of most cases below


# ------------------------------------------------------------------------------------------------
# Alphabets, corpora, models
# ------------------------------------------------------------------------------------------------
def _letter_ids(layout):
    """The labels of 'abcde': five ids spread over the labels that are neither the blank nor the
    space.  'a', which every lexicon here uses, gets the LAST such id; an alphabet with fewer
    than five free labels shares them."""
    classes, blank, space = layout
    free = [c for c in range(classes) if c not in (blank, space)]
    spread = [free[i * (len(free) - 1) // 4] for i in range(5)]
    return {'a': spread[4], 'b': spread[0], 'c': spread[1], 'd': spread[2], 'e': spread[3]}


def _spell(text, layout):
    ids = _letter_ids(layout)
    return tuple(layout[2] if ch == ' ' else ids[ch] for ch in text)


@functools.lru_cache(maxsize=None)
def _zipf_corpus(layout, lexicon=tuple(LEXICON), sentences=40, shortest=1, longest=5):
    rng = np.random.default_rng(7)
    rows = []
    for _ in range(sentences):
        words = [lexicon[min(int(rng.zipf(1.4)) - 1, len(lexicon) - 1)]
                 for _ in range(int(rng.integers(shortest, longest + 1)))]
        rows.append(_spell(' '.join(words), layout))
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def _pair(layout, order, rows=None, vocab_size=0):
    """(the product's model, the restated one) of a corpus of label rows."""
    classes, blank, space = layout
    rows = _zipf_corpus(layout) if rows is None else rows
    return (lm.build_word_ngram(rows, order, classes, space, vocab_size, blank=blank),
            ref.WordNgram(rows, order, space, vocab_size))


@functools.lru_cache(maxsize=None)
def _setup(layout, order, weight, bonus, oov, ahead, rows=None, vocab_size=0):
    """(scaled scorer of the product, dense `LmScorer` of the restated rules, back-offs per dense
    state, the restated n-gram)."""
    model, restated = _pair(layout, order, rows, vocab_size)
    kind = laref.LookaheadScorer if ahead else ref.Scorer
    nxt, score, final, _, backoffs = ref.dense_automaton(kind(restated, weight, bonus, oov),
                                                         layout[0], layout[1])
    return (model.scaled(weight, bonus, oov, lookahead=ahead), lm.LmScorer(nxt, score, final),
            backoffs, restated)


def _lean(rng, num_steps, layout, texts, noise=0.6, peak=3.0, blank_bias=2.5):
    """Noise, and row b leans towards a spelling of ``texts[b]`` - test_gpu_word_lm.py's `_logits`
    for any alphabet."""
    classes, blank, _ = layout
    logits = rng.normal(size=(num_steps, len(texts), classes)) * noise
    logits[:, :, blank] += blank_bias
    for b, text in enumerate(texts):
        labels = _spell(text, layout)
        stride = max(num_steps // (len(labels) + 1), 1)
        for i, c in enumerate(labels):
            if i * stride + 1 < num_steps:
                logits[i * stride + 1, b, c] += peak
                logits[i * stride + 1, b, blank] -= blank_bias
    return logits.astype(np.float32)


# ------------------------------------------------------------------------------------------------
# The oracles
# ------------------------------------------------------------------------------------------------
def _against_cpu(got, logits, seq_len, width, dense, blank, norm):
    """Oracle 2 on the top path of ``got``; returns the reference's paths."""
    paths, logp = lref.beam_search_decode(logits, seq_len, width, dense.next, dense.score,
                                          dense.final, blank=blank, normalization=norm)
    for b, path in enumerate(paths):
        n = int(got[1][b, 0])
        assert got[0][b, 0, :n].tolist() == path, (b, width, norm)
        assert (got[0][b, 0, n:] == 0).all()
    assert np.allclose(got[2][:, 0], logp, rtol=1e-5, atol=1e-3), (got[2][:, 0], logp)
    return paths


def _dense_top(hip, logits, seq_len, width, dense, blank, norm):
    got = hip.ctc_beam_decode_lm(_t(logits), _t(np.asarray(seq_len), torch.int32), width, dense,
                                 blank=blank, normalization=norm)
    return tuple(t.cpu().numpy() for t in got)


def _against_dense(hip, logits, seq_len, width, scorer, dense, blank, norm, tops=(1,)):
    """Oracle 3: the n-best lists of every ``tops`` and the top-1 decode.  Returns the last list."""
    for top_paths in tops:
        got = _word(hip, logits, seq_len, width, scorer, top_paths, blank, norm)
        want = _dense_nbest(hip, logits, seq_len, width, dense, top_paths, blank, norm)
        assert _same_bits(got, want), (width, norm, top_paths)
    top = _dense_top(hip, logits, seq_len, width, dense, blank, norm)
    assert _same_bits((got[0][:, 0], got[1][:, 0], got[2][:, 0]), top), (width, norm)
    return got


def _empty_beyond(got):
    """Ranks k >= n_paths: out_len 0, logp -inf, labels 0; rows are zero beyond out_len."""
    out, out_len, logp, n_paths = got
    for b in range(out.shape[0]):
        for k in range(out.shape[1]):
            if k >= n_paths[b]:
                assert out_len[b, k] == 0 and np.isneginf(logp[b, k]) and (out[b, k] == 0).all()
            assert (out[b, k, out_len[b, k]:] == 0).all()


# ------------------------------------------------------------------------------------------------
# 1. Truth on the device (oracle 1)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('classes,num_steps,blank,space', truth.CASES)
def test_unpruned_search_finds_the_best_sentences(hip, classes, num_steps, blank, space):
    """Width 1024 prunes nothing here, so both rules must return the truth's best labelling at
    its value (check_truth's protocol and bar) - and its eight best, in order: the exact form of
    "the table only steers pruning".  Adjacent ranks within 1e-4 relative are near-ties and are
    not compared.  The two launches also expand the same branches and look up the same words."""
    layout = (classes, blank, space)
    rows, vocab_size = truth.corpus(*layout), truth.VOCAB_SIZE[classes - 2]
    seq_len = [num_steps] * truth.SEEDS
    lists = {}

    def decode(logits, order, weight, bonus, oov, ahead):
        scorer = _pair(layout, order, rows, vocab_size)[0].scaled(weight, bonus, oov,
                                                                  lookahead=ahead)
        stats = torch.full((truth.SEEDS, 2), -1, dtype=torch.int64, device=DEV)
        got = _word(hip, np.array(logits), seq_len, 1024, scorer, 8, blank, 'log_softmax',
                    stats=stats)       # (a copy: the shared inputs are read-only)
        lists[(order, oov, ahead)] = got + (stats.cpu().numpy(),)
        return ([got[0][b, 0, :got[1][b, 0]].tolist() for b in range(truth.SEEDS)], got[2][:, 0])

    check_word_truth(decode, classes, num_steps, blank, space)
    logits, _ = truth.inputs(classes, num_steps, blank)
    compared = 0
    for order, weight, bonus in truth.SETTINGS:
        for oov in (NEG_INF, truth.OOV_ON):
            plain, ahead = lists[(order, oov, False)], lists[(order, oov, True)]
            assert np.array_equal(plain[4], ahead[4]), (order, oov, plain[4], ahead[4])
            assert (plain[4][:, 1] <= plain[4][:, 0]).all() and (plain[4][:, 0] > 0).all()
            tables = [dense_tables(classes, blank, space, order, weight, bonus, oov, rule)
                      for rule in (False, True)]
            best = truth.ranked(classes, num_steps, blank, space, order, weight, bonus, oov, 9)
            for b, entries in enumerate(best):
                values = [value for _, value, _ in entries]
                for got in (plain, ahead):
                    assert got[3][b] >= min(len(entries), 8)
                    if len(entries) < 8:        # whatever else the beam holds is worth -inf
                        assert np.isneginf(got[2][b, len(entries):]).all()
                for k, (label, value, _) in enumerate(entries[:8]):
                    if any(0 <= j < len(values) - 1 and truth.near_tie(values[j], values[j + 1])
                           for j in (k - 1, k)):
                        continue
                    size = max(largest_intermediate(logits[:, b], blank, label, t) for t in tables)
                    for got in (plain, ahead):
                        assert tuple(got[0][b, k, :got[1][b, k]].tolist()) == label, (order, oov,
                                                                                      b, k)
                        assert abs(float(got[2][b, k]) - value) <= truth.bar(value, size)
                    assert abs(float(plain[2][b, k]) - float(ahead[2][b, k])) <= \
                        truth.bar(value, size)
                    compared += 1
    print('ranks compared with the truth, both rules:', compared)
    assert compared >= 6 * truth.SEEDS * 4


# ------------------------------------------------------------------------------------------------
# 2. Alphabet layouts (oracles 2 and 3)
# ------------------------------------------------------------------------------------------------
LAYOUTS = [(3, 2, 0), (3, 0, 1), (3, 1, 2), (29, 0, 28), (29, 5, 6), (64, 63, 0), (64, 0, 63),
           (64, 20, 21)]
LAYOUT_TEXTS = ['ab d a', 'acbd a a', 'bb a', 'c']       # rows 1, 2: word pairs the corpus lacks
ONE_LETTER_TEXTS = ['a a a', 'aaa a a', 'a aaa', 'a']     # 'a a' is such a pair there


@pytest.mark.parametrize('layout', LAYOUTS, ids=lambda layout: '-'.join(map(str, layout)))
def test_alphabet_layouts(hip, layout):
    """The blank first, last and in the middle; the space label 0, the last label and beside the
    blank; C = 3, the smallest alphabet there is (blank, space, one letter: the corpus of the
    truth cases), and C = 64, where lane 63 is a letter, the space or the blank.  The last free
    label is a letter of the lexicon."""
    classes, blank, space = layout
    rows, vocab_size = (truth.corpus(*layout), truth.VOCAB_SIZE[1]) if classes == 3 else (None, 0)
    texts = ONE_LETTER_TEXTS if classes == 3 else LAYOUT_TEXTS
    free = [c for c in range(classes) if c not in (blank, space)]
    assert any(free[-1] in word for word in _pair(layout, 1, rows, vocab_size)[1].vocab)
    rng = np.random.default_rng(1000 * classes + 10 * blank + space)
    num_steps = 20
    logits = _lean(rng, num_steps, layout, texts, peak=4.0)
    seq_len = np.array([num_steps - 3, num_steps, num_steps, 1], dtype=np.int32)
    most_words, most_backoffs = 0, 0
    for order, weight, bonus in ((1, 1.0, 0.0), (2, 0.7, 0.4)):
        for oov in (NEG_INF, -4.0):
            for ahead in (False, True):
                scorer, dense, backoffs, _ = _setup(layout, order, weight, bonus, oov, ahead,
                                                    rows, vocab_size)
                for norm in NORMS:
                    got = _against_dense(hip, logits, seq_len, 8, scorer, dense, blank, norm,
                                         (8, 1))
                    paths = _against_cpu(got, logits, seq_len, 8, dense, blank, norm)
                    _against_dense(hip, logits, seq_len, 100, scorer, dense, blank, norm, (8,))
                    words, backed = _facts(paths, dense, backoffs, space)
                    most_words = max(most_words, words)
                    if order > 1:
                        most_backoffs = max(most_backoffs, backed)
    assert most_words >= 2, 'no decoded hypothesis of this layout holds two words'
    assert most_backoffs >= 1, 'no scored space edge of this layout backed off'


# ------------------------------------------------------------------------------------------------
# 3. Width seams (oracle 2 at widths <= 65, oracle 3 at all)
# ------------------------------------------------------------------------------------------------
WIDTHS = [1, 2, 63, 64, 65, 256, 257, 1023, 1024]


@pytest.mark.parametrize('width', WIDTHS)
def test_width_seams(hip, width):
    """Both sides of the `PER` seams of `beam_expand` (64 / 65, 256 / 257), the narrowest beams and
    the widest, for the dense scorer (the device-side oracle of the other two: against the CPU
    reference at widths <= 65 and, on a short row, at 256 / 257), the word scorer and look-ahead
    (against the dense kernels, bit for bit).  With OOV on every label extends every hypothesis,
    so the beam is full: `n_paths` is the width."""
    rng = np.random.default_rng(width)
    num_steps = 12
    logits = _lean(rng, num_steps, MAIN, ['ab d a', 'dd bb', 'c'], noise=1.0)
    seq_len = np.array([num_steps, num_steps - 4, num_steps], dtype=np.int32)
    for ahead in (False, True):
        scorer, dense, _, _ = _setup(MAIN, 2, 0.7, 0.4, -4.0, ahead)
        for norm in NORMS:
            tops = (1, width) if width > 1 else (1,)
            got = _against_dense(hip, logits, seq_len, width, scorer, dense, 28, norm, tops)
            assert (got[3] == width).all(), got[3]
            _empty_beyond(got)
            if width <= 65:
                _against_cpu(got, logits, seq_len, width, dense, 28, norm)
            elif width in (256, 257) and norm == NORMS[ahead]:
                # the dense kernels go through the same `PER` dispatch as the word kernels, so at
                # this seam the CPU reference judges too - every leaf of the final beam, which a
                # slip of the dispatch changes long before it changes the best one: one row, five
                # frames, the beam full
                short = np.array([5], dtype=np.int32)
                one = _word(hip, logits[:, :1], short, width, scorer, width, 28, norm)
                leaves = nbest_reference.nbest(logits[:, :1], short, width, dense.next, dense.score,
                                               dense.final, blank=28, normalization=norm)[0]
                totals = {tuple(path): total for path, total in leaves}
                assert one[3][0] == width == len(totals)
                held = {tuple(one[0][0, k, :one[1][0, k]].tolist()): one[2][0, k]
                        for k in range(width)}
                assert set(held) == set(totals)
                assert all(np.isclose(held[path], totals[path], rtol=1e-5, atol=1e-3)
                           for path in held)
                assert tuple(leaves[0][0]) == tuple(one[0][0, 0, :one[1][0, 0]].tolist())


@pytest.mark.parametrize('ahead', [False, True], ids=['plain', 'look-ahead'])
def test_a_final_beam_smaller_than_top_paths(hip, ahead):
    """Closed vocabulary, one frame: the beam holds the empty prefix and the first letters of the
    lexicon - fewer leaves than `top_paths`.  The ranks beyond are empty."""
    scorer, dense, _, restated = _setup(MAIN, 2, 1.0, 0.0, NEG_INF, ahead)
    firsts = {word[0] for word in restated.vocab}
    rng = np.random.default_rng(8)
    logits = _lean(rng, 6, MAIN, ['ab', 'c', 'd'], noise=1.0)
    seq_len = np.array([1, 0, 6], dtype=np.int32)
    for norm in NORMS:
        for width, top_paths in ((8, 8), (64, 64), (1024, 12)):
            got = _word(hip, logits, seq_len, width, scorer, top_paths, 28, norm)
            want = _dense_nbest(hip, logits, seq_len, width, dense, top_paths, 28, norm)
            assert _same_bits(got, want)
            assert got[3][0] == 1 + len(firsts) < top_paths and got[3][1] == 1
            _empty_beyond(got)
            _against_cpu(got, logits, seq_len, width, dense, 28, norm)


# ------------------------------------------------------------------------------------------------
# 4. Frames and lengths (oracles 2 and 3)
# ------------------------------------------------------------------------------------------------
RULES = pytest.mark.parametrize('ahead', [False, True], ids=['plain', 'look-ahead'])


@RULES
@pytest.mark.parametrize('batch', [1, 5])
@pytest.mark.parametrize('num_steps', [1, 2, 3])
def test_one_to_three_frames(hip, num_steps, batch, ahead):
    rng = np.random.default_rng(10 * num_steps + batch)
    scorer, dense, _, _ = _setup(MAIN, 2, 0.7, 0.4, -4.0, ahead)
    logits = _lean(rng, num_steps, MAIN, ['a', 'd', 'ab', 'c', 'a d'][:batch], noise=1.5)
    seq_len = np.array([num_steps, 1, 0, num_steps, max(1, num_steps - 1)][:batch], dtype=np.int32)
    for norm in NORMS:
        for width in (1, 8, 1024):
            got = _against_dense(hip, logits, seq_len, width, scorer, dense, 28, norm, (1, ))
            _against_cpu(got, logits, seq_len, width, dense, 28, norm)


@RULES
@pytest.mark.parametrize('lengths', [[0, 12, 1, 0], [0, 0, 0, 0], [0]])
def test_rows_of_length_zero(hip, lengths, ahead):
    """A row of length 0 decodes to the empty string, and its logp is the end score of the start
    state: Wd((), </s>) rounded to float32 - exactly, for both rules (la[0] = 0)."""
    scorer, dense, _, restated = _setup(MAIN, 2, 0.7, 0.4, -4.0, ahead)
    want = np.float32(restated.wd((), ref.EOS, 0.7)[0])
    assert np.isfinite(want) and want < 0
    rng = np.random.default_rng(len(lengths))
    logits = _lean(rng, 12, MAIN, ['ab d', 'a d a', 'c', 'dd'][:len(lengths)])
    for norm in NORMS:
        for width in (1, 64):
            got = _against_dense(hip, logits, lengths, width, scorer, dense, 28, norm,
                                 (min(width, 2), 1))
            _against_cpu(got, logits, lengths, width, dense, 28, norm)
            for b, length in enumerate(lengths):
                if length == 0:
                    assert got[1][b, 0] == 0 and (got[0][b] == 0).all() and got[3][b] == 1
                    assert got[2][b, 0].view(np.int32) == want.view(np.int32)


@RULES
def test_lengths_outside_0_T_are_clamped_and_frames_past_them_never_read(hip, ahead):
    num_steps = 16
    scorer, dense, _, _ = _setup(MAIN, 2, 0.7, 0.4, -4.0, ahead)
    rng = np.random.default_rng(33)
    logits = _lean(rng, num_steps, MAIN, ['ab d a', 'c', 'dd bb', 'a', 'd a'])
    wild = np.array([num_steps + 7, -2, num_steps, 3, 2 ** 31 - 1], dtype=np.int32)
    tame = np.array([num_steps, 0, num_steps, 3, num_steps], dtype=np.int32)
    short = np.array([num_steps, 9, 0, 1, 5], dtype=np.int32)
    zeros, nans = logits.copy(), logits.copy()
    for b, length in enumerate(short):
        zeros[length:, b] = 0.0
        nans[length:, b] = np.nan
    for norm in NORMS:
        for width in (8, 100):
            want = _against_dense(hip, logits, tame, width, scorer, dense, 28, norm, (4,))
            assert _same_bits(_word(hip, logits, wild, width, scorer, 4, 28, norm), want)
            want = _against_dense(hip, zeros, short, width, scorer, dense, 28, norm, (4,))
            assert _same_bits(_word(hip, nans, short, width, scorer, 4, 28, norm), want)
        _against_cpu(_word(hip, logits, wild, 8, scorer, 1, 28, norm), logits, tame, 8, dense, 28,
                     norm)


# ------------------------------------------------------------------------------------------------
# 5. Batch positions
# ------------------------------------------------------------------------------------------------
@RULES
@pytest.mark.parametrize('batch', [63, 65, 300])
def test_a_row_inside_a_batch_is_the_row_alone(hip, batch, ahead):
    """One workgroup per utterance; each of the seven pools (parent, label, slot, children,
    context, memo context, memo score) starts at the utterance's first node.  Rows 0, 62, 64 and
    299 equal the same rows decoded alone, bit for bit, and row 0 the CPU reference."""
    num_steps = 16
    rng = np.random.default_rng(batch)
    texts = [' '.join(LEXICON[int(i)] for i in rng.integers(0, len(LEXICON), size=2))
             for _ in range(batch)]
    logits = _lean(rng, num_steps, MAIN, texts, noise=1.0)
    seq_len = rng.integers(0, num_steps + 1, size=batch).astype(np.int32)
    rows = [b for b in (0, 62, 64, 299) if b < batch]
    seq_len[rows] = num_steps
    scorer, dense, _, _ = _setup(MAIN, 3, 0.7, 0.4, -4.0, ahead)
    got = _word(hip, logits, seq_len, 16, scorer, 4, 28)
    for b in rows:
        one = _word(hip, logits[:, b:b + 1], seq_len[b:b + 1], 16, scorer, 4, 28)
        assert _same_bits(one, tuple(x[b:b + 1] for x in got)), b
    _against_cpu(tuple(x[:1] for x in got), logits[:, :1], seq_len[:1], 16, dense, 28, 'max')


# ------------------------------------------------------------------------------------------------
# 6. Non-finite rows
# ------------------------------------------------------------------------------------------------
@RULES
@pytest.mark.parametrize('poison', [np.nan, np.inf])
def test_a_non_finite_row_does_not_spread(hip, poison, ahead):
    """test_gpu_beam_edges.py::test_beam_non_finite_row_does_not_spread under a word model: the
    poisoned row comes back in range, its neighbours bit for bit as without it, and the next call
    is sound."""
    rng = np.random.default_rng(70)
    clean = _lean(rng, 24, MAIN, ['ab d a', 'dd bb', 'c a', 'a'], noise=1.0)
    seq_len = np.array([24, 20, 24, 11], dtype=np.int32)
    dirty = clean.copy()
    dirty[7, 1, 3] = poison
    scorer, dense, _, _ = _setup(MAIN, 2, 0.7, 0.4, -4.0, ahead)
    others = [0, 2, 3]
    for norm in NORMS:
        for width in (8, 100):
            want = _against_dense(hip, clean, seq_len, width, scorer, dense, 28, norm, (4,))
            out, out_len, logp, n_paths = _word(hip, dirty, seq_len, width, scorer, 4, 28, norm)
            assert _same_bits((out[others], out_len[others], logp[others], n_paths[others]),
                              tuple(x[others] for x in want))
            assert 0 <= n_paths[1] <= 4
            for k in range(4):
                n = int(out_len[1, k])
                assert 0 <= n <= seq_len[1]
                assert ((out[1, k, :n] >= 0) & (out[1, k, :n] < 28)).all()
                assert (out[1, k, n:] == 0).all()
            assert _same_bits(_word(hip, clean, seq_len, width, scorer, 4, 28, norm), want)


# ------------------------------------------------------------------------------------------------
# 7. Orders 4 and 5 (oracles 2 and 3)
# ------------------------------------------------------------------------------------------------
SMALL = (6, 5, 4)                                   # a, b, c, d are labels 3, 0, 0, 1
SMALL_LEXICON = ('a', 'd', 'ab', 'ba', 'cab')


@functools.lru_cache(maxsize=None)
def _long_corpus():
    return _zipf_corpus(SMALL, SMALL_LEXICON, 14, 5, 7)


@pytest.mark.parametrize('order', [4, 5])
def test_orders_4_and_5(hip, order):
    rows = _long_corpus()
    contexts = [_pair(SMALL, n, rows)[0].num_contexts for n in range(1, 6)]
    assert all(a < b for a, b in zip(contexts, contexts[1:])), contexts
    restated = _pair(SMALL, order, rows)[1]
    assert max(len(h) for h in restated.contexts) == order - 1
    rng = np.random.default_rng(order)
    num_steps = 24
    logits = _lean(rng, num_steps, SMALL, ['a d a d ab a', 'ab a d a a d', 'd d a a ab'])
    seq_len = np.array([num_steps, num_steps, num_steps - 3], dtype=np.int32)
    most_words, most_backoffs = 0, 0
    for oov in (NEG_INF, -4.0):
        for ahead in (False, True):
            scorer, dense, backoffs, _ = _setup(SMALL, order, 0.7, 0.4, oov, ahead, rows)
            assert scorer.order == order
            for norm in NORMS:
                got = _against_dense(hip, logits, seq_len, 8, scorer, dense, 5, norm, (8, 1))
                paths = _against_cpu(got, logits, seq_len, 8, dense, 5, norm)
                _against_dense(hip, logits, seq_len, 100, scorer, dense, 5, norm, (8,))
                words, backed = _facts(paths, dense, backoffs, 4)
                most_words, most_backoffs = max(most_words, words), max(most_backoffs, backed)
    assert most_words >= order, 'no decoded hypothesis holds a context of order - 1 words'
    assert most_backoffs >= 1, 'no scored space edge backed off'


# ------------------------------------------------------------------------------------------------
# 8. Lexicon shapes
# ------------------------------------------------------------------------------------------------
def _both_oracles(hip, logits, seq_len, layout, scorer, dense, widths=(8, 100)):
    """Oracles 2 and 3 under both normalisations at every width.  Returns the last n-best list
    and the reference's paths of every run, the first run's rows first."""
    paths = []
    for norm in NORMS:
        for width in widths:
            got = _against_dense(hip, logits, seq_len, width, scorer, dense, layout[1], norm,
                                 (min(width, 8), 1))
            paths += _against_cpu(got, logits, seq_len, width, dense, layout[1], norm)
    return got, paths


@RULES
@pytest.mark.parametrize('oov', [NEG_INF, -4.0])
def test_a_single_one_letter_word(hip, oov, ahead):
    rows = (_spell('a', MAIN), _spell('a a', MAIN))
    scorer, dense, _, restated = _setup(MAIN, 2, 0.7, 0.4, oov, ahead, rows)
    assert restated.vocab == [_spell('a', MAIN)] and scorer.num_nodes == 3
    rng = np.random.default_rng(81)
    logits = _lean(rng, 12, MAIN, ['a a a', 'a', 'ab a'], noise=1.0)
    _, paths = _both_oracles(hip, logits, [12, 7, 12], MAIN, scorer, dense)
    assert max(len(ref.words_of(path, 1)) for path in paths) >= 2


@RULES
def test_an_empty_vocabulary(hip, ahead):
    """The trie is the root and the sink.  With OOV on every word is unknown; with OOV off nothing
    can be emitted, and the empty hypothesis ends with Wd((), </s>)."""
    rows = ((),)
    scorer, dense, _, restated = _setup(MAIN, 2, 1.0, 0.0, -2.0, ahead, rows)
    assert scorer.num_nodes == 2 and restated.vocab == []
    rng = np.random.default_rng(82)
    logits = _lean(rng, 12, MAIN, ['ab d', 'c', 'a a'], noise=1.0, peak=7.0)
    seq_len = np.array([12, 0, 9], dtype=np.int32)
    _, paths = _both_oracles(hip, logits, seq_len, MAIN, scorer, dense)
    assert any(len(ref.words_of(path, 1)) >= 2 for path in paths)
    closed, dense, _, _ = _setup(MAIN, 2, 1.0, 0.0, NEG_INF, ahead, rows)
    end = restated.wd((), ref.EOS)[0]
    for norm in NORMS:
        for width in (1, 16):
            out, out_len, logp, n_paths = _word(hip, logits, seq_len, width, closed, 1, 28, norm)
            assert (out_len == 0).all() and (out == 0).all() and (n_paths == 1).all()
            for b in range(3):
                x = logits[:seq_len[b], b].astype(np.float64)
                x = octc.log_softmax(x) if norm == 'log_softmax' else \
                    x - x.max(axis=1, keepdims=True)
                assert float(logp[b, 0]) == pytest.approx(x[:, 28].sum() + end, rel=1e-5,
                                                          abs=1e-5)


@RULES
@pytest.mark.parametrize('word', ['abcd', 'abbd'])
def test_a_word_of_exactly_T_letters(hip, word, ahead):
    """Closed vocabulary, T = 4 frames and one word of four letters: without a doubled letter it
    fits exactly, a frame per letter; with one it needs a blank between the two and cannot be
    finished - no complete hypothesis but the empty one exists."""
    rows = (_spell(word, MAIN),)
    scorer, dense, _, _ = _setup(MAIN, 1, 1.0, 0.0, NEG_INF, ahead, rows)
    logits = np.full((4, 2, 29), -4.0, dtype=np.float32)
    for t, c in enumerate(_spell(word, MAIN)):
        logits[t, :, c] = 4.0
    logits += np.random.default_rng(83).normal(size=logits.shape).astype(np.float32) * 0.1
    seq_len = np.array([4, 3], dtype=np.int32)
    got, paths = _both_oracles(hip, logits, seq_len, MAIN, scorer, dense, (8, 64))
    if word == 'abcd':
        assert tuple(paths[0]) == _spell(word, MAIN) and np.isfinite(got[2][0, 0])
    else:
        assert paths[0] == [] and np.isfinite(got[2][0, 0])
    assert paths[1] == []


BIG = (7, 6, 5)                                     # letters a..e are labels 4, 0, 1, 2, 3


@functools.lru_cache(maxsize=None)
def _big_corpus():
    """75 words over a..e of at most three letters: every word at least once, two per sentence."""
    letters = 'abcde'
    words = list(letters) + [x + y for x in letters for y in letters]
    words += [x + y + z for x in letters for y in letters for z in letters][::2][:45]
    rng = np.random.default_rng(70)
    rows = [_spell(' '.join((word, words[int(rng.integers(0, 12))])), BIG) for word in words]
    return tuple(rows), len(words)


@pytest.mark.parametrize('order', [1, 2])
def test_a_successor_range_longer_than_64(hip, order):
    """The empty context lists 77 successors, so `wordlm_wd` runs its 64-way probe loop inside
    `beam_expand` and inside the end pass - at order 2 after a back-off."""
    rows, count = _big_corpus()
    assert count >= 70
    rng = np.random.default_rng(84 + order)
    logits = _lean(rng, 16, BIG, ['eb ca', 'abd e dc', 'c'], noise=0.8)
    seq_len = np.array([16, 16, 5], dtype=np.int32)
    most_words, most_backoffs = 0, 0
    for oov in (NEG_INF, -4.0):
        for ahead in (False, True):
            scorer, dense, backoffs, _ = _setup(BIG, order, 0.7, 0.4, oov, ahead, rows)
            assert scorer.ctx_begin[1] - scorer.ctx_begin[0] > 64
            _, paths = _both_oracles(hip, logits, seq_len, BIG, scorer, dense)
            words, backed = _facts(paths, dense, backoffs, 5)
            most_words, most_backoffs = max(most_words, words), max(most_backoffs, backed)
    assert most_words >= 2
    assert order == 1 or most_backoffs >= 1


# ------------------------------------------------------------------------------------------------
# 9. Stats at the edges
# ------------------------------------------------------------------------------------------------
def test_stats_at_the_edges(hip):
    """A length-0 row counts (0, 0); lookups never exceed the branches expanded; and the numbers
    are the same from call to call on a workspace that was filled with 0xff and is reused.  (That
    the two rules count the same where nothing is pruned is asserted with the truth cases.)"""
    rng = np.random.default_rng(9)
    logits = _t(_lean(rng, 16, MAIN, ['ab d a', 'c', 'dd bb', 'a']))
    seq_len = _t(np.array([16, 0, 11, 1]), torch.int32)
    need = hip.ctc_beam_wordlm_workspace_bytes(16, 4, 29, 32)
    shared = torch.full((need,), 0xff, dtype=torch.uint8, device=DEV)
    for oov in (NEG_INF, -4.0):
        for ahead in (False, True):
            scorer = _setup(MAIN, 3, 1.0, 0.0, oov, ahead)[0]
            counted = []
            for _ in range(3):
                stats = torch.full((4, 2), -1, dtype=torch.int64, device=DEV)
                status, got = _raw(hip, logits, seq_len, 32, scorer, shared, stats=stats)
                assert status == 0
                counted.append((stats.cpu().numpy(), got))
            first = counted[0][0]
            print('branches expanded / lookups performed:', first.tolist())
            assert first[1].tolist() == [0, 0]
            assert (first[:, 1] <= first[:, 0]).all() and (first >= 0).all()
            assert first[0, 0] > 16 and first[3, 0] == 1
            for again, got in counted[1:]:
                assert np.array_equal(again, first) and _same_bits(got, counted[0][1])


# ------------------------------------------------------------------------------------------------
# 10. Refusals through the C entry points
# ------------------------------------------------------------------------------------------------
def _launch(hip, scorer, ahead, change, width=8, top_paths=2, blank=28, table=True):
    """(status, outputs) of the C entry point of the rule on tables that ``change`` has edited;
    the outputs are pre-filled with -7 / NaN."""
    rng = np.random.default_rng(1)
    logits = _t(_lean(rng, 12, MAIN, ['ab a', 'c']))
    seq_len = _t(np.array([12, 12]), torch.int32)
    tables, keep = hip._wordlm_struct(scorer, logits.device)
    for name, value in change.items():
        setattr(tables, name, value)
    rows = max(top_paths, 1)
    out = torch.full((2, rows, 12), -7, dtype=torch.int32, device=DEV)
    out_len = torch.full((2, rows), -7, dtype=torch.int32, device=DEV)
    logp = torch.full((2, rows), float('nan'), dtype=torch.float32, device=DEV)
    n_paths = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    need = hip.ctc_beam_wordlm_workspace_bytes(12, 2, 29, 8)
    workspace = torch.zeros((need,), dtype=torch.uint8, device=DEV)
    head = (logits.data_ptr(), seq_len.data_ptr(), 12, 2, 29, blank, width, 0, top_paths,
            ctypes.addressof(tables))
    tail = (out.data_ptr(), out_len.data_ptr(), logp.data_ptr(), n_paths.data_ptr(),
            workspace.data_ptr(), workspace.numel(), torch.cuda.current_stream().cuda_stream)
    if ahead:
        pointer = scorer.lookahead_to(logits.device).data_ptr() if table else None
        status = hip.load().ctcasr_ctc_beam_decode_wordlm_lookahead(*(head + (pointer,) + tail))
    else:
        status = hip.load().ctcasr_ctc_beam_decode_wordlm(*(head + tail))
    torch.cuda.synchronize()
    del keep
    return status, tuple(t.cpu().numpy() for t in (out, out_len, logp, n_paths))


REFUSED = [('space is the blank', {'space': 28}, {}),
           ('space is C', {'space': 29}, {}),
           ('space is -1', {'space': -1}, {}),
           ('one trie node', {'num_nodes': 1}, {}),
           ('bonus NaN', {'bonus': float('nan')}, {}),
           ('bonus +inf', {'bonus': float('inf')}, {}),
           ('bonus -inf', {'bonus': float('-inf')}, {}),
           ('oov_score NaN', {'oov_score': float('nan')}, {}),
           ('oov_score +inf', {'oov_score': float('inf')}, {}),
           ('order 6', {'order': 6}, {}),
           ('order 0', {'order': 0}, {}),
           ('top_paths above the width', {}, {'top_paths': 9}),
           ('top_paths 0', {}, {'top_paths': 0})]


@RULES
def test_refusals_through_the_c_entry_points(hip, ahead):
    scorer = _setup(MAIN, 2, 1.0, 0.0, -4.0, ahead)[0]
    status, got = _launch(hip, scorer, ahead, {})
    assert status == 0 and (got[3] == 2).all() and np.isfinite(got[2]).all()
    cases = REFUSED + ([('no look-ahead table', {}, {'table': False})] if ahead else [])
    for name, change, arguments in cases:
        status, got = _launch(hip, scorer, ahead, change, **arguments)
        assert status == BAD_ARGUMENT, name
        assert (got[0] == -7).all() and (got[1] == -7).all() and (got[3] == -7).all(), name
        assert np.isnan(got[2]).all(), name
    # -inf is a legal oov_score (the closed vocabulary), and the call after a refusal is sound
    status, again = _launch(hip, scorer, ahead, {'oov_score': float('-inf')})
    assert status == 0 and (again[3] >= 1).all()
    # the lookup refuses order 6 too, and writes nothing
    tables, keep = hip._wordlm_struct(scorer, torch.device(DEV, torch.cuda.current_device()))
    tables.order = 6
    ctx, word = _t(np.array([0, 0]), torch.int32), _t(np.array([2, 3]), torch.int32)
    score = torch.full((2,), float('nan'), device=DEV)
    after = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    assert hip.load().ctcasr_wordlm_lookup(ctypes.addressof(tables), ctx.data_ptr(),
                                           word.data_ptr(), 2, score.data_ptr(), after.data_ptr(),
                                           None) == BAD_ARGUMENT
    torch.cuda.synchronize()
    assert np.isnan(score.cpu().numpy()).all() and (after.cpu().numpy() == -7).all()
    del keep
