"""The word n-gram on the host (`lm.build_word_ngram`, `lm.WordLmScorer`, its file and flags)
against tests/word_lm_reference.py: the estimate, the back-off form, the array invariants, the
refusals, and `sequence_scores` against the reference's dense automaton.  No GPU."""

import numpy as np
import pytest

from ctc_asr_amd import lm
from ctc_asr_amd.params import FLAGS
from tests import lm_beam_reference as lref
from tests import word_lm_reference as ref

CLASSES, BLANK, SPACE = 6, 5, 4
LEXICON = [[0], [0, 1], [0, 1, 2], [1, 0], [2, 0, 1], [3], [1, 0, 3], [2, 0], [3, 3], [0, 2, 1, 3],
           [1, 1], [2]]


def _rows(seed=0, count=30):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(count):
        row = []
        for _ in range(int(rng.integers(1, 6))):
            row += ([SPACE] if row else []) + LEXICON[min(int(rng.zipf(1.5)) - 1,
                                                          len(LEXICON) - 1)]
        rows.append(row)
    return rows


@pytest.fixture(scope='module', params=[1, 2, 3, 4])
def pair(request):
    rows = _rows()
    return (lm.build_word_ngram(rows, request.param, CLASSES, SPACE, blank=BLANK),
            ref.WordNgram(rows, request.param, SPACE))


def test_every_context_sums_to_one_and_equals_the_interpolated_formula(pair):
    """exp of the scores of all words plus <unk> plus </s> sums to 1 within 1e-12 in every
    context, and the back-off walk equals the interpolated formula evaluated directly, for seen
    and unseen pairs - to the bit against the reference's walk, 1e-14 against the formula."""
    model, restated = pair
    assert model.vocab == [list(word) for word in restated.vocab]
    assert model.num_contexts == len(restated.contexts)
    seen = unseen = 0
    for h in restated.contexts:
        total = 0.0
        for w in range(restated.events):
            got, after = model.word_score(restated.context_id[h], w)
            want, want_after, steps = restated.wd(h, w)
            assert got == want and after == restated.context_id[want_after], (h, w)
            assert np.exp(got) == pytest.approx(restated.prob(h, w), rel=1e-13, abs=1e-300)
            total += np.exp(got)
            seen, unseen = seen + (steps == 0), unseen + (steps > 0)
        assert abs(total - 1.0) < 1e-12, h
    assert seen and (unseen or model.order == 1)


def test_array_invariants(pair):
    model, restated = pair
    begin = model.ctx_begin
    assert begin[0] == 0 and begin[-1] == model.num_successors
    assert model.succ_word[:begin[1]].tolist() == list(range(restated.events))
    for h, context in enumerate(restated.contexts):
        words = model.succ_word[begin[h]:begin[h + 1]]
        assert (np.diff(words) > 0).all() and len(words) >= 1
        if h:
            assert model.ctx_parent[h] < h
            assert restated.contexts[model.ctx_parent[h]] == context[1:]
            assert sorted(restated.counts[context]) == words.tolist()
        for w, after in zip(words, model.succ_ctx[begin[h]:begin[h + 1]]):
            # the longest suffix of h + w that is a context
            full = (context + (int(w),))[-(model.order - 1):] if model.order > 1 else ()
            suffixes = [full[i:] for i in range(len(full) + 1)]
            assert restated.contexts[after] == next(s for s in suffixes
                                                    if s in restated.context_id)
    assert model.trie_word[0] == -1 and model.trie_word[1] == -1
    assert (model.trie_next[1] == -1).all()
    assert sorted(model.trie_word[model.trie_word >= 0].tolist()) == \
        list(range(2, restated.events))
    # contexts are sorted shorter first, and lengths never exceed order - 1
    lengths = [len(h) for h in restated.contexts]
    assert lengths == sorted(lengths) and max(lengths) == min(model.order - 1, max(lengths))


def test_save_and_load_round_trip_bit_for_bit(pair, tmp_path):
    model, _ = pair
    path = str(tmp_path / 'words.npz')
    model.save(path)
    with np.load(path, allow_pickle=False) as data:
        assert str(data['kind']) == 'word_ngram' and int(data['space']) == SPACE
        assert int(data['order']) == model.order and int(data['num_classes']) == CLASSES
    back = lm.load(path, CLASSES)
    assert isinstance(back, lm.WordLmScorer)
    for name in lm.WORD_ARRAYS:
        a, b = getattr(model, name), getattr(back, name)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    assert back.vocab == model.vocab and back.order == model.order and back.space == SPACE
    with pytest.raises(ValueError, match='6 classes'):
        lm.load(path, 29)


def test_a_character_file_still_loads_as_before(tmp_path):
    chars = lm.build_char_ngram(_rows(), 3, CLASSES, blank=BLANK)
    path = str(tmp_path / 'chars.npz')
    chars.save(path)
    with np.load(path, allow_pickle=False) as data:
        assert 'kind' not in data.files
    back = lm.load(path, CLASSES)
    assert type(back) is lm.LmScorer and back.order == 3
    assert back.next.tobytes() == chars.next.tobytes()
    assert back.score.tobytes() == chars.score.tobytes()
    assert back.final.tobytes() == chars.final.tobytes()


def _arrays(model):
    return {name: getattr(model, name).copy() for name in lm.WORD_ARRAYS}


def _build(arrays, order=2, space=SPACE, **kwargs):
    return lm.WordLmScorer(*[arrays[name] for name in lm.WORD_ARRAYS], order=order, space=space,
                           **kwargs)


def test_every_refusal_fires_and_names_its_array():
    model = lm.build_word_ngram(_rows(), 2, CLASSES, SPACE, blank=BLANK)
    good = _arrays(model)
    _build(good)
    contexts, total, nodes = model.num_contexts, model.num_successors, model.num_nodes

    def spoil(name, change, match=None):
        arrays = _arrays(model)
        arrays[name] = change(arrays[name])
        with pytest.raises(ValueError, match=match or name):
            _build(arrays)

    def poke(index, value):
        def change(a):
            a[index] = value
            return a
        return change
    # shapes
    spoil('trie_next', lambda a: a[0])
    spoil('trie_next', lambda a: a[:1])
    spoil('trie_word', lambda a: a[:-1])
    spoil('ctx_begin', lambda a: a[:1])
    spoil('succ_lp', lambda a: a[:-1])
    spoil('succ_ctx', lambda a: a[:-1])
    spoil('ctx_backoff', lambda a: a[:-1])
    spoil('ctx_parent', lambda a: np.append(a, 0))
    spoil('succ_word', lambda a: a.astype(np.float32))
    # every index in range
    spoil('trie_next', poke((2, 0), nodes))
    spoil('trie_next', poke((2, 0), -2))
    spoil('trie_word', poke(3, model.num_words))
    spoil('trie_word', poke(3, 1))              # </s> ends no spelling
    spoil('trie_word', poke(0, 2))
    spoil('ctx_begin', poke(-1, total + 1))
    spoil('ctx_begin', poke(2, int(good['ctx_begin'][3]) + 1))
    spoil('succ_word', poke(total - 1, model.num_words))
    spoil('succ_ctx', poke(0, contexts))
    spoil('succ_ctx', poke(0, -1))
    spoil('ctx_parent', poke(1, contexts))
    # ascending successors, context 0 complete, ctx_parent[h] < h
    begin = good['ctx_begin']
    wide = next(h for h in range(1, contexts) if begin[h + 1] - begin[h] >= 2)
    spoil('succ_word', poke(begin[wide] + 1, int(good['succ_word'][begin[wide]])))
    spoil('succ_word', poke(1, 2))
    spoil('ctx_parent', poke(2, 2))
    spoil('ctx_parent', poke(0, 1))
    # no NaN, no +inf (-inf is a forbidden word and legal)
    spoil('succ_lp', poke(0, np.nan))
    spoil('succ_lp', poke(0, np.inf))
    spoil('succ_lp', poke(0, 1e39))             # +inf once rounded to float32
    spoil('ctx_backoff', poke(1, np.nan))
    spoil('ctx_backoff', poke(1, np.inf))
    arrays = _arrays(model)
    arrays['succ_lp'][3] = -np.inf
    _build(arrays)
    for order in (0, 6):
        with pytest.raises(ValueError, match='order'):
            _build(good, order=order)
    for space in (-1, CLASSES):
        with pytest.raises(ValueError, match='space'):
            _build(good, space=space)
    with pytest.raises(ValueError, match='vocab'):
        _build(good, vocab=[[0]])
    for bad in (dict(bonus=np.inf), dict(bonus=np.nan), dict(oov_score=np.inf),
                dict(oov_score=np.nan)):
        with pytest.raises(ValueError, match='bonus|oov_score'):
            _build(good, **bad)
    with pytest.raises(ValueError, match='weight'):
        model.scaled(np.inf)
    for kwargs in (dict(order=0), dict(order=6), dict(vocab_size=-1), dict(space=BLANK),
                   dict(space=CLASSES)):
        call = dict(order=2, space=SPACE, vocab_size=0)
        call.update(kwargs)
        with pytest.raises(ValueError):
            lm.build_word_ngram(_rows(), call['order'], CLASSES, call['space'],
                                vocab_size=call['vocab_size'], blank=BLANK)
    with pytest.raises(ValueError, match='label'):
        lm.build_word_ngram([[0, BLANK]], 2, CLASSES, SPACE, blank=BLANK)


ROWS = {'one word': [0, 1], 'several words': [0, 1, SPACE, 2, 0, 1, SPACE, 3],
        'ends mid-word': [0, 1, SPACE, 0, 2], 'an OOV word': [0, SPACE, 3, 1, 3, SPACE, 2],
        'a leading space': [SPACE, 0], 'a doubled space': [0, SPACE, SPACE, 1, 0],
        'ends at a space': [2, 0, SPACE], 'empty': []}


@pytest.mark.parametrize('order', [1, 2, 3])
@pytest.mark.parametrize('oov', [-np.inf, -4.0])
@pytest.mark.parametrize('weight,bonus', [(1.0, 0.0), (0.7, 0.4), (0.0, 0.0)])
def test_sequence_scores_walk_the_dense_automaton(order, oov, weight, bonus):
    rows = _rows()
    scaled = lm.build_word_ngram(rows, order, CLASSES, SPACE, blank=BLANK).scaled(weight, bonus,
                                                                                  oov)
    nxt, score, final, _, _ = ref.dense_automaton(
        ref.Scorer(ref.WordNgram(rows, order, SPACE), weight, bonus, oov), CLASSES, BLANK)
    got = scaled.sequence_scores(list(ROWS.values()))
    want = [lref.automaton_score(row, nxt, score, final) for row in ROWS.values()]
    for name, a, b in zip(ROWS, got, want):
        assert a == b or (np.isneginf(a) and np.isneginf(b)), (name, a, b)
    by_name = dict(zip(ROWS, got))
    assert np.isfinite(by_name['one word']) and np.isfinite(by_name['several words'])
    assert np.isfinite(by_name['ends at a space']) and np.isfinite(by_name['empty'])
    assert np.isneginf(by_name['a leading space']) and np.isneginf(by_name['a doubled space'])
    # [0, 2] spells no word and is no prefix's end: finite only with OOV on; so is the OOV word
    assert np.isfinite(by_name['ends mid-word']) == np.isfinite(oov)
    assert np.isfinite(by_name['an OOV word']) == np.isfinite(oov)
    with pytest.raises(ValueError, match='label 6'):
        scaled.sequence_scores([[0, 6]])


def test_the_vocabulary_cut_moves_the_right_words_to_unk():
    a, b, c, d = [0], [1], [2], [3, 3]
    text = [a + [SPACE] + b + [SPACE] + a, c + [SPACE] + b, d + [SPACE] + a, c]
    # counts: a 3, b 2, c 2, d 1 - the cut at 2 keeps a and, of the tie b / c, the smaller row
    cut = lm.build_word_ngram(text, 2, CLASSES, SPACE, vocab_size=2, blank=BLANK)
    assert cut.vocab == [a, b] and cut.num_words == 4
    restated = ref.WordNgram(text, 2, SPACE, vocab_size=2)
    assert [list(w) for w in restated.vocab] == cut.vocab
    # c and d are counted as <unk>: three of the nine events at the empty context
    unk = cut.word_score(0, lm.UNK)[0]
    assert unk == restated.wd((), ref.UNK)[0]
    full = lm.build_word_ngram(text, 2, CLASSES, SPACE, blank=BLANK)
    assert full.vocab == [a, b, c, d] and np.exp(unk) > np.exp(full.word_score(0, lm.UNK)[0])
    # closed vocabulary: 'c' is now forbidden; open: it scores as <unk> + the penalty
    assert np.isneginf(cut.scaled(1.0, 0.0).sequence_scores([c])[0])
    opened = cut.scaled(1.0, 0.0, -2.0)
    # [2] has no trie edge at the root: the edge pays oov + bonus, the end <unk> in the sink
    unk_score, after = opened.word_score(0, lm.UNK)
    want = float(np.float32(-2.0)) + float(np.float32(unk_score +
                                                      opened.word_score(after, lm.EOS)[0]))
    assert opened.sequence_scores([c])[0] == want
    assert lm.build_word_ngram(text, 2, CLASSES, SPACE, vocab_size=9, blank=BLANK).vocab == \
        full.vocab


def test_flag_refusals_fire(tmp_path):
    FLAGS.reset()
    try:
        for bad in (['--lm_unit', 'syllable'], ['--lm_vocab_size', '-1'],
                    ['--lm_oov_score', 'nan'], ['--lm_oov_score', 'inf']):
            with pytest.raises(ValueError, match=bad[0][2:]):
                FLAGS.parse(bad)
            FLAGS.reset()
        assert FLAGS.parse(['--lm_oov_score=-inf', '--lm_unit', 'word', '--lm_vocab_size', '0',
                            '--lm_oov_score', '-3.5']) == []
        assert FLAGS.lm_oov_score == -3.5 and FLAGS.lm_unit == 'word'
        FLAGS.reset()
        assert FLAGS.lm_unit == 'char' and np.isneginf(FLAGS.lm_oov_score)
        # both path flags take both kinds, refuse a class mismatch, and refuse a word model
        # whose space is not the alphabet's
        from ctc_asr_amd.labels import ctoi
        words, other, small = (str(tmp_path / name) for name in ('w.npz', 'o.npz', 's.npz'))
        rows = [[ctoi(ch) for ch in 'ab cab a']]
        lm.build_word_ngram(rows, 2, 29, ctoi(' ')).save(words)
        lm.build_word_ngram([[3, 2, 3]], 2, 29, 2).save(other)          # its space is 'a'
        lm.build_word_ngram(_rows(), 2, CLASSES, SPACE, blank=BLANK).save(small)
        assert FLAGS.parse(['--lm_path', words]) == []
        assert isinstance(lm.from_flags(29), lm.WordLmScorer)
        FLAGS.reset()
        assert FLAGS.parse(['--nbest', '2', '--rescore_lm_path', words, '--lm_oov_score=-7',
                            '--rescore_lm_oov_score=-2']) == []
        rescorer = lm.rescorer_from_flags(29)
        assert isinstance(rescorer, lm.WordLmScorer) and rescorer.oov_score == -2.0
        FLAGS.reset()
        for flag, extra in (('--lm_path', []), ('--rescore_lm_path', ['--nbest', '2'])):
            with pytest.raises(ValueError, match='space'):
                FLAGS.parse(extra + [flag, other])
            FLAGS.reset()
            with pytest.raises(ValueError, match='6 classes'):
                FLAGS.parse(extra + [flag, small])
            FLAGS.reset()
        FLAGS.update(lm_path=other)
        with pytest.raises(ValueError, match='space'):
            lm.from_flags(29)
        FLAGS.reset()
        # a mistyped path is refused when the flags are parsed, and so is a file that is no model
        with pytest.raises(ValueError, match='lm_path'):
            FLAGS.parse(['--lm_path', str(tmp_path / 'nope.npz')])
        FLAGS.reset()
        (tmp_path / 'junk.npz').write_bytes(b'not an archive')
        for flag, extra in (('--lm_path', []), ('--rescore_lm_path', ['--nbest', '2'])):
            with pytest.raises(ValueError, match=flag[2:]):
                FLAGS.parse(extra + [flag, str(tmp_path / 'junk.npz')])
            FLAGS.reset()
        for bad in ('nan', 'inf'):
            with pytest.raises(ValueError, match='rescore_lm_oov_score'):
                FLAGS.parse(['--rescore_lm_oov_score', bad])
            FLAGS.reset()
        # a word model's file that lacks an array is refused by name
        with np.load(words, allow_pickle=False) as data:
            kept = {name: data[name] for name in data.files}
        for name in ('succ_ctx', 'vocab_offsets', 'space'):
            np.savez(str(tmp_path / 'short.npz'), **{k: v for k, v in kept.items() if k != name})
            with pytest.raises(ValueError, match=name):
                lm.load(str(tmp_path / 'short.npz'), 29)
    finally:
        FLAGS.reset()


def test_the_command_line_builds_a_word_model_that_load_accepts(tmp_path, capsys):
    FLAGS.reset()
    try:
        text = tmp_path / 'text.txt'
        text.write_text("The cat sat.\n\nA cat's mat -- the MAT!\nthe end\n", encoding='utf-8')
        path = str(tmp_path / 'words.npz')
        assert lm.main(['--lm_unit', 'word', '--lm_corpus_text', str(text), '--lm_order', '3',
                        '--lm_path', path, '--lm_vocab_size', '4']) == 0
        assert 'word model of 3 transcripts, 4 words' in capsys.readouterr().out
        from ctc_asr_amd.labels import ctoi, decode
        model = lm.load(path, 29)
        assert isinstance(model, lm.WordLmScorer) and model.order == 3
        assert model.space == ctoi(' ')
        # the / cat / mat twice or more, then the smallest row of the singletons: 'a'
        assert sorted(decode(word) for word in model.vocab) == ['a', 'cat', 'mat', 'the']
        assert np.isfinite(model.sequence_scores([[ctoi(ch) for ch in 'the cat']])[0])
        # a digit is refused with its line number
        text.write_text('one\ntwo 2\n', encoding='utf-8')
        with pytest.raises(ValueError, match='line 2'):
            lm.main(['--lm_unit', 'word', '--lm_corpus_text', str(text), '--lm_path', path])
        FLAGS.reset()
        with pytest.raises(ValueError, match='lm_corpus'):
            lm.main(['--lm_unit', 'word', '--lm_path', path])
    finally:
        FLAGS.reset()
