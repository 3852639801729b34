"""Host side of the language-model fusion, no GPU: the Witten-Bell n-gram builder and the
`LmScorer` container (ctc_asr_amd/lm.py), and the numpy reference of the fused search
(tests/lm_beam_reference.py) - against the project's beam-search oracles with a scorer that
scores nothing, and against the truth: an unpruned search must return the argmax over labellings
of ln p_ctc(label) + sum of edge scores + final(end state), p_ctc from all C^T paths."""

import math

import numpy as np
import pytest

from ctc_asr_amd import lm
from ctc_asr_amd.params import FLAGS
from oracle import cref
from oracle import ctc as octc
from tests import lm_beam_reference as ref

CORPUS = [[1, 2, 3, 1, 2], [2, 2, 1], [3, 1, 2, 3, 3, 1], [1], [], [4, 1, 2, 1, 2, 3]]


# ------------------------------------------------------------------------------------------------
# n-gram
# ------------------------------------------------------------------------------------------------
def _counts(rows, order, classes):
    """{context: {event: count}} of every context length below ``order``; the end event is
    ``classes``."""
    table = {}
    for row in rows:
        events = list(row) + [classes]
        for i, event in enumerate(events):
            for m in range(min(order - 1, i) + 1):
                follow = table.setdefault(tuple(row[i - m:i]), {})
                follow[event] = follow.get(event, 0) + 1
    return table


def _witten_bell(table, classes, context, event):
    """P(event | context) by the textbook recursion, one event at a time."""
    if context is None:
        return 1.0 / classes                  # uniform: classes - 1 labels and the end event
    lower = _witten_bell(table, classes, context[1:] if context else None, event)
    follow = table.get(context)
    if not follow:
        return lower
    total, seen = sum(follow.values()), len(follow)
    return (follow.get(event, 0) + seen * lower) / (total + seen)


@pytest.mark.parametrize('order', [1, 2, 3, 5])
def test_ngram_rows_normalise(order):
    classes = 6
    scorer = lm.build_char_ngram(CORPUS, order, classes)
    assert scorer.score.dtype == np.float64 and scorer.final.dtype == np.float64
    assert scorer.order == order and scorer.num_classes == classes
    labels = [c for c in range(classes) if c != classes - 1]
    total = np.exp(scorer.score[:, labels]).sum(axis=1) + np.exp(scorer.final)
    assert np.abs(total - 1.0).max() <= 1e-12
    assert np.isneginf(scorer.score[:, classes - 1]).all()
    assert np.isfinite(scorer.score[:, labels]).all()      # back-off resolved: every edge scored


def test_ngram_with_the_blank_elsewhere():
    """``blank=1``: labels 0, 2, 3 carry the model, column 1 is the one that is never read."""
    rows = [[0, 2, 3, 0, 2], [2, 2, 0], [3, 0]]
    scorer = lm.build_char_ngram(rows, 3, 4, blank=1)
    total = np.exp(scorer.score[:, [0, 2, 3]]).sum(axis=1) + np.exp(scorer.final)
    assert np.abs(total - 1.0).max() <= 1e-12
    assert np.isneginf(scorer.score[:, 1]).all() and np.isfinite(scorer.score[:, 3]).all()
    with pytest.raises(ValueError):
        lm.build_char_ngram([[0, 1]], 3, 4, blank=1)
    with pytest.raises(ValueError):
        lm.build_char_ngram(rows, 3, 4, blank=4)


def test_ngram_order_1_is_a_single_state():
    scorer = lm.build_char_ngram(CORPUS, 1, 6)
    assert scorer.num_states == 1 and (scorer.next == 0).all()
    unigram = np.zeros(7)
    for row in CORPUS:
        for event in list(row) + [6]:
            unigram[event] += 1
    seen = np.count_nonzero(unigram)
    uniform = np.full(7, 1 / 6.0)
    uniform[5] = 0.0
    expect = (unigram + seen * uniform) / (unigram.sum() + seen)
    assert np.allclose(np.exp(scorer.score[0, :5]), expect[:5], rtol=1e-14, atol=0)
    assert math.exp(scorer.final[0]) == pytest.approx(expect[6], rel=1e-14)


@pytest.mark.parametrize('order', [2, 3, 4])
def test_ngram_scores_equal_the_recursive_witten_bell(order):
    classes = 6
    scorer = lm.build_char_ngram(CORPUS, order, classes)
    table = _counts(CORPUS, order, classes)
    # states: the observed contexts, the empty one first, each the longest-suffix state
    states = sorted(table, key=lambda h: (len(h), h))
    assert scorer.num_states == len(states) and states[0] == ()
    for s, context in enumerate(states):
        for c in range(classes - 1):
            p = _witten_bell(table, classes, context, c)
            assert scorer.score[s, c] == pytest.approx(math.log(p), rel=1e-13, abs=1e-13)
            target = (context + (c,))[max(0, len(context) + 2 - order):]
            while target not in table:
                target = target[1:]
            assert states[int(scorer.next[s, c])] == target, (context, c)
        p_end = _witten_bell(table, classes, context, classes)
        assert scorer.final[s] == pytest.approx(math.log(p_end), rel=1e-13, abs=1e-13)
    # a context that was never seen scores as its longest seen suffix: (4, 2) never occurs
    s = 0
    for c in (4, 4, 2):
        s = int(scorer.next[s, c])
    assert (4, 2) not in table and states[s] == (2,)


def test_ngram_refuses_bad_input():
    with pytest.raises(ValueError):
        lm.build_char_ngram(CORPUS, 0, 6)
    with pytest.raises(ValueError):
        lm.build_char_ngram([[5]], 2, 6)            # the blank is no label
    with pytest.raises(ValueError):
        lm.build_char_ngram([[-1]], 2, 6)
    empty = lm.build_char_ngram([], 3, 4)           # no corpus: the uniform model, one state
    assert empty.num_states == 1
    assert np.allclose(np.exp(empty.score[0, :3]), 0.25) and math.exp(empty.final[0]) == 0.25


def test_save_load_round_trips_bit_for_bit(tmp_path):
    scorer = lm.build_char_ngram(CORPUS, 3, 6)
    path = str(tmp_path / 'model.npz')
    scorer.save(path)
    back = lm.load(path, 6)
    assert back.order == 3 and back.next.dtype == np.int32
    assert np.array_equal(back.next, scorer.next)
    assert back.score.dtype == np.float64 and back.score.tobytes() == scorer.score.tobytes()
    assert back.final.tobytes() == scorer.final.tobytes()
    with pytest.raises(ValueError, match='6 classes'):
        lm.load(path, 29)
    # without `final`, float32 tables, no order
    plain = lm.LmScorer(np.zeros((2, 3), dtype=np.int64), np.zeros((2, 3), dtype=np.float32))
    plain.save(path)
    back = lm.load(path)
    assert back.final is None and back.order is None and back.score.dtype == np.float32
    with np.load(path, allow_pickle=False) as data:
        assert sorted(data.files) == ['next', 'num_classes', 'order', 'score']


def test_scorer_refuses_bad_tables():
    nxt, score = np.zeros((2, 3), dtype=np.int32), np.zeros((2, 3))
    lm.LmScorer(nxt, score, np.zeros(2))
    lm.LmScorer(nxt, np.full((2, 3), -np.inf), np.full(2, -np.inf))      # -inf is allowed
    for bad in (2, -1):
        wrong = nxt.copy()
        wrong[1, 2] = bad
        with pytest.raises(ValueError, match='outside'):
            lm.LmScorer(wrong, score)
    for bad in (np.nan, np.inf, 1e39):              # 1e39 is +inf in the float32 the kernel reads
        wrong = score.copy()
        wrong[0, 1] = bad
        with pytest.raises(ValueError, match='NaN or'):
            lm.LmScorer(nxt, wrong)
        with pytest.raises(ValueError, match='NaN or'):
            lm.LmScorer(nxt, score, np.array([0.0, bad]))
    with pytest.raises(ValueError):
        lm.LmScorer(nxt, np.zeros((2, 4)))
    with pytest.raises(ValueError):
        lm.LmScorer(nxt, np.zeros((3, 3)))
    with pytest.raises(ValueError):
        lm.LmScorer(nxt, score, np.zeros(3))
    with pytest.raises(ValueError):
        lm.LmScorer(nxt, score, np.zeros((2, 1)))
    with pytest.raises(ValueError):
        lm.LmScorer(np.zeros(3, dtype=np.int32), np.zeros(3))
    with pytest.raises(ValueError):
        lm.LmScorer(np.zeros((0, 3), dtype=np.int32), np.zeros((0, 3)))
    with pytest.raises(ValueError):
        lm.LmScorer(np.zeros((2, 3)), score)         # float states


def test_scaled_is_computed_in_float64_and_rounded_once():
    rng = np.random.default_rng(5)
    score = -np.abs(rng.normal(size=(3, 4))) * 3
    score[1, 2] = -np.inf
    final = -np.abs(rng.normal(size=3))
    scorer = lm.LmScorer(rng.integers(0, 3, size=(3, 4)), score, final)
    got = scorer.scaled(0.37, 1.25)
    assert got.score.dtype == np.float32 and got.final.dtype == np.float32
    finite = np.isfinite(score)
    assert np.array_equal(got.score[finite], (0.37 * score[finite] + 1.25).astype(np.float32))
    assert np.isneginf(got.score[1, 2])
    assert np.array_equal(got.final, (0.37 * final).astype(np.float32))
    assert np.array_equal(got.next, scorer.next)
    zero = scorer.scaled(0.0, 0.0)                   # weight 0: forbidden edges stay forbidden
    assert np.isneginf(zero.score[1, 2]) and (zero.score[finite] == 0).all()
    assert (zero.final == 0).all()
    with pytest.raises(ValueError):
        scorer.scaled(np.inf, 0.0)


def test_cli_builds_from_a_manifest(tmp_path):
    manifest = tmp_path / 'train.csv'
    manifest.write_text('path;label;length\na.wav;hello world;1.0\nb.wav;hold the door;1.2\n')
    out = str(tmp_path / 'lm.npz')
    FLAGS.reset()
    try:
        assert lm.main(['--lm_corpus_csv', str(manifest), '--lm_order', '3', '--lm_path',
                        out]) == 0
        FLAGS.update(lm_path=out, lm_weight=0.5, lm_bonus=0.25)
        scorer = lm.from_flags(29)
        with pytest.raises(ValueError):
            lm.from_flags(30)
        FLAGS.update(lm_path='')
        assert lm.from_flags(29) is None
    finally:
        FLAGS.reset()
    from ctc_asr_amd.labels import encode
    built = lm.build_char_ngram([encode('hello world'), encode('hold the door')], 3, 29)
    assert np.array_equal(scorer.next, built.next)
    assert np.array_equal(scorer.score, built.scaled(0.5, 0.25).score)
    bad = tmp_path / 'bad.csv'
    bad.write_text('path;label;length\na.wav;Hello;1.0\n')
    with pytest.raises(ValueError):
        lm.corpus_label_rows(str(bad))
    assert FLAGS.lm_path == '' and FLAGS.lm_weight == 1.0 and FLAGS.lm_bonus == 0.0


# ------------------------------------------------------------------------------------------------
# The reference of the fused search
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm', ['max', 'log_softmax'])
@pytest.mark.parametrize('classes,blank,width', [(29, 28, 1), (29, 28, 8), (29, 0, 32), (3, 1, 4),
                                                 (64, 63, 16)])
def test_reference_with_a_zero_scorer_is_the_plain_oracle(classes, blank, width, norm):
    rng = np.random.default_rng(100 * classes + width)
    logits = (rng.normal(size=(40, 5, classes)) * 2).astype(np.float32)
    logits[:, :, blank] += 1.0
    seq_len = np.array([40, 0, 1, 23, 37], dtype=np.int32)
    zero_next = np.zeros((1, classes), dtype=np.int32)
    zero_score = np.zeros((1, classes), dtype=np.float32)
    paths, logp = ref.beam_search_decode(logits, seq_len, width, zero_next, zero_score, None,
                                         blank, norm)
    np_paths, np_logp = octc.beam_search_decode(logits, seq_len, width, blank, norm)
    assert paths == np_paths
    assert logp.tobytes() == np_logp.tobytes()
    c_paths, c_logp = cref.beam_search_decode(logits, seq_len, width, blank, norm)
    assert paths == c_paths
    assert np.allclose(logp, c_logp, rtol=1e-5, atol=1e-3)
    # ... and a zero `final` changes nothing either
    again = ref.beam_search_decode(logits, seq_len, width, zero_next, zero_score,
                                   np.zeros(1, dtype=np.float32), blank, norm)
    assert again[0] == paths and again[1].tobytes() == logp.tobytes()


TRUTH_SEEDS = 10
TRUTH_CASES = [(2, 10), (3, 9), (4, 5), (5, 4)]


def truth_inputs(classes, num_steps, blank):
    """TRUTH_SEEDS utterances as one batch, a random 4-state automaton (`next` uniform, `score`
    and `final` ~ N(0, 1)) and, per utterance, the two best labellings by the fused posterior
    ln p_ctc + automaton score of the exhaustive enumeration: (label, value), (runner-up, value).
    Logits are drawn first, then next, score, final."""
    rng = np.random.default_rng(20000 * classes + 100 * num_steps + blank)
    logits = (rng.normal(size=(num_steps, TRUTH_SEEDS, classes)) * 2).astype(np.float32)
    lm_next = rng.integers(0, 4, size=(4, classes)).astype(np.int32)
    lm_score = rng.normal(size=(4, classes)).astype(np.float32)
    lm_final = rng.normal(size=4).astype(np.float32)
    ranked = []
    for b in range(TRUTH_SEEDS):
        post = octc.brute_force_posteriors(logits[:, b].astype(np.float64), blank)
        assert abs(sum(post.values()) - 1.0) < 1e-12
        fused = {label: math.log(p) + ref.automaton_score(label, lm_next, lm_score, lm_final)
                 for label, p in post.items() if p > 0}
        ranked.append(sorted(fused.items(), key=lambda kv: -kv[1])[:2])
    return logits, (lm_next, lm_score, lm_final), ranked


def check_truth(decode, classes, num_steps):
    """``decode(logits, seq_len, (next, score, final), blank)`` -> (paths, logp) must be an
    unpruned `log_softmax` search.  A seed whose two best fused posteriors are closer than 1e-4
    relative is a near-tie and is skipped; at most 1 seed in 10 may be.  The value: logp within
    1e-5 relative (the bar of the plain search's truth test) plus 5e-5 absolute.  The absolute
    term is there because the fused value adds O(1) scores of either sign to a log-posterior and
    can sit near zero; its size is the float32 worst case of the sum itself: about 3 T <= 30
    rounded operations (edge score, lse, frame value per frame) on intermediates below 32 in
    magnitude, each off by at most 2^-24 * 32 = 1.9e-6."""
    assert sum((classes - 1) ** k for k in range(num_steps + 1)) <= 1023
    for blank in sorted({0, classes // 2, classes - 1}):
        logits, tables, ranked = truth_inputs(classes, num_steps, blank)
        paths, logp = decode(logits, [num_steps] * TRUTH_SEEDS, tables, blank)
        skipped, worst = 0, 0.0
        for b, ((best, v_best), (_, v_next)) in enumerate(ranked):
            if math.exp(v_next - v_best) > 1 - 1e-4:
                skipped += 1
                continue
            assert tuple(paths[b]) == best, (blank, b)
            err = abs(float(logp[b]) - v_best)
            worst = max(worst, err)
            assert err <= 1e-5 * abs(v_best) + 5e-5, (blank, b, float(logp[b]), v_best)
        print('fused truth C {} T {} blank {}: skipped {} of {}, max |logp - value| {:.3g}'
              .format(classes, num_steps, blank, skipped, TRUTH_SEEDS, worst))
        assert skipped * 10 <= TRUTH_SEEDS, skipped


@pytest.mark.parametrize('classes,num_steps', TRUTH_CASES)
def test_reference_unpruned_search_finds_the_best_fused_labelling(classes, num_steps):
    def decode(logits, seq_len, tables, blank):
        return ref.beam_search_decode(logits, seq_len, 1024, *tables, blank=blank,
                                      normalization='log_softmax')
    check_truth(decode, classes, num_steps)


def test_reference_never_takes_a_forbidden_edge():
    """Label 1 is forbidden from every state: no decode holds it, though the logits favour it;
    everything forbidden from the start state decodes to the empty string with the empty
    prefix's total plus final[0]."""
    rng = np.random.default_rng(9)
    logits = (rng.normal(size=(20, 1, 4)) * 2).astype(np.float32)
    logits[:, :, 1] += 3.0
    free, _ = octc.beam_search_decode(logits, [20], 8, 3)
    assert 1 in free[0]
    score = np.zeros((1, 4), dtype=np.float32)
    score[0, 1] = -np.inf
    paths, _ = ref.beam_search_decode(logits, [20], 8, np.zeros((1, 4), dtype=np.int32), score,
                                      None, 3)
    assert paths[0] and 1 not in paths[0]
    paths, logp = ref.beam_search_decode(logits, [20], 8, np.zeros((1, 4), dtype=np.int32),
                                         np.full((1, 4), -np.inf, dtype=np.float32),
                                         np.array([0.5], dtype=np.float32), 3, 'log_softmax')
    assert paths == [[]]
    blanks = octc.log_softmax(logits[:, 0].astype(np.float64))[:, 3].sum()
    assert float(logp[0]) == pytest.approx(blanks + 0.5, rel=1e-5)
