"""The host side of n-best decoding and rescoring (no GPU): the flags and their refusals,
`LmScorer.sequence_scores`, the posterior / selection arithmetic of `CTCModel.nbest_posteriors`
and the oracle-rate arithmetic of `metrics.oracle_errors` / `metrics.corpus_rate`."""

import math

import numpy as np
import pytest

from ctc_asr_amd import lm, metrics
from ctc_asr_amd.model import CTCModel
from ctc_asr_amd.params import FLAGS
from tests.lm_beam_reference import automaton_score


@pytest.fixture()
def flags():
    FLAGS.reset()
    yield FLAGS
    FLAGS.reset()


def _tiny_lm(path, classes):
    rows = [[1, 2, 3], [2, 2, 1], [3, 1]]
    lm.build_char_ngram(rows, 2, classes).save(str(path))
    return str(path)


# ------------------------------------------------------------------------------------------------
def test_flag_defaults_and_what_parses(flags, tmp_path):
    assert (flags.nbest, flags.rescore_lm_path, flags.rescore_lm_weight,
            flags.rescore_lm_bonus) == (0, '', 1.0, 0.0)
    flags.parse(['--nbest', '1'])
    flags.parse(['--nbest', '1024'])
    flags.parse(['--nbest', '8', '--beam_width', '8'])
    path = _tiny_lm(tmp_path / 'second.npz', flags.num_classes)
    flags.parse(['--nbest', '2', '--rescore_lm_path', path, '--rescore_lm_weight', '0.5',
                 '--rescore_lm_bonus', '-1'])
    assert flags.rescore_lm_weight == 0.5 and flags.rescore_lm_bonus == -1.0
    scorer = lm.rescorer_from_flags(flags.num_classes)
    assert scorer.order == 2 and scorer.score.dtype == np.float32
    flags.reset()
    assert lm.rescorer_from_flags(flags.num_classes) is None


@pytest.mark.parametrize('argv', [
    ['--nbest', '-1'], ['--nbest', '1025'],
    ['--nbest', '9', '--beam_width', '8'],
    ['--rescore_lm_weight', '0.5'], ['--rescore_lm_bonus', '0.1'],
    ['--nbest', '1', '--rescore_lm_weight', '2'],
    ['--nbest', '4', '--rescore_lm_weight', 'nan'], ['--nbest', '4', '--rescore_lm_bonus', 'inf'],
    ['--nbest', '4', '--rescore_lm_path', '/nonexistent/second.npz'],
], ids=' '.join)
def test_flag_refusals(flags, argv):
    with pytest.raises(ValueError):
        flags.parse(argv)


def test_rescoring_file_is_checked_at_parse_time(flags, tmp_path):
    path = _tiny_lm(tmp_path / 'second.npz', flags.num_classes)
    for argv in (['--rescore_lm_path', path], ['--nbest', '1', '--rescore_lm_path', path]):
        with pytest.raises(ValueError, match='nbest'):
            flags.parse(argv)
        flags.reset()
    other = _tiny_lm(tmp_path / 'other.npz', flags.num_classes + 1)
    with pytest.raises(ValueError, match='classes'):
        flags.parse(['--nbest', '4', '--rescore_lm_path', other])


# ------------------------------------------------------------------------------------------------
def test_sequence_scores_of_a_hand_computed_automaton():
    """Two states over four classes (3: the blank).  State 0 -a-> 1, 1 -b-> 0, 1 -a-> 1;
    label 2 is forbidden in state 1; ending in state 1 is forbidden."""
    inf = np.inf
    nxt = np.array([[1, 0, 0, 0], [1, 0, 1, 1]])
    score = np.array([[-1.0, -2.0, -0.5, 0.0], [-0.25, -4.0, -inf, 0.0]])
    final = np.array([-0.125, -inf])
    scorer = lm.LmScorer(nxt, score, final)
    rows = [[], [1], [0, 1], [0, 0, 1], [0], [0, 2], [2, 2, 1]]
    want = [-0.125, -2.125, -5.125, -5.375, -inf, -inf, -3.125]
    got = scorer.sequence_scores(rows)
    assert got.dtype == np.float64 and got.tolist() == want
    for row, value in zip(rows, got):
        assert value == automaton_score(row, nxt, score, final)
    # without `final` the end adds nothing
    assert lm.LmScorer(nxt, score).sequence_scores([[0], [0, 0]]).tolist() == [-1.0, -1.25]
    assert scorer.sequence_scores([]).shape == (0,)
    with pytest.raises(ValueError):
        scorer.sequence_scores([[4]])
    # float64 sums of the float64 tables: no float32 rounding on the way
    fine = lm.LmScorer(np.zeros((1, 3), dtype=np.int64), np.full((1, 3), -0.1))
    assert fine.sequence_scores([[0] * 10])[0] == sum([-0.1] * 10)


# ------------------------------------------------------------------------------------------------
def test_posteriors_and_selection_on_hand_made_totals():
    post, selected = CTCModel.nbest_posteriors([math.log(0.5), math.log(0.25), math.log(0.25)])
    assert selected == 0 and np.allclose(post, [0.5, 0.25, 0.25], rtol=0, atol=1e-15)
    # unnormalised totals: the softmax normalises
    post, selected = CTCModel.nbest_posteriors([-1000.0, -1000.0 + math.log(3.0)])
    assert selected == 1 and np.allclose(post, [0.25, 0.75], rtol=0, atol=1e-12)
    # ties go to the lower rank
    post, selected = CTCModel.nbest_posteriors([-3.0, -2.0, -2.0, -5.0])
    assert selected == 1 and post[1] == post[2]
    # a -inf hypothesis has posterior 0 and is never selected
    post, selected = CTCModel.nbest_posteriors([-np.inf, -7.0, -7.0 + math.log(3.0)])
    assert selected == 2 and post[0] == 0.0 and np.allclose(post[1:], [0.25, 0.75])
    # a single hypothesis has posterior 1, whatever its total
    for total in (0.0, -1234.5):
        post, selected = CTCModel.nbest_posteriors([total])
        assert selected == 0 and post.tolist() == [1.0]
    # hypotheses whose score has a non-zero status stay out of the softmax
    post, selected = CTCModel.nbest_posteriors([0.0, math.log(0.5), math.log(0.5)],
                                               [False, True, True])
    assert selected == 1 and post.tolist() == [0.0, 0.5, 0.5]
    post, selected = CTCModel.nbest_posteriors([-1.0, -2.0], [False, False])
    assert selected == -1 and post.tolist() == [0.0, 0.0]
    post, selected = CTCModel.nbest_posteriors([-np.inf, -np.inf])
    assert selected == 0 and post.tolist() == [0.5, 0.5]
    assert post.dtype == np.float64


# ------------------------------------------------------------------------------------------------
def test_oracle_rates_on_hand_made_count_tables():
    # three utterances with 3, 1 and 2 hypotheses
    label_distances = [4, 2, 3, 0, 5, 5]
    word_distances = [2, 2, 1, 0, 1, 3]
    sizes = [3, 1, 2]
    assert metrics.oracle_errors(label_distances, sizes).tolist() == [2, 0, 5]
    assert metrics.oracle_errors(word_distances, sizes).tolist() == [1, 0, 1]
    # the oracle picks per metric: labels take hypothesis 1 of the first utterance, words 2
    assert metrics.corpus_rate(2 + 0 + 5, 10 + 4 + 6) == 7 / 20
    assert metrics.corpus_rate(1 + 0 + 1, 3 + 1 + 2) == 2 / 6
    # never above the rate of rank 0
    assert metrics.oracle_errors(label_distances, sizes).sum() <= 4 + 0 + 5
    assert math.isnan(metrics.corpus_rate(0, 0))
    assert metrics.oracle_errors([], []).shape == (0,)
    assert metrics.oracle_errors([7], [1]).tolist() == [7]
    for bad in (([1, 2], [1, 0, 1]), ([1, 2, 3], [1, 1]), ([1], [2])):
        with pytest.raises(ValueError):
            metrics.oracle_errors(*bad)
