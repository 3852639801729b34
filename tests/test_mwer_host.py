"""The host side of minimum word error rate training (no GPU): the float64 reference of
``ctcasr_ctc_mwer`` (tests/mwer_reference.py) against ``oracle.ctc``, against central differences
of the expected risk and against the exact Bayes risk of a complete hypothesis set; the flags and
their refusals; the argument errors of the entry point."""

import itertools

import numpy as np
import pytest

from ctc_asr_amd.params import FLAGS, check_mwer_settings
from oracle import ctc as octc
from tests import mwer_reference as ref


@pytest.fixture()
def flags():
    FLAGS.reset()
    yield FLAGS
    FLAGS.reset()


def test_reference_lattices_are_the_oracles():
    """occ = softmax - (the oracle's CTC gradient), ln p = -(its loss): the vectorised recursions
    of the reference are `oracle.ctc.ctc_loss_single`'s."""
    rng = np.random.RandomState(3)
    for steps, classes, label in ((1, 3, []), (1, 3, [1]), (5, 4, [0, 0]), (7, 5, [1, 2, 1]),
                                  (9, 4, [2, 2, 2, 0]), (6, 3, [])):
        logits = rng.randn(steps, classes) * 2.0
        loss, grad = octc.ctc_loss_single(logits, label)
        logp = octc.log_softmax(logits)
        occ, log_pyx = ref.occupancy(logp, label, classes - 1)
        assert abs(log_pyx + loss) <= 1e-12 * max(1.0, abs(loss))
        np.testing.assert_allclose(occ, np.exp(logp) - grad, rtol=0, atol=1e-12)
        np.testing.assert_allclose(occ.sum(axis=1), 1.0, rtol=0, atol=1e-12)


def test_analytic_gradient_against_central_differences():
    """T = 6, C = 4, three hypotheses with distinct risks; step 1e-5, bar 1e-6 absolute: the
    truncation error is O(h^2) ~ 1e-10 times a third derivative of order one and the round-off
    about eps / h ~ 2e-11, both far below the bar."""
    rng = np.random.RandomState(11)
    steps, classes = 6, 4
    logits = rng.randn(steps, classes)
    hyps, risks = [[0, 1], [1], [2, 2, 0]], [0.0, 1.0, 3.0]
    out = ref.mwer(logits[:, None, :], [steps], [hyps], [risks])
    assert (out['status'] == 0).all()
    step, worst = 1e-5, 0.0
    for t, k in itertools.product(range(steps), range(classes)):
        hi, lo = logits.copy(), logits.copy()
        hi[t, k] += step
        lo[t, k] -= step
        numeric = (ref.expected_risk(hi, hyps, risks) - ref.expected_risk(lo, hyps, risks)) / \
            (2 * step)
        worst = max(worst, abs(numeric - out['grad'][t, 0, k]))
    print('largest |analytic - central difference| = {:.3g}'.format(worst))
    assert worst <= 1e-6
    assert np.abs(out['grad']).max() > 1e-2                # (the check is not vacuous)
    assert abs(out['expected_risk'][0] - ref.expected_risk(logits, hyps, risks)) <= 1e-12


def test_complete_hypothesis_set_gives_the_bayes_risk():
    """Over ALL label sequences of T = 4, C = 3 (`oracle.ctc.brute_force_posteriors`) the list's
    posterior is the model's, so R_b is the exact Bayes risk."""
    rng = np.random.RandomState(5)
    logits = rng.randn(4, 3) * 1.5
    table = octc.brute_force_posteriors(logits)
    hyps = sorted(table, key=lambda label: -table[label])
    assert abs(sum(table.values()) - 1.0) <= 1e-12
    truth = (0, 1)
    risks = [float(_levenshtein(label, truth)) for label in hyps]
    bayes = sum(table[label] * risk for label, risk in zip(hyps, risks))
    out = ref.mwer(logits[:, None, :], [4], [[list(label) for label in hyps]], [risks])
    assert (out['status'] == 0).all()
    assert abs(out['expected_risk'][0] - bayes) <= 1e-12
    np.testing.assert_allclose(out['posterior'][0], [table[label] for label in hyps], rtol=0,
                               atol=1e-12)
    # the gradient of a risk that the model cannot lower by moving mass inside the list alone is
    # still a zero-sum redistribution per frame
    np.testing.assert_allclose(out['grad'].sum(axis=2), 0.0, rtol=0, atol=1e-12)


def _levenshtein(a, b):
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        prev, row[0] = row[0], i
        for j, y in enumerate(b, 1):
            prev, row[j] = row[j], min(row[j] + 1, row[j - 1] + 1, prev + (x != y))
    return row[-1]


def test_gradient_rows_sum_to_zero_and_rows_behind_seq_len_are_zero():
    rng = np.random.RandomState(7)
    logits = rng.randn(7, 3, 5) * 2.0
    hyps = [[[0, 1], [1], [], [3, 3]], [[2], [2, 0], [0], []], [[1], [], [2], [3]]]
    risks = [[2.0, 1.0, 3.0, 0.0], [0.0, 1.0, 1.0, 2.0], [1.0, 2.0, 3.0, 4.0]]
    out = ref.mwer(logits, [7, 4, 0], hyps, risks, scale=0.25)
    np.testing.assert_allclose(out['grad'].sum(axis=2), 0.0, rtol=0, atol=1e-13)
    assert np.abs(out['grad'][:, 0]).max() > 1e-3 and np.abs(out['grad'][:4, 1]).max() > 1e-3
    assert not out['grad'][4:, 1].any() and not out['grad'][:, 2].any()
    np.testing.assert_allclose(out['c'].sum(axis=1), 0.0, rtol=0, atol=1e-13)
    # seq_len 0: only the empty hypothesis is feasible - one valid row, risk 2, no gradient
    assert out['status'][2].tolist() == [1, 0, 1, 1] and out['expected_risk'][2] == 2.0
    # equal risks: no gradient at all
    flat = ref.mwer(logits, [7, 4, 0], hyps, [[1.0] * 4] * 3)
    assert np.abs(flat['grad']).max() <= 1e-15


def test_weights_of_short_and_degenerate_lists():
    post, risk, coeff = ref.weights([-1.0, -2.0, -3.0], [5.0, 1.0, 2.0], [False, True, False])
    assert post.tolist() == [0.0, 1.0, 0.0] and risk == 1.0 and not coeff.any()
    post, risk, coeff = ref.weights([-1.0, -2.0], [5.0, 1.0], [False, False])
    assert not post.any() and risk == 0.0 and not coeff.any()
    post, risk, coeff = ref.weights([-np.inf, -np.inf], [4.0, 2.0], [True, True])
    assert post.tolist() == [0.5, 0.5] and risk == 3.0 and coeff.tolist() == [0.5, -0.5]
    post, risk, coeff = ref.weights([np.log(0.25), np.log(0.75)], [4.0, 0.0], [True, True])
    np.testing.assert_allclose(post, [0.25, 0.75], atol=1e-15)
    assert abs(risk - 1.0) <= 1e-15 and abs(coeff.sum()) <= 1e-15


# ------------------------------------------------------------------------------------------------
def test_flag_defaults_and_what_parses(flags):
    assert (flags.mwer_nbest, flags.mwer_beam_width, flags.mwer_ctc_weight, flags.mwer_risk) == \
        (0, 64, 0.01, 'word')
    flags.parse(['--mwer_nbest', '2'])
    flags.parse(['--mwer_nbest', '64', '--mwer_beam_width', '64'])
    flags.parse(['--mwer_nbest', '8', '--mwer_beam_width', '1024', '--mwer_ctc_weight', '0',
                 '--mwer_risk', 'label'])
    assert flags.mwer_risk == 'label' and flags.mwer_ctc_weight == 0.0
    # the training search has a width of its own: --beam_width does not bound the list
    flags.reset()
    flags.parse(['--mwer_nbest', '16', '--beam_width', '8'])
    flags.reset()
    flags.parse(['--mwer_nbest', '0'])


@pytest.mark.parametrize('argv', [
    ['--mwer_nbest', '1'], ['--mwer_nbest', '-1'], ['--mwer_nbest', '65'],
    ['--mwer_nbest', '4', '--mwer_beam_width', '3'],
    ['--mwer_nbest', '4', '--mwer_beam_width', '1025'],
    ['--mwer_nbest', '64', '--mwer_beam_width', '63'],
    ['--mwer_nbest', '4', '--mwer_ctc_weight', '-0.1'],
    ['--mwer_nbest', '4', '--mwer_ctc_weight', 'nan'],
    ['--mwer_nbest', '4', '--mwer_ctc_weight', 'inf'],
    ['--mwer_nbest', '4', '--mwer_risk', 'char'],
    ['--mwer_beam_width', '32'], ['--mwer_ctc_weight', '0.5'], ['--mwer_risk', 'label'],
], ids=' '.join)
def test_flag_refusals(flags, argv):
    with pytest.raises(ValueError):
        flags.parse(argv)


def test_settings_check_is_the_trainers_too():
    check_mwer_settings(0, 1, -1.0, 'nothing')              # off: nothing else is looked at
    check_mwer_settings(4, 4, 0.0, 'label')
    for bad in ((1, 64, 0.01, 'word'), (65, 128, 0.01, 'word'), (4, 3, 0.01, 'word'),
                (4, 2048, 0.01, 'word'), (4, 64, float('nan'), 'word'), (4, 64, -1.0, 'word'),
                (4, 64, 0.01, 'sentence')):
        with pytest.raises(ValueError):
            check_mwer_settings(*bad)


# ------------------------------------------------------------------------------------------------
def test_entry_point_refuses_bad_arguments_before_the_device():
    from ctc_asr_amd import build, hip
    build.build(verbose=False)
    lib = hip.load()
    one = 1                                                  # (any non-null address: never read)

    def call(steps=4, batch=2, classes=5, blank=4, nbest=3, max_label_len=4, pointer=one,
             workspace=one, nbytes=1 << 40):
        return lib.ctcasr_ctc_mwer(pointer, one, steps, batch, classes, blank, one, one, one, one,
                                   nbest, max_label_len, 1.0, 0, one, one, one, one, one,
                                   workspace, nbytes, None)

    assert call(pointer=None) == -1
    for wrong in ({'steps': 0}, {'batch': 0}, {'classes': 1}, {'blank': 5}, {'blank': -1},
                  {'nbest': 0}, {'max_label_len': -1}):
        assert call(**wrong) == -1, wrong
    for unsupported in ({'classes': 65, 'blank': 0}, {'max_label_len': 576}, {'batch': 65536}):
        assert call(**unsupported) == -2, unsupported
    need = lib.ctcasr_ctc_mwer_workspace_bytes(4, 2, 5, 3, 4)
    assert call(nbytes=need - 1) == -3 and call(workspace=None) == -3
    # the table, two fp64 lattices of [B N][T][64 * states per lane], two fp64 per row, one word
    # per utterance, each rounded up to 256 bytes
    assert need == 256 + 2 * (6 * 4 * 64 * 8) + 2 * 256 + 256
    query = lib.ctcasr_ctc_mwer_workspace_bytes
    assert query(500, 32, 29, 16, 100) == \
        500 * 32 * 29 * 4 + 2 * (512 * 500 * 6 * 64 * 8) + 2 * 4096 + 256
    assert query(4, 2, 5, 3, 576) == 0 and query(4, 2, 5, 0, 4) == 0 and query(0, 2, 5, 3, 4) == 0
