"""CTC forced alignment on the host: the float64 Viterbi reference of ``ctcasr_ctc_align``
(tests/align_reference.py) against brute-force enumeration and its tie rule, and the host-side
turning of states into timed words (`ctc_asr_amd.alignment`)."""

import itertools

import numpy as np
import pytest

from ctc_asr_amd import alignment
from ctc_asr_amd.labels import encode
from ctc_asr_amd.model import ModelConfig
from tests import align_reference as ref


def _labels(classes, blank, max_len, repeats):
    ids = [c for c in range(classes) if c != blank]
    for length in range(max_len + 1):
        for label in itertools.product(ids, repeat=length):
            if repeats or all(a != b for a, b in zip(label, label[1:])):
                yield list(label)


@pytest.mark.parametrize('num_steps,classes,blank', [(1, 3, 2), (3, 3, 0), (4, 4, 3), (5, 3, 1),
                                                      (6, 3, 2), (7, 2, 1), (5, 5, 4)])
def test_reference_matches_brute_force(num_steps, classes, blank):
    """Best score and best frame path of every label with L <= 3 (repeats included) equal those
    of enumerating all C^T frame paths; infeasible labels have no path."""
    rng = np.random.default_rng(num_steps * 100 + classes)
    logits = rng.normal(size=(num_steps, classes)) * 2.0
    max_len = 3 if classes ** num_steps <= 20000 else 2
    seen = 0
    for label in _labels(classes, blank, max_len, repeats=True):
        best, frames = ref.brute_force(logits, label, blank)
        score, path = ref.viterbi(logits, label, blank)
        if frames is None:
            assert path is None and score == -np.inf, label
            continue
        seen += 1
        assert abs(score - best) <= 1e-9 * max(1.0, abs(best)), (label, score, best)
        assert ref.path_classes(path, label, blank) == frames, label
        assert ref.is_valid_path(path, label, blank, num_steps) is None
        assert abs(ref.rescore(logits, label, path, blank) - score) <= 1e-9 * max(1.0, abs(score))
    assert seen > 0


def test_uniform_logits_take_the_documented_tie_path():
    """With every path tied, the rule (stay before s - 1 before s - 2; S - 1 before S - 2 at the
    end) keeps the backtrace in the final blank for as long as that state is reachable and then
    steps down one state at a time: every label as early as it can be, one frame each, the blank
    between the repeated labels, and the final blank over the rest."""
    logits = np.zeros((9, 4))
    blank = 3
    score, path = ref.viterbi(logits, [0, 1, 1], blank)
    # S = 7: state 6 is reachable from t = 4 on (1, 3, 4, 5, 6)
    assert path == [1, 3, 4, 5, 6, 6, 6, 6, 6]
    assert score == pytest.approx(9 * np.log(0.25))
    # a tight row leaves one path, whatever the rule
    _, path = ref.viterbi(np.zeros((4, 4)), [0, 1, 1], blank)
    assert path == [1, 3, 4, 5]
    # L = 0: the all-blank path
    score, path = ref.viterbi(np.zeros((3, 4)), [], blank)
    assert path == [0, 0, 0] and score == pytest.approx(3 * np.log(0.25))


def test_margin_is_the_gap_to_the_second_best_alignment():
    rng = np.random.default_rng(3)
    for _ in range(20):
        logits = rng.normal(size=(5, 3)) * 3.0
        label = [int(v) for v in rng.integers(0, 2, size=int(rng.integers(1, 3)))]
        score, path = ref.viterbi(logits, label, 2)
        if path is None:
            continue
        scores = sorted((ref.rescore(logits, label, list(p), 2)
                         for p in itertools.product(range(2 * len(label) + 1), repeat=5)
                         if ref.is_valid_path(list(p), label, 2, 5) is None), reverse=True)
        second = scores[1] if len(scores) > 1 else -np.inf
        assert ref.margin(logits, label, path, 2) == pytest.approx(score - second, abs=1e-9)


def test_validity_check_rejects_bad_paths():
    label, blank = [0, 0], 2                    # ext = [b, 0, b, 0, b]
    assert ref.is_valid_path([1, 2, 3], label, blank, 3) is None
    assert ref.is_valid_path([1, 3, 4], label, blank, 3) is not None      # skip between repeats
    assert ref.is_valid_path([2, 3, 4], label, blank, 3) is not None      # starts in 2
    assert ref.is_valid_path([1, 2, 2], label, blank, 3) is not None      # ends in 2
    assert ref.is_valid_path([1, 1, 0, 3], label, blank, 4) is not None   # not monotone


# ---------------------------------------------------------------------------------------------
# states -> words
# ---------------------------------------------------------------------------------------------
def _path_for(frame_labels, num_labels):
    """State path from a per-frame list of label positions (None = blank before the next)."""
    path, k_next = [], 0
    for pos in frame_labels:
        if pos is None:
            path.append(2 * k_next)
        else:
            path.append(2 * pos + 1)
            k_next = pos + 1
    return path


def test_segments_leading_trailing_blanks_and_one_frame_words():
    labels = encode('ab c')            # positions 0 a, 1 b, 2 ' ', 3 c
    path = _path_for([None, None, 0, 0, 1, None, 2, 3, None, None], 4)
    logp = np.linspace(-0.1, -1.0, len(path))
    words = alignment.segments(path, labels, 0.02, logp)
    assert [w['word'] for w in words] == ['ab', 'c']
    assert words[0]['start'] == pytest.approx(2 * 0.02) and \
        words[0]['end'] == pytest.approx(5 * 0.02)
    assert words[1]['start'] == pytest.approx(7 * 0.02) and \
        words[1]['end'] == pytest.approx(8 * 0.02)
    assert words[0]['confidence'] == pytest.approx(np.mean(logp[[2, 3, 4]]))
    assert words[1]['confidence'] == pytest.approx(logp[7])
    assert alignment.segments(path, labels, 0.02)[0]['confidence'] is None


def test_segments_spaces_at_the_ends_and_double_spaces():
    labels = encode(' hi  yo ')        # 0 ' ', 1 h, 2 i, 3 ' ', 4 ' ', 5 y, 6 o, 7 ' '
    path = _path_for([0, 1, 2, 3, None, 4, 5, 6, 7, None], 8)
    words = alignment.segments(path, labels, 0.01)
    assert [w['word'] for w in words] == ['hi', 'yo']
    assert [(w['start'], w['end']) for w in words] == [(0.01, 0.03), (0.06, 0.08)]
    assert alignment.segments(_path_for([0, None, 1], 2), encode('  '), 0.01) == []


def test_segments_repeated_letters_split_by_a_blank():
    labels = encode('all')             # a, l, l: the second l needs a blank before it
    path = _path_for([0, 1, 1, None, 2, 2, None], 3)
    words = alignment.segments(path, labels, 0.04)
    assert words == [{'word': 'all', 'start': 0.0, 'end': 0.24, 'confidence': None}]
    spans = alignment.label_spans(path, 3)
    assert spans == [(0, 0), (1, 2), (4, 5)]


def test_segments_of_a_row_without_a_path():
    assert alignment.segments([-1] * 5, encode('ab'), 0.02) == []
    assert alignment.segments([0, 0, -1], [], 0.02) == []


@pytest.mark.parametrize('model,drop,expected', [('ds1', False, 0.01), ('ds1', True, 0.02),
                                                 ('ds2', False, 0.02), ('ds2', True, 0.04)])
def test_frame_seconds(model, drop, expected):
    cfg = ModelConfig(used_model=model, conv_filters=(4, 4))
    assert alignment.frame_seconds(cfg, drop) == pytest.approx(expected)
    # ds2 halves the frames: one logit frame per two feature frames
    assert cfg.output_time(100) * alignment.frame_seconds(cfg, drop) == \
        pytest.approx(100 * 0.01 * (2 if drop else 1))
