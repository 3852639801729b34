"""The host half of phrase spotting (``ctcasr_ctc_search``, `ctc_asr_amd.search`): the numpy
restatement of the pinned arithmetic (tests/search_reference.py) on properties that must hold
exactly, the hit pass on hand-made per-frame arrays, the flags, the phrase file, frames to
samples, and the export list."""

import numpy as np
import pytest

from tests import search_reference as sref

CLASSES, BLANK = 29, 28
NEG = -np.inf


# ---- the reference's own properties ------------------------------------------------------------

def _plant(logits, lab, at, run, gap, peak=8.0):
    """Raise ``lab`` on consecutive frames from ``at``: ``run`` frames a label, ``gap`` blanks
    between labels (one at least between equal ones).  Returns (first, last) frame."""
    t = at
    for i, c in enumerate(lab):
        if i:
            for _ in range(max(gap, 1 if lab[i - 1] == c else 0)):
                logits[t, BLANK] += peak
                t += 1
        for _ in range(run):
            logits[t, c] += peak
            t += 1
    return at, t - 1


@pytest.fixture(scope='module')
def planted():
    rng = np.random.default_rng(0)
    logits = rng.normal(0, 1, (300, CLASSES)).astype(np.float32)
    lab = [3, 3, 7, 1, 12]
    spans = [_plant(logits, lab, 40, 2, 1), _plant(logits, lab, 200, 3, 0)]
    return sref.table_of(logits), lab, spans


def test_a_phrase_planted_twice_comes_back_as_two_hits_of_score_zero(planted):
    table, lab, spans = planted
    end_score, end_start = sref.lattice(table, lab, BLANK, table.shape[0])
    hits = sref.hit_pass(end_score, end_start, -1.0 * len(lab))
    assert hits == [(0.0, spans[0][0], spans[0][1]), (0.0, spans[1][0], spans[1][1])]
    # the best is the FIRST frame that reaches the largest score: the last label's first frame
    # (it is held for two); the hit is extended over the second
    assert sref.best_of(end_score, end_start) == (0.0, (spans[0][0], spans[0][1] - 1))
    assert (end_score <= 0.0).all()


def test_the_greedy_phrase_of_a_span_scores_zero_over_that_span(planted):
    table, _, _ = planted
    greedy = table.argmax(-1)
    a, b = 37, 120
    while greedy[a] == BLANK:
        a += 1
    while greedy[b] == BLANK:
        b -= 1
    phrase, before = [], -1
    for t in range(a, b + 1):
        if greedy[t] != before and greedy[t] != BLANK:
            phrase.append(int(greedy[t]))
        before = greedy[t]
    end_score, end_start = sref.lattice(table, phrase, BLANK, table.shape[0])
    assert end_score[b] == 0.0 and end_start[b] == a
    assert end_score.max() == 0.0
    hits = sref.hit_pass(end_score, end_start, 0.0)
    assert (0.0, a, b) in hits


def test_all_zero_logits_tie_every_path_at_zero():
    table = sref.table_of(np.zeros((12, CLASSES), np.float32))
    end_score, end_start = sref.lattice(table, [1, 1, 2], BLANK, 12)
    assert end_score[:3].tolist() == [NEG] * 3 and end_start[:3].tolist() == [-1] * 3
    assert end_score[3:].tolist() == [0.0] * 9 and end_start[3:].tolist() == [0] * 9
    assert sref.hit_pass(end_score, end_start, 0.0) == [(0.0, 0, 11)]


def test_reference_statuses_and_no_hit_values():
    rng = np.random.default_rng(1)
    logits = rng.normal(size=(6, 2, 5)).astype(np.float32)
    logits[2, 1, 3] = np.nan
    table = sref.table_of(logits)
    phrases = [[1, 1], [1, 4], [], [7], [2]]
    out = sref.search(table, [2, 6], 4, phrases, [NEG] * 5,
                      [0, 0, 0, 0, 1, 5, 0, 0], [0, 1, 2, 3, 4, 0, 9, 4], 3)
    assert out['status'].tolist() == [1, 2, 2, 2, 3, 2, 2, 0]
    assert np.isnan(out['best_score'][4]) and np.isnan(out['end_score'][4]).all()
    for h in range(7):
        assert out['n_hits'][h] == 0 and (out['hits'][h] == -1).all()
        assert np.isneginf(out['hit_score'][h]).all() and (out['best_span'][h] == -1).all()
        assert (out['end_start'][h] == -1).all()
    assert np.isneginf(out['end_score'][[0, 1, 2, 3, 5, 6]]).all()
    assert np.isneginf(out['end_score'][7, 2:]).all() and np.isfinite(out['end_score'][7, :2]).all()
    assert out['n_hits'][7] >= 1


def test_fill_keeps_a_nan_row_and_ignores_nothing_else():
    table = np.array([[-1.0, -2.0], [np.nan, np.nan], [NEG, -0.5]], dtype=np.float32)
    fill = sref.fill_of(table)
    assert fill[0] == -1.0 and np.isnan(fill[1]) and fill[2] == -0.5


# ---- the hit pass on hand-made arrays -----------------------------------------------------------

def _pass(frames, min_score=-10.0, length=None):
    """``frames``: {t: (score, start)}; every other frame holds no candidate."""
    length = max(frames) + 1 if length is None else length
    end_score = np.full(length, NEG)
    end_start = np.full(length, -1, dtype=np.int64)
    for t, (score, start) in frames.items():
        end_score[t], end_start[t] = score, start
    return sref.hit_pass(end_score, end_start, min_score)


def test_hit_pass_drops_a_candidate_that_starts_under_the_flushed_end():
    # (0, 4) is flushed by the candidate that starts at 6; the one starting at 3 comes too late
    assert _pass({4: (-1.0, 0), 8: (-2.0, 6), 9: (-0.5, 3), 12: (-1.0, 10)}) == \
        [(-1.0, 0, 4), (-2.0, 6, 8), (-1.0, 10, 12)]
    # start == flushed_end is dropped too
    assert _pass({4: (-1.0, 0), 8: (-2.0, 6), 9: (-0.5, 4)}) == [(-1.0, 0, 4), (-2.0, 6, 8)]


def test_hit_pass_replaces_pending_on_a_strictly_better_score():
    assert _pass({4: (-2.0, 0), 5: (-1.0, 2)}) == [(-1.0, 2, 5)]
    assert _pass({4: (-1.0, 0), 5: (-2.0, 2)}) == [(-1.0, 0, 4)]
    # start == pending.end still overlaps
    assert _pass({4: (-2.0, 0), 6: (-1.0, 4)}) == [(-1.0, 4, 6)]


def test_hit_pass_extends_on_an_equal_score_with_the_same_start():
    assert _pass({4: (-1.0, 0), 5: (-1.0, 0), 6: (-1.0, 0)}) == [(-1.0, 0, 6)]


def test_hit_pass_keeps_pending_on_an_equal_score_with_another_start():
    assert _pass({4: (-1.0, 0), 5: (-1.0, 2)}) == [(-1.0, 0, 4)]


def test_hit_pass_flushes_at_the_end_and_applies_the_threshold():
    assert _pass({7: (-3.0, 5)}, length=20) == [(-3.0, 5, 7)]
    assert _pass({7: (-3.0, 5)}, min_score=-2.0) == []
    assert _pass({7: (-2.0, 5)}, min_score=-2.0) == [(-2.0, 5, 7)]
    assert _pass({7: (-2.0, 5)}, min_score=np.nan) == []
    assert _pass({}, length=5) == []
    # -inf is never a candidate, whatever the threshold
    assert sref.hit_pass(np.full(4, NEG), np.full(4, -1), NEG) == []


def test_n_hits_counts_beyond_max_hits():
    found = _pass({2: (-1.0, 0), 5: (-1.0, 3), 8: (-1.0, 6), 11: (-0.5, 9)})
    assert len(found) == 4
    hits, hit_score, n_hits = sref.pack_hits(found, 2)
    assert n_hits == 4 and hits.tolist() == [[0, 2], [3, 5]] and hit_score.tolist() == [-1.0, -1.0]
    hits, hit_score, n_hits = sref.pack_hits(found, 6)
    assert n_hits == 4 and hits[4:].tolist() == [[-1, -1]] * 2
    assert hit_score[3] == -0.5 and np.isneginf(hit_score[4:]).all()
    hits, hit_score, n_hits = sref.pack_hits(found, 0)
    assert n_hits == 4 and hits.shape == (0, 2) and hit_score.shape == (0,)


# ---- flags --------------------------------------------------------------------------------------

@pytest.fixture
def flags():
    from ctc_asr_amd.params import FLAGS
    FLAGS.reset()
    yield FLAGS
    FLAGS.reset()


def test_flag_defaults(flags):
    assert flags.phrases == '' and flags.search_output == ''
    assert flags.search_min_score == -1.0 and flags.search_max_hits == 16


@pytest.mark.parametrize('argv', [
    ['--search_min_score', '0.5'], ['--search_min_score', 'nan'], ['--search_min_score', '-inf'],
    ['--search_min_score', 'inf'], ['--search_min_score', 'low'], ['--search_min_score=1e-9'],
    ['--search_max_hits', '0'], ['--search_max_hits', '1025'], ['--search_max_hits', '-3'],
    ['--search_max_hits', 'many'], ['--search_max_hits', '2.5']])
def test_bad_flag_values_are_refused_at_parse_time(flags, argv):
    with pytest.raises(ValueError):
        flags.parse(argv)


def test_good_flag_values_parse(flags):
    flags.parse(['--search_min_score', '-0.25', '--search_max_hits', '1024', '--phrases', 'p.txt',
                 '--search_output=hits.jsonl'])
    assert flags.search_min_score == -0.25 and flags.search_max_hits == 1024
    assert flags.phrases == 'p.txt' and flags.search_output == 'hits.jsonl'
    flags.parse(['--search_min_score', '0', '--search_max_hits', '1'])
    assert flags.search_min_score == 0.0 and flags.search_max_hits == 1
    with pytest.raises(ValueError):
        flags.search_max_hits = 0
    with pytest.raises(ValueError):
        flags.search_min_score = 0.1


def test_driver_refuses_nbest_lm_and_missing_files(flags, tmp_path):
    from ctc_asr_amd import search
    wav, phrases = tmp_path / 'a.wav', tmp_path / 'p.txt'
    wav.write_bytes(b'')
    phrases.write_text('hello\n')
    base = ['--input', str(wav), '--phrases', str(phrases)]
    with pytest.raises(ValueError, match='nbest'):
        search.main(base + ['--nbest', '2', '--beam_width', '8'])
    flags.reset()                     # (flags keep their values from one parse to the next)
    with pytest.raises(ValueError, match='lm_path'):
        search.main(base + ['--lm_path', str(tmp_path / 'lm.arpa')])
    flags.reset()
    with pytest.raises(ValueError, match='input'):
        search.main(['--input', str(tmp_path / 'none.wav'), '--phrases', str(phrases)])
    with pytest.raises(ValueError, match='phrases'):
        search.main(['--input', str(wav), '--phrases', str(tmp_path / 'none.txt')])
    flags.reset()
    with pytest.raises(ValueError, match='phrases'):
        search.main(['--input', str(wav)])
    phrases.write_text('\n  \n')
    with pytest.raises(ValueError, match='no phrase'):
        search.main(base)
    phrases.write_text('fine\n\nroom 12\n')
    with pytest.raises(ValueError, match='line 3'):
        search.main(base)


# ---- the phrase file ----------------------------------------------------------------------------

def test_phrase_file_is_normalised_and_blank_lines_are_skipped(tmp_path):
    from ctc_asr_amd import search
    from ctc_asr_amd.labels import ctoi
    path = tmp_path / 'p.txt'
    path.write_text("Hello,  World!\n\n   \nit's\nNEW york\n", encoding='utf-8')
    assert search.read_phrases(str(path)) == ['hello world', 'its', 'new york']
    # the space is a label like any other
    from ctc_asr_amd.labels import encode
    assert encode('a b') == [ctoi('a'), ctoi(' '), ctoi('b')]


def test_phrase_file_errors_name_the_line():
    from ctc_asr_amd import search
    with pytest.raises(ValueError, match=r'line 2: .*digit "4"'):
        search.parse_phrases(['good', 'room 4'])
    with pytest.raises(ValueError, match=r'line 3: .*nothing is left'):
        search.parse_phrases(['good', '', '?!'])
    assert search.parse_phrases([]) == []


# ---- frames to samples --------------------------------------------------------------------------

def test_hit_samples_follow_the_hop_and_clip_at_the_piece_end():
    from ctc_asr_amd import search
    hop = 320
    assert search.hit_samples(1000, 3300, 0, 0, hop) == (1000, 1320)
    assert search.hit_samples(1000, 3300, 2, 5, hop) == (1640, 2920)
    # the piece holds 10 frames and a bit: frame 10 begins inside it, frame 11 would not
    assert search.hit_samples(1000, 3300, 9, 9, hop) == (3880, 4200)
    assert search.hit_samples(1000, 3300, 9, 10, hop) == (3880, 4300)
    assert search.hit_samples(1000, 3300, 10, 12, hop) == (4200, 4300)
    assert search.hit_samples(0, 100, 1, 1, hop) == (100, 100)


# ---- the export list ----------------------------------------------------------------------------

def test_signatures_hold_both_new_names():
    from ctc_asr_amd import hip
    for name in ('ctcasr_ctc_search', 'ctcasr_ctc_search_workspace_bytes'):
        assert name in hip.SIGNATURES
    restype, argtypes = hip.SIGNATURES['ctcasr_ctc_search']
    assert len(argtypes) == 26
    assert len(hip.SIGNATURES['ctcasr_ctc_search_workspace_bytes'][1]) == 3
    assert hip.SEARCH_MAX_LABEL_LEN == 576 and hip.SEARCH_MAX_HITS == 1024
    assert callable(hip.ctc_search) and callable(hip.ctc_search_workspace_bytes)
