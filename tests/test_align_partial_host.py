"""The host half of alignment with wildcard spans (`align_long.parse_transcript`, ``skipped``,
`cut_utterances(barriers=...)`, the two flags) and the proof of the reference the GPU tests
compare with: `tests.align_partial_reference.on_table` against the enumeration of every legal
path, for every position of one or two wildcards.  The C-ABI argument checks at the end run
before the device is touched.  No GPU."""

import ctypes
import itertools
import json

import numpy as np
import pytest
from scipy.io import wavfile

from oracle import ctc as octc
from tests import align_partial_reference as pref

RATE = 16000
W = pref.WILDCARD


# ---- 1. the reference against brute force ---------------------------------------------------------
def _table(rng, num_steps, classes):
    logits = rng.normal(size=(num_steps, classes)) * 2.0
    return octc.log_softmax(logits).astype(np.float32)


def _wildcard_rows(length):
    """Every way to put one wildcard, or two that are not neighbours, into ``length`` labels."""
    rows = [(k,) for k in range(length)]
    rows += [(a, b) for a, b in itertools.combinations(range(length), 2) if b - a >= 2]
    return rows


def test_reference_equals_brute_force_for_every_wildcard_position():
    rng = np.random.default_rng(7)
    classes, blank = 4, 3
    cases = 0
    for length in (1, 2, 3):
        for where in _wildcard_rows(length):
            for repeat in (False, True):
                label = [int(v) for v in rng.integers(0, 3, size=length)]
                if repeat:                      # equal labels around and beside the wildcard
                    label = [label[0]] * length
                for k in where:
                    label[k] = W
                for num_steps in range(pref.required_time(label), 7):
                    table = _table(rng, num_steps, classes)
                    want, winners = pref.brute_force(table, label, blank)
                    score, path, flp = pref.on_table(table, label, blank)
                    assert winners, (label, num_steps)
                    assert score == want, (label, num_steps, score, want)
                    assert path.tolist() in winners, (label, num_steps)
                    fill = table.max(axis=1)
                    wild = pref.wildcard_frames(path, label)
                    assert wild.any()           # a wildcard takes at least one frame
                    assert (flp[wild] == fill[wild]).all()
                    cases += 1
    assert cases > 60


def test_reference_without_a_path_and_status_rules():
    rng = np.random.default_rng(8)
    logits = rng.normal(size=(3, 5)).astype(np.float32)
    assert pref.required_time([W, 1, 1, W]) == 5 and pref.required_time([1, W, 1]) == 3
    assert pref.expected_status(logits, [1, W, 1], 4) == 0
    assert pref.expected_status(logits, [W], 4) == 0
    assert pref.expected_status(logits, [W, W], 4) == 2
    assert pref.expected_status(logits, [1, -2], 4) == 2
    assert pref.expected_status(logits, [W, 4], 4) == 2          # the blank
    assert pref.expected_status(logits, [W, 1, W, 2], 4) == 1    # T = 3 < 4
    assert pref.expected_status(logits, [W, 1, 1], 4) == 1       # 3 labels + 1 repeat
    bad = logits.copy()
    bad[1, 2] = np.nan
    assert pref.expected_status(bad, [W, 1], 4) == 3
    assert pref.expected_status(bad, [W, W], 4) == 2 and pref.expected_status(bad, [W] + [1] * 3, 4) == 1
    # too few frames: the enumeration finds nothing either
    table = _table(rng, 2, 5)
    assert pref.brute_force(table, [1, W, 2], 4) == (-np.inf, [])
    # a transcript that is one wildcard: the score is the greedy sum, taken in time order
    table = _table(rng, 6, 5)
    table[:, 4] -= 50                                            # (the blank never wins)
    score, path, flp = pref.on_table(table, [W], 4)
    assert path.tolist() == [1] * 6 and (flp == table.max(axis=1)).all()
    assert score == np.cumsum(table.max(axis=1).astype(np.float64))[-1]


def test_replacing_labels_by_a_wildcard_never_lowers_the_score():
    rng = np.random.default_rng(9)
    classes, blank = 6, 5
    for _ in range(30):
        length = int(rng.integers(3, 7))
        label = [int(v) for v in rng.integers(0, 5, size=length)]
        a = int(rng.integers(0, length - 1))
        b = int(rng.integers(a + 1, length + 1))
        partial = label[:a] + [W] + label[b:]
        table = _table(rng, ref_time(label) + int(rng.integers(0, 5)), classes)
        full = pref.on_table(table, label, blank)[0]
        assert pref.on_table(table, partial, blank)[0] >= full


def ref_time(label):
    return octc.required_time(label)


# ---- 2. parse_transcript -------------------------------------------------------------------------
def test_parse_transcript_merging_ends_and_no_space_beside_a_wildcard():
    from ctc_asr_amd.align_long import normalize_transcript, parse_transcript
    from ctc_asr_amd.labels import encode
    # without a wildcard: normalize_transcript and encode
    assert parse_transcript("Hello,  World") == ('hello world', encode('hello world'))
    assert parse_transcript('a [x] b') == ('a x b', encode('a x b'))     # (off: a token like any)
    # one in the middle: no space label on either side
    text, labels = parse_transcript('Ab cd [x] Ef', '[x]')
    assert text == 'ab cd [x] ef'
    assert labels == encode('ab cd') + [W] + encode('ef') and 1 not in labels[5:7]
    # neighbours merge, also across text that normalises to nothing
    assert parse_transcript('a [x] [x] b', '[x]') == ('a [x] b', [2, W, 3])
    assert parse_transcript("a [x] -- ' [x] ... [x] b", '[x]') == ('a [x] b', [2, W, 3])
    # at the ends; free ends merge with one that is there
    assert parse_transcript('[x] a b', '[x]') == ('[x] a b', [W, 2, 1, 3])
    assert parse_transcript('a b [x] ?', '[x]') == ('a b [x]', [2, 1, 3, W])
    assert parse_transcript('a b', '', True) == ('* a b *', [W, 2, 1, 3, W])
    assert parse_transcript('[x] a b', '[x]', True) == ('[x] a b *', [W, 2, 1, 3, W])
    assert parse_transcript('-- [x] a [x] b [x] !', '[x]', True) == \
        ('[x] a [x] b [x]', [W, 2, W, 3, W])
    # the token must stand alone between whitespace
    assert parse_transcript('a[x] b', '[x]') == ('a x b', encode('a x b'))
    assert parse_transcript('a\n<*>\tb', '<*>') == ('a <*> b', [2, W, 3])
    # never two wildcards side by side, never a space beside one
    for text in ('[x] a  [x] [x] b c [x]', 'a b c', '[x] [x] q'):
        for free in (False, True):
            labels = parse_transcript(text, '[x]', free)[1]
            for before, after in zip(labels, labels[1:]):
                assert not (before == W and after in (W, 1)) and not (before == 1 and after == W)
    assert normalize_transcript('a [x] b') == 'a x b'                    # (unchanged)


def test_parse_transcript_digits_and_refusals():
    from ctc_asr_amd.align_long import parse_transcript
    with pytest.raises(ValueError, match='"6" at offset 13'):
        parse_transcript('hi [x] route 66', '[x]')
    with pytest.raises(ValueError, match='"7" at offset 0'):
        parse_transcript('7 [x] a', '[x]')
    with pytest.raises(ValueError, match='offset 8'):
        parse_transcript('chapter 12 begins', '', True)
    for empty in ('', '  ', '[x]', '[x] [x]', "[x] ... ' [x]"):
        for free in (False, True):
            with pytest.raises(ValueError, match='nothing is left'):
                parse_transcript(empty, '[x]', free)


def test_parse_transcript_equals_its_restatement():
    from ctc_asr_amd.align_long import parse_transcript
    rng = np.random.default_rng(11)
    tokens = ['[x]', '[x]', 'Hello', "don't", '--', 'a', 'B.', '[x],', "'", 'zz', '\n', '  ', '\t']
    for _ in range(300):
        text = ' '.join(tokens[int(v)] for v in rng.integers(0, len(tokens), size=rng.integers(0, 9)))
        for wildcard, free in (('[x]', False), ('[x]', True), ('', True), ('', False)):
            try:
                want = pref.parse_transcript(text, wildcard, free)
            except ValueError:
                with pytest.raises(ValueError):
                    parse_transcript(text, wildcard, free)
                continue
            assert parse_transcript(text, wildcard, free) == want, (text, wildcard, free)


# ---- 3. skipped and words from a hand-made path ---------------------------------------------------
def test_skipped_and_words_from_a_hand_made_path():
    from ctc_asr_amd import align_long
    text, labels = align_long.parse_transcript('[x] ab c [x] d', '[x]')
    assert labels == [W, 2, 3, 1, 4, W, 5]
    # states: 1 wildcard, 3 a, 5 b, 7 space, 9 c, 11 wildcard, 13 d; even: blanks
    path = np.array([1, 1, 1, 2, 3, 5, 5, 7, 9, 11, 11, 12, 13, 14])
    logp = -np.arange(len(path), dtype=np.float32) / 8
    begin, end = align_long.frame_samples([1000], [len(path) * 160], [len(path)], 160)
    words = align_long.words_on_samples(path, labels, begin, end, logp)
    assert [w['word'] for w in words] == ['ab', 'c', 'd']
    assert [(w['start_sample'], w['end_sample'], w['frames']) for w in words] == \
        [(1000 + 4 * 160, 1000 + 7 * 160, 3), (1000 + 8 * 160, 1000 + 9 * 160, 1),
         (1000 + 12 * 160, 1000 + 13 * 160, 1)]
    assert words[0]['confidence'] == float(np.mean(logp[4:7].astype(np.float64)))
    skipped = align_long.skipped_on_samples(path, labels, begin, end)
    assert skipped == [
        {'after_word': -1, 'start': round(1000 / RATE, 6), 'end': round(1480 / RATE, 6),
         'start_sample': 1000, 'end_sample': 1480, 'frames': 3},
        {'after_word': 1, 'start': round(2440 / RATE, 6), 'end': round(2760 / RATE, 6),
         'start_sample': 2440, 'end_sample': 2760, 'frames': 2}]
    for span in skipped:
        assert json.loads(json.dumps(span)) == span
    summary = align_long.partial_summary(path, labels, logp)
    covered = [t for t in range(len(path)) if t not in (0, 1, 2, 9, 10)]
    total = 0.0
    for t in covered:
        total += float(logp[t])
    assert summary == {'wildcard_frames': 5, 'covered_frames': 9,
                       'score_per_covered_frame': total / 9}
    # a wildcard at the end: after the last word
    labels = [2, W]
    skipped = align_long.skipped_on_samples(np.array([0, 1, 3, 3]), labels, begin[:4], end[:4])
    assert [(s['after_word'], s['frames']) for s in skipped] == [(0, 2)]
    assert align_long.skipped_on_samples(np.full(4, -1), labels, begin[:4], end[:4]) == []
    # a transcript that is covered nowhere has no covered frame
    assert align_long.partial_summary(np.array([1, 1]), [W], logp[:2]) == \
        {'wildcard_frames': 2, 'covered_frames': 0, 'score_per_covered_frame': None}


# ---- 4. cut_utterances with barriers --------------------------------------------------------------
def _word(name, start, end, confidence=-0.5, frames=10):
    return {'word': name, 'start_sample': start, 'end_sample': end, 'confidence': confidence,
            'frames': frames, 'start': start / RATE, 'end': end / RATE}


def _spans(utterances):
    return [(u['first_word'], u['last_word'], u['start_sample'], u['end_sample'], u['status'],
             u['forced']) for u in utterances]


def test_a_barrier_is_a_mandatory_cut_and_the_pad_takes_at_most_half_the_gap():
    from ctc_asr_amd.align_long import cut_utterances
    # max 2 s = 32000, min gap 200 ms = 3200, pad 100 ms = 1600 (the words of
    # tests/test_align_long_host.py::test_plain_cut_at_a_pause)
    words = [_word('a', 10000, 14000), _word('b', 15000, 20000), _word('c', 30000, 36000),
             _word('d', 36500, 40000)]
    plain = [(0, 1, 8400, 21600, 'ok', False), (2, 3, 28400, 41600, 'ok', False)]
    for got in (cut_utterances(words, 100000, 2, 200, 100, None),
                cut_utterances(words, 100000, 2, 200, 100, None, barriers=None)):
        assert _spans(got) == plain and all('beside_wildcard' not in u for u in got)
    # no wildcard anywhere: the same cuts, and the field says so
    got = cut_utterances(words, 100000, 2, 200, 100, None, barriers=[])
    assert _spans(got) == plain and [u['beside_wildcard'] for u in got] == [False, False]
    # wildcards before the first word and after the last: nothing else changes
    got = cut_utterances(words, 100000, 2, 200, 100, None, barriers=[-1, 3])
    assert _spans(got) == plain and [u['beside_wildcard'] for u in got] == [True, True]
    got = cut_utterances(words, 100000, 2, 200, 100, None, barriers=[-1])
    assert _spans(got) == plain and [u['beside_wildcard'] for u in got] == [True, False]
    # a wildcard between a and b, 1000 samples apart (no candidate by its gap):
    # from a: reach stops at a.  8400 .. min(15600, midpoint 14500) = 14500: 6100 samples, short
    # from b: 40000 - 15000 + 3200 <= 32000 -> reach d; candidates after b and d -> d
    #   max(13400, 14500) = 14500 .. 41600
    got = cut_utterances(words, 100000, 2, 200, 100, None, barriers=[0])
    assert _spans(got) == [(0, 0, 8400, 14500, 'short', False), (1, 3, 14500, 41600, 'ok', False)]
    assert [u['beside_wildcard'] for u in got] == [True, True]
    assert [u['label'] for u in got] == ['a', 'b c d']
    # a wildcard between c and d, 500 samples apart: from a, 36000 - 10000 + 3200 <= 32000 ->
    # reach c, where it stops; the largest candidate is the barrier itself: a b c | d, which
    # meet at the midpoint 36250
    got = cut_utterances(words, 100000, 2, 200, 100, None, barriers=[2])
    assert [(u['first_word'], u['last_word']) for u in got] == [(0, 2), (3, 3)]
    assert [u['beside_wildcard'] for u in got] == [True, True]
    assert got[0]['end_sample'] == 36250 and got[1]['start_sample'] == 36250
    assert not any(u['forced'] for u in got)
    # max 1 s = 16000 and the wildcard between a and b: a | b | c d, the last beside none
    #   from b: 36000 - 15000 + 3200 > 16000 -> reach b; from c: 40000 - 30000 + 3200 -> reach d
    got = cut_utterances(words, 100000, 1, 200, 100, None, barriers=[0])
    assert [(u['first_word'], u['last_word']) for u in got] == [(0, 0), (1, 1), (2, 3)]
    assert [u['beside_wildcard'] for u in got] == [True, True, False]


def test_no_utterance_spans_a_barrier_whatever_the_settings():
    from ctc_asr_amd.align_long import cut_utterances
    rng = np.random.default_rng(5)
    edges = np.sort(rng.choice(np.arange(400000), size=120, replace=False))
    words = [_word('w{}'.format(k), int(edges[2 * k]), int(edges[2 * k + 1])) for k in range(60)]
    for max_seconds, gap_ms, pad_ms in ((1, 0, 0), (2, 200, 100), (15, 5000, 1000), (1, 300, 50)):
        for count in (1, 5, 30):
            barriers = sorted(int(v) for v in rng.choice(np.arange(-1, 60), size=count,
                                                         replace=False))
            got = cut_utterances(words, 400000, max_seconds, gap_ms, pad_ms, None,
                                 barriers=barriers)
            assert [k for u in got for k in range(u['first_word'], u['last_word'] + 1)] == \
                list(range(60))
            for before, after in zip(got, got[1:]):
                assert before['end_sample'] <= after['start_sample']
            for u in got:
                a, b = u['first_word'], u['last_word']
                assert not any(a <= k < b for k in barriers), (u, barriers)
                assert u['beside_wildcard'] == (a - 1 in barriers or b in barriers)
                head = words[a]['start_sample'] - u['start_sample']
                tail = u['end_sample'] - words[b]['end_sample']
                pad = pad_ms * RATE // 1000
                assert 0 <= head <= pad and 0 <= tail <= pad
                if a > 0:
                    assert head <= -(-(words[a]['start_sample'] - words[a - 1]['end_sample']) // 2)
                if b < 59:
                    assert tail <= (words[b + 1]['start_sample'] - words[b]['end_sample']) // 2
            cuts = {u['last_word'] for u in got}
            assert {k for k in barriers if k >= 0} <= cuts


def test_write_corpus_copies_beside_wildcard_into_the_report(tmp_path):
    from ctc_asr_amd import align_long
    audio = np.arange(60000, dtype=np.int16)
    words = [_word('a', 1000, 20000), _word('b', 30000, 50000)]
    out, csv_path = tmp_path / 'corpus', tmp_path / 'train.csv'
    utterances = align_long.cut_utterances(words, len(audio), 2, 200, 100, None, barriers=[0])
    align_long.write_corpus(audio, utterances, str(out), str(csv_path), 'r')
    lines = [json.loads(line) for line in open(align_long.report_path(str(csv_path)))]
    assert [line['beside_wildcard'] for line in lines] == [True, True]
    utterances = align_long.cut_utterances(words, len(audio), 2, 200, 100, None)
    align_long.write_corpus(audio, utterances, str(out), str(csv_path), 'r')
    lines = [json.loads(line) for line in open(align_long.report_path(str(csv_path)))]
    assert all('beside_wildcard' not in line for line in lines)


# ---- 5. flags -------------------------------------------------------------------------------------
def test_flags_defaults_and_refusals():
    from ctc_asr_amd.params import FLAGS
    FLAGS.reset()
    try:
        assert FLAGS.transcript_wildcard == '' and FLAGS.align_free_ends is False
        for bad, why in ((['--transcript_wildcard', 'a b'], 'whitespace'),
                         (['--transcript_wildcard', '[x]\t'], 'whitespace'),
                         (['--transcript_wildcard', 'um'], 'word "um"'),
                         (['--transcript_wildcard', '[Noise]'], 'word "noise"'),
                         (['--transcript_wildcard', '<7>'], 'digit')):
            with pytest.raises(ValueError, match=why):
                FLAGS.parse(bad)
        FLAGS.parse(['--transcript_wildcard', '[...]', '--align_free_ends'])
        assert FLAGS.transcript_wildcard == '[...]' and FLAGS.align_free_ends is True
        FLAGS.parse(['--transcript_wildcard', ''])
        assert FLAGS.transcript_wildcard == ''
    finally:
        FLAGS.reset()


def test_the_driver_checks_the_transcript_before_anything_is_loaded(tmp_path):
    from ctc_asr_amd import align_long
    from ctc_asr_amd.params import FLAGS
    wav, text = tmp_path / 'a.wav', tmp_path / 'a.txt'
    wavfile.write(str(wav), RATE, np.zeros(1000, dtype=np.int16))
    base = ['--input', str(wav), '--transcript', str(text), '--align_output',
            str(tmp_path / 'w.jsonl')]
    try:
        text.write_text('[*] -- [*]')
        with pytest.raises(ValueError, match='nothing is left'):
            align_long.main(base + ['--transcript_wildcard', '[*]', '--align_free_ends'])
        FLAGS.reset()
        text.write_text('hi [*] route 66')
        with pytest.raises(ValueError, match='offset 13'):
            align_long.main(base + ['--transcript_wildcard', '[*]'])
        FLAGS.reset()
        with pytest.raises(ValueError, match='offset 13'):
            align_long.main(base + ['--align_free_ends'])
        FLAGS.reset()
        with pytest.raises(ValueError, match='reads as the word'):
            align_long.main(base + ['--transcript_wildcard', 'hi'])
    finally:
        FLAGS.reset()


# ---- 6. the C ABI: arguments are checked before the device is touched ------------------------------
@pytest.fixture(scope='module')
def lib():
    from ctc_asr_amd import build, hip as module
    build.build(verbose=False)
    return module.load()


def _call(lib, num_steps=10, classes=29, blank=28, num_labels=3, tile_frames=0, nulls=(),
          workspace_bytes=None):
    buffers = [ctypes.create_string_buffer(4096) for _ in range(8)]
    names = ('logits', 'labels', 'path', 'score', 'frame_logp', 'logp', 'status', 'workspace')
    p = {name: None if name in nulls else ctypes.addressof(buf)
         for name, buf in zip(names, buffers)}
    if workspace_bytes is None:
        workspace_bytes = lib.ctcasr_ctc_align_long_workspace_bytes(num_steps, classes,
                                                                    num_labels, tile_frames)
    return lib.ctcasr_ctc_align_partial(p['logits'], p['labels'], num_steps, classes, blank,
                                        num_labels, tile_frames, p['path'], p['score'],
                                        p['frame_logp'], p['logp'], p['status'], p['workspace'],
                                        workspace_bytes, None)


def test_bad_arguments_are_refused_before_the_device_is_touched(lib):
    bad, unsupported, short = -1, -2, -3
    for name in ('logits', 'labels', 'path', 'score', 'status'):
        assert _call(lib, nulls=(name,)) == bad, name
    assert _call(lib, num_steps=-1) == bad
    assert _call(lib, num_labels=-1) == bad
    assert _call(lib, classes=1, blank=0) == bad
    assert _call(lib, blank=29) == bad and _call(lib, blank=-1) == bad
    assert _call(lib, tile_frames=-1) == bad
    assert _call(lib, classes=65, blank=64) == unsupported       # 64 REAL classes is the limit
    assert _call(lib, num_steps=(1 << 22) + 1, workspace_bytes=1 << 40) == unsupported
    assert _call(lib, num_steps=1 << 21, num_labels=(1 << 20) + 1,
                 workspace_bytes=1 << 40) == unsupported
    assert _call(lib, num_steps=1 << 22, tile_frames=1, workspace_bytes=1 << 40) == unsupported
    need = lib.ctcasr_ctc_align_long_workspace_bytes(10, 29, 3, 0)
    assert need > 0
    assert _call(lib, workspace_bytes=need - 1) == short
    assert _call(lib, nulls=('workspace',)) == short
    assert _call(lib, nulls=('frame_logp', 'logp'), workspace_bytes=need - 1) == short
    assert _call(lib, classes=64, blank=63, workspace_bytes=0) == short   # (served: not -2)


def test_the_wrapper_raises_what_ctc_align_long_raises(lib):
    import torch
    from ctc_asr_amd import hip
    from ctc_asr_amd.model import CTCModel
    assert hip.ALIGN_WILDCARD == -1 and hasattr(CTCModel, 'align_partial_fn')
    logits = torch.zeros(5000, 29)
    labels = torch.full((2000,), hip.ALIGN_WILDCARD, dtype=torch.int32)
    need = hip.ctc_align_long_workspace_bytes(5000, 29, 2000)
    with pytest.raises(ValueError, match='ctc_align_partial.*{}.*{}'.format(need, 1 << 20)):
        hip.ctc_align_partial(logits, labels, max_workspace_bytes=1 << 20)
    with pytest.raises(hip.CtcAsrError, match='ctc_align_partial.*C = 65'):
        hip.ctc_align_partial(torch.zeros(10, 65), labels[:3])
    with pytest.raises(hip.CtcAsrError, match=r'\[T, C\]'):
        hip.ctc_align_partial(torch.zeros(10, 2, 29), labels[:3])
    with pytest.raises(hip.CtcAsrError):                 # enough room allowed: no CPU path
        hip.ctc_align_partial(logits[:10], labels[:3])
