"""The host half of `ctc_asr_amd.align_long`: transcript normalisation, the cut rules on
hand-made word tables (every expected number is worked out in the comments, at 16 kHz: 100 ms =
1600 samples), the new flags' refusals and the corpus writer.  No GPU."""

import json

import numpy as np
import pytest
from scipy.io import wavfile

from ctc_asr_amd import align_long
from ctc_asr_amd.align_long import cut_utterances, normalize_transcript

RATE = 16000


def _word(name, start, end, confidence=-0.5, frames=10):
    return {'word': name, 'start_sample': start, 'end_sample': end, 'confidence': confidence,
            'frames': frames, 'start': start / RATE, 'end': end / RATE}


def _spans(utterances):
    return [(u['first_word'], u['last_word'], u['start_sample'], u['end_sample'], u['status'],
             u['forced']) for u in utterances]


# ---- normalize_transcript ------------------------------------------------------------------------
def test_normalize_transcript():
    assert normalize_transcript('Hello, World') == 'hello world'
    assert normalize_transcript("Don't  stop") == 'dont stop'
    assert normalize_transcript('it’s the dog’s') == 'its the dogs'
    assert normalize_transcript('  a -- b\n\tc.  ') == 'a b c'
    assert normalize_transcript('naïve café—“quoted”') == 'na ve caf quoted'
    assert normalize_transcript('ABC xyz') == 'abc xyz'
    with pytest.raises(ValueError, match='offset 8'):
        normalize_transcript('chapter 12 begins')
    with pytest.raises(ValueError, match='"7" at offset 0'):
        normalize_transcript('7 dwarfs')
    for empty in ('', '   ', "'’", '... !?'):
        with pytest.raises(ValueError, match='nothing is left'):
            normalize_transcript(empty)
    from ctc_asr_amd.labels import encode
    assert encode(normalize_transcript("A b'C")) == [2, 1, 3, 4]


# ---- cut_utterances ------------------------------------------------------------------------------
def test_plain_cut_at_a_pause():
    # max 2 s = 32000, min gap 200 ms = 3200, pad 100 ms = 1600
    words = [_word('a', 10000, 14000), _word('b', 15000, 20000),      # gap 1000: no candidate
             _word('c', 30000, 36000),                                # gap 10000: candidate after b
             _word('d', 36500, 40000)]                                # gap 500; last: candidate
    got = cut_utterances(words, 100000, 2, 200, 100, None)
    # from a: end <= 10000 + 32000 - 3200 = 38800 -> reach c; largest candidate <= c is b
    # from c: reach d (the last word)
    # a-b: 10000 - 1600 = 8400 .. min(20000 + 1600, midpoint 25000) = 21600
    # c-d: max(30000 - 1600, 25000) = 28400 .. 40000 + 1600 = 41600
    assert _spans(got) == [(0, 1, 8400, 21600, 'ok', False), (2, 3, 28400, 41600, 'ok', False)]
    assert [u['label'] for u in got] == ['a b', 'c d']
    assert [u['index'] for u in got] == [0, 1]
    assert cut_utterances([], 100000, 2, 200, 100, None) == []


def test_no_candidate_in_reach_forces_the_cut_at_the_largest_gap():
    # max 1 s = 16000, pad 0, min gap 3200: no gap below is a candidate but the last word's
    words = [_word('a', 0, 4000), _word('b', 5000, 9000), _word('c', 11000, 14000),
             _word('d', 15000, 19000), _word('e', 20000, 23000)]      # gaps 1000 2000 1000 1000
    got = cut_utterances(words, 50000, 1, 200, 0, None)
    # from a: end <= 16000 -> reach c; gaps behind a, b, c: 1000, 2000, 1000 -> after b, forced
    #   0 .. 9000 (pad 0): 9000 samples < 0.7 s = 11200 -> short
    # from c: end <= 27000 -> reach e, the last word: a candidate, not forced
    #   max(11000, midpoint 10000) = 11000 .. 23000: 12000 samples
    assert _spans(got) == [(0, 1, 0, 9000, 'short', True), (2, 4, 11000, 23000, 'ok', False)]


def test_forced_cut_takes_the_later_of_equal_gaps():
    words = [_word('a', 0, 4000), _word('b', 5000, 9000), _word('c', 10000, 14000),
             _word('d', 15000, 19000), _word('e', 20000, 23000)]      # every gap 1000
    got = cut_utterances(words, 50000, 1, 200, 0, None)
    # from a: reach c (14000 <= 16000 < 19000); a tie of three: the latest, after c
    # from d: reach e; 15000 .. 23000 = 8000 samples -> short
    assert _spans(got) == [(0, 2, 0, 14000, 'ok', True), (3, 4, 15000, 23000, 'short', False)]


def test_a_word_longer_than_the_cap_stands_alone_and_spans_clip_to_the_recording():
    # max 1 s = 16000, pad 1600: 'long' needs 19000 + 3200 > 16000
    words = [_word('long', 1000, 20000), _word('next', 30000, 42000)]   # 12000 + 3200 fits
    got = cut_utterances(words, 43000, 1, 200, 100, None)
    # long: 1000 - 1600 < 0 -> 0 .. min(21600, midpoint 25000) = 21600
    # next: max(28400, 25000) = 28400 .. 43600 -> the recording ends at 43000
    assert _spans(got) == [(0, 0, 0, 21600, 'too_long', False), (1, 1, 28400, 43000, 'ok', False)]
    # a word that fits, then one that does not, no pause between: a forced cut, then too_long
    words = [_word('a', 0, 12000), _word('long', 12500, 40000), _word('b', 40100, 52000)]
    got = cut_utterances(words, 60000, 1, 200, 0, None)
    # a: 0 .. min(12000, midpoint 12250); long: max(12500, 12250) .. min(40000, 40050); b alike
    assert _spans(got) == [(0, 0, 0, 12000, 'ok', True), (1, 1, 12500, 40000, 'too_long', False),
                           (2, 2, 40100, 52000, 'ok', False)]


def test_neighbours_meet_at_the_midpoint_when_the_gap_is_below_two_pads():
    # max 2 s = 32000, min gap 100 ms = 1600, pad 1600: the gap 2001 is a candidate, < 3200
    words = [_word('a', 5000, 20000), _word('b', 22001, 40000)]
    got = cut_utterances(words, 100000, 2, 100, 100, None)
    # from a: 40000 - 5000 + 3200 > 32000 -> reach a.  Midpoint 20000 + 2001 // 2 = 21000
    assert _spans(got) == [(0, 0, 3400, 21000, 'ok', False), (1, 1, 21000, 41600, 'ok', False)]


def test_short_and_low_confidence_statuses():
    # max 1 s = 16000, min gap 3200, pad 0: a b | c d | e, each cut at a pause of 8000 or more
    words = [_word('a', 0, 6000, -0.5, 10), _word('b', 6100, 12000, -2.0, 30),
             _word('c', 20000, 26000, -0.5, 30), _word('d', 26100, 32000, -1.2, 10),
             _word('e', 40000, 45000, -9.0, 10)]
    # a b: (-0.5 * 10 - 2.0 * 30) / 40 = -1.625; c d: (-15 - 12) / 40 = -0.675; e: 5000 samples
    got = cut_utterances(words, 50000, 1, 200, 0, -1.0)
    assert [u['status'] for u in got] == ['low_confidence', 'ok', 'short']
    assert [u['confidence'] for u in got] == [-1.625, -0.675, -9.0]
    got = cut_utterances(words, 50000, 1, 200, 0, None)
    assert [u['status'] for u in got] == ['ok', 'ok', 'short']
    got = cut_utterances(words, 50000, 1, 200, 0, -1.625)            # (below, not at)
    assert [u['status'] for u in got] == ['ok', 'ok', 'short']
    # exactly 0.7 s = 11200 samples is not short
    got = cut_utterances([_word('x', 100, 11300)], 50000, 2, 200, 0, None)
    assert _spans(got) == [(0, 0, 100, 11300, 'ok', False)]
    got = cut_utterances([_word('x', 100, 11299)], 50000, 2, 200, 0, None)
    assert got[0]['status'] == 'short'


def test_the_last_word_always_ends_an_utterance():
    words = [_word('only', 2000, 18000)]
    got = cut_utterances(words, 18500, 15, 200, 100, None)
    assert _spans(got) == [(0, 0, 400, 18500, 'ok', False)]          # 19600 clipped to 18500
    # every word exactly once, in order, whatever the settings
    rng = np.random.default_rng(5)
    edges = np.sort(rng.choice(np.arange(400000), size=120, replace=False))
    words = [_word('w{}'.format(k), int(edges[2 * k]), int(edges[2 * k + 1])) for k in range(60)]
    for max_seconds, gap_ms, pad_ms in ((1, 0, 0), (2, 200, 100), (15, 5000, 1000), (1, 300, 50)):
        got = cut_utterances(words, 400000, max_seconds, gap_ms, pad_ms, None)
        assert [k for u in got for k in range(u['first_word'], u['last_word'] + 1)] == \
            list(range(60))
        assert ' '.join(u['label'] for u in got) == ' '.join(w['word'] for w in words)
        for before, after in zip(got, got[1:]):
            assert before['end_sample'] <= after['start_sample']
        for u in got:
            assert 0 <= u['start_sample'] <= words[u['first_word']]['start_sample']
            assert words[u['last_word']]['end_sample'] <= u['end_sample'] <= 400000
            if u['status'] != 'too_long':
                assert u['end_sample'] - u['start_sample'] <= max_seconds * RATE


# ---- flags ----------------------------------------------------------------------------------------
def test_flags_defaults_and_refusals():
    from ctc_asr_amd.params import FLAGS, parse_cut_min_confidence
    FLAGS.reset()
    try:
        assert (FLAGS.transcript, FLAGS.corpus_out_dir, FLAGS.corpus_out_csv) == ('', '', '')
        assert (FLAGS.cut_max_seconds, FLAGS.cut_min_gap_ms, FLAGS.cut_pad_ms) == (15, 200, 100)
        assert FLAGS.cut_min_confidence == '' and parse_cut_min_confidence('') is None
        for bad in (['--cut_max_seconds', '0'], ['--cut_max_seconds', '18'],
                    ['--cut_min_gap_ms', '-1'], ['--cut_min_gap_ms', '5001'],
                    ['--cut_pad_ms', '-1'], ['--cut_pad_ms', '1001'],
                    ['--cut_min_confidence', 'low'], ['--cut_min_confidence', 'nan'],
                    ['--cut_min_confidence', '-inf']):
            with pytest.raises(ValueError, match=bad[0][2:]):
                FLAGS.parse(bad)
        FLAGS.parse(['--cut_max_seconds', '17', '--cut_min_gap_ms', '0', '--cut_pad_ms', '1000',
                     '--cut_min_confidence', '-1.5', '--transcript', 'a.txt'])
        assert (FLAGS.cut_max_seconds, FLAGS.cut_min_gap_ms, FLAGS.cut_pad_ms) == (17, 0, 1000)
        assert parse_cut_min_confidence(FLAGS.cut_min_confidence) == -1.5
        assert FLAGS.transcript == 'a.txt'
    finally:
        FLAGS.reset()


def test_the_driver_refuses_nbest_and_half_a_corpus_request(tmp_path):
    from ctc_asr_amd.params import FLAGS
    wav, text = tmp_path / 'a.wav', tmp_path / 'a.txt'
    wavfile.write(str(wav), RATE, np.zeros(1000, dtype=np.int16))
    text.write_text('hello')
    base = ['--input', str(wav), '--transcript', str(text)]
    try:
        with pytest.raises(ValueError, match='nbest'):
            align_long.main(base + ['--align_output', str(tmp_path / 'w.jsonl'), '--nbest', '2',
                                    '--beam_width', '8'])
        FLAGS.reset()
        with pytest.raises(ValueError, match='go together'):
            align_long.main(base + ['--corpus_out_dir', str(tmp_path / 'out')])
        FLAGS.reset()
        with pytest.raises(ValueError, match='needs --align_output'):
            align_long.main(base)
        FLAGS.reset()
        with pytest.raises(ValueError, match='transcript'):
            align_long.main(['--input', str(wav), '--transcript', str(tmp_path / 'none.txt'),
                             '--align_output', str(tmp_path / 'w.jsonl')])
        FLAGS.reset()
        text.write_text('route 66')
        with pytest.raises(ValueError, match='offset 6'):
            align_long.main(base + ['--align_output', str(tmp_path / 'w.jsonl')])
    finally:
        FLAGS.reset()


# ---- write_corpus ---------------------------------------------------------------------------------
def test_write_corpus_order_format_doubled_last_row_and_exact_slices(tmp_path):
    from ctc_asr_amd.csv_helper import read_csv_rows
    rng = np.random.default_rng(9)
    audio = rng.integers(-32768, 32768, size=200000).astype(np.int16)

    def utt(index, low, high, status, label, forced=False):
        return {'index': index, 'first_word': index, 'last_word': index, 'start_sample': low,
                'end_sample': high, 'label': label, 'status': status, 'forced': forced,
                'confidence': -0.25 * index}
    utterances = [utt(0, 0, 30001, 'ok', 'long one'),            # 1.8751 s (30001 / 16000)
                  utt(1, 30001, 35000, 'short', 'tiny'),
                  utt(2, 40000, 60000, 'ok', 'tie first'),       # 1.2500 s
                  utt(3, 60000, 100000, 'too_long', 'never'),
                  utt(4, 100000, 120000, 'ok', 'tie second', True),   # 1.2500 s: after index 2
                  utt(5, 120000, 140000, 'low_confidence', 'mumble'),
                  utt(6, 150000, 161200, 'ok', 'shortest')]      # 0.7000 s
    out, csv_path = tmp_path / 'corpus', tmp_path / 'lists' / 'train.csv'
    rows = align_long.write_corpus(audio, utterances, str(out), str(csv_path), 'chapter')
    want = [('chapter_00006.wav', 'shortest', '0.7000'), ('chapter_00002.wav', 'tie first', '1.2500'),
            ('chapter_00004.wav', 'tie second', '1.2500'), ('chapter_00000.wav', 'long one', '1.8751')]
    assert rows == want + [want[-1]]
    assert csv_path.read_text().splitlines() == ['path;label;length'] + \
        [';'.join(row) for row in want + [want[-1]]]
    read = read_csv_rows(str(csv_path))
    assert [(r['path'], r['label'], r['length']) for r in read[1:]] == want + [want[-1]]
    assert sorted(p.name for p in out.iterdir()) == sorted(row[0] for row in want)
    for u in utterances:
        if u['status'] == 'ok':
            rate, samples = wavfile.read(str(out / 'chapter_{:05d}.wav'.format(u['index'])))
            assert rate == RATE and samples.dtype == np.int16
            assert samples.tobytes() == audio[u['start_sample']:u['end_sample']].tobytes()
    report = [json.loads(line) for line in
              open(align_long.report_path(str(csv_path)), encoding='utf-8')]
    assert align_long.report_path(str(csv_path)) == str(tmp_path / 'lists' / 'train.report.jsonl')
    assert [r['index'] for r in report] == list(range(7))
    assert [r['status'] for r in report] == [u['status'] for u in utterances]
    assert [r['forced'] for r in report] == [False] * 4 + [True, False, False]
    assert [(r['start_sample'], r['end_sample']) for r in report] == \
        [(u['start_sample'], u['end_sample']) for u in utterances]
    assert [r['path'] for r in report] == ['chapter_00000.wav', None, 'chapter_00002.wav', None,
                                           'chapter_00004.wav', None, 'chapter_00006.wav']
    assert report[4]['confidence'] == -1.0 and report[0]['end'] == round(30001 / RATE, 6)
    # no ok utterance: a header and nothing else
    rows = align_long.write_corpus(audio, utterances[1:2], str(out), str(csv_path), 'chapter')
    assert rows == [] and csv_path.read_text() == 'path;label;length\n'
    with pytest.raises(ValueError, match='int16'):
        align_long.write_corpus(audio.astype(np.int32), utterances, str(out), str(csv_path), 'c')


def test_words_on_samples_restates_alignment_segments():
    """On a single piece that starts at sample 0 with a hop of 160 samples, the words are those of
    `alignment.segments` with 0.01 s frames; a second piece shifts and clips."""
    from ctc_asr_amd import alignment
    labels = [3, 4, 1, 5, 1, 1, 6, 6]                  # 'bc d  ee'
    path = np.array([0, 1, 1, 2, 3, 4, 5, 6, 7, 7, 8, 9, 10, 11, 12, 13, 14, 15, 15, 16])
    logp = -np.arange(len(path), dtype=np.float32) / 8
    begin, end = align_long.frame_samples([0], [len(path) * 160], [len(path)], 160)
    got = align_long.words_on_samples(path, labels, begin, end, logp)
    want = alignment.segments(path, labels, 0.01, logp)
    assert [{k: w[k] for k in ('word', 'start', 'end', 'confidence')} for w in got] == want
    assert [w['word'] for w in got] == ['bc', 'd', 'ee']
    assert [(w['start_sample'], w['end_sample'], w['frames']) for w in got] == \
        [(160, 800, 3), (1280, 1600, 2), (2400, 3040, 3)]
    # two pieces of 10 frames: from sample 1000 (1600 samples: frame 9 ends with the piece), and
    # from 5000 (1500 samples: frame 9 begins at 6440 and would end at 6600: clipped to 6500)
    begin, end = align_long.frame_samples([1000, 5000], [1600, 1500], [10, 10], 160)
    assert begin.tolist() == [1000 + 160 * g for g in range(10)] + [5000 + 160 * g for g in range(10)]
    assert end.tolist()[:10] == [1160 + 160 * g for g in range(10)]
    assert end.tolist()[10:] == [5160 + 160 * g for g in range(9)] + [6500]
    got = align_long.words_on_samples(path, labels, begin, end, logp)
    # 'd' sits on frames 8..9 of piece 0; 'ee' on concatenated frames 15..18: piece 1, 5..8
    assert (got[1]['start_sample'], got[1]['end_sample']) == (1000 + 8 * 160, 1000 + 10 * 160)
    assert (got[2]['start_sample'], got[2]['end_sample']) == (5000 + 5 * 160, 5000 + 9 * 160)
    # a word across the two pieces: 'bc' when the first piece keeps 3 frames only
    begin, end = align_long.frame_samples([1000, 5000], [480, 2720], [3, 17], 160)
    got = align_long.words_on_samples(path, labels, begin, end, logp)
    assert (got[0]['start_sample'], got[0]['end_sample']) == (1000 + 160, 5000 + 2 * 160)
    assert align_long.words_on_samples(np.full(5, -1), labels, begin, end, logp) == []
