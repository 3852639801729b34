"""What of the segmentation of long recordings can be checked without a GPU: the vectorised rules
of ctc_asr_amd/vad.py against the slow restatement (tests/vad_reference.py), the properties every
table has, the flags, the argument checks of the C ABI, and the assembly of the result of
`transcribe` from fabricated per-piece results.  Every comparison is exact."""

import json

import numpy as np
import pytest

from tests import vad_reference as ref

BAD_FLAGS = [
    '--vad_margin_db=-1', '--vad_margin_db=61', '--vad_margin_db=9.5',
    '--vad_floor_permille=0', '--vad_floor_permille=1000',
    '--vad_min_rms=-1', '--vad_min_rms=32768',
    '--vad_rms=-1', '--vad_rms=32768', '--vad_rms=loud',
    '--vad_pad_ms=-10', '--vad_pad_ms=2001',
    '--vad_min_speech_ms=9', '--vad_min_speech_ms=2001',
    '--max_segment_seconds=0', '--max_segment_seconds=31', '--max_segment_seconds=1.5',
]


@pytest.fixture()
def flags():
    from ctc_asr_amd.params import FLAGS
    FLAGS.reset()
    yield FLAGS
    FLAGS.reset()


@pytest.mark.parametrize('bad', BAD_FLAGS)
def test_bad_flag_values_are_refused_when_parsed(flags, bad):
    with pytest.raises(ValueError):
        flags.parse([bad])


def test_flags_and_settings(flags):
    from ctc_asr_amd import vad
    assert (flags.vad_margin_db, flags.vad_floor_permille, flags.vad_min_rms, flags.vad_rms,
            flags.vad_pad_ms, flags.vad_min_speech_ms, flags.max_segment_seconds,
            flags.transcribe_output) == (9, 100, 16, 0, 200, 50, 15, '')
    s = vad.VadSettings.from_flags(flags)
    assert (s.margin_db, s.floor_permille, s.min_rms, s.rms, s.pad, s.min_raw, s.max_segment) == \
        (9, 100, 16, 0, 20, 5, 1500)
    # both ends of every range parse; milliseconds are whole hops, rounded down
    assert flags.parse(['--vad_margin_db=0', '--vad_floor_permille=1', '--vad_min_rms=0',
                        '--vad_rms=32767', '--vad_pad_ms=0', '--vad_min_speech_ms=10',
                        '--max_segment_seconds=1', '--transcribe_output=x.jsonl']) == []
    assert flags.parse(['--vad_margin_db=60', '--vad_floor_permille=999', '--vad_min_rms=32767',
                        '--vad_rms=0', '--vad_pad_ms=2000', '--vad_min_speech_ms=2000',
                        '--max_segment_seconds=30']) == []
    flags.parse(['--vad_pad_ms=199', '--vad_min_speech_ms=59'])
    s = vad.VadSettings.from_flags(flags)
    assert (s.pad, s.min_raw, s.max_segment) == (19, 5, 3000)
    with pytest.raises(ValueError):
        flags.update(max_segment_seconds=31)         # assignments are checked like the parser's
    with pytest.raises(ValueError):
        vad.VadSettings(max_segment=5)         # (M // 2 would be a piece of 2 hops)


def test_constants_agree(flags):
    from ctc_asr_amd import hip, vad
    header = open(__file__.replace('tests/test_vad_host.py', 'include/ctcasr.h')).read()
    for name, value in (('HOP', ref.HOP), ('LEVELS', ref.LEVELS), ('CHUNK', ref.CHUNK)):
        assert '#define CTCASR_VAD_{} {}\n'.format(name, value) in header
        assert getattr(hip, 'VAD_' + name) == value
    assert ref.CHUNK % ref.HOP == 0
    assert (vad.HOP, vad.LEVELS) == (ref.HOP, ref.LEVELS)


def test_level_round_trip_and_monotone():
    from ctc_asr_amd import vad
    top = ref.HOP << 30                                   # the largest energy of a hop
    assert ref.level(top) == 145 and ref.level(0) == 0 and ref.level_floor(0) == 0
    for lvl in range(1, 148):
        assert ref.level(ref.level_floor(lvl)) == lvl
        assert ref.level(ref.level_floor(lvl) - 1) == lvl - 1
        assert ref.level_floor(lvl + 1) * 4 <= ref.level_floor(lvl) * 5 or lvl < 4
    assert vad.level_floor(np.arange(160)).tolist() == [ref.level_floor(v) for v in range(160)]
    rng = np.random.default_rng(3)
    values = np.concatenate([np.arange(70), rng.integers(0, 1 << 38, size=4000),
                             1 << np.arange(1, 38), (1 << np.arange(1, 38)) - 1,
                             [top, top - 1]]).astype(np.int64)
    got = vad.level(values)
    assert got.dtype == np.int64 and got.tolist() == [ref.level(v) for v in values]
    order = np.argsort(values, kind='stable')
    assert (np.diff(got[order]) >= 0).all() and got.max() < ref.LEVELS


# ------------------------------------------------------------------------------------------
def _settings(**kwargs):
    base = dict(margin_db=9, floor_permille=100, min_rms=16, rms=0, pad=20, min_raw=5,
                max_segment=1500)
    base.update(kwargs)
    return base


def _check_table(energies, n, **kwargs):
    """`vad.segment_table` against the reference, and what holds for every table; returns the
    pieces in hops."""
    from ctc_asr_amd import vad
    settings = _settings(**kwargs)
    energies = np.asarray(energies, dtype=np.int64)
    assert len(energies) == -(-n // ref.HOP)
    hist = ref.histogram(energies)
    want_start, want_len, want_thr = ref.table(energies, hist, n, **settings)
    start, length, thr = vad.segment_table(energies, hist, n, vad.VadSettings(**settings))
    assert thr == want_thr
    assert start.dtype == np.int64 and length.dtype == np.int32
    assert start.tolist() == want_start.tolist() and length.tolist() == want_len.tolist()
    found, _, raw, kept = ref.pieces(energies, hist, **settings)
    covered = np.zeros(len(energies), dtype=bool)
    stop = start + length
    assert (start % ref.HOP == 0).all()
    assert (start[1:] >= stop[:-1]).all() and (np.diff(start) > 0).all()     # ascending, disjoint
    for (a, b), s, e in zip(found, start.tolist(), stop.tolist()):
        assert 3 <= b - a <= settings['max_segment']
        assert s == ref.HOP * a and e == min(ref.HOP * b, n) and e <= n
        covered[a:b] = True
    for a, b in kept:                       # every raw hop of a kept region lies in some piece
        assert covered[a:b].all() or not any(raw[a:b])
        assert all(covered[f] for f in range(a, b) if raw[f])
    if len(found) and found[-1][1] == len(energies):
        assert stop[-1] == n                                   # the last piece is cut to n
    return found


def _bursts(frames, spans, loud=3000, quiet=30, seed=0):
    """Energies of a noise floor with loud spans [(a, b)] in hops."""
    rng = np.random.default_rng(seed)
    rms = np.full(frames, quiet, dtype=np.int64)
    for a, b in spans:
        rms[a:b] = loud
    jitter = rng.integers(90, 111, size=frames)
    return ref.HOP * rms * rms * jitter // 100


def test_thresholds_against_the_reference():
    from ctc_asr_amd import vad
    rng = np.random.default_rng(11)
    for trial in range(40):
        frames = int(rng.integers(1, 400))
        energies = rng.integers(0, 1 << int(rng.integers(1, 38)), size=frames)
        hist = ref.histogram(energies)
        for margin, permille, min_rms, rms in ((9, 100, 16, 0), (0, 1, 0, 0), (60, 999, 0, 0),
                                               (25, 500, 3000, 0), (9, 100, 16, 77)):
            want = ref.threshold(hist, margin, permille, min_rms, rms)
            got = vad.threshold(hist, vad.VadSettings(margin, permille, min_rms, rms))
            assert got == want and got >= 1
    assert vad.threshold(ref.histogram([0] * 9), vad.VadSettings(min_rms=0)) == 16
    assert vad.threshold(ref.histogram([0] * 9), vad.VadSettings(min_rms=0, margin_db=0)) == 1
    assert vad.threshold(None, vad.VadSettings(rms=100)) == 160 * 100 * 100


def test_random_energies():
    rng = np.random.default_rng(5)
    for trial in range(30):
        frames = int(rng.integers(1, 700))
        n = ref.HOP * frames - int(rng.integers(0, ref.HOP))
        loud = rng.random(frames) < rng.choice([0.02, 0.2, 0.6])
        energies = np.where(loud, rng.integers(1 << 24, 1 << 34, size=frames),
                            rng.integers(0, 1 << 18, size=frames))
        _check_table(energies, n, pad=int(rng.integers(0, 12)), min_raw=int(rng.integers(1, 6)),
                     max_segment=int(rng.integers(6, 60)),
                     margin_db=int(rng.integers(0, 30)),
                     floor_permille=int(rng.integers(1, 1000)))


def test_dilation_against_the_reference():
    from ctc_asr_amd import vad
    rng = np.random.default_rng(8)
    for frames in (1, 2, 5, 64, 300):
        for pad in (0, 1, 3, 20, 400):
            raw = rng.random(frames) < 0.1
            want = ref.mark(raw.astype(np.int64), 1, pad)[1]
            assert vad.dilate(raw, pad).tolist() == want


def test_all_zero_and_single_frame():
    assert _check_table(np.zeros(500, dtype=np.int64), 80000) == []
    assert _check_table([0], 1) == []
    assert _check_table([ref.HOP << 30], 160, pad=0, min_raw=1) == []      # shorter than 3 hops
    assert _check_table([ref.HOP << 30] * 2, 161, pad=5, min_raw=1, rms=10) == []
    assert _check_table([ref.HOP << 30] * 3, 321, pad=5, min_raw=1, rms=10) == [(0, 3)]


@pytest.mark.parametrize('run, count', [(100, 1), (101, 2), (201, 3)])
def test_regions_of_exactly_m_and_just_above(run, count):
    m = 100
    # padded by 10 hops on both sides: the region is the burst plus 20
    energies = _bursts(400, [(50, 50 + run - 20)], seed=run)
    found = _check_table(energies, 64000, pad=10, max_segment=m)
    assert found[0][0] == 40 and found[-1][1] == 40 + run and len(found) == count
    assert all(b - a >= m // 2 for a, b in found[:-1])
    # ... and a loud run of the same lengths without an edge to cut at
    # (all of it loud: only a fixed threshold finds speech there)
    found = _check_table(_bursts(run, [(0, run)], seed=run), run * ref.HOP, pad=10, max_segment=m,
                         rms=100)
    assert found[0][0] == 0 and found[-1][1] == run and len(found) == count


def test_equal_energies_cut_at_the_lowest_frame():
    from ctc_asr_amd import vad
    energies = np.full(1000, 5_000_000, dtype=np.int64)
    found = _check_table(energies, 160000, rms=10, pad=0, min_raw=1, max_segment=100)
    # every cut falls on the first hop of its window: a + M // 2
    assert found[:3] == [(0, 50), (50, 100), (100, 150)] and found[-1][1] == 1000
    assert all(3 <= b - a <= 100 for a, b in found)
    assert vad.split(energies, 0, 103, 100) == ref.split(energies, 0, 103, 100) == \
        [(0, 50), (50, 103)]
    assert vad.split(energies, 7, 108, 100) == [(7, 57), (57, 108)]
    # one hop quieter than the rest draws the cut, the lower of two equal ones wins
    energies[70] = energies[80] = 10_000_000 - 5_000_001
    assert vad.split(energies, 0, 101, 100) == ref.split(energies, 0, 101, 100) == \
        [(0, 70), (70, 101)]


def test_pad_zero_and_clicks():
    energies = _bursts(300, [(10, 12), (40, 43), (100, 160), (200, 204)])
    found = _check_table(energies, 48000, pad=0, min_raw=3)
    assert found == [(40, 43), (100, 160), (200, 204)]           # 2 raw hops: a click, dropped
    found = _check_table(energies, 48000, pad=0, min_raw=1)
    assert found == [(40, 43), (100, 160), (200, 204)]           # ... or shorter than 3 hops
    found = _check_table(energies, 48000, pad=15, min_raw=5)
    assert found == [(0, 58), (85, 175)]       # two clicks within 2 pad make a piece; 4 raw: none
    found = _check_table(energies, 48000, pad=20, min_raw=1)
    assert found == [(0, 63), (80, 224)]       # gaps of up to 2 pad are closed, longer ones stay


def test_speech_touching_both_ends():
    energies = _bursts(250, [(0, 30), (200, 250)])
    n = 250 * ref.HOP - 59
    found = _check_table(energies, n, pad=20)
    assert found == [(0, 50), (180, 250)]
    found = _check_table(_bursts(250, [(0, 250)]), n, pad=20, max_segment=120, rms=100)
    assert found[0][0] == 0 and found[-1][1] == 250 and len(found) >= 3


def test_two_minutes_like_the_issue():
    """A floor of rms 30 with bursts of rms 3000: every burst found and padded by 0.2 s, the
    long ones cut, every piece within the cap."""
    spans = [(300, 330), (600, 2600), (2700, 2900), (3100, 4800), (5000, 5050), (5300, 7100),
             (7200, 7800), (8000, 9000)]
    energies = _bursts(12000, spans, seed=4)
    found = _check_table(energies, 12000 * ref.HOP)
    assert found[0] == (280, 350)
    joined = []
    for a, b in found:
        if joined and joined[-1][1] == a:
            joined[-1] = (joined[-1][0], b)
        else:
            joined.append((a, b))
    # (2600..2700 is a gap of 100 hops: above 2 pad, it stays open)
    assert joined == [(a - 20, b + 20) for a, b in spans]
    assert len(found) == len(spans) + 3


# ------------------------------------------------------------------------------------------
def test_argument_errors_of_the_c_abi():
    import ctypes
    from ctc_asr_amd import build, hip
    build.build(verbose=False)
    lib = hip.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    assert lib.ctcasr_vad_energy(None, 160, p, p, None) == -1
    assert lib.ctcasr_vad_energy(p, 160, None, p, None) == -1
    assert lib.ctcasr_vad_energy(p, 160, p, None, None) == -1
    assert lib.ctcasr_vad_energy(p, 0, p, p, None) == -1
    assert lib.ctcasr_vad_energy(p, -5, p, p, None) == -1
    unsupported = lib.ctcasr_vad_energy(p, 1 << 31, p, p, None)
    assert unsupported == -2
    for hole in range(5):
        args = [p, 100, p, p, 2, 16, p, p, None]
        args[(0, 2, 3, 6, 7)[hole]] = None
        assert lib.ctcasr_gather_segments(*args) == -1
    assert lib.ctcasr_gather_segments(p, 100, p, p, 0, 16, p, p, None) == -1
    assert lib.ctcasr_gather_segments(p, 100, p, p, 2, 0, p, p, None) == -1
    assert lib.ctcasr_gather_segments(p, 100, p, p, 2, (1 << 30) + 1, p, p, None) == unsupported


def test_wrappers_refuse_what_is_no_recording():
    import torch
    from ctc_asr_amd import hip
    with pytest.raises(hip.CtcAsrError, match='HBM'):
        hip.vad_energy(torch.zeros(400, dtype=torch.int16))
    with pytest.raises(hip.CtcAsrError, match='one recording'):
        hip.vad_energy(torch.zeros((2, 400), dtype=torch.int16))
    with pytest.raises(hip.CtcAsrError, match='empty'):
        hip.vad_energy(torch.zeros(0, dtype=torch.int16))
    with pytest.raises(hip.CtcAsrError, match='1 entries for a batch of 2'):
        hip.gather_segments(torch.zeros(400, dtype=torch.int16),
                            torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32))


# ------------------------------------------------------------------------------------------
def test_batches_are_longest_first_and_stable():
    from ctc_asr_amd import transcribe
    assert transcribe.batch_order([5, 9, 5, 7, 9, 1], 4) == [[1, 4, 3, 0], [2, 5]]
    assert transcribe.batch_order([], 4) == []
    assert transcribe.batch_order([3], 1) == [[0]]


def test_assembly_shifts_words_and_joins_texts():
    from ctc_asr_amd import transcribe
    start = np.array([1600, 48000, 160000], dtype=np.int64)
    length = np.array([16000, 32001, 480], dtype=np.int32)
    words = [[{'word': 'ab', 'start': 0.02, 'end': 0.1, 'confidence': -0.5},
              {'word': 'c', 'start': 0.5, 'end': 0.52, 'confidence': -1.25}],
             [],
             [{'word': 'z', 'start': 0.0, 'end': 0.02, 'confidence': None}]]
    got = transcribe.assemble(start, length, ['ab c', '', 'z'], 163840, words)
    assert got['plaintext'] == 'ab c z'
    assert got['audio_seconds'] == 10.24 and got['speech_seconds'] == 48481 / 16000
    assert got['segments'] == [
        {'start': 0.1, 'end': 1.1, 'plaintext': 'ab c', 'words': [
            {'word': 'ab', 'start': 0.12, 'end': 0.2, 'confidence': -0.5},
            {'word': 'c', 'start': 0.6, 'end': 0.62, 'confidence': -1.25}]},
        {'start': 3.0, 'end': 5.000063, 'plaintext': '', 'words': []},
        {'start': 10.0, 'end': 10.03, 'plaintext': 'z', 'words': [
            {'word': 'z', 'start': 10.0, 'end': 10.02, 'confidence': None}]}]
    assert words[0][0]['start'] == 0.02                          # the per-piece lists are kept
    for piece in got['segments']:
        assert json.loads(json.dumps(piece)) == piece
    plain = transcribe.assemble(start, length, ['ab c', '', 'z'], 163840)
    assert all(sorted(piece) == ['end', 'plaintext', 'start'] for piece in plain['segments'])
    empty = transcribe.assemble(start[:0], length[:0], [], 16000)
    assert empty == {'plaintext': '', 'segments': [], 'audio_seconds': 1.0, 'speech_seconds': 0.0}


def test_nbest_is_refused_before_anything_is_read():
    from ctc_asr_amd import transcribe
    with pytest.raises(ValueError, match='nbest'):
        transcribe.transcribe(None, '/no/such/file.wav', nbest=2)
