"""Augmentation without a GPU: the pinned integer draws, the sample-count formula, the argument
errors of the C entry points, the flags, the host side of the pipeline, and the float64
resampler of tests/augment_reference.py against an analytic sine."""

import ctypes
import random

import numpy as np
import pytest

from tests import augment_reference as ref


@pytest.fixture(scope='module')
def lib():
    from ctc_asr_amd import build, hip
    build.build(verbose=False)
    return hip.load()


def test_r24_matches_values_from_the_formula():
    # seed 0, counters 0..3: the first outputs of splitmix64 seeded with 0, as published with
    # the generator (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F,
    # 0xF88BB8A8724C81EC), top 24 bits
    assert [ref.r24(0, i) for i in range(4)] == [0xE220A8, 0x6E789E, 0x06C45D, 0xF88BB8]
    # computed once from the formula with exact integers
    table = {(1, 0): 0x910A2D, (0xDEADBEEF, 12345): 0x48A45C,
             ((1 << 64) - 1, (1 << 40) + 7): 0x886EF5, (42, 64 * 5 + 33): 0x94C3C3}
    for (seed, idx), want in table.items():
        assert ref.r24(seed, idx) == want, (seed, idx)


def test_below_never_reaches_n():
    rng = random.Random(5)
    for n in (1, 2, 3, 28, 81, 101, 1000, (1 << 24) - 1, 1 << 24):
        seen = set()
        for _ in range(400):
            value = ref.below(rng.getrandbits(64), rng.getrandbits(40), n)
            assert 0 <= value < n
            seen.add(value)
        if n <= 3:
            assert seen == set(range(n))
    # the largest r24 there is still stays below n
    assert ((1 << 24) - 1) * (1 << 24) >> 24 == (1 << 24) - 1


@pytest.mark.parametrize('time_width, permille', [(100, 1000), (3, 1000), (100, 500), (100, 0)])
def test_intervals_stay_inside_the_row(time_width, permille):
    lengths = [0, 1, 2, 3, 4, 5]
    for seed in range(40):
        for freq_width in (0, 27, 80, 500):
            got = ref.mask_intervals(seed, lengths, 7, 16, freq_width, 16, time_width, permille)
            assert got.shape == (6, 32, 2) and (got >= 0).all()
            assert not got[0].any()                                   # L == 0: no masks
            assert (got[:, :16].sum(axis=2) <= 80).all()
            assert (got[:, :16, 1] <= min(freq_width, 80)).all()
            for b, length in enumerate(lengths):
                assert (got[b, 16:].sum(axis=1) <= length).all()
                assert (got[b, 16:, 1] <= min(time_width, length * permille // 1000)).all()
            cells = ref.mask_cells(got, lengths, 7, 16)
            for b, length in enumerate(lengths):
                assert not cells[b, length:].any()


def test_resample_num_samples_equals_the_reference(lib):
    from ctc_asr_amd import hip
    for percent in (50, 90, 100, 110, 200, 49, 201):
        for n in list(range(-1, 3001)) + [272000]:
            assert lib.ctcasr_resample_num_samples(n, percent) == \
                ref.resample_num_samples(n, percent), (n, percent)
    assert hip.resample_num_samples(272000, 90) == 302222
    assert hip.resample_num_samples(1, 200) == 1 and hip.resample_num_samples(0, 100) == 0
    assert lib.ctcasr_resample_num_samples(2 ** 31 - 1, 50) == 2 ** 31 - 1      # saturates


def test_entry_points_report_argument_errors_before_any_launch(lib):
    # all pointers null
    assert lib.ctcasr_spec_augment(None, None, 4, 100, 1, 2, 27, 2, 100, 1000, None, None) == -1
    assert lib.ctcasr_speed_perturb(None, None, None, 4, 1000, None, 1000, None, None) == -1
    # host memory stands in for the buffers: a refused call never touches them
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)

    def spec(feat=p, lengths=p, batch=1, frames=4, n_freq=2, freq_width=27, n_time=2,
             time_width=100, permille=1000):
        return lib.ctcasr_spec_augment(feat, lengths, batch, frames, 7, n_freq, freq_width, n_time,
                                       time_width, permille, None, None)

    assert spec(feat=None) == -1 and spec(lengths=None) == -1
    assert spec(n_freq=17) == -1 and spec(n_freq=-1) == -1
    assert spec(n_time=17) == -1 and spec(n_time=-1) == -1
    assert spec(freq_width=-1) == -1 and spec(time_width=-1) == -1
    assert spec(permille=-1) == -1 and spec(permille=1001) == -1
    assert spec(frames=-1) == -1 and spec(batch=0) == -1
    assert spec(n_freq=0, n_time=0) == 0            # nothing to mask: no launch, no device needed

    def speed(pcm=p, num=p, pct=p, batch=1, max_in=16, out=p, max_out=16, count=p):
        return lib.ctcasr_speed_perturb(pcm, num, pct, batch, max_in, out, max_out, count, None)

    for name in ('pcm', 'num', 'pct', 'out', 'count'):
        assert speed(**{name: None}) == -1, name
    assert speed(batch=0) == -1 and speed(max_in=0) == -1 and speed(max_out=0) == -1


def test_wrappers_refuse_mismatched_batches_and_cpu_tensors(lib):
    import torch
    from ctc_asr_amd import hip
    feats = torch.zeros(5, 9, 80)
    with pytest.raises(hip.CtcAsrError, match='4 entries for a batch of 5'):
        hip.spec_augment(feats, torch.zeros(4, dtype=torch.int32), 1, 2, 27, 2, 100, 1000)
    with pytest.raises(hip.CtcAsrError, match=r'\[B, T, 80\]'):
        hip.spec_augment(feats[:, :, :40], torch.zeros(5, dtype=torch.int32), 1, 2, 27, 2, 100)
    with pytest.raises(hip.CtcAsrError, match='n_time is 17'):
        hip.spec_augment(feats, torch.zeros(5, dtype=torch.int32), 1, 2, 27, 17, 100)
    with pytest.raises(hip.CtcAsrError, match='intervals holds 10 elements, 40 expected'):
        hip.spec_augment(feats, torch.zeros(5, dtype=torch.int32), 1, 2, 27, 2, 100, 1000,
                         torch.zeros(10, dtype=torch.int32))
    with pytest.raises(hip.CtcAsrError, match='CPU tensor'):
        hip.spec_augment(feats, torch.zeros(5, dtype=torch.int32), 1, 2, 27, 2, 100)
    pcm = torch.zeros(5, 64, dtype=torch.int16)
    counts = torch.zeros(5, dtype=torch.int32)
    with pytest.raises(hip.CtcAsrError, match='num_samples holds 3 entries for a batch of 5'):
        hip.speed_perturb(pcm, counts[:3], counts)
    with pytest.raises(hip.CtcAsrError, match='percent holds 6 entries for a batch of 5'):
        hip.speed_perturb(pcm, counts, torch.zeros(6, dtype=torch.int32))
    with pytest.raises(hip.CtcAsrError, match='CPU tensor'):
        hip.speed_perturb(pcm, counts, counts)


def test_header_binding_and_flags_agree_on_the_limits():
    import os
    import re
    from ctc_asr_amd import hip, params
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'ctcasr.h')).read()
    limit = int(re.search(r'#define CTCASR_SPEC_AUGMENT_MAX_MASKS (\d+)', text).group(1))
    assert limit == hip.SPEC_AUGMENT_MAX_MASKS == params.SPECAUG_MAX_MASKS == 16
    for name in ('ctcasr_spec_augment', 'ctcasr_speed_perturb', 'ctcasr_resample_num_samples'):
        assert name in hip.SIGNATURES
    assert hip.ABI_VERSION == 8


def test_flags_parse_and_refuse_bad_values():
    from ctc_asr_amd import params
    flags = params.FLAGS
    flags.reset()
    try:
        assert flags.spec_augment is False and flags.speed_perturb == ''
        assert (flags.specaug_freq_masks, flags.specaug_freq_width, flags.specaug_time_masks,
                flags.specaug_time_width, flags.specaug_time_permille) == (2, 27, 2, 100, 1000)
        plain = params.get_parameters()
        assert 'Augmentation' not in plain
        flags.parse(['--spec_augment', '--specaug_freq_masks=16', '--specaug_time_masks', '0',
                     '--specaug_time_permille=200', '--speed_perturb=90,100,110'])
        assert flags.spec_augment is True and flags.specaug_freq_masks == 16
        assert flags.specaug_time_masks == 0 and flags.specaug_time_permille == 200
        assert params.parse_speed_perturb(flags.speed_perturb) == [90, 100, 110]
        shown = params.get_parameters()
        assert shown.startswith(plain) and 'speed_perturb=90,100,110' in shown
        assert 'spec_augment=True' in shown
        for bad in ('--speed_perturb=49', '--speed_perturb=90,201', '--speed_perturb=fast',
                    '--specaug_freq_masks=17', '--specaug_time_masks=17',
                    '--specaug_time_masks=-1', '--specaug_freq_width=-1',
                    '--specaug_time_width=-3', '--specaug_time_permille=1001'):
            with pytest.raises(ValueError):
                flags.parse([bad])
        with pytest.raises(ValueError):
            flags.speed_perturb = '300'
        assert params.parse_speed_perturb(flags.speed_perturb) == [90, 100, 110]   # kept
        assert params.parse_speed_perturb('') == [] and params.parse_speed_perturb('50 200') == \
            [50, 200]
    finally:
        flags.reset()


def test_speeds_ride_with_the_batches_and_leave_their_composition_alone(tmp_path):
    """`host_batches(speed_percents=...)`: the same utterances in the same batches as without,
    one of the percents on each, the same draw for the same seed, and two ranks holding the
    slices of the list a single process draws."""
    from ctc_asr_amd import input_functions as inp
    from ctc_asr_amd import synth
    from ctc_asr_amd.params import FLAGS
    FLAGS.reset()
    try:
        synth.write_corpus(str(tmp_path / 'corpus'), str(tmp_path / 'train.csv'),
                           [0.7 + 0.05 * i for i in range(12)], seed=3, chars_per_second=5.0)
        FLAGS.update(corpus_dir=str(tmp_path / 'corpus'), train_csv=str(tmp_path / 'train.csv'),
                     batch_size=2, shuffle_buffer_size=4, num_buckets=2)
        bounds = inp.get_bucket_boundaries(FLAGS.train_csv, 2)
        for use_buckets in (False, True):
            plain = list(inp.host_batches(FLAGS.train_csv, use_buckets, bounds, seed=9))
            fast = list(inp.host_batches(FLAGS.train_csv, use_buckets, bounds, seed=9,
                                         speed_percents=[90, 110]))
            again = list(inp.host_batches(FLAGS.train_csv, use_buckets, bounds, seed=9,
                                          speed_percents=[90, 110]))
            assert [[it[2] for it in b] for b in fast] == [[it[2] for it in b] for b in plain]
            assert all(len(it) == 3 for b in plain for it in b)
            speeds = [it[3] for b in fast for it in b]
            assert set(speeds) == {90, 110}
            assert speeds == [it[3] for b in again for it in b]
            other = [it[3] for b in inp.host_batches(FLAGS.train_csv, use_buckets, bounds, seed=10,
                                                     speed_percents=[90, 110]) for it in b]
            assert other != speeds
        FLAGS.update(batch_size=1)
        ranks = [list(inp.host_batches(FLAGS.train_csv, False, bounds, rank, 2, seed=9,
                                       speed_percents=[90, 110])) for rank in (0, 1)]
        FLAGS.update(batch_size=2)
        single = list(inp.host_batches(FLAGS.train_csv, False, bounds, seed=9,
                                       speed_percents=[90, 110]))
        for group, first, second in zip(single, *ranks):
            assert [(it[2], it[3]) for it in group] == \
                [(it[2], it[3]) for it in first + second]
    finally:
        FLAGS.reset()


@pytest.mark.parametrize('percent, measured', [(90, 4.93e-5), (110, 6.02e-5)])
def test_float64_resampler_reproduces_a_sine(percent, measured):
    """A 440 Hz sine of amplitude A at 16 kHz, resampled, against the same sine evaluated at the
    output positions j P / 100, 60 samples (more than the filter's reach) away from both ends.
    What is left is the pass-band ripple of the windowed sinc.  Measured with this very code:
    4.93e-5 A at 90 %, 6.02e-5 A at 110 %; asserted with a margin of 2."""
    amplitude, n = 20000.0, 16000
    x = amplitude * np.sin(2 * np.pi * 440 * np.arange(n) / 16000)
    y = ref.resample_float64(x, percent)
    assert len(y) == ref.resample_num_samples(n, percent)
    exact = amplitude * np.sin(2 * np.pi * 440 * np.arange(len(y)) * percent / 100 / 16000)
    worst = np.abs(y - exact)[60:-60].max() / amplitude
    print('P = {}: worst deviation {:.3e} of the amplitude'.format(percent, worst))
    assert worst < 2 * measured
    # at 100 % the reference is a copy, and its rounding is to nearest even with saturation
    assert np.array_equal(ref.speed_perturb(np.array([5, -7, 32767], dtype=np.int16), 100),
                          [5, -7, 32767])


# ------------------------------------------------------------------------------------------
# the fp32 restatement of the resampler (tests/augment_reference.py: speed_perturb_f32)
def _round_to_f32(value):
    """A nonzero Fraction rounded to the nearest fp32, ties to even, in integers (normal range)."""
    from fractions import Fraction
    sign, mag = (-1, -value) if value < 0 else (1, value)
    e = mag.numerator.bit_length() - mag.denominator.bit_length()
    if Fraction(2) ** e > mag:
        e -= 1
    assert Fraction(2) ** e <= mag < Fraction(2) ** (e + 1)
    scaled = mag / Fraction(2) ** (e - 23)                   # in [2^23, 2^24)
    whole = scaled.numerator // scaled.denominator
    rest = scaled - whole
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and whole & 1):
        whole += 1
    return sign * float(whole * Fraction(2) ** (e - 23))


def test_fma_f32_rounds_once():
    """`fma_f32` against exact rational arithmetic: random operands of the kernel's ranges, and
    products that sit exactly on an fp32 tie with an accumulator far below the last float64 bit
    on either side of it - where a float64 sum rounded again to fp32 goes wrong."""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a = rng.integers(-32768, 32768, size=600).astype(np.float64)
    b = (rng.normal(size=600) * 0.3).astype(np.float32).astype(np.float64)
    acc = (rng.normal(size=600) * 10.0 ** rng.integers(-3, 6, size=600)).astype(np.float32)
    # a = 3, b = 1 + k 2^-23 with k odd: 3 b lies halfway between two fp32 values of [2, 4)
    k = 2 * rng.integers(0, 1 << 21, size=200) + 1
    a = np.concatenate([a, np.full(200, 3.0)])
    b = np.concatenate([b, 1.0 + k * 2.0 ** -23])
    tiny = np.where(rng.integers(0, 2, size=200) == 0, -1.0, 1.0) * 2.0 ** -60
    acc = np.concatenate([acc.astype(np.float64), tiny])
    assert np.array_equal(b, b.astype(np.float32).astype(np.float64))
    got = ref.fma_f32(a, b, acc)
    twice = (a * b + acc).astype(np.float32).astype(np.float64)
    for i in range(len(a)):
        exact = Fraction(a[i]) * Fraction(b[i]) + Fraction(acc[i])
        want = _round_to_f32(exact) if exact else 0.0
        assert got[i] == want, (a[i], b[i], acc[i])
    assert (twice[600:] != got[600:]).any()                 # the crafted ties tell the two apart


@pytest.fixture(scope='module')
def every_percent():
    """One full-scale random row of 257 samples at every percent: the restatement, its
    accumulator and the float64 result."""
    x = np.random.default_rng(7).integers(-32768, 32768, size=257).astype(np.int16)
    return x, {p: ref.speed_perturb_f32(x, p) + (ref.speed_perturb(x, p),) for p in range(50, 201)}


def test_restatement_is_within_one_lsb_of_float64_at_every_percent(every_percent):
    """The existing budget (tests/test_gpu_augment.py) holds for the header's arithmetic itself,
    at all 151 percents.  Seen on this row: largest difference 1 LSB, 0.11 % of samples differ."""
    x, results = every_percent
    differing = total = 0
    for percent, (y, acc, want) in results.items():
        assert len(y) == len(acc) == len(want) == ref.resample_num_samples(257, percent)
        assert y.dtype == np.int16 and acc.dtype == np.float32
        diff = np.abs(y.astype(np.int64) - want.astype(np.int64))
        assert diff.max() <= 1, (percent, int(diff.max()))
        differing += int((diff > 0).sum())
        total += len(y)
    assert np.array_equal(results[100][0], x) and np.array_equal(results[100][1], x)
    print('restatement: {} of {} samples differ from float64 ({:.4%})'
          .format(differing, total, differing / total))
    assert 0 < differing < total // 100                     # fp32 is visible, and rare


def test_restatement_rounds_to_even_and_saturates():
    # one sample at 50 %: out[0] = x[0] h(0) with h(0) = c = 0.95, out[1] sits at t = 0.5
    for value in (32767, -32768, 10, -10):
        y, acc = ref.speed_perturb_f32(np.array([value], dtype=np.int16), 50)
        want = np.float32(value) * np.float32(0.95)
        assert len(y) == 2 and acc[0] == want and y[0] == np.rint(want)
    square = (32767 * np.where((np.arange(400) // 20) % 2 == 0, 1, -1)).astype(np.int16)
    y, acc = ref.speed_perturb_f32(square, 90)
    assert acc.max() > 32768 and acc.min() < -32769
    assert y.max() == 32767 and y.min() == -32768
    assert ref.tie_eligible([0.5, -2.5, 7.515, 7.52, 3.0, -0.484375]).tolist() == \
        [True, True, True, False, False, True]


def test_kernel_tap_window_covers_the_filter():
    """m in [-R, R + 1] loses nothing: for every percent and every phase a row reaches (the
    multiples of gcd(P, 100)), sum |h| over the kernel's taps equals sum |h| over the wider walk of
    `resample_float64`.  The largest is 2.17, at P = 50: the '< 3' of the error budget in
    tests/test_gpu_augment.py holds at all percents."""
    import math
    largest = (0.0, None)
    for percent in range(50, 201):
        g = math.gcd(percent, 100)
        phase = np.arange(0, 100, g) / 100.0
        c = 95.0 / max(percent, 100)
        radius = ref.tap_radius(percent)
        assert 2 * radius + 2 <= 52 and (100 // g) * (2 * radius + 2) <= 5200
        reach = int(np.ceil(12.0 / c)) + 2
        assert reach > radius + 1
        narrow = sum(np.abs(ref.tap_weight(c, phase - m)) for m in range(-radius, radius + 2))
        wide = sum(np.abs(ref.tap_weight(c, phase - m)) for m in range(-reach, reach + 1))
        assert np.abs(narrow - wide).max() <= 1e-12, percent
        largest = max(largest, (float(wide.max()), -percent))
    # (phase 0.5 at c = 0.95: every percent up to 100 that reaches it ties with P = 50)
    assert largest[1] == -50 and 2.16 < largest[0] < 2.18
    assert ref.tap_radius(199) == 25 and ref.tap_radius(200) == 25 and ref.tap_radius(100) == 12
    assert sorted({ref.tap_radius(p) for p in range(101, 201)}) == list(range(12, 26))


def test_seeds_put_the_masks_on_the_edges():
    """The seeds tests/test_gpu_augment_edges.py relies on give the intervals it expects."""
    for seed, want in ref.TIME_SEAM_SEEDS.items():
        got = ref.mask_intervals(seed, [129], 129, 0, 27, 1, 200, 1000)
        assert tuple(got[0, 0]) == want, seed
    for seed, want in ref.FREQ_EDGE_SEEDS.items():
        got = ref.mask_intervals(seed, [5], 5, 1, 27, 0, 200, 1000)
        assert tuple(got[0, 0]) == want, seed
    assert ref.TIME_SEAM_SEEDS[74][0] == 64 and sum(ref.TIME_SEAM_SEEDS[1263]) == 64
    assert ref.TIME_SEAM_SEEDS[125] == (0, 129) and ref.TIME_SEAM_SEEDS[46192] == (128, 1)
    assert ref.FREQ_EDGE_SEEDS[38][0] == 0 and sum(ref.FREQ_EDGE_SEEDS[45]) == 80
    assert ref.TIME_SEAM_SEEDS[454][1] == 0 and ref.FREQ_EDGE_SEEDS[10][1] == 0


def test_spec_augment_takes_no_features_only_for_no_frames(lib):
    """An empty [B, 0, 80] buffer has a null address; the header serves out_frames == 0, so a
    null `features` is an error only where there are frames.  (With masks to draw the call
    launches: tests/test_gpu_augment_edges.py.)"""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert lib.ctcasr_spec_augment(None, p, 3, 0, 7, 0, 27, 0, 100, 1000, None, None) == 0
    assert lib.ctcasr_spec_augment(None, p, 3, 1, 7, 0, 27, 0, 100, 1000, None, None) == -1
    assert lib.ctcasr_spec_augment(None, None, 3, 0, 7, 0, 27, 0, 100, 1000, None, None) == -1
    assert lib.ctcasr_spec_augment(None, p, 3, -1, 7, 0, 27, 0, 100, 1000, None, None) == -1
