"""The augmentation kernels at every speed and every seam, against tests/augment_reference.py.

Speed perturbation is held to three references at once:
  * the float64 resampler, 1 LSB on every sample (the budget of tests/test_gpu_augment.py; the
    sum |h| < 3 in it holds at all percents: tests/test_augment_host.py);
  * `ref.speed_perturb_f32`, the header's fp32 arithmetic stated tap for tap, sample for sample.
    A mismatch is tolerated only where that restatement's accumulator before rounding lies within
    2^-6 of a half-integer: the device's and the host's fp64 sin / cos may differ in the last
    place; one weight off by one fp32 ulp (relative 2^-24 of a weight below 1, times |x| <= 2^15)
    moves the sum by at most 2^-9, and can flip the rounding of one partial sum, worth at most
    one fp32 ulp of a sum below 2^17, 2^-7;
  * itself: the same row gives the same bits wherever it sits in a batch, whatever lies past its
    end, and whatever buffer the caller hands in.
The rows run all 151 percents (1, 2, 4, 5, 10, 20, 25, 50 and 100 phases in the tap table, 26 to
52 taps), lengths below the filter's, and outputs that end one short of, on and one past the
2048-sample chunk of a workgroup.

SpecAugment stays bit-exact: `intervals` equals the reference's draws, every cell keeps its word
or becomes the all-zero word exactly where the reference says, and the words around the feature
buffer and around `intervals` keep theirs.  Row lengths and masks are placed on the 64-frame tile
seams with seeds the reference found (ref.TIME_SEAM_SEEDS, ref.FREQ_EDGE_SEEDS).

Seen on the MI355X: 0 mismatches with the restatement in the 35868 samples of
test_every_percent_* (1198 of them, 3.34 %, lie within 2^-6 of a tie), 0 in the 3638 of the short
rows, 0 in the 448359 of the chunk seams and 0 in the 98777 of the pipeline case.  The kernel
differs from float64 in 41 of the 35868 samples (0.1143 %); the restatement differs in the same
41 (0.1143 %)."""

import functools

import numpy as np
import pytest
import torch

from tests import augment_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL_BITS = 0x7FC12345            # a NaN with a payload: survives only if it is never stored to
GUARD = 256                           # words in front of and behind a buffer under test
ALL_PERCENTS = list(range(50, 201))


# ------------------------------------------------------------------------------------------
# speed perturbation
@functools.lru_cache(maxsize=None)
def _expected_cached(data, percent):
    x = np.frombuffer(data, dtype=np.int16)
    y32, acc = ref.speed_perturb_f32(x, percent)
    return ref.speed_perturb(x, percent), y32, acc


def _expected(x, percent):
    """(float64 result, fp32 restatement, its accumulator) of one row, computed once."""
    return _expected_cached(np.ascontiguousarray(x, dtype=np.int16).tobytes(), percent)


def _random_row(n, seed):
    return np.random.default_rng(seed).integers(-32768, 32768, size=n).astype(np.int16)


def _pcm_of(rows, max_in, garbage_seed):
    """Rows in a wider buffer whose every other column holds +-32767."""
    assert max_in > max(len(r) for r in rows)
    rng = np.random.default_rng(garbage_seed)
    pcm = (32767 * (2 * rng.integers(0, 2, size=(len(rows), max_in)) - 1)).astype(np.int16)
    for i, row in enumerate(rows):
        pcm[i, :len(row)] = row
    return pcm


def _launch(hip, rows, percents, max_out, garbage_seed=1):
    max_in = max(len(r) for r in rows) + 11
    pcm = _pcm_of(rows, max_in, garbage_seed)
    counts = [len(r) for r in rows]
    out, out_n = hip.speed_perturb(torch.from_numpy(pcm).to(DEV),
                                   torch.tensor(counts, dtype=torch.int32, device=DEV),
                                   torch.tensor(percents, dtype=torch.int32, device=DEV), max_out)
    assert out.shape == (len(rows), max_out) and out.dtype == torch.int16
    return out.cpu().numpy(), out_n.cpu().numpy()


class _Tally:
    def __init__(self):
        self.total = self.mismatches = self.eligible = self.kernel_differs = self.f32_differs = 0


def _verify(out, out_n, rows, percents, tally=None):
    """Every row of a launch against all references; a row with n == 0 or a percent outside
    50..200 is the header's bad row: count 0, all zero."""
    tally = tally or _Tally()
    max_out = out.shape[1]
    for i, (x, percent) in enumerate(zip(rows, percents)):
        n_out = min(ref.resample_num_samples(len(x), percent), max_out)
        assert out_n[i] == n_out, (i, len(x), percent)
        assert not out[i, n_out:].any(), (i, len(x), percent)            # zero padding
        if n_out == 0:
            continue
        y64, y32, acc = (part[:n_out] for part in _expected(x, percent))
        got = out[i, :n_out]
        if percent == 100:
            assert np.array_equal(got, x[:n_out])                         # a bit copy
        diff = np.abs(got.astype(np.int64) - y64.astype(np.int64))
        assert diff.max() <= 1, (i, len(x), percent, int(diff.max()))
        miss = got != y32
        eligible = ref.tie_eligible(acc)
        bad = np.flatnonzero(miss & ~eligible)
        assert not len(bad), ('row {} (n = {}, P = {}): {} samples differ from the fp32 '
                              'restatement away from a tie, first at {}: got {}, want {}, '
                              'accumulator {!r}').format(i, len(x), percent, len(bad), bad[0],
                                                         got[bad[0]], y32[bad[0]], acc[bad[0]])
        tally.total += n_out
        tally.mismatches += int(miss.sum())
        tally.eligible += int(eligible.sum())
        tally.kernel_differs += int((diff > 0).sum())
        tally.f32_differs += int((y32 != y64).sum())
    return tally


@pytest.fixture(scope='module')
def every_percent(hip):
    """One launch of 151 rows: the same 257 samples at P = 50..200."""
    x = _random_row(257, 7)
    rows = [x] * len(ALL_PERCENTS)
    out, out_n = _launch(hip, rows, ALL_PERCENTS, 514)
    return x, rows, out, out_n


def test_every_percent_matches_the_fp32_restatement(every_percent):
    """Seen on the MI355X: 0 mismatches in 35868 samples."""
    x, rows, out, out_n = every_percent
    # the escape is narrow, and that is a property of the inputs alone
    eligible = sum(int(ref.tie_eligible(_expected(x, p)[2]).sum()) for p in ALL_PERCENTS)
    total = sum(ref.resample_num_samples(257, p) for p in ALL_PERCENTS)
    assert eligible <= 0.05 * total, (eligible, total)
    tally = _verify(out, out_n, rows, ALL_PERCENTS)
    assert tally.total == total == 35868 and tally.eligible == eligible
    assert np.array_equal(out[ALL_PERCENTS.index(100), :257], x)
    assert out_n[0] == 514 and out_n[-1] == 128
    print('speed_perturb, P = 50..200: {} of {} samples differ from the fp32 restatement '
          '({} lie within 2^-6 of a tie)'.format(tally.mismatches, total, eligible))


def test_every_percent_differs_from_float64_no_more_than_fp32_must(every_percent):
    """The kernel's share of samples that differ from float64 against the share of the header's
    arithmetic itself, with a factor of 3 for the fp64 libm differences.  Seen on the MI355X:
    0.1143 % (41 of 35868) against 0.1143 % (41)."""
    x, rows, out, out_n = every_percent
    tally = _verify(out, out_n, rows, ALL_PERCENTS)
    print('speed_perturb, P = 50..200: kernel differs from float64 in {} of {} samples ({:.4%}), '
          'the restatement in {} ({:.4%})'.format(tally.kernel_differs, tally.total,
                                                  tally.kernel_differs / tally.total,
                                                  tally.f32_differs,
                                                  tally.f32_differs / tally.total))
    assert tally.f32_differs > 0
    assert tally.kernel_differs <= 3 * tally.f32_differs


SHORT_COUNTS = [1, 2, 3, 12, 13, 25, 26, 27, 51, 52, 53]
SHORT_PERCENTS = [50, 51, 95, 99, 101, 150, 199, 200]


def _short_rows():
    """Rows shorter than the filter (26 taps up to 100 %, 52 at 200 %): both tap clamps are
    active at once.  Three impulses in 53 samples show a tap index off by one as a shifted copy
    of the filter."""
    rows, percents = [], []
    for n in SHORT_COUNTS:
        for percent in SHORT_PERCENTS:
            rows.append(_random_row(n, 100 + n))
            percents.append(percent)
    for at in (0, 52, 26):
        impulse = np.zeros(53, dtype=np.int16)
        impulse[at] = 32767
        for percent in SHORT_PERCENTS:
            rows.append(impulse)
            percents.append(percent)
    return rows, percents


def test_rows_shorter_than_the_filter(hip):
    rows, percents = _short_rows()
    out, out_n = _launch(hip, rows, percents, 106, garbage_seed=1)
    tally = _verify(out, out_n, rows, percents)
    assert out_n.max() == 106 and out_n.min() == 1 and tally.total == int(out_n.sum())
    # nothing past a row's n is read: other garbage there and in the padding, the same bits
    again, again_n = _launch(hip, rows, percents, 106, garbage_seed=2)
    assert np.array_equal(again, out) and np.array_equal(again_n, out_n)
    print('speed_perturb, short rows: {} of {} samples differ from the fp32 restatement'
          .format(tally.mismatches, tally.total))


@pytest.mark.parametrize('sentinel', [0x5A5A, ~0x5A5A])
def test_the_callers_buffers_are_written_fully_and_nothing_around_them(hip, sentinel):
    """The library entry with the caller's own `out` and `out_samples` between sentinel words.
    With two complementary sentinels no column can hold its expected value by not being written
    both times."""
    rows, percents = _short_rows()
    batch, max_out, max_in = len(rows), 106, 64
    want, want_n = _launch(hip, rows, percents, max_out)
    pcm = torch.from_numpy(_pcm_of(rows, max_in, 3)).to(DEV)
    counts = torch.tensor([len(r) for r in rows], dtype=torch.int32, device=DEV)
    pct = torch.tensor(percents, dtype=torch.int32, device=DEV)
    held = torch.full((GUARD + batch * max_out + GUARD,), sentinel, dtype=torch.int16, device=DEV)
    held_n = torch.full((GUARD + batch + GUARD,), sentinel, dtype=torch.int32, device=DEV)
    out, out_n = held[GUARD:GUARD + batch * max_out], held_n[GUARD:GUARD + batch]
    assert out.data_ptr() == held.data_ptr() + 2 * GUARD
    code = hip.load().ctcasr_speed_perturb(
        pcm.data_ptr(), counts.data_ptr(), pct.data_ptr(), batch, max_in, out.data_ptr(), max_out,
        out_n.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert code == 0
    torch.cuda.synchronize()
    got, got_n = held.cpu().numpy(), held_n.cpu().numpy()
    for buf, size in ((got, batch * max_out), (got_n, batch)):
        assert (buf[:GUARD] == sentinel).all() and (buf[GUARD + size:] == sentinel).all()
    assert np.array_equal(got[GUARD:GUARD + batch * max_out].reshape(batch, max_out), want)
    assert np.array_equal(got_n[GUARD:GUARD + batch], want_n)


@pytest.mark.parametrize('percent', [97, 150, 199])
def test_rows_do_not_see_each_other(hip, percent):
    """The same row first and last in a batch of other percents (100 phases, 2 phases, the copy,
    a bad row) and alone: the same bits."""
    x = _random_row(300, 40 + percent)
    others = [(_random_row(257, 50), 199), (_random_row(300, 51), 50), (_random_row(150, 52), 100),
              (_random_row(300, 53), 97), (_random_row(40, 54), 150), (_random_row(300, 55), 49),
              (_random_row(299, 56), 143)]
    rows = [x] + [r for r, _ in others] + [x]
    percents = [percent] + [p for _, p in others] + [percent]
    out, out_n = _launch(hip, rows, percents, 600)
    _verify(out, out_n, rows, percents)
    alone, alone_n = _launch(hip, [x], [percent], 600, garbage_seed=9)
    assert np.array_equal(out[0], out[-1]) and out_n[0] == out_n[-1] == alone_n[0]
    assert np.array_equal(out[0], alone[0])


SEAM_TARGETS = [2047, 2048, 2049, 4096, 4097]


@pytest.mark.parametrize('percent', [97, 150, 199])
def test_chunk_seams(hip, percent):
    """Rows whose n_out ends one short of, on and one past the 2048-sample chunk of a workgroup
    (and of two), each with max_out = n_out, one less (the row is cut and out_samples says so)
    and 2048 more (a whole trailing chunk of zeros).  Beside them in every launch: the two kinds
    of bad row, a cut bit copy and a short bit copy."""
    tally = _Tally()
    for target in SEAM_TARGETS:
        n = -(-target * percent // 100)                    # the smallest n with n * 100 // P == target
        assert n * 100 // percent == target and (n - 1) * 100 // percent == target - 1
        x = _random_row(n, 1000 * percent + target)
        for max_out in (target, target - 1, target + 2048):
            rows = [x, np.zeros(0, dtype=np.int16), _random_row(500, 60),
                    _random_row(max_out + 5, 61), _random_row(max_out - 3, 62)]
            percents = [percent, 97, 49, 100, 100]
            out, out_n = _launch(hip, rows, percents, max_out)
            _verify(out, out_n, rows, percents, tally)
            assert out_n.tolist() == [min(target, max_out), 0, 0, max_out, max_out - 3]
            assert not out[1:3].any()
    print('speed_perturb, chunk seams at P = {}: {} of {} samples differ from the fp32 '
          'restatement'.format(percent, tally.mismatches, tally.total))


# ------------------------------------------------------------------------------------------
# SpecAugment
DEFAULTS = (2, 27, 2, 100, 1000)          # n_freq, freq_width, n_time, time_width, time_permille
SIXTEEN_EACH = (16, 27, 16, 100, 1000)
SPECIALS = np.array([-0.0, np.inf, -np.inf, np.nan, 1.5], dtype=np.float32)


def _spec_run(hip, lengths, out_frames, seed, settings, cells=None, with_intervals=True):
    """One launch on a feature tensor that is a contiguous view in the middle of a larger
    allocation of NaN words, with `intervals` in the middle of one of -7s.  Frames at or beyond a
    row's length hold the NaN word too.  Checks the intervals, every cell and every guard word
    against the reference; -> (intervals, mask, words before)."""
    n_freq, freq_width, n_time, time_width, permille = settings
    lengths = np.asarray(lengths, dtype=np.int32)
    batch, masks = len(lengths), n_freq + n_time
    size = batch * out_frames * 80
    rng = np.random.default_rng(seed % 1000 + out_frames)
    feats = rng.normal(size=(batch, out_frames, 80)).astype(np.float32) if cells is None else \
        np.array(cells, dtype=np.float32).reshape(batch, out_frames, 80)
    words = feats.view(np.int32)
    for b, length in enumerate(lengths):
        words[b, min(max(int(length), 0), out_frames):] = SENTINEL_BITS
    host = np.full(GUARD + size + GUARD, SENTINEL_BITS, dtype=np.int32)
    host[GUARD:GUARD + size] = words.reshape(-1)
    held = torch.from_numpy(host).to(DEV)
    x = held[GUARD:GUARD + size].view(torch.float32).view(batch, out_frames, 80)
    held_iv = torch.full((GUARD + batch * masks * 2 + GUARD,), -7, dtype=torch.int32, device=DEV)
    iv = held_iv[GUARD:GUARD + batch * masks * 2].view(batch, masks, 2)
    out = hip.spec_augment(x, torch.from_numpy(lengths).to(DEV), seed, n_freq, freq_width, n_time,
                           time_width, permille, iv if with_intervals else None)
    assert out is x
    want_iv = ref.mask_intervals(seed, lengths, out_frames, n_freq, freq_width, n_time,
                                 time_width, permille)
    mask = ref.mask_cells(want_iv, lengths, out_frames, n_freq)
    got, got_iv = held.cpu().numpy(), held_iv.cpu().numpy()
    assert (got[:GUARD] == SENTINEL_BITS).all() and (got[GUARD + size:] == SENTINEL_BITS).all()
    assert (got_iv[:GUARD] == -7).all() and (got_iv[GUARD + batch * masks * 2:] == -7).all()
    inner_iv = got_iv[GUARD:GUARD + batch * masks * 2].reshape(batch, masks, 2)
    if with_intervals and masks:
        assert np.array_equal(inner_iv, want_iv)
    else:
        assert (inner_iv == -7).all()
    expect = np.where(mask, 0, words)                       # +0.0 is the all-zero word
    inner = got[GUARD:GUARD + size].reshape(batch, out_frames, 80)
    wrong = np.argwhere(inner != expect)
    assert not len(wrong), 'first wrong cell (row, frame, column) {} of {}'.format(wrong[0],
                                                                                   len(wrong))
    return want_iv, mask, words


SEAM_LENGTHS = [0, 1, 63, 64, 65, 127, 128, 129]


@pytest.mark.parametrize('out_frames', [1, 63, 64, 65, 128, 129])
def test_spec_augment_row_lengths_on_the_tile_seams(hip, out_frames):
    """Lengths one short of, on and one past a 64-frame tile, clamped to out_frames as the kernel
    clamps them: each alone (B = 1) and all in one batch."""
    for i, length in enumerate(SEAM_LENGTHS):
        _, mask, _ = _spec_run(hip, [length], out_frames, 900 + i, DEFAULTS)
        assert not mask[0, min(length, out_frames):].any()
    _, mask, _ = _spec_run(hip, SEAM_LENGTHS, out_frames, 77, SIXTEEN_EACH)
    assert mask[1:].any() and not mask[0].any()
    _spec_run(hip, SEAM_LENGTHS[::-1], out_frames, 78, DEFAULTS, with_intervals=False)


@pytest.mark.parametrize('seed', sorted(ref.TIME_SEAM_SEEDS))
def test_spec_augment_time_masks_on_the_tile_seams(hip, seed):
    """One time mask of row 0, 129 frames in tiles of 64, 64 and 1: it starts on a seam, ends on
    one, spans three tiles, covers the row, is the last frame alone, or is empty."""
    start, width = ref.TIME_SEAM_SEEDS[seed]
    iv, mask, _ = _spec_run(hip, [129, 129, 64], 129, seed, (0, 27, 1, 200, 1000))
    assert tuple(iv[0, 0]) == (start, width)
    frames = mask[0].all(axis=1)
    assert frames.sum() == width == mask[0].any(axis=1).sum()
    assert frames[start:start + width].all()


@pytest.mark.parametrize('seed', sorted(ref.FREQ_EDGE_SEEDS))
def test_spec_augment_frequency_masks_on_the_outer_columns(hip, seed):
    start, width = ref.FREQ_EDGE_SEEDS[seed]
    iv, mask, _ = _spec_run(hip, [5, 5], 5, seed, (1, 27, 0, 200, 1000))
    assert tuple(iv[0, 0]) == (start, width)
    columns = mask[0].all(axis=0)
    assert columns.sum() == width and columns[start:start + width].all()


@pytest.mark.parametrize('settings', [DEFAULTS, SIXTEEN_EACH], ids=['defaults', 'sixteen_each'])
def test_spec_augment_many_rows_of_two_tiles(hip, settings):
    """B = 257 at 65 frames: workgroup -> (row, tile) with two tiles a row, draw counters
    64 b + ... up to row 256."""
    lengths = np.random.default_rng(5).integers(0, 66, size=257)
    lengths[[0, 1, 2, 255, 256]] = [65, 64, 0, 1, 65]
    iv, mask, _ = _spec_run(hip, lengths, 65, 0xFEDCBA9876543210, settings)
    assert iv[256].any() and mask[256].any() and mask[:, 64].any() and not mask[2].any()


def test_spec_augment_stores_zero_over_any_value_and_reads_none(hip):
    """-0.0, +-inf and NaN inside a mask become the +0 word; outside they keep their bits."""
    cells = np.resize(SPECIALS, 2 * 70 * 80)
    _, mask, words = _spec_run(hip, [70, 70], 70, 31, (2, 27, 2, 20, 1000), cells=cells)
    flat_mask, flat_words = mask.reshape(-1), words.reshape(-1)
    for k in range(len(SPECIALS)):
        assert flat_mask[k::5].any() and not flat_mask[k::5].all()
    assert (flat_words[0::5] == np.int32(-2 ** 31)).all()              # -0.0 went in as itself


def test_spec_augment_serves_a_batch_without_frames(hip):
    """out_frames == 0 (include/ctcasr.h): every row has L = 0, `intervals` is written all zero
    and no cell exists to store to - through the wrapper with an empty tensor, whose address is
    null or not, and at the entry point with a null `features`."""
    lengths = torch.tensor([0, 5, -1], dtype=torch.int32, device=DEV)
    iv, _, _ = _spec_run(hip, [0, 5, -1], 0, 3, DEFAULTS)
    assert iv.shape == (3, 4, 2) and not iv.any()
    empty = torch.empty((3, 0, 80), dtype=torch.float32, device=DEV)
    got = torch.full((3, 4, 2), -7, dtype=torch.int32, device=DEV)
    assert hip.spec_augment(empty, lengths, 3, 2, 27, 2, 100, 1000, got) is empty
    assert not got.cpu().numpy().any()
    got.fill_(-7)
    code = hip.load().ctcasr_spec_augment(None, lengths.data_ptr(), 3, 0, 3, 2, 27, 2, 100, 1000,
                                          got.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert code == 0 and not got.cpu().numpy().any()


# ------------------------------------------------------------------------------------------
# through the pipeline
@pytest.fixture()
def corpus(tmp_path):
    """(The recipe of tests/test_gpu_augment.py.)"""
    from ctc_asr_amd import synth
    from ctc_asr_amd.params import FLAGS
    FLAGS.reset()
    csv = str(tmp_path / 'train.csv')
    synth.write_corpus(str(tmp_path / 'corpus'), csv, [0.9 + 0.03 * i for i in range(8)], seed=3,
                       chars_per_second=5.0)
    FLAGS.update(corpus_dir=str(tmp_path / 'corpus'), train_csv=csv, dev_csv=csv, batch_size=4,
                 num_buckets=2, feature_type='mel', feature_normalization='local',
                 shuffle_buffer_size=8)
    yield FLAGS
    FLAGS.reset()


def _batches(target):
    from ctc_asr_amd import input_functions
    torch.cuda.synchronize()
    got = list(input_functions.input_fn_generator(target, device=DEV, seed=5, prefetch=0)())
    torch.cuda.synchronize()
    return got


def test_pipeline_perturbs_at_percents_of_a_hundred_phases(hip, corpus):
    """--speed_perturb 97,103,199: every training row is the fp32 restatement of its source row
    at the percent its new length reveals, and the batch is as wide as its longest row."""
    percents = (97, 103, 199)
    plain = _batches('train_batch')
    corpus.update(speed_perturb='97,103,199')
    fast = _batches('train_batch')
    assert len(plain) == len(fast) == 2
    seen, tally = set(), _Tally()
    for before, after in zip(plain, fast):
        assert before.features['label_plaintext'] == after.features['label_plaintext']
        src_n, new_n = before.num_samples.cpu().numpy(), after.num_samples.cpu().numpy()
        src, new = before.pcm.cpu().numpy(), after.pcm.cpu().numpy()
        rows, used = [], []
        for i, (n, m) in enumerate(zip(src_n, new_n)):
            fits = [p for p in percents if ref.resample_num_samples(int(n), p) == m]
            assert len(fits) == 1, (n, m)
            rows.append(src[i, :n])
            used.append(fits[0])
        assert new.shape[1] == max(ref.resample_num_samples(len(r), p) for r, p in zip(rows, used))
        _verify(new, new_n, rows, used, tally)
        seen.update(used)
    assert len(seen) >= 2
    print('speed_perturb through the pipeline: {} of {} samples differ from the fp32 restatement'
          .format(tally.mismatches, tally.total))
