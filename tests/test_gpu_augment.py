"""The augmentation kernels on the GPU against tests/augment_reference.py, and through the input
pipeline.

SpecAugment is exact: the `intervals` output equals the reference's draws and every cell of the
buffer is, bit for bit, either what it was or +0.0 - exactly where the reference says.

Speed perturbation is compared with the float64 resampler.  Bound: 1 LSB on every sample.  The
kernel rounds each tap weight once to fp32 (relative 2^-24) and adds at most 52 products (26 up to
100 %, 28 at 110 %, 52 at 200 %) of |x| <= 32768 in fp32 by fused multiply-adds; with
sum |h| < 3 the weights put the value before rounding off by at most 32768 * 3 * 2^-24 = 0.006 LSB
and the 52 roundings of partial sums below 2^17 by at most 52 * 2^-8 = 0.2 LSB (far less in
practice: the errors do not line up).  Two values less than half an LSB apart round to integers
at most 1 apart.  The share of samples that differ at all is printed, not asserted."""

import numpy as np
import pytest
import torch

from tests import augment_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL_BITS = 0x7FC12345            # a NaN with a payload: survives only if it is never stored to

# (n_freq, freq_width, n_time, time_width, time_permille)
SETTINGS = {
    'defaults': (2, 27, 2, 100, 1000),
    'no_freq': (0, 27, 2, 100, 1000),
    'no_time': (2, 27, 0, 100, 1000),
    'none': (0, 27, 0, 100, 1000),
    'sixteen_each': (16, 27, 16, 100, 1000),
    'whole_band': (2, 80, 2, 100, 1000),
    'time_width_past_length': (2, 27, 2, 5000, 1000),
    'cap_zero': (2, 27, 2, 100, 1),
}


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _spec_case(out_frames, seed=3):
    """Random features, a NaN sentinel in every frame at or beyond its row's length."""
    lengths = np.array([0, 1, 2, 37, 300, out_frames], dtype=np.int32)
    rng = np.random.default_rng(seed)
    feats = rng.normal(size=(6, out_frames, 80)).astype(np.float32)
    bits = feats.view(np.int32)
    for b, length in enumerate(lengths):
        bits[b, length:] = SENTINEL_BITS
    return feats, lengths


# 301 = 4 frame tiles of 64 and 45 frames of a fifth; 320 = 5 whole tiles
@pytest.mark.parametrize('out_frames', [301, 320])
@pytest.mark.parametrize('name', sorted(SETTINGS))
def test_spec_augment_matches_the_reference_cell_for_cell(hip, name, out_frames):
    n_freq, freq_width, n_time, time_width, permille = SETTINGS[name]
    seed = 0x1234567887654321 + sorted(SETTINGS).index(name)
    feats, lengths = _spec_case(out_frames)
    want_iv = ref.mask_intervals(seed, lengths, out_frames, n_freq, freq_width, n_time,
                                 time_width, permille)
    mask = ref.mask_cells(want_iv, lengths, out_frames, n_freq)
    assert not mask[0].any()
    if name == 'cap_zero':
        assert not want_iv[:, n_freq:, 1].any()
    # one NaN inside a mask and one outside, in the valid frames of the 300-frame row
    inside, outside = np.argwhere(mask[4, :300]), np.argwhere(~mask[4, :300])
    for cells in (inside, outside):
        if len(cells):
            feats[4, cells[len(cells) // 2][0], cells[len(cells) // 2][1]] = np.nan
    before = feats.view(np.int32).copy()
    x = torch.from_numpy(feats).to(DEV)
    iv = torch.full((6, n_freq + n_time, 2), -7, dtype=torch.int32, device=DEV)
    out = hip.spec_augment(x, torch.from_numpy(lengths).to(DEV), seed, n_freq, freq_width,
                           n_time, time_width, permille, iv)
    assert out is x
    if n_freq + n_time:
        assert np.array_equal(iv.cpu().numpy(), want_iv)
    expect = np.where(mask, 0, before)            # +0.0 is the all-zero word
    got = _bits(x)
    assert np.array_equal(got, expect)
    if name == 'none':
        assert np.array_equal(got, before)
    else:
        assert mask.any()
    # the intervals are optional
    y = torch.from_numpy(before.view(np.float32)).to(DEV)
    hip.spec_augment(y, torch.from_numpy(lengths).to(DEV), seed, n_freq, freq_width, n_time,
                     time_width, permille)
    assert np.array_equal(_bits(y), expect)


def test_spec_augment_is_a_function_of_the_seed(hip):
    feats, lengths = _spec_case(301)
    len_d = torch.from_numpy(lengths).to(DEV)
    runs = []
    for seed in (11, 11, 12):
        x = torch.from_numpy(feats).to(DEV)
        iv = torch.empty((6, 4, 2), dtype=torch.int32, device=DEV)
        hip.spec_augment(x, len_d, seed, 2, 27, 2, 100, 1000, iv)
        runs.append((_bits(x), iv.cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert not np.array_equal(runs[0][1], runs[2][1])
    assert not np.array_equal(runs[0][0], runs[2][0])
    # seeds are taken modulo 2^64, as the dropout seeds are
    x = torch.from_numpy(feats).to(DEV)
    hip.spec_augment(x, len_d, 11 + (1 << 64), 2, 27, 2, 100, 1000)
    assert np.array_equal(_bits(x), runs[0][0])


def test_spec_augment_clamps_lengths_into_the_buffer(hip):
    """A length past out_frames counts as out_frames, a negative one as 0: nothing is stored
    outside the row."""
    feats = np.ones((3, 70, 80), dtype=np.float32)
    lengths = np.array([500, -3, 70], dtype=np.int32)
    x = torch.from_numpy(feats).to(DEV)
    iv = torch.empty((3, 4, 2), dtype=torch.int32, device=DEV)
    hip.spec_augment(x, torch.from_numpy(lengths).to(DEV), 5, 2, 27, 2, 100, 1000, iv)
    want_iv = ref.mask_intervals(5, lengths, 70, 2, 27, 2, 100, 1000)
    assert np.array_equal(iv.cpu().numpy(), want_iv)
    assert np.array_equal(want_iv[0], ref.mask_intervals(5, [70], 70, 2, 27, 2, 100, 1000)[0])
    mask = ref.mask_cells(want_iv, lengths, 70, 2)
    assert np.array_equal(x.cpu().numpy(), np.where(mask, 0.0, 1.0).astype(np.float32))
    assert not mask[1].any()


# ------------------------------------------------------------------------------------------
PERCENTS = [90, 100, 110, 50, 200]
COUNTS = [1, 400, 401, 16000, 4097]


@pytest.fixture(scope='module')
def pcm_rows():
    """Full-scale random int16 rows, one per count, and their float64 results at every percent
    (computed once)."""
    rng = np.random.default_rng(21)
    rows = {n: rng.integers(-32768, 32768, size=n).astype(np.int16) for n in COUNTS}
    square = (32767 * np.where((np.arange(4097) // 20) % 2 == 0, 1, -1)).astype(np.int16)
    rows['square'] = square
    expect = {(key, p): ref.speed_perturb(row, p) for key, row in rows.items() for p in PERCENTS}
    return rows, expect


def _run(hip, rows, percents, max_in=None, max_out=None, fill=0):
    max_in = max_in or max(len(r) for r in rows)
    pcm = np.full((len(rows), max_in), fill, dtype=np.int16)
    for i, row in enumerate(rows):
        pcm[i, :len(row)] = row
    counts = np.array([len(r) for r in rows], dtype=np.int32)
    out, out_n = hip.speed_perturb(torch.from_numpy(pcm).to(DEV), torch.from_numpy(counts).to(DEV),
                                   torch.tensor(percents, dtype=torch.int32, device=DEV), max_out)
    return out.cpu().numpy(), out_n.cpu().numpy()


def _compare(out, out_n, keys, percents, rows, expect):
    differing = total = 0
    for i, (key, percent) in enumerate(zip(keys, percents)):
        want = expect[(key, percent)]
        assert out_n[i] == len(want) == ref.resample_num_samples(len(rows[key]), percent)
        assert not out[i, len(want):].any(), (key, percent)              # zero padding
        diff = np.abs(out[i, :len(want)].astype(np.int64) - want.astype(np.int64))
        if percent == 100:
            assert np.array_equal(out[i, :len(want)], rows[key])          # a bit copy
        assert diff.max() <= 1, (key, percent, int(diff.max()))
        differing += int((diff > 0).sum())
        total += len(want)
    return differing, total


def test_speed_perturb_each_row_alone(hip, pcm_rows):
    rows, expect = pcm_rows
    for n, percent in zip(COUNTS, PERCENTS):
        out, out_n = _run(hip, [rows[n]], [percent])
        assert out.shape == (1, 2 * n)                   # sized for the slowest speed served
        _compare(out, out_n, [n], [percent], rows, expect)


def test_speed_perturb_mixed_batches(hip, pcm_rows):
    rows, expect = pcm_rows
    out, out_n = _run(hip, [rows[n] for n in COUNTS], PERCENTS, fill=-1)
    differing, total = _compare(out, out_n, COUNTS, PERCENTS, rows, expect)
    # every count at every percent, in one batch, sized from the host-side lengths
    keys = [n for n in COUNTS for _ in PERCENTS]
    percents = PERCENTS * len(COUNTS)
    max_out = max(ref.resample_num_samples(n, p) for n, p in zip(keys, percents))
    out, out_n = _run(hip, [rows[k] for k in keys], percents, max_out=max_out, fill=-1)
    assert out.shape == (25, 32000)
    more = _compare(out, out_n, keys, percents, rows, expect)
    differing, total = differing + more[0], total + more[1]
    print('speed_perturb: {} of {} samples differ from the float64 reference ({:.4%})'
          .format(differing, total, differing / total))


def test_speed_perturb_saturates(hip, pcm_rows):
    rows, expect = pcm_rows
    percents = [90, 110, 50, 200, 100]
    out, out_n = _run(hip, [rows['square']] * 5, percents)
    _compare(out, out_n, ['square'] * 5, percents, rows, expect)
    for i, percent in enumerate(percents[:2]):
        raw = ref.resample_float64(rows['square'], percent)
        assert raw.max() > 32768 and raw.min() < -32769          # the overshoot at the edges clips
        assert out[i].max() == 32767 and out[i].min() == -32768
        hit = raw > 32768.5
        assert (out[i, :len(raw)][hit] == 32767).all()


def test_speed_perturb_bad_rows_and_clipping(hip, pcm_rows):
    rows, expect = pcm_rows
    pcm = np.full((4, 500), 1234, dtype=np.int16)
    pcm[3, :401] = rows[401]
    counts = torch.tensor([0, 400, 501, 401], dtype=torch.int32, device=DEV)
    percents = torch.tensor([90, 49, 110, 90], dtype=torch.int32, device=DEV)
    out, out_n = hip.speed_perturb(torch.from_numpy(pcm).to(DEV), counts, percents)
    out, out_n = out.cpu().numpy(), out_n.cpu().numpy()
    assert list(out_n) == [0, 0, 0, 445]
    assert not out[:3].any() and not out[3, 445:].any()
    assert np.abs(out[3, :445].astype(int) - expect[(401, 90)].astype(int)).max() <= 1
    percents[1] = 201
    counts[0] = -5
    out2, out_n2 = hip.speed_perturb(torch.from_numpy(pcm).to(DEV), counts, percents, max_out=100)
    assert out_n2.cpu().tolist() == [0, 0, 0, 100]                   # cut to max_out, and says so
    assert np.array_equal(out2.cpu().numpy()[3], out[3, :100]) and not out2[:3].cpu().numpy().any()


# ------------------------------------------------------------------------------------------
@pytest.fixture()
def corpus(tmp_path):
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


def _batches(target, prefetch=0):
    from ctc_asr_amd import input_functions
    torch.cuda.synchronize()
    got = list(input_functions.input_fn_generator(target, device=DEV, seed=5,
                                                  prefetch=prefetch)())
    torch.cuda.synchronize()
    return got


def _same(a, b):
    """Bit equality of two device tensors of one dtype."""
    a, b = a.cpu().contiguous().numpy(), b.cpu().contiguous().numpy()
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_pipeline_augments_training_batches_only(hip, corpus):
    flags = corpus
    plain_dev, plain_train = _batches('dev'), _batches('train_batch')
    flags.update(spec_augment=True, speed_perturb='90,110')
    aug_dev, aug_train, again = _batches('dev'), _batches('train_batch'), _batches('train_batch')
    threaded = _batches('train_batch', prefetch=2)
    assert len(plain_dev) == len(aug_dev) >= 2 and len(plain_train) == len(aug_train) == 2
    for a, b in zip(plain_dev, aug_dev):
        assert _same(a.features['spectrogram'], b.features['spectrogram'])
        assert _same(a.features['spectrogram_length'], b.features['spectrogram_length'])
        assert _same(a.pcm, b.pcm) and np.array_equal(a.labels, b.labels)
    for plain, aug, twin, thr in zip(plain_train, aug_train, again, threaded):
        # the same utterances in the same order, their labels untouched
        assert plain.features['label_plaintext'] == aug.features['label_plaintext']
        assert np.array_equal(plain.labels, aug.labels)
        assert plain.audio_seconds == aug.audio_seconds          # source seconds
        src = plain.num_samples.cpu().numpy()
        new = aug.num_samples.cpu().numpy()
        assert all(m in (n * 100 // 90, n * 100 // 110) for n, m in zip(src, new))
        assert aug.pcm.shape[1] == new.max()                     # sized from the host's lengths
        a_len = aug.features['spectrogram_length'].cpu().numpy()
        assert not np.array_equal(a_len, plain.features['spectrogram_length'].cpu().numpy())
        assert [hip.features_num_frames(int(m)) for m in new] == list(a_len)
        # the features: those of the perturbed audio, with cells set to +0.0 and nothing else
        clean, _ = hip.features(aug.pcm, aug.num_samples, 'mel', 'local')
        got, base = _bits(aug.features['spectrogram']), _bits(clean)
        changed = got != base
        assert changed.any() and not got[changed].any()
        assert not _same(aug.features['spectrogram'], plain.features['spectrogram'])
        # one seed: the same batches bit for bit, with and without the reader thread
        for other in (twin, thr):
            assert _same(aug.features['spectrogram'], other.features['spectrogram'])
            assert _same(aug.pcm, other.pcm) and _same(aug.num_samples, other.num_samples)


def test_one_training_step_on_an_augmented_batch(hip, corpus):
    from ctc_asr_amd.engine import Trainer
    from ctc_asr_amd.model import ModelConfig
    corpus.update(spec_augment=True, speed_perturb='90,100,110')
    batch = _batches('train_bucket')[0]
    trainer = Trainer(ModelConfig(num_units_rnn=64, num_layers_rnn=1, num_units_dense=32),
                      device=DEV, seed=3)
    loss = trainer.train_step(batch.features['spectrogram'], batch.features['spectrogram_length'],
                              batch.packed_labels)
    value = float(trainer.global_mean(loss))
    trainer.drain_checks()
    assert np.isfinite(value) and value > 0
