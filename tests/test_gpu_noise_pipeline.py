"""Noise mixing through the input pipeline: which batches get it, that nothing else about a batch
moves, that the draws are the reference's and repeat, and that a model trains on the result.

The SNR check is a condition, not a measurement: the speech of the synthetic corpus has a scale of
3000, so rounding the mix to integers moves the ratio of the two powers by far less than 1e-3 dB
(tests/test_noise_host.py checks that margin on the reference); 0.05 dB is the bar here."""

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from tests import noise_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NOISE_LENGTHS = [401, 3000, 20000]


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
    rng = np.random.default_rng(8)
    noise_dir = tmp_path / 'noise'
    noise_dir.mkdir()
    with open(tmp_path / 'noise.csv', 'w', encoding='utf-8') as handle:
        handle.write('path;label;length\n')
        for i, n in enumerate(NOISE_LENGTHS):
            wavfile.write(str(noise_dir / 'n{}.wav'.format(i)), 16000,
                          synth.random_pcm(rng, n, scale=1000.0))
            handle.write('n{}.wav;;{:.3f}\n'.format(i, n / 16000))
    FLAGS.noise_dir = str(noise_dir)
    yield FLAGS, str(tmp_path / 'noise.csv')
    FLAGS.reset()


def _batches(target, prefetch=0):
    from ctc_asr_amd import input_functions
    torch.cuda.synchronize()
    got = list(input_functions.input_fn_generator(target, device=DEV, seed=5,
                                                  prefetch=prefetch)())
    torch.cuda.synchronize()
    return got


def _same(a, b):
    a, b = a.cpu().contiguous().numpy(), b.cpu().contiguous().numpy()
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same_batch(a, b):
    return _same(a.features['spectrogram'], b.features['spectrogram']) and \
        _same(a.features['spectrogram_length'], b.features['spectrogram_length']) and \
        _same(a.pcm, b.pcm) and _same(a.num_samples, b.num_samples) and \
        np.array_equal(a.labels, b.labels) and \
        a.features['label_plaintext'] == b.features['label_plaintext']


def _statuses(batches):
    return np.concatenate([b.noise_draws.cpu().numpy()[:, 0] for b in batches])


def test_flags_off_and_dev_batches_are_what_they_were(hip, corpus):
    flags, noise_csv = corpus
    plain_dev, plain_train = _batches('dev'), _batches('train_batch')
    for batch in plain_dev + plain_train:
        assert batch.noise_draws is None
        feats, lengths = hip.features(batch.pcm, batch.num_samples, 'mel', 'local')
        assert _same(feats, batch.features['spectrogram'])
        assert _same(lengths, batch.features['spectrogram_length'])
    flags.update(noise_csv=noise_csv, noise_permille=1000)
    noisy_dev = _batches('dev')
    assert len(noisy_dev) == len(plain_dev) >= 2
    for a, b in zip(plain_dev, noisy_dev):
        assert b.noise_draws is None and _same_batch(a, b)
    # --noise_permille 0: the kernel's path is taken and nothing changes
    flags.update(noise_permille=0)
    zero = _batches('train_batch')
    assert len(zero) == len(plain_train) == 2
    for a, b in zip(plain_train, zero):
        assert _same_batch(a, b) and not b.noise_draws.cpu().numpy().any()


def test_training_batches_get_the_drawn_noise(hip, corpus):
    from ctc_asr_amd import input_functions, noise
    flags, noise_csv = corpus
    plain = _batches('train_batch')
    flags.update(noise_csv=noise_csv, noise_permille=600)
    noisy, again, threaded = _batches('train_batch'), _batches('train_batch'), \
        _batches('train_batch', prefetch=2)
    assert len(noisy) == len(plain) == 2
    assert set(_statuses(noisy)) == {0, 1}                      # both kinds of row are here
    bank, offsets = noise.load_clips(noise_csv, flags.noise_dir, flags.noise_max_seconds)
    assert list(offsets) == [0] + list(np.cumsum(NOISE_LENGTHS))
    seeds = input_functions._Augmenter(5)
    for a, b, twin, thr in zip(plain, noisy, again, threaded):
        assert a.features['label_plaintext'] == b.features['label_plaintext']
        assert np.array_equal(a.labels, b.labels) and a.audio_seconds == b.audio_seconds
        assert _same(a.num_samples, b.num_samples)
        assert _same(a.features['spectrogram_length'], b.features['spectrogram_length'])
        assert a.features['spectrogram'].shape == b.features['spectrogram'].shape
        # the draws, and through them the clip, its offset and the SNR, are the reference's
        x, y = a.pcm.cpu().numpy(), b.pcm.cpu().numpy()
        nums, draws = a.num_samples.cpu().numpy(), b.noise_draws.cpu().numpy()
        want = ref.mix(x, nums, bank, offsets, seeds.next_noise_seed(), 10, 30, 600)
        assert np.array_equal(draws, want['draws'])
        assert np.abs(y.astype(int) - ref.expected_pcm(x, nums, want).astype(int)).max() <= 1
        for row in range(len(nums)):
            n = int(nums[row])
            if draws[row, 0] != 1:
                assert np.array_equal(y[row], x[row])
                continue
            assert not np.array_equal(y[row], x[row]) and np.array_equal(y[row, n:], x[row, n:])
            assert 10 <= draws[row, 3] <= 30
            if y[row].max() < 32767 and y[row].min() > -32768:
                assert abs(ref.snr_db(x[row, :n], y[row, :n].astype(np.float64)) -
                           draws[row, 3]) < 0.05, row
        # the features are those of the mixed audio
        feats, lengths = hip.features(b.pcm, b.num_samples, 'mel', 'local')
        assert _same(feats, b.features['spectrogram'])
        assert _same(a.features['spectrogram'], b.features['spectrogram']) == \
            (not (draws[:, 0] == 1).any())
        # one seed: the same bits again, with and without the reader thread
        for other in (twin, thr):
            assert _same_batch(b, other) and _same(b.noise_draws, other.noise_draws)


def test_noise_moves_no_mask_and_no_speed(hip, corpus):
    flags, noise_csv = corpus
    flags.update(spec_augment=True, speed_perturb='90,110')
    quiet = _batches('train_batch')
    flags.update(noise_csv=noise_csv, noise_permille=600)
    noisy = _batches('train_batch')
    assert set(_statuses(noisy)) == {0, 1}
    for a, b in zip(quiet, noisy):
        assert _same(a.num_samples, b.num_samples) and a.pcm.shape == b.pcm.shape   # the speeds
        assert _same(a.features['spectrogram_length'], b.features['spectrogram_length'])
        fa, fb = a.features['spectrogram'].cpu().numpy(), b.features['spectrogram'].cpu().numpy()
        za, zb = fa.view(np.int32) == 0, fb.view(np.int32) == 0     # +0.0: the masked cells
        assert za.any() and np.array_equal(za, zb)
        status = b.noise_draws.cpu().numpy()[:, 0]
        x, y = a.pcm.cpu().numpy(), b.pcm.cpu().numpy()
        for row in range(len(status)):
            same = np.array_equal(fa[row].view(np.int32), fb[row].view(np.int32))
            assert same == (status[row] != 1) == np.array_equal(x[row], y[row])
        clean, _ = hip.features(b.pcm, b.num_samples, 'mel', 'local')
        changed = fb.view(np.int32) != clean.cpu().numpy().view(np.int32)
        assert changed.any() and not fb.view(np.int32)[changed].any()


def test_evaluation_noise_is_the_same_at_every_evaluation(hip, corpus):
    flags, noise_csv = corpus
    plain = _batches('dev')
    flags.update(noise_csv=noise_csv, eval_noise_snr_db='10')
    first, second = _batches('dev'), _batches('dev')
    assert len(first) == len(second) == len(plain) >= 2
    # (bucketed targets shuffle by the seed they are given: the same one here)
    for a, b, c in zip(plain, first, second):
        assert _same_batch(b, c) and _same(b.noise_draws, c.noise_draws)
        draws = b.noise_draws.cpu().numpy()
        assert (draws[:, 0] == 1).all() and (draws[:, 3] == 10).all()
        assert _same(a.num_samples, b.num_samples) and np.array_equal(a.labels, b.labels)
        x, y = a.pcm.cpu().numpy(), b.pcm.cpu().numpy()
        for row, n in enumerate(a.num_samples.cpu().numpy()):
            assert abs(ref.snr_db(x[row, :n], y[row, :n].astype(np.float64)) - 10) < 0.05
    # the training noise does not follow the evaluation flag
    train = _batches('train_batch')
    snrs = np.concatenate([b.noise_draws.cpu().numpy() for b in train])
    assert ((snrs[:, 0] == 0) | ((snrs[:, 3] >= 10) & (snrs[:, 3] <= 30))).all()
    flags.update(eval_noise_snr_db='', noise_csv='')
    flags.eval_noise_snr_db = '10'
    with pytest.raises(ValueError, match='noise_csv'):
        _batches('dev')


def test_one_training_step_on_a_noisy_batch(hip, corpus):
    from ctc_asr_amd.engine import Trainer
    from ctc_asr_amd.model import ModelConfig
    flags, noise_csv = corpus
    flags.update(noise_csv=noise_csv, noise_permille=1000, noise_snr_db='5')
    batch = _batches('train_bucket')[0]
    draws = batch.noise_draws.cpu().numpy()
    assert (draws[:, 0] == 1).all() and (draws[:, 3] == 5).all()
    trainer = Trainer(ModelConfig(num_units_rnn=64, num_layers_rnn=1, num_units_dense=32),
                      device=DEV, seed=3)
    loss = trainer.train_step(batch.features['spectrogram'], batch.features['spectrogram_length'],
                              batch.packed_labels)
    value = float(trainer.global_mean(loss))
    trainer.drain_checks()
    assert np.isfinite(value) and value > 0
    assert trainer.skipped_step_count() == 0
