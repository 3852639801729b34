"""Reverberation through the input pipeline: which batches get it, that nothing else about a
batch moves, that the samples and the draws are the reference's bit for bit, that the noise goes
in behind it, and that a model trains on the result.

The noise behind the reverberation is judged twice.  Exactly, against `hip.noise_mix` called
here on the reference's reverberated audio with the seed the iterator used.  And against
tests/noise_reference.py within what `ctcasr_noise_mix` pins - its gain is held to one fp32 ulp
of the float64 gain, not to its bits, so a mixed sample may sit 1 off the float64 mix (the bound
of tests/test_gpu_noise_pipeline.py); the reverberation itself gets no such margin."""

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from tests import noise_reference as noise_ref
from tests import reverb_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NOISE_LENGTHS = [401, 3000, 20000]
ROOMS = [(0.02, 500), (0.08, 2500), (0.3, 7000)]          # (T60 in s, samples) of the responses


@pytest.fixture()
def corpus(tmp_path):
    from ctc_asr_amd import synth
    from ctc_asr_amd.params import FLAGS
    FLAGS.reset()
    csv = str(tmp_path / 'train.csv')
    synth.write_corpus(str(tmp_path / 'corpus'), csv, [0.9 + 0.03 * i for i in range(8)], seed=3,
                       chars_per_second=5.0)
    FLAGS.update(corpus_dir=str(tmp_path / 'corpus'), train_csv=csv, dev_csv=csv, test_csv=csv,
                 batch_size=4, num_buckets=2, feature_type='mel', feature_normalization='local',
                 shuffle_buffer_size=8)
    rng = np.random.default_rng(8)
    for folder, name, clips in (
            ('noise', 'noise.csv', [synth.random_pcm(rng, n, scale=1000.0) for n in NOISE_LENGTHS]),
            ('rir', 'rir.csv', [ref.synthetic_rir(rng, t60, taps) for t60, taps in ROOMS])):
        (tmp_path / folder).mkdir()
        with open(tmp_path / name, 'w', encoding='utf-8') as handle:
            handle.write('path;label;length\n')
            for i, clip in enumerate(clips):
                wavfile.write(str(tmp_path / folder / 'c{}.wav'.format(i)), 16000, clip)
                handle.write('c{}.wav;;{:.3f}\n'.format(i, len(clip) / 16000))
    FLAGS.noise_dir, FLAGS.rir_dir = str(tmp_path / 'noise'), str(tmp_path / 'rir')
    yield FLAGS, str(tmp_path / 'rir.csv'), str(tmp_path / 'noise.csv')
    FLAGS.reset()


@pytest.fixture()
def calls(hip, monkeypatch):
    """Counts the calls of `hip.reverb` that the pipeline makes."""
    made = []
    real = hip.reverb

    def counted(*args, **kwargs):
        made.append(1)
        return real(*args, **kwargs)

    monkeypatch.setattr(hip, 'reverb', counted)
    return made


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
        np.array_equal(a.labels, b.labels) and a.audio_seconds == b.audio_seconds and \
        a.features['label_plaintext'] == b.features['label_plaintext']


def _bank(flags, rir_csv):
    from ctc_asr_amd import reverb
    return ref.Bank(*reverb.load_rirs(rir_csv, flags.rir_dir, flags.rir_max_taps))


def test_flag_off_dev_and_test_batches_are_what_they_were(hip, corpus, calls):
    from ctc_asr_amd import input_functions
    flags, rir_csv, _ = corpus
    plain = {target: _batches(target) for target in ('train_batch', 'dev', 'test')}
    assert not calls and len(plain['train_batch']) == 2
    # ... bit for bit the batches of the path that knows no augmentation at all
    bare = [input_functions._make_batch(items, torch.device(DEV, torch.cuda.current_device()))
            for items in input_functions.host_batches(flags.train_csv, False, [], seed=5)]
    assert len(bare) == 2
    for a, b in zip(bare, plain['train_batch']):
        assert _same_batch(a, b) and b.reverb_draws is None and b.noise_draws is None
    flags.update(rir_csv=rir_csv, rir_permille=1000)
    for target in ('dev', 'test'):
        again = _batches(target)
        assert len(again) == len(plain[target]) >= 2
        for a, b in zip(plain[target], again):
            assert _same_batch(a, b) and b.reverb_draws is None
    assert not calls
    wet = _batches('train_batch')
    assert len(calls) == len(wet) == 2
    for a, b in zip(plain['train_batch'], wet):
        assert (b.reverb_draws.cpu().numpy()[:, 0] == 1).all() and not _same(a.pcm, b.pcm)
    # --rir_permille 0: the call is made and nothing changes
    flags.update(rir_permille=0)
    for a, b in zip(plain['train_batch'], _batches('train_batch')):
        assert _same_batch(a, b) and not b.reverb_draws.cpu().numpy().any()
    assert len(calls) == 4


def test_training_batches_are_the_reference_on_the_perturbed_audio(hip, corpus, calls):
    from ctc_asr_amd import input_functions
    flags, rir_csv, _ = corpus
    flags.update(speed_perturb='90,110')
    dry = _batches('train_bucket')
    flags.update(rir_csv=rir_csv, rir_permille=600)
    wet, again, threaded = _batches('train_bucket'), _batches('train_bucket'), \
        _batches('train_bucket', prefetch=2)
    assert len(wet) == len(dry) >= 2 and len(calls) == 3 * len(wet)
    bank = _bank(flags, rir_csv)
    assert len(bank.delay) == 3 and (bank.delay == 32).all()
    seeds = input_functions._Augmenter(5)
    statuses = set()
    for a, b, twin, thr in zip(dry, wet, again, threaded):
        # composition, lengths and labels: as without the flag
        assert a.features['label_plaintext'] == b.features['label_plaintext']
        assert np.array_equal(a.labels, b.labels) and a.audio_seconds == b.audio_seconds
        assert _same(a.num_samples, b.num_samples) and a.pcm.shape == b.pcm.shape
        assert _same(a.features['spectrogram_length'], b.features['spectrogram_length'])
        x, nums = a.pcm.cpu().numpy(), a.num_samples.cpu().numpy()
        want, want_draws = ref.reverb_rows(x, nums, bank, seeds.next_reverb_seed(), 600)
        assert np.array_equal(b.reverb_draws.cpu().numpy(), want_draws)
        assert b.pcm.cpu().numpy().tobytes() == want.tobytes()
        statuses |= set(want_draws[:, 0])
        for row in np.flatnonzero(want_draws[:, 0] == 1):
            assert not np.array_equal(want[row, :nums[row]], x[row, :nums[row]])
        # the features are those of the reverberated audio
        feats, lengths = hip.features(b.pcm, b.num_samples, 'mel', 'local')
        assert _same(feats, b.features['spectrogram'])
        # one seed: the same bits again, with and without the reader thread
        for other in (twin, thr):
            assert _same_batch(b, other) and _same(b.reverb_draws, other.reverb_draws)
    assert statuses == {0, 1}                                    # both kinds of row are here


def test_the_noise_goes_in_behind_the_reverberation(hip, corpus):
    from ctc_asr_amd import input_functions, noise
    flags, rir_csv, noise_csv = corpus
    flags.update(speed_perturb='90,110', spec_augment=True)
    dry = _batches('train_batch')
    flags.update(noise_csv=noise_csv, noise_permille=600)
    noisy = _batches('train_batch')
    flags.update(rir_csv=rir_csv, rir_permille=600)
    both = _batches('train_batch')
    bank = _bank(flags, rir_csv)
    clips, offsets = noise.load_clips(noise_csv, flags.noise_dir, flags.noise_max_seconds)
    seeds = input_functions._Augmenter(5)
    mixed = reverberated = 0
    for a, n, b in zip(dry, noisy, both):
        # the reverberation moves no speed, no noise draw and no mask
        assert _same(a.num_samples, b.num_samples) and a.pcm.shape == b.pcm.shape
        assert _same(n.noise_draws, b.noise_draws)
        fa, fb = a.features['spectrogram'].cpu().numpy(), b.features['spectrogram'].cpu().numpy()
        assert np.array_equal(fa.view(np.int32) == 0, fb.view(np.int32) == 0)
        x, nums = a.pcm.cpu().numpy(), a.num_samples.cpu().numpy()
        wet, want_draws = ref.reverb_rows(x, nums, bank, seeds.next_reverb_seed(), 600)
        assert np.array_equal(b.reverb_draws.cpu().numpy(), want_draws)
        noise_seed = seeds.next_noise_seed()
        got = b.pcm.cpu().numpy()
        exact = hip.noise_mix(torch.from_numpy(wet).to(DEV), a.num_samples,
                              torch.from_numpy(clips).to(DEV), torch.from_numpy(offsets).to(DEV),
                              noise_seed, 10, 30, 600)
        assert got.tobytes() == exact.cpu().numpy().tobytes()
        want = noise_ref.mix(wet, nums, clips, offsets, noise_seed, 10, 30, 600)
        assert np.array_equal(b.noise_draws.cpu().numpy(), want['draws'])
        expected = noise_ref.expected_pcm(wet, nums, want)
        assert np.abs(got.astype(int) - expected.astype(int)).max() <= 1
        mixed += int((want['draws'][:, 0] == 1).sum())
        reverberated += int((want_draws[:, 0] == 1).sum())
    assert 0 < mixed < 8 and 0 < reverberated < 8


def test_one_training_step_on_a_reverberated_noisy_batch(hip, corpus):
    from ctc_asr_amd.engine import Trainer
    from ctc_asr_amd.model import ModelConfig
    flags, rir_csv, noise_csv = corpus
    flags.update(rir_csv=rir_csv, rir_permille=1000, noise_csv=noise_csv, noise_permille=1000)
    batch = _batches('train_bucket')[0]
    assert (batch.reverb_draws.cpu().numpy()[:, 0] == 1).all()
    assert (batch.noise_draws.cpu().numpy()[:, 0] == 1).all()
    trainer = Trainer(ModelConfig(num_units_rnn=64, num_layers_rnn=1, num_units_dense=32),
                      device=DEV, seed=3)
    loss = trainer.train_step(batch.features['spectrogram'], batch.features['spectrogram_length'],
                              batch.packed_labels)
    value = float(trainer.global_mean(loss))
    trainer.drain_checks()
    assert np.isfinite(value) and value > 0
    assert trainer.skipped_step_count() == 0
