"""``--resample_input`` through the drivers, on a tiny model with random weights.  One synthetic
16 kHz utterance is turned into a 48 kHz stereo int16 file and a 44.1 kHz mono float32 file.
`read_audio` of each must be `hip.resample` of its samples; and predict, transcribe, align and the
two banks with the flag on the original file must give what they give without the flag on that
result written out as a 16 kHz mono WAV - the same launches on the same data, so every comparison
is exact."""

import json

import numpy as np
import pytest
import torch
from scipy import signal
from scipy.io import wavfile

pytestmark = pytest.mark.gpu
RATE = 16000


def _utterance(seconds=4.0, seed=41):
    """A noise floor of rms 30 and two bursts of rms 3000 (what `vad.segment` cuts at)."""
    rng = np.random.default_rng(seed)
    n = int(seconds * RATE) + 33
    rms = np.full(n, 30.0)
    for begin, end in ((0.5, 1.4), (2.1, 3.6)):
        rms[int(begin * RATE):int(end * RATE)] = 3000.0
    return rng.normal(size=n) * rms


def _manifest(path, names, labels=None):
    with open(path, 'w', encoding='utf-8') as handle:
        handle.write('path;label;length\n')
        for i, name in enumerate(names):
            handle.write('{};{};1.0\n'.format(name, labels[i] if labels else 'x'))
    return str(path)


@pytest.fixture(scope='module')
def setup(tmp_path_factory, hip):
    from ctc_asr_amd.model import CTCModel, ModelConfig, init_params
    from ctc_asr_amd.params import FLAGS
    FLAGS.reset()
    FLAGS.update(feature_type='mel', feature_normalization='local', batch_size=3,
                 max_segment_seconds=2, beam_width=8)
    folder = tmp_path_factory.mktemp('resample')
    x = _utterance()
    up48 = signal.resample_poly(x, 3, 1)
    stereo = np.stack([up48 * 0.9, up48 * 0.7 + np.random.default_rng(2).normal(size=len(up48))],
                      axis=1)
    files = {
        'a48.wav': (48000, np.clip(np.rint(stereo), -32768, 32767).astype(np.int16)),
        'b441.wav': (44100, (signal.resample_poly(x, 441, 160) / 32768.0).astype(np.float32)),
    }
    converted = {}
    for name, (rate, samples) in files.items():
        wavfile.write(str(folder / name), rate, samples)
        converted[name] = hip.resample(torch.from_numpy(samples).cuda(), rate)
        wavfile.write(str(folder / ('c_' + name)), RATE, converted[name].cpu().numpy())
    cfg = ModelConfig(used_model='ds2', conv_filters=(32, 32), rnn_cell='lstm', cudnn=True,
                      num_units_dense=64, num_layers_rnn=1, num_units_rnn=64,
                      dense_dropout_rate=0.0, beam_width=8)
    params = init_params(cfg, 3)
    params['logits/kernel'] = params['logits/kernel'] * 60.0    # random, but decisive: it emits labels
    model = CTCModel(cfg, 'cuda', params=params)
    yield model, folder, files, converted
    FLAGS.reset()


class _Flag:
    """``--resample_input`` for the length of a ``with``."""

    def __enter__(self):
        from ctc_asr_amd.params import FLAGS
        FLAGS.resample_input = True

    def __exit__(self, *exc):
        from ctc_asr_amd.params import FLAGS
        FLAGS.resample_input = False
        return False


def test_read_audio_is_resample_of_the_files_samples(setup, hip):
    from ctc_asr_amd import input_functions as inp
    _, folder, files, converted = setup
    for name, (rate, samples) in files.items():
        got = inp.read_audio(str(folder / name), 'cuda')
        assert got.is_cuda and got.dtype == torch.int16 and got.dim() == 1
        assert got.numel() == hip.resample_out_samples(len(samples), rate) >= 4 * RATE
        assert torch.equal(got, converted[name])
        # the file written from it is 16 kHz mono int16: read_audio and read_wav agree on it
        plain = inp.read_wav(str(folder / ('c_' + name)))
        assert np.array_equal(plain, converted[name].cpu().numpy())
        assert np.array_equal(inp.read_audio(str(folder / ('c_' + name)), 'cuda').cpu().numpy(),
                              plain)
    # the two files carry one utterance, so their conversions are alike: not equal - two host
    # up-samplers with their own transition bands made the files - but a swapped channel, a lost
    # gain or a shift by one sample of this white signal would each cost more than its own rms
    a = converted['a48.wav'].cpu().numpy().astype(np.float64)
    b = converted['b441.wav'].cpu().numpy().astype(np.float64)
    n = min(len(a), len(b))
    apart = np.sqrt(np.mean((a[:n] / 0.8 - b[:n]) ** 2)) / np.sqrt(np.mean(b ** 2))
    print('the two conversions of one utterance: relative rms distance {:.4f}'.format(apart))
    assert abs(len(a) - len(b)) <= 1 and apart < 0.2


@pytest.mark.parametrize('name', ['a48.wav', 'b441.wav'])
def test_predict_and_transcribe(setup, name):
    from ctc_asr_amd import predict, transcribe
    model, folder, _, converted = setup
    original, plain = str(folder / name), str(folder / ('c_' + name))
    with pytest.raises(RuntimeError, match='Sampling rate is'):
        predict.predict(model, original)                       # without the flag: as ever
    with pytest.raises(RuntimeError, match='Sampling rate is'):
        transcribe.transcribe(model, original)
    want = predict.predict(model, plain, timestamps=True)
    want_long = transcribe.transcribe(model, plain, timestamps=True)
    with _Flag():
        got = predict.predict(model, original, timestamps=True)
        got_long = transcribe.transcribe(model, original, timestamps=True)
    assert got['decoded'].tolist() == want['decoded'].tolist() and len(want['decoded']) > 0
    assert got['plaintext'] == want['plaintext'] and got['words'] == want['words']
    assert got_long == want_long and json.loads(json.dumps(got_long)) == got_long
    assert len(got_long['segments']) >= 2 and got_long['plaintext']
    assert got_long['audio_seconds'] == converted[name].numel() / RATE     # the converted length
    assert 4.0 <= got_long['audio_seconds'] < 4.01                          # seconds of the recording
    assert any(piece['words'] for piece in got_long['segments'])


def test_align(setup):
    from ctc_asr_amd import align
    model, folder, _, _ = setup
    labels = ['ab c', 'de']
    originals = [{'path': name, 'label': label}
                 for name, label in zip(('a48.wav', 'b441.wav'), labels)]
    plains = [{'path': 'c_' + row['path'], 'label': row['label']} for row in originals]
    with pytest.raises(RuntimeError, match='Sampling rate is'):
        list(align.align_rows(model, originals, str(folder), 2))
    want = list(align.align_rows(model, plains, str(folder), 2))
    with _Flag():
        got = list(align.align_rows(model, originals, str(folder), 2))
    assert [row.pop('path') for row in got] == ['a48.wav', 'b441.wav']
    assert [row.pop('path') for row in want] == ['c_a48.wav', 'c_b441.wav']
    assert got == want and len(got) == 2
    assert all(row['status'] == 'ok' and row['words'] for row in got)


def test_the_banks(setup, hip):
    from ctc_asr_amd import noise, reverb
    _, folder, _, _ = setup
    rng = np.random.default_rng(9)
    clip = (rng.normal(size=(30000, 2)) * 2000).astype(np.int16)            # 44.1 kHz stereo
    decay = np.exp(-np.arange(3000) / 400.0)
    rir = (rng.normal(size=3000) * decay * 0.3).astype(np.float32)           # 48 kHz float32
    rir[40] = 0.9
    wavfile.write(str(folder / 'clip.wav'), 44100, clip)
    wavfile.write(str(folder / 'rir.wav'), 48000, rir)
    for name, rate, samples in (('clip.wav', 44100, clip), ('rir.wav', 48000, rir)):
        wavfile.write(str(folder / ('c_' + name)), RATE,
                      hip.resample(torch.from_numpy(samples).cuda(), rate).cpu().numpy())
    clips = _manifest(folder / 'clips.csv', ['clip.wav', 'c_a48.wav'])
    plain_clips = _manifest(folder / 'plain_clips.csv', ['c_clip.wav', 'c_a48.wav'])
    rirs = _manifest(folder / 'rirs.csv', ['rir.wav'])
    plain_rirs = _manifest(folder / 'plain_rirs.csv', ['c_rir.wav'])
    with pytest.raises(RuntimeError, match='Sampling rate is 44,100'):
        noise.load_clips(clips, str(folder), 3600)
    with pytest.raises(RuntimeError, match='Sampling rate is 48,000'):
        reverb.load_rirs(rirs, str(folder))
    want_bank = noise.load_clips(plain_clips, str(folder), 3600)
    want_rirs = reverb.load_rirs(plain_rirs, str(folder))
    with _Flag():
        got_bank = noise.load_clips(clips, str(folder), 3600, 'cuda')
        got_rirs = reverb.load_rirs(rirs, str(folder), device='cuda')
        cut = noise.load_clips(clips, str(folder), 1)                       # seconds of CONVERTED audio
    assert len(got_bank) == len(want_bank) == 2 and len(got_rirs) == len(want_rirs) == 4
    for got, want in zip(got_bank + got_rirs, want_bank + want_rirs):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    assert got_bank[1][1] == 30000 * 160 // 441 and got_bank[0].dtype == np.int16
    assert list(cut[1]) == [0, 10884, 16000]
