"""`transcribe.transcribe` on a tiny model with random weights: the table of pieces equals the
reference's, and every piece's labels, text and word times equal what the same pieces give when
the batches are rebuilt on the host - numpy slices of the table in the same order through
`features_from_pcm`, `inference_fn` and `decode_fn` per batch.  Those are the same launches on the
same data, and `decode_many` is documented as identical to per-batch decoding, so every comparison
is exact."""

import json

import numpy as np
import pytest
from scipy.io import wavfile

from tests import vad_reference as ref

pytestmark = pytest.mark.gpu
RATE = 16000
SETTINGS = dict(margin_db=9, floor_permille=100, min_rms=16, rms=0, pad=20, min_raw=5,
                max_segment=200)
BATCH = 3


def _recording(seconds=12.0, seed=31):
    """A noise floor of rms 30 and four bursts of rms 3000, the third longer than two seconds;
    the length is no multiple of a hop."""
    rng = np.random.default_rng(seed)
    n = int(seconds * RATE) + 77
    rms = np.full(n, 30.0)
    for begin, end in ((0.8, 1.6), (2.4, 3.1), (4.0, 8.3), (9.5, 10.9)):
        rms[int(begin * RATE):int(end * RATE)] = 3000.0
    return np.clip(rng.normal(size=n) * rms, -32768, 32767).astype(np.int16)


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    from ctc_asr_amd.model import CTCModel, ModelConfig, init_params
    from ctc_asr_amd.params import FLAGS
    FLAGS.reset()
    FLAGS.update(feature_type='mel', feature_normalization='local', batch_size=BATCH,
                 max_segment_seconds=2)
    folder = tmp_path_factory.mktemp('transcribe')
    audio = _recording()
    wavfile.write(str(folder / 'long.wav'), RATE, audio)
    wavfile.write(str(folder / 'silent.wav'), RATE,
                  np.random.default_rng(1).integers(-3, 4, size=3 * RATE).astype(np.int16))
    cfg = ModelConfig(used_model='ds2', conv_filters=(32, 32), rnn_cell='lstm', cudnn=True,
                      num_units_dense=64, num_layers_rnn=1, num_units_rnn=64,
                      dense_dropout_rate=0.0, beam_width=8)
    params = init_params(cfg, 3)
    params['logits/kernel'] = params['logits/kernel'] * 60.0    # random, but decisive: it emits labels
    model = CTCModel(cfg, 'cuda', params=params)
    energies = ref.energy(audio)
    table = ref.table(energies, ref.histogram(energies), len(audio), **SETTINGS)
    yield model, folder, audio, table
    FLAGS.reset()


def _by_hand(model, audio, table, timestamps):
    """Per piece in time order: (labels, text, words) from batches rebuilt on the host."""
    from ctc_asr_amd import alignment
    from ctc_asr_amd.input_functions import features_from_pcm
    start, length, _ = table
    order = sorted(range(len(start)), key=lambda i: (-int(length[i]), i))
    hop = alignment.frame_seconds(model.cfg, False)
    result = {}
    for first in range(0, len(order), BATCH):
        rows = order[first:first + BATCH]
        feats, lengths = features_from_pcm(
            [audio[int(start[i]):int(start[i]) + int(length[i])] for i in rows], model.device)
        logits, seq_len = model.inference_fn(feats, lengths, training=False)
        model.check_rnn_error()
        decoded, plaintext, _ = model.decode_fn(logits, seq_len, None)
        words = [None] * len(rows)
        if timestamps:
            ids = [[v for v in labels if v != 0] for labels in decoded]
            path, _, frame_logp, _ = model.align_fn(logits, seq_len, ids)
            for b in range(len(rows)):
                words[b] = alignment.segments(path[b].cpu().numpy(), ids[b], hop,
                                              frame_logp[b].cpu().numpy())
        for b, i in enumerate(rows):
            result[i] = (decoded[b], plaintext[b], words[b])
    return [result[i] for i in range(len(start))]


def test_the_table_is_the_references(setup):
    from ctc_asr_amd import transcribe
    model, folder, audio, table = setup
    report = {}
    got = transcribe.transcribe(model, str(folder / 'long.wav'), report=report)
    start, length, thr = table
    assert report['start'].tolist() == start.tolist()
    assert report['length'].tolist() == length.tolist() and report['threshold'] == thr
    # four bursts, the long one cut: every piece within the cap, the padding of 0.2 s shows
    assert len(start) >= 6 and (length <= 2 * RATE).all() and (length >= 3 * ref.HOP).all()
    assert start[0] == int(0.8 * RATE) - 20 * ref.HOP
    assert [piece['start'] for piece in got['segments']] == [s / RATE for s in start.tolist()]
    assert [piece['end'] for piece in got['segments']] == \
        [round((s + n) / RATE, 6) for s, n in zip(start.tolist(), length.tolist())]
    assert got['audio_seconds'] == len(audio) / RATE
    assert got['speech_seconds'] == int(length.sum()) / RATE


@pytest.mark.parametrize('timestamps', [False, True])
def test_pieces_equal_batches_rebuilt_on_the_host(setup, timestamps):
    from ctc_asr_amd import transcribe
    model, folder, audio, table = setup
    report = {}
    got = transcribe.transcribe(model, str(folder / 'long.wav'), timestamps=timestamps,
                                report=report)
    want = _by_hand(model, audio, table, timestamps)
    assert len(got['segments']) == len(want) == len(report['decoded'])
    assert any(text for _, text, _ in want)              # (the model does emit something)
    for i, (piece, (labels, text, words)) in enumerate(zip(got['segments'], want)):
        assert report['decoded'][i] == labels and piece['plaintext'] == text
        assert ('words' in piece) == timestamps
        if timestamps:
            shift = int(table[0][i]) / RATE
            assert piece['words'] == [dict(w, start=round(w['start'] + shift, 6),
                                           end=round(w['end'] + shift, 6)) for w in words]
            # (no upper bound: the ds2 front end decodes every row over the batch's length)
            assert all(piece['start'] <= w['start'] < w['end'] for w in piece['words'])
            assert ' '.join(w['word'] for w in piece['words']) == ' '.join(text.split())
    assert got['plaintext'] == ' '.join(text for _, text, _ in want if text)
    if timestamps:
        assert any(piece['words'] for piece in got['segments'])
    for piece in got['segments']:
        assert json.loads(json.dumps(piece)) == piece


def test_a_silent_recording_has_no_segments(setup):
    from ctc_asr_amd import transcribe
    model, folder, _, _ = setup
    got = transcribe.transcribe(model, str(folder / 'silent.wav'), timestamps=True)
    assert got == {'plaintext': '', 'segments': [], 'audio_seconds': 3.0, 'speech_seconds': 0.0}


def test_nbest_is_refused(setup):
    from ctc_asr_amd import transcribe
    model, folder, _, _ = setup
    with pytest.raises(ValueError, match='nbest'):
        transcribe.transcribe(model, str(folder / 'long.wav'), nbest=2)
    with pytest.raises(ValueError, match='nbest'):
        transcribe.main(['--input', str(folder / 'long.wav'), '--nbest', '2', '--beam_width', '8'])
    from ctc_asr_amd.params import FLAGS
    FLAGS.update(nbest=0, input='')
