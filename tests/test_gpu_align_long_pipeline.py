"""`align_long.align_recording` and the corpus cutter on the tiny random model and the burst
recording of tests/test_gpu_transcribe.py (rebuilt here).  The transcript is the joined text
`transcribe` decodes from the same recording, so an alignment exists.

The concatenated logits equal those of batches rebuilt on the host in the same order (the same
launches on the same data: exact); the path equals the float64 reference on the device's own
table; word times equal a restatement of the frame-to-sample map; and with ``--cut_max_seconds
2`` the utterances cover the transcript's words in order, each once, every WAV is its slice of
the recording, the manifest reads back, and each ``ok`` row aligns through `align.align_rows`."""

import json

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from tests import align_long_reference as lref

pytestmark = pytest.mark.gpu
RATE = 16000
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
    from ctc_asr_amd import align_long, transcribe
    from ctc_asr_amd.model import CTCModel, ModelConfig, init_params
    from ctc_asr_amd.params import FLAGS
    FLAGS.reset()
    FLAGS.update(feature_type='mel', feature_normalization='local', batch_size=BATCH,
                 max_segment_seconds=2)
    folder = tmp_path_factory.mktemp('align_long')
    audio = _recording()
    wavfile.write(str(folder / 'long.wav'), RATE, audio)
    cfg = ModelConfig(used_model='ds2', conv_filters=(32, 32), rnn_cell='lstm', cudnn=True,
                      num_units_dense=64, num_layers_rnn=1, num_units_rnn=64,
                      dense_dropout_rate=0.0, beam_width=8)
    params = init_params(cfg, 3)
    params['logits/kernel'] = params['logits/kernel'] * 60.0    # random, but decisive: it emits labels
    model = CTCModel(cfg, 'cuda', params=params)
    text = transcribe.transcribe(model, str(folder / 'long.wav'))['plaintext']
    assert text.strip()
    report = {}
    result = align_long.align_recording(model, str(folder / 'long.wav'), text, report=report)
    yield model, folder, audio, text, result, report
    FLAGS.reset()


def test_status_is_ok_and_the_result_is_complete(setup):
    model, folder, audio, text, result, report = setup
    assert result['status'] == 'ok'
    assert report['text'] == ' '.join(text.split())
    assert result['pieces'] == len(report['start']) >= 6
    assert result['audio_seconds'] == len(audio) / RATE
    assert result['speech_seconds'] == int(report['length'].sum()) / RATE
    assert result['score'] < 0 and \
        result['score_per_frame'] == result['score'] / report['logits'].shape[0]
    assert ' '.join(w['word'] for w in result['words']) == report['text']
    assert (report['audio'] == audio).all()
    for word in result['words']:
        assert json.loads(json.dumps(word)) == word


def test_concatenated_logits_equal_batches_rebuilt_on_the_host(setup):
    from ctc_asr_amd.input_functions import features_from_pcm, num_frames
    model, folder, audio, text, result, report = setup
    assert result['status'] == 'ok'
    start, length = report['start'], report['length']
    order = sorted(range(len(start)), key=lambda i: (-int(length[i]), i))
    kept = {}
    for first in range(0, len(order), BATCH):
        rows = order[first:first + BATCH]
        feats, lengths = features_from_pcm(
            [audio[int(start[i]):int(start[i]) + int(length[i])] for i in rows], model.device)
        logits, _ = model.inference_fn(feats, lengths, training=False)
        model.check_rnn_error()
        for b, i in enumerate(rows):
            own = model.cfg.output_time(num_frames(int(length[i]), False))
            assert own == report['frames'][i] and own <= logits.shape[0]
            kept[i] = logits[:own, b, :].clone()
    want = torch.cat([kept[i] for i in range(len(start))], dim=0)
    assert report['logits'].shape == want.shape
    assert torch.equal(report['logits'], want)
    assert report['offset'].tolist() == [int(sum(report['frames'][:i])) for i in range(len(start))]


def test_path_equals_the_reference_on_the_device_table(setup, hip):
    model, folder, audio, text, result, report = setup
    assert result['status'] == 'ok'
    labels = torch.tensor(report['labels'], dtype=torch.int32, device='cuda')
    path, score, flp, logp, status = hip.ctc_align_long(report['logits'], labels, logp=True)
    assert int(status.cpu()[0]) == 0
    want = lref.on_table(logp.cpu().numpy(), report['labels'], model.cfg.num_classes - 1)
    for got in ((report['path'], report['frame_logp']), (path.cpu().numpy(), flp.cpu().numpy())):
        assert lref.same_bits(got[0], want[1]) and lref.same_bits(got[1], want[2])
    assert lref.same_bits(np.float64(result['score']), want[0])
    assert lref.same_bits(score.cpu().numpy()[0], want[0])


def test_word_times_restate_the_frame_to_sample_map(setup):
    from ctc_asr_amd import alignment
    model, folder, audio, text, result, report = setup
    assert result['status'] == 'ok'
    hop = 160 * 2                                   # ds2: two feature hops per logit frame
    assert report['hop_samples'] == hop
    assert alignment.frame_seconds(model.cfg, False) == hop / RATE
    start, length, frames, offset = (report[k] for k in ('start', 'length', 'frames', 'offset'))

    def sample(g, edge):
        """Where concatenated frame g begins (edge 0) or ends (edge 1)."""
        p = max(i for i in range(len(offset)) if offset[i] <= g)
        assert g < offset[p] + frames[p]
        return int(start[p]) + min((g + edge - int(offset[p])) * hop, int(length[p]))
    # `alignment.segments` with one "second" per frame: start = first frame, end = last frame + 1
    in_frames = alignment.segments(report['path'], report['labels'], 1.0, report['frame_logp'])
    assert len(in_frames) == len(result['words']) > 0
    crossing = 0
    for word, frame_word in zip(result['words'], in_frames):
        first, last = int(frame_word['start']), int(frame_word['end']) - 1
        assert word['word'] == frame_word['word']
        assert word['confidence'] == frame_word['confidence']
        assert word['start_sample'] == sample(first, 0) and word['end_sample'] == sample(last, 1)
        assert word['start'] == round(word['start_sample'] / RATE, 6)
        assert word['end'] == round(word['end_sample'] / RATE, 6)
        assert 0 <= word['start_sample'] < word['end_sample'] <= len(audio)
        crossing += int(np.searchsorted(offset, first, 'right') !=
                        np.searchsorted(offset, last, 'right'))
    for before, after in zip(result['words'], result['words'][1:]):
        assert before['end_sample'] <= after['start_sample']
    print('words {}, of which {} span two pieces'.format(len(in_frames), crossing))


def test_cut_corpus_covers_the_transcript_and_aligns_row_by_row(setup):
    from ctc_asr_amd import align, align_long
    from ctc_asr_amd.csv_helper import read_csv_rows
    model, folder, audio, text, result, report = setup
    assert result['status'] == 'ok'
    utterances = align_long.cut_utterances(result['words'], len(audio), 2, 200, 100, None)
    out, csv_path = folder / 'corpus', folder / 'corpus' / 'train.csv'
    rows = align_long.write_corpus(audio, utterances, str(out), str(csv_path), 'long')
    lines = [json.loads(line) for line in open(align_long.report_path(str(csv_path)))]
    assert len(lines) == len(utterances) > 1
    # the words of the transcript in order, each exactly once
    assert [k for u in lines for k in range(u['first_word'], u['last_word'] + 1)] == \
        list(range(len(result['words'])))
    assert ' '.join(u['label'] for u in lines) == report['text']
    print('utterances:', [(u['status'], u['forced'], u['end_sample'] - u['start_sample'])
                          for u in lines])
    ok = [u for u in lines if u['status'] == 'ok']
    assert ok and all(u['end_sample'] - u['start_sample'] <= 2 * RATE for u in ok)
    for u in ok:
        rate, samples = wavfile.read(str(out / u['path']))
        assert rate == RATE and samples.dtype == np.int16
        assert samples.tobytes() == audio[u['start_sample']:u['end_sample']].tobytes()
    read = read_csv_rows(str(csv_path))
    assert [(r['path'], r['label'], r['length']) for r in read[1:]] == rows
    assert rows[-1] == rows[-2] and len(rows) == len(ok) + 1
    assert [float(r[2]) for r in rows] == sorted(float(r[2]) for r in rows)
    by_path = {u['path']: u for u in ok}
    for row in rows[:-1]:
        u = by_path[row[0]]
        assert row[1] == u['label']
        assert row[2] == '{:.4f}'.format((u['end_sample'] - u['start_sample']) / RATE)
    aligned = list(align.align_rows(model, read[1:-1], str(out), BATCH))
    print('row statuses:', [(r['path'], r['status']) for r in aligned])
    assert [r['status'] for r in aligned] == ['ok'] * len(ok)
    for r, row in zip(aligned, rows):
        assert ' '.join(w['word'] for w in r['words']) == row[1]
