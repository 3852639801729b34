"""`align_long.align_recording` with wildcard spans, the barrier cuts and the driver, on the tiny
random model and the burst recording of tests/test_gpu_align_long_pipeline.py (rebuilt here).

The transcript is the text `transcribe` decodes from the recording with its first and its last
word dropped (``free_ends``) and a run of words in the middle replaced by the token: an
alignment exists, the kept words must come back in order, three spans are skipped, and the score
cannot be below the whole text's (every frame of the dropped words may go to a wildcard at the
best class's price).  Without the new flags the driver writes what it wrote before them: its
files equal, byte for byte, those made from a direct `align_long_fn` alignment."""

import json

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from tests import align_long_reference as lref
from tests import align_partial_reference as pref

pytestmark = pytest.mark.gpu
RATE = 16000
BATCH = 3
TOKEN = '[...]'


def _recording(seconds=12.0, seed=31):
    """A noise floor of rms 30 and four bursts of rms 3000, the third longer than two seconds;
    the length is no multiple of a hop."""
    rng = np.random.default_rng(seed)
    n = int(seconds * RATE) + 77
    rms = np.full(n, 30.0)
    for begin, end in ((0.8, 1.6), (2.4, 3.1), (4.0, 8.3), (9.5, 10.9)):
        rms[int(begin * RATE):int(end * RATE)] = 3000.0
    return np.clip(rng.normal(size=n) * rms, -32768, 32767).astype(np.int16)


MODEL = dict(used_model='ds2', conv_filters=[32, 32], rnn_cell='lstm', cudnn=True,
             num_units_dense=64, num_layers_rnn=1, num_units_rnn=64, dense_dropout_rate=0.0,
             beam_width=8)


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    from ctc_asr_amd import align_long, transcribe
    from ctc_asr_amd.model import CTCModel, ModelConfig, init_params
    from ctc_asr_amd.params import FLAGS
    FLAGS.reset()
    FLAGS.update(feature_type='mel', feature_normalization='local', batch_size=BATCH,
                 max_segment_seconds=2)
    folder = tmp_path_factory.mktemp('align_partial')
    audio = _recording()
    wavfile.write(str(folder / 'long.wav'), RATE, audio)
    cfg = ModelConfig(**MODEL)
    params = init_params(cfg, 3)
    params['logits/kernel'] = params['logits/kernel'] * 60.0    # random, but decisive: it emits labels
    model = CTCModel(cfg, 'cuda', params=params)
    said = transcribe.transcribe(model, str(folder / 'long.wav'))['plaintext'].split()
    assert len(said) >= 5, said
    inner = said[1:-1]
    p = max(1, len(inner) // 3)
    q = min(max(p + 1, 2 * len(inner) // 3), len(inner) - 1)
    kept = (inner[:p], inner[q:])
    assert kept[0] and inner[p:q] and kept[1]
    text = '{}\n{} {}  {}'.format(' '.join(kept[0]), TOKEN, TOKEN, ' '.join(kept[1]))
    report = {}
    result = align_long.align_recording(model, str(folder / 'long.wav'), text, report=report,
                                        wildcard=TOKEN, free_ends=True)
    full = align_long.align_recording(model, str(folder / 'long.wav'), ' '.join(said))
    yield model, folder, audio, said, kept, text, result, report, full
    FLAGS.reset()


def test_status_words_and_skipped_spans(setup):
    model, folder, audio, said, kept, text, result, report, full = setup
    assert result['status'] == 'ok' and full['status'] == 'ok'
    assert report['text'] == '* {} {} {} *'.format(' '.join(kept[0]), TOKEN, ' '.join(kept[1]))
    assert report['labels'] == pref.parse_transcript(text, TOKEN, True)[1]
    assert report['labels'].count(pref.WILDCARD) == 3
    words, skipped = result['words'], result['skipped']
    assert [w['word'] for w in words] == kept[0] + kept[1]
    assert [s['after_word'] for s in skipped] == [-1, len(kept[0]) - 1, len(words) - 1]
    for span in skipped:
        assert json.loads(json.dumps(span)) == span
        assert span['frames'] >= 1 and 0 <= span['start_sample'] < span['end_sample'] <= len(audio)
        assert span['start'] == round(span['start_sample'] / RATE, 6)
        assert span['end'] == round(span['end_sample'] / RATE, 6)
        for k, word in enumerate(words):        # disjoint from every word, on its own side
            if k <= span['after_word']:
                assert word['end_sample'] <= span['start_sample'], (span, word)
            else:
                assert span['end_sample'] <= word['start_sample'], (span, word)
    wild = pref.wildcard_frames(report['path'], report['labels'])
    assert result['wildcard_frames'] == int(wild.sum()) == sum(s['frames'] for s in skipped)
    assert result['covered_frames'] == len(wild) - int(wild.sum()) > 0
    total = 0.0
    for value in report['frame_logp'][~wild]:
        total += float(value)
    assert result['score_per_covered_frame'] == total / result['covered_frames']
    assert result['score_per_frame'] == result['score'] / len(wild)
    print('words {} of {}, skipped {}'.format(len(words), len(said),
                                              [(s['after_word'], s['frames']) for s in skipped]))
    # the whole text needs no wildcard: today's keys, today's call
    assert 'skipped' not in full and 'wildcard_frames' not in full
    assert [w['word'] for w in full['words']] == said


def test_path_equals_the_kernel_and_the_reference_and_the_score_is_not_below_the_full_text(
        setup, hip):
    model, folder, audio, said, kept, text, result, report, full = setup
    assert result['status'] == 'ok'
    labels = torch.tensor(report['labels'], dtype=torch.int32, device='cuda')
    path, score, flp, logp, status = hip.ctc_align_partial(report['logits'], labels, logp=True)
    assert int(status.cpu()[0]) == 0
    want = pref.on_table(logp.cpu().numpy(), report['labels'], model.cfg.num_classes - 1)
    for got in ((report['path'], report['frame_logp']), (path.cpu().numpy(), flp.cpu().numpy())):
        assert lref.same_bits(got[0], want[1]) and lref.same_bits(got[1], want[2])
    assert lref.same_bits(np.float64(result['score']), want[0])
    assert lref.same_bits(score.cpu().numpy()[0], want[0])
    assert result['score'] >= full['score']
    # K21 refuses these labels
    assert int(hip.ctc_align_long(report['logits'], labels)[4].cpu()[0]) == 2


def test_no_cut_utterance_spans_a_wildcard_and_every_wav_is_its_slice(setup):
    from ctc_asr_amd import align_long
    model, folder, audio, said, kept, text, result, report, full = setup
    assert result['status'] == 'ok'
    barriers = [s['after_word'] for s in result['skipped']]
    utterances = align_long.cut_utterances(result['words'], len(audio), 2, 200, 100, None,
                                           barriers=barriers)
    out, csv_path = folder / 'corpus', folder / 'corpus' / 'train.csv'
    rows = align_long.write_corpus(audio, utterances, str(out), str(csv_path), 'long')
    lines = [json.loads(line) for line in open(align_long.report_path(str(csv_path)))]
    assert len(lines) == len(utterances) >= 2
    assert [k for u in lines for k in range(u['first_word'], u['last_word'] + 1)] == \
        list(range(len(result['words'])))
    middle = len(kept[0]) - 1
    assert not any(u['first_word'] <= middle < u['last_word'] for u in lines)
    assert [u['beside_wildcard'] for u in lines] == \
        [u['first_word'] - 1 in barriers or u['last_word'] in barriers for u in lines]
    assert lines[0]['beside_wildcard'] and lines[-1]['beside_wildcard']
    assert any(u['last_word'] == middle and u['beside_wildcard'] for u in lines)
    # an utterance takes at most half of the gap that holds the wildcard's span
    words = result['words']
    for u in lines:
        if u['last_word'] + 1 < len(words):
            gap = words[u['last_word'] + 1]['start_sample'] - words[u['last_word']]['end_sample']
            assert u['end_sample'] - words[u['last_word']]['end_sample'] <= gap // 2
    ok = [u for u in lines if u['status'] == 'ok']
    print('utterances:', [(u['status'], u['beside_wildcard'], u['end_sample'] - u['start_sample'])
                          for u in lines])
    for u in ok:
        rate, samples = wavfile.read(str(out / u['path']))
        assert rate == RATE and samples.dtype == np.int16
        assert samples.tobytes() == audio[u['start_sample']:u['end_sample']].tobytes()
    assert len(rows) == (len(ok) + 1 if ok else 0)


def test_the_driver_without_the_flags_writes_what_it_wrote_and_with_them_the_spans(setup):
    from ctc_asr_amd import align_long, storage
    from ctc_asr_amd.params import FLAGS
    model, folder, audio, said, kept, text, result, report, full = setup
    kept_flags = FLAGS.flag_values_dict()
    storage.save_checkpoint(str(folder / 'ckpt'), model, 1)
    (folder / 'full.txt').write_text(' '.join(said) + '\n')
    (folder / 'part.txt').write_text(text)
    base = ['--input', str(folder / 'long.wav'), '--train_dir', str(folder / 'ckpt'),
            '--cut_max_seconds', '2']
    try:
        FLAGS.update(**MODEL)
        # 1. no new flag: the files of a direct `align_long_fn` alignment
        assert align_long.main(base + [
            '--transcript', str(folder / 'full.txt'), '--align_output', str(folder / 'a.jsonl'),
            '--corpus_out_dir', str(folder / 'a'), '--corpus_out_csv', str(folder / 'a.csv')]) == 0
        labels = torch.tensor(report_labels(said), dtype=torch.int32, device='cuda')
        direct = {}
        again = align_long.align_recording(model, str(folder / 'long.wav'), ' '.join(said),
                                           report=direct)
        path, score, flp, _, status = model.align_long_fn(direct['logits'], labels)
        assert lref.same_bits(path.cpu().numpy(), direct['path'])
        assert float(score.cpu()[0]) == again['score'] == full['score']
        want_words = align_long.words_on_samples(
            path.cpu().numpy(), direct['labels'], direct['frame_begin'], direct['frame_end'],
            flp.cpu().numpy(), RATE)
        assert (folder / 'a.jsonl').read_text() == \
            ''.join(json.dumps(word) + '\n' for word in want_words)
        utterances = align_long.cut_utterances(want_words, len(audio), 2, 200, 100, None, RATE)
        align_long.write_corpus(audio, utterances, str(folder / 'b'), str(folder / 'b.csv'), 'long')
        assert (folder / 'a.csv').read_bytes() == (folder / 'b.csv').read_bytes()
        assert (folder / 'a.report.jsonl').read_bytes() == (folder / 'b.report.jsonl').read_bytes()
        assert b'beside_wildcard' not in (folder / 'a.report.jsonl').read_bytes()
        assert sorted(p.name for p in (folder / 'a').iterdir()) == \
            sorted(p.name for p in (folder / 'b').iterdir())
        # 2. with them: the words, then one line per skipped span
        assert align_long.main(base + [
            '--transcript', str(folder / 'part.txt'), '--align_output', str(folder / 'p.jsonl'),
            '--corpus_out_dir', str(folder / 'p'), '--corpus_out_csv', str(folder / 'p.csv'),
            '--transcript_wildcard', TOKEN, '--align_free_ends']) == 0
        lines = [json.loads(line) for line in open(str(folder / 'p.jsonl'))]
        assert lines[:len(result['words'])] == result['words']
        assert lines[len(result['words']):] == [dict({'skipped': True}, **s)
                                                for s in result['skipped']]
        cut = [json.loads(line) for line in open(str(folder / 'p.report.jsonl'))]
        assert cut and all('beside_wildcard' in line for line in cut)
    finally:
        FLAGS.reset()
        FLAGS.update(**kept_flags)


def report_labels(said):
    from ctc_asr_amd.labels import encode
    return encode(' '.join(said))
