"""`search.search` and `CTCModel.search_fn` on the tiny random model and the burst recording of
tests/test_gpu_transcribe.py (rebuilt here).

The phrase read off the greedy path of a span scores exactly 0.0 over that span; the driver's
hits equal `search_fn` called by hand on batches rebuilt on the host in the same order (the same
launches on the same data: exact), with times restated from the frame-to-sample map; no hit
reaches beyond its piece's own frame count; a silent recording gives no hits and the summary
lines; ``--nbest`` and ``--lm_path`` are refused."""

import json
import math

import numpy as np
import pytest
import torch
from scipy.io import wavfile

pytestmark = pytest.mark.gpu
RATE = 16000
BATCH = 3
HOP = 160 * 2                         # ds2: two feature hops per logit frame
THRESHOLD = -2.5
MAX_HITS = 4


def _recording(seconds=12.0, seed=31):
    """A noise floor of rms 30 and four bursts of rms 3000, the third longer than two seconds;
    the length is no multiple of a hop."""
    rng = np.random.default_rng(seed)
    n = int(seconds * RATE) + 77
    rms = np.full(n, 30.0)
    for begin, end in ((0.8, 1.6), (2.4, 3.1), (4.0, 8.3), (9.5, 10.9)):
        rms[int(begin * RATE):int(end * RATE)] = 3000.0
    return np.clip(rng.normal(size=n) * rms, -32768, 32767).astype(np.int16)


def _batches(model, audio, start, length):
    """(rows, logits, own frame counts) per batch, rebuilt on the host in the driver's order."""
    from ctc_asr_amd.input_functions import features_from_pcm, num_frames
    order = sorted(range(len(start)), key=lambda i: (-int(length[i]), i))
    for first in range(0, len(order), BATCH):
        rows = order[first:first + BATCH]
        feats, lengths = features_from_pcm(
            [audio[int(start[i]):int(start[i]) + int(length[i])] for i in rows], model.device)
        logits, seq_len = model.inference_fn(feats, lengths, training=False)
        model.check_rnn_error()
        own = [model.cfg.output_time(num_frames(int(length[i]), False)) for i in rows]
        assert max(own) <= logits.shape[0]
        yield rows, logits, own, seq_len


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    from ctc_asr_amd import search, transcribe
    from ctc_asr_amd.labels import decode
    from ctc_asr_amd.model import CTCModel, ModelConfig, init_params
    from ctc_asr_amd.params import FLAGS
    FLAGS.reset()
    FLAGS.update(feature_type='mel', feature_normalization='local', batch_size=BATCH,
                 max_segment_seconds=2)
    folder = tmp_path_factory.mktemp('search')
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
    # phrases from what the model itself says in the recording: runs of letters in the decoded
    # labels of its pieces (id 0 renders as nothing, so the transcript's text is no guide), two
    # runs with the space between them as one phrase, and one phrase it does not say
    told = {}
    transcribe.transcribe(model, str(folder / 'long.wav'), report=told)
    words, joined = set(), set()
    for ids in told['decoded']:
        text = ''.join(decode([v]) if v > 1 else '\n' if v == 0 else ' ' for v in ids)
        for chunk in text.split('\n'):
            parts = chunk.split(' ')
            words.update(part for part in parts if len(part) >= 2)
            joined.update(a + ' ' + b for a, b in zip(parts, parts[1:]) if a and b)
    assert len(words) >= 3
    phrases = sorted(words, key=lambda w: (-len(w), w))[:4] + sorted(joined)[:1] + ['zzzzqqqq']
    report = {}
    result = search.search(model, str(folder / 'long.wav'), phrases, THRESHOLD, MAX_HITS,
                           report=report)
    yield model, folder, audio, phrases, result, report
    FLAGS.reset()


def test_the_greedy_phrase_of_a_span_scores_zero_over_it(setup):
    model, folder, audio, phrases, result, report = setup
    blank = model.cfg.num_classes - 1
    rows, logits, own, _ = next(_batches(model, audio, report['start'], report['length']))
    greedy = logits[:, 0, :].argmax(-1).cpu().numpy()[:own[0]]
    # frames [a, b], trimmed to non-blank ends: from the first frame of the second run of a label
    # to the last frame of the last run but one
    begins = [t for t in range(own[0]) if greedy[t] != blank and
              (t == 0 or greedy[t - 1] != greedy[t])]
    ends = [t for t in range(own[0]) if greedy[t] != blank and
            (t + 1 == own[0] or greedy[t + 1] != greedy[t])]
    assert len(begins) >= 4, 'the random model emits labels'
    a, b = begins[1], ends[-2]
    phrase, before = [], -1
    for t in range(a, b + 1):
        if greedy[t] != before and greedy[t] != blank:
            phrase.append(int(greedy[t]))
        before = greedy[t]
    seq_len = torch.tensor(own, dtype=torch.int32, device=model.device)
    found, per_pair = model.search_fn(logits, seq_len, [phrase], 0.0, max_hits=MAX_HITS,
                                      pairs=[(0, 0)])
    assert per_pair['status'].tolist() == [0] and per_pair['best_score'].tolist() == [0.0]
    assert found and found[0]['score'] == 0.0 and found[0]['score_per_label'] == 0.0
    first = found[0]
    assert (first['phrase'], first['utt']) == (0, 0) and first['start'] <= first['end'] < own[0]
    collapsed, before = [], -1
    for t in range(first['start'], first['end'] + 1):
        if greedy[t] != before and greedy[t] != blank:
            collapsed.append(int(greedy[t]))
        before = greedy[t]
    assert collapsed == phrase
    # and the span it was read off is one of the hits, frame for frame
    assert (a, b) in [(hit['start'], hit['end']) for hit in found], (found, a, b)


def test_driver_hits_equal_search_fn_by_hand(setup):
    from ctc_asr_amd import search
    from ctc_asr_amd.labels import encode
    model, folder, audio, phrases, result, report = setup
    start, length = report['start'], report['length']
    assert report['hop_samples'] == HOP and report['texts'] == phrases
    labels = [encode(text) for text in phrases]
    assert report['labels'] == labels
    want, best = [], {}
    for rows, logits, own, seq_len in _batches(model, audio, start, length):
        assert [int(report['frames'][i]) for i in rows] == own
        found, per_pair = model.search_fn(
            logits, torch.tensor(own, dtype=torch.int32, device=model.device), labels, THRESHOLD,
            max_hits=MAX_HITS)
        assert len(per_pair['status']) == len(rows) * len(labels)
        assert per_pair['utt'].tolist() == [b for b in range(len(rows)) for _ in labels]
        for hit in found:
            i = rows[hit['utt']]
            assert 0 <= hit['start'] <= hit['end'] < own[hit['utt']]   # inside the piece's own frames
            assert hit['score'] >= THRESHOLD * len(labels[hit['phrase']])
            begin = int(start[i]) + min(hit['start'] * HOP, int(length[i]))
            end = int(start[i]) + min((hit['end'] + 1) * HOP, int(length[i]))
            assert search.hit_samples(start[i], length[i], hit['start'], hit['end'], HOP) == \
                (begin, end)
            want.append((begin, end, hit['phrase'], i, hit['score'], hit['score_per_label'],
                         hit['start'], hit['end']))
        for h in range(len(per_pair['status'])):
            score, p = float(per_pair['best_score'][h]), int(per_pair['phrase'][h])
            if per_pair['status'][h] == 0 and math.isfinite(score):
                i = rows[int(per_pair['utt'][h])]
                span = search.hit_samples(start[i], length[i], *per_pair['best_span'][h], HOP)
                key = (-score / len(labels[p]), span[0])
                if p not in best or key < best[p][0]:
                    best[p] = (key, span)
    want.sort(key=lambda hit: hit[:4])
    assert len(want) >= 1, 'the transcript\'s own words are found'
    assert result['hits'] == [
        {'phrase': phrases[p], 'start': round(begin / RATE, 6), 'end': round(end / RATE, 6),
         'score': score, 'score_per_label': per_label, 'piece': int(i)}
        for begin, end, p, i, score, per_label, _, _ in want]
    assert report['hit_frames'] == [(i, p, a, b) for _, _, p, i, _, _, a, b in want]
    for line in result['hits']:
        assert json.loads(json.dumps(line)) == line
        assert 0 <= line['start'] < line['end'] <= len(audio) / RATE
    for p, line in enumerate(result['phrases']):
        assert line['phrase'] == phrases[p]
        assert line['hits'] == sum(1 for hit in want if hit[2] == p)
        key, span = best[p]
        assert line['best_score_per_label'] == -key[0]
        assert (line['best_start'], line['best_end']) == \
            (round(span[0] / RATE, 6), round(span[1] / RATE, 6))
    # what the decode spells is there, at 0.0 where the greedy path spells it too.  (What it does
    # not spell scores below 0, but a random model gives no margin to assert.)
    exact = [line for line in result['phrases'] if line['best_score_per_label'] == 0.0]
    assert exact and all(line['hits'] >= 1 for line in exact)
    assert all(line['best_score_per_label'] <= 0.0 for line in result['phrases'])
    assert result['phrases'][-1]['best_score_per_label'] < 0.0
    assert result['pieces'] == len(start) >= 6
    assert result['audio_seconds'] == len(audio) / RATE


def test_a_silent_recording_gives_no_hits_and_the_summary_lines(setup):
    from ctc_asr_amd import search
    model, folder, audio, phrases, _, _ = setup
    result = search.search(model, str(folder / 'silent.wav'), phrases, THRESHOLD, MAX_HITS)
    assert result['hits'] == [] and result['pieces'] == 0
    assert result['phrases'] == [{'phrase': text, 'hits': 0, 'best_score_per_label': None,
                                  'best_start': None, 'best_end': None} for text in phrases]
    assert result['speech_seconds'] == 0.0


def test_nbest_and_lm_path_are_refused(setup):
    from ctc_asr_amd import search
    from ctc_asr_amd.params import FLAGS
    model, folder, audio, phrases, _, _ = setup
    kept = FLAGS.flag_values_dict()
    (folder / 'p.txt').write_text('\n'.join(phrases) + '\n')
    base = ['--input', str(folder / 'long.wav'), '--phrases', str(folder / 'p.txt')]
    try:
        with pytest.raises(ValueError, match='nbest'):
            search.main(base + ['--nbest', '2', '--beam_width', '8'])
        FLAGS.update(nbest=0)
        with pytest.raises(ValueError, match='lm_path'):
            search.main(base + ['--lm_path', str(folder / 'lm.npz')])
    finally:
        FLAGS.reset()
        FLAGS.update(**kept)
