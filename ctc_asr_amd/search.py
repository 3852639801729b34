"""Search a recording for spoken phrases: ``python -m ctc_asr_amd.search --input long.wav
--phrases phrases.txt [--search_min_score -1.0] [--search_max_hits 16] [--search_output
hits.jsonl] [--resample_input] [--eval_ema] [vad flags] [model flags]``.

`transcribe` and a search of its text find a phrase only where the 1-best decode spells it
right; one wrong character in a name hides it.  The logits hold more: a phrase the decode
dropped can still have a path nearly as probable as the best one.  Here every phrase is scored
against the logits directly (``ctcasr_ctc_search``, K22: a Viterbi lattice with a free start and
a free end per (piece, phrase) pair, the hits picked on the device):

1. the recording is read and uploaded as `transcribe` does (``--resample_input`` included);
2. ``vad.segment`` -> the pieces;
3. the same batches in the same order through ``gather_segments``, ``features`` and
   ``inference_fn(training=False)`` (`transcribe.forward_pieces`);
4. per batch ONE `CTCModel.search_fn` call over all (piece, phrase) pairs, grouped by piece.
   Each piece is given its own frame count ``output_time(num_frames(length_p))`` - not the
   batch's ``seq_len``, which the ``ds2`` front end reports for every row alike: a hit must not
   land in the zeros behind a piece;
5. frame g of piece p begins at sample ``start_p + g * hop_samples``; a hit runs from the
   beginning of its start frame to the beginning of frame ``end + 1``, both clipped to the
   piece's end (the convention of `align_long`).

A hit's score is the log of (the best path through the phrase over the hit's frames) over (the
greedy path on the same frames): 0 when the greedy decode spells the phrase there, negative
otherwise; ``score_per_label`` divides it by the phrase's length, and ``--search_min_score`` is
the lowest ``score_per_label`` kept.  The space is a label like any other.  A phrase that
straddles two pieces is not found.
"""

import json
import math
import os
import sys

import numpy as np
import torch

from ctc_asr_amd import hip, storage, transcribe, vad
from ctc_asr_amd.align_long import hop_samples, normalize_transcript
from ctc_asr_amd.input_functions import _check_feature_args, num_frames
from ctc_asr_amd.labels import encode
from ctc_asr_amd.model import CTCModel, ModelConfig
from ctc_asr_amd.params import FLAGS


def parse_phrases(lines):
    """The phrases of a ``--phrases`` file, normalised as `align_long.normalize_transcript`
    spells them; blank lines are skipped.  A digit, or a line of which nothing is left, raises
    ``ValueError`` naming the line (counted from 1)."""
    phrases = []
    for number, line in enumerate(lines, 1):
        if not line.strip():
            continue
        try:
            phrases.append(normalize_transcript(line))
        except ValueError as error:
            raise ValueError('phrases, line {}: {}'.format(number, error)) from None
    return phrases


def read_phrases(path):
    with open(path, 'r', encoding='utf-8') as handle:
        return parse_phrases(handle.read().splitlines())


def hit_samples(piece_start, piece_length, start_frame, end_frame, hop):
    """(begin, end) sample of a hit over frames ``start_frame .. end_frame`` (inclusive) of a
    piece: from the beginning of its start frame to the beginning of frame ``end + 1``, both
    clipped to the piece's end."""
    begin = int(piece_start) + min(int(start_frame) * int(hop), int(piece_length))
    end = int(piece_start) + min((int(end_frame) + 1) * int(hop), int(piece_length))
    return begin, end


def search(model, wav_path, phrases, min_score_per_label=None, max_hits=None, settings=None,
           batch_size=None, timings=None, report=None):
    """Where in the recording ``wav_path`` are the ``phrases`` (texts) said?  Returns ``{'hits',
    'phrases', 'pieces', 'audio_seconds', 'speech_seconds'}``: ``hits`` one ``{'phrase',
    'start', 'end', 'score', 'score_per_label', 'piece'}`` per hit in time order (seconds of the
    recording; ``piece`` counts the pieces in time order), ``phrases`` one ``{'phrase', 'hits',
    'best_score_per_label', 'best_start', 'best_end'}`` per phrase - the best span anywhere,
    whatever the threshold (None where no piece can hold the phrase).  ``min_score_per_label``
    and ``max_hits`` default to the flags; ``timings`` receives the seconds spent in 'upload',
    'segmentation', 'forward' and 'search'; ``report`` receives the table of pieces ('start',
    'length' in samples, 'frames' searched of each), 'hop_samples', the normalised 'texts' and
    their 'labels', and per hit its 'hit_frames' (piece, phrase, start frame, end frame)."""
    settings = vad.VadSettings.from_flags(FLAGS) if settings is None else settings
    batch_size = FLAGS.batch_size if batch_size is None else int(batch_size)
    threshold = FLAGS.search_min_score if min_score_per_label is None else \
        float(min_score_per_label)
    max_hits = FLAGS.search_max_hits if max_hits is None else int(max_hits)
    feature_type, normalization = _check_feature_args(None, None)
    texts = [normalize_transcript(text) for text in phrases]
    labels = [encode(text) for text in texts]
    for text, ids in zip(texts, labels):
        if len(ids) > hip.SEARCH_MAX_LABEL_LEN:
            raise ValueError('search: the phrase "{}..." has {} labels; the kernel serves {}.'
                             .format(text[:24], len(ids), hip.SEARCH_MAX_LABEL_LEN))
    pcm, clock = transcribe.upload_recording(model, wav_path, timings)
    start, length, _ = vad.segment(pcm, settings)
    clock.lap('segmentation')
    drop = FLAGS.features_drop_every_second_frame
    hop = hop_samples(model.cfg, drop)
    frames = np.array([model.cfg.output_time(num_frames(int(n), drop)) for n in length],
                      dtype=np.int64)
    rate = FLAGS.sampling_rate
    hits, hit_frames = [], []
    best = [(-math.inf, None, None)] * len(texts)       # score per label, begin, end sample
    for rows, logits, _ in transcribe.forward_pieces(model, pcm, start, length, batch_size,
                                                     feature_type, normalization):
        clock.lap('forward')
        own = np.minimum(frames[rows], int(logits.shape[0])).astype(np.int32)
        found, per_pair = model.search_fn(logits, torch.from_numpy(own).to(model.device), labels,
                                          threshold, max_hits=max_hits)
        for hit in found:
            piece = rows[hit['utt']]
            begin, end = hit_samples(start[piece], length[piece], hit['start'], hit['end'], hop)
            hits.append((begin, end, hit['phrase'], piece, hit['score'],
                         hit['score_per_label']))
            hit_frames.append((piece, hit['phrase'], hit['start'], hit['end']))
        for h in range(len(per_pair['utt'])):
            p, piece = int(per_pair['phrase'][h]), rows[int(per_pair['utt'][h])]
            score = float(per_pair['best_score'][h])
            if per_pair['status'][h] != 0 or not math.isfinite(score):
                continue
            begin, end = hit_samples(start[piece], length[piece], *per_pair['best_span'][h], hop)
            # the best of a phrase: the larger score, then the earlier span
            per_label = score / len(labels[p])
            if best[p][1] is None or per_label > best[p][0] or \
                    (per_label == best[p][0] and begin < best[p][1]):
                best[p] = (per_label, begin, end)
        clock.lap('search')
    order = sorted(range(len(hits)), key=lambda k: hits[k][:4])
    lines = [{'phrase': texts[hits[k][2]], 'start': round(hits[k][0] / rate, 6),
              'end': round(hits[k][1] / rate, 6), 'score': hits[k][4],
              'score_per_label': hits[k][5], 'piece': int(hits[k][3])} for k in order]
    summary = []
    for p, text in enumerate(texts):
        score, begin, end = best[p]
        summary.append({'phrase': text, 'hits': sum(1 for hit in hits if hit[2] == p),
                        'best_score_per_label': score if begin is not None else None,
                        'best_start': round(begin / rate, 6) if begin is not None else None,
                        'best_end': round(end / rate, 6) if end is not None else None})
    if report is not None:
        report.update(start=start, length=length, frames=frames, hop_samples=hop, texts=texts,
                      labels=labels, hit_frames=[hit_frames[k] for k in order])
    return {'hits': lines, 'phrases': summary, 'pieces': len(start),
            'audio_seconds': int(pcm.numel()) / rate,
            'speech_seconds': int(sum(int(v) for v in length)) / rate}


def check_flags():
    """What the driver needs of the flags, checked before anything is loaded."""
    if FLAGS.nbest:
        raise ValueError('ctc_asr_amd.search does not serve --nbest.')
    if FLAGS.lm_path:
        raise ValueError('ctc_asr_amd.search does not serve --lm_path: phrases are scored '
                         'against the logits, no language model takes part.')
    if not os.path.isfile(FLAGS.input):
        raise ValueError('The input file "{}" does not exist.'.format(FLAGS.input))
    if not os.path.isfile(FLAGS.phrases):
        raise ValueError('The phrases file "{}" does not exist.'.format(FLAGS.phrases))


def main(argv=None):
    FLAGS.parse(sys.argv[1:] if argv is None else argv)
    check_flags()
    phrases = read_phrases(FLAGS.phrases)
    if not phrases:
        raise ValueError('The phrases file "{}" holds no phrase.'.format(FLAGS.phrases))
    if not torch.cuda.is_available():
        raise SystemExit('ctc_asr_amd.search needs an MI355X; no GPU is visible.')
    model = CTCModel(ModelConfig.from_flags(FLAGS), 'cuda', seed=FLAGS.random_seed or 1)
    latest = storage.latest_checkpoint(FLAGS.train_dir)
    if latest is None:
        raise SystemExit('No checkpoint found in {}.'.format(FLAGS.train_dir))
    storage.restore_checkpoint(latest, model, weights='ema' if FLAGS.eval_ema else 'param')
    print('Inputs: {} / {}'.format(FLAGS.input, FLAGS.phrases))
    result = search(model, FLAGS.input, phrases)
    lines = [json.dumps(line) for line in result['hits'] + result['phrases']]
    if FLAGS.search_output:
        with open(FLAGS.search_output, 'w', encoding='utf-8') as handle:
            for line in lines:
                handle.write(line + '\n')
        print('{} hits of {} phrases -> {}'.format(len(result['hits']), len(phrases),
                                                   FLAGS.search_output))
    else:
        for line in lines:
            print(line)
    print('{} pieces, audio {:.2f} s, speech {:.2f} s'.format(
        result['pieces'], result['audio_seconds'], result['speech_seconds']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
