"""Align a long recording to its whole transcript, and cut the pair into a training corpus:
``python -m ctc_asr_amd.align_long --input chapter.wav --transcript chapter.txt --align_output
words.jsonl [--corpus_out_dir out --corpus_out_csv out/train.csv] [--resample_input] [--eval_ema]
[vad flags] [model flags]``.

`align` places a transcript on ONE utterance that fits the model and K11's lattice (575
characters); `transcribe` cuts a recording at its pauses but decodes each piece on its own.  Here
a GIVEN text is placed on the whole recording, which is how CTC corpora are made from an
audiobook chapter and its text:

1. the recording is read and uploaded as `transcribe` does (``--resample_input`` included);
2. ``vad.segment`` -> the pieces; the same batches in the same order through
   ``gather_segments``, ``features`` and ``inference_fn(training=False)``
   (`transcribe.forward_pieces`);
3. of piece p the first ``output_time(num_frames(length_p))`` logit frames are kept - the piece's
   own count, not the batch's - and the pieces are concatenated in time order into ``[T, C]``;
4. `normalize_transcript` -> label ids -> ONE `CTCModel.align_long_fn` call (the tiled lattice of
   ``ctcasr_ctc_align_long``: no ceiling on the text but the workspace, 2 bits per cell);
5. frame g of piece p sits at sample ``start_p + (g - offset_p) * hop_samples`` of the recording,
   clipped to the piece's end; words are the runs of labels between spaces, as
   `alignment.segments` makes them, on these sample times.  A word may span two pieces;
6. `cut_utterances` groups the words into utterances at the pauses between them and
   `write_corpus` writes the ``ok`` ones as WAV files with a ``path;label;length`` manifest.

The path has to spend every frame somewhere: audio the text does not cover is not skipped, it
shows as words of low confidence around it - unless the transcript says where such audio lies.
With ``--transcript_wildcard TOKEN`` every TOKEN of the transcript stands for "something is said
here that the text does not hold", and ``--align_free_ends`` puts one before the first word and
after the last: `parse_transcript` turns them into `hip.ALIGN_WILDCARD` labels, step 4 becomes one
`CTCModel.align_partial_fn` call (``ctcasr_ctc_align_partial``: the wildcard takes one frame or
more at the log-probability of each frame's best class), the result lists the spans it took as
``skipped``, and no cut utterance reaches across one.  With neither flag nothing changes.
"""

import json
import math
import os
import sys

import numpy as np
import torch
from scipy.io import wavfile

from ctc_asr_amd import alignment, storage, transcribe, vad
from ctc_asr_amd.input_functions import _check_feature_args, num_frames
from ctc_asr_amd.hip import ALIGN_WILDCARD
from ctc_asr_amd.labels import decode, encode
from ctc_asr_amd.model import CTCModel, ModelConfig
from ctc_asr_amd.params import (CSV_DELIMITER, CSV_FIELDNAMES, FLAGS, MIN_EXAMPLE_LENGTH,
                                parse_cut_min_confidence)

FEATURE_HOP = 160       # samples per feature frame (hip.VAD_HOP: WIN_STEP at 16 kHz)


def _normalize(text, base=0):
    """`normalize_transcript` of a stretch of text that begins at offset ``base`` of the whole;
    the result may be empty."""
    out = []
    for offset, char in enumerate(text, base):
        if char.isdigit():
            raise ValueError('transcript: the digit "{}" at offset {} must be spelled out as it '
                             'is spoken.'.format(char, offset))
        low = char.lower()
        if len(low) == 1 and 'a' <= low <= 'z':
            out.append(low)
        elif char not in "'’":
            out.append(' ')
    return ' '.join(''.join(out).split())


def normalize_transcript(text):
    """The text as the alphabet spells it: lower case, ``a-z`` kept, apostrophes (``'`` and
    ``’``) deleted, every other character a space, runs of spaces collapsed, ends stripped.  A
    digit raises ``ValueError`` naming its offset: numbers must be spelled out, since dropping
    spoken words silently would misalign everything after them.  An empty result is refused."""
    result = _normalize(text)
    if not result:
        raise ValueError('transcript: nothing is left of the text after normalisation.')
    return result


def parse_transcript(text, wildcard='', free_ends=False):
    """A transcript that may cover only part of the recording -> ``(text, labels)``.

    The text is split on whitespace; a token equal to ``wildcard`` (unless that is empty) is a
    wildcard, and every run of tokens between two of them goes through `normalize_transcript`'s
    rules as one stretch (a digit is refused with its offset in the text given).  Wildcards with
    nothing between them that normalises to a word are one wildcard; ``free_ends`` adds one
    before the first word and one after the last unless one is there already.  ``labels`` are the
    words of each run joined by single spaces, with `hip.ALIGN_WILDCARD` between the runs and NO
    space label beside a wildcard: it takes the pauses around it.  ``text`` is the same in
    words: the runs and, for each wildcard, the token given, or ``*`` for one that only
    ``free_ends`` put there.  A transcript without a word is refused."""
    items, run_begin, run_end = [], None, None        # items: ('words', str) or ('wild', str)

    def close_run():
        if run_begin is not None:
            words = _normalize(text[run_begin:run_end], run_begin)
            if words:
                items.append(('words', words))

    position = 0
    for token in text.split():
        begin = text.index(token, position)
        position = begin + len(token)
        if wildcard and token == wildcard:
            close_run()
            run_begin = None
            if not items or items[-1][0] != 'wild':
                items.append(('wild', token))
        else:
            run_begin = begin if run_begin is None else run_begin
            run_end = position
    close_run()
    if not any(kind == 'words' for kind, _ in items):
        raise ValueError('transcript: nothing is left of the text after normalisation.')
    if free_ends:
        if items[0][0] != 'wild':
            items.insert(0, ('wild', '*'))
        if items[-1][0] != 'wild':
            items.append(('wild', '*'))
    labels = []
    for kind, value in items:
        labels.extend(encode(value) if kind == 'words' else [ALIGN_WILDCARD])
    return ' '.join(value for _, value in items), labels


def hop_samples(cfg, drop_every_second_frame):
    """Samples per logit frame: `alignment.frame_seconds` at 16 kHz, as an integer."""
    stride = (2 if cfg.used_model == 'ds2' else 1) * (2 if drop_every_second_frame else 1)
    return FEATURE_HOP * stride


def frame_samples(start, length, frames, hop):
    """(begin, end) sample of every concatenated frame, int64 [T] each: frame g of piece p, which
    holds frames ``offset_p .. offset_p + frames_p``, begins at ``start_p + (g - offset_p) * hop``
    and ends where the next would begin, both clipped to the piece's end."""
    begin, end = [], []
    for s, n, f in zip(start, length, frames):
        local = np.arange(int(f) + 1, dtype=np.int64) * hop
        local = np.minimum(local, int(n)) + int(s)
        begin.append(local[:-1])
        end.append(local[1:])
    if not begin:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(begin), np.concatenate(end)


def words_on_samples(path, labels, frame_begin, frame_end, frame_logp, sampling_rate=16000):
    """`alignment.segments` on sample times: the runs of labels between space labels, each from
    the first frame of its first label to the end of the last frame of its last label, with the
    mean ``frame_logp`` over the frames of its labels; a wildcard label ends a word as a space
    does.  Returns ``{'word', 'start', 'end',
    'confidence', 'start_sample', 'end_sample', 'frames'}`` per word; times in seconds of the
    recording.  One pass over the path, whatever the number of labels."""
    path = np.asarray(path)
    labels = [int(v) for v in labels]
    if path.size == 0 or (path < 0).all():
        return []
    odd = (path & 1) == 1
    frames = np.nonzero(odd)[0]
    position = path[frames] >> 1
    # the path is monotone: the frames of a label are one run
    first = np.full(len(labels), -1, dtype=np.int64)
    last = np.full(len(labels), -1, dtype=np.int64)
    seen, where, times = np.unique(position, return_index=True, return_counts=True)
    first[seen] = frames[where]
    last[seen] = frames[where + times - 1]
    logp = np.asarray(frame_logp, dtype=np.float64)
    words, current = [], []

    def close():
        if not current:
            return
        a, b = int(first[current[0]]), int(last[current[-1]])
        inside = logp[a:b + 1][odd[a:b + 1]]
        words.append({'word': decode([labels[k] for k in current]),
                      'start': round(int(frame_begin[a]) / sampling_rate, 6),
                      'end': round(int(frame_end[b]) / sampling_rate, 6),
                      'confidence': float(np.mean(inside)),
                      'start_sample': int(frame_begin[a]), 'end_sample': int(frame_end[b]),
                      'frames': int(inside.size)})
        del current[:]

    for k, label in enumerate(labels):
        if label == alignment.SPACE_ID or label == ALIGN_WILDCARD:
            close()
        else:
            current.append(k)
    close()
    return words


def skipped_on_samples(path, labels, frame_begin, frame_end, sampling_rate=16000):
    """What the wildcards of ``labels`` took: ``{'after_word', 'start', 'end', 'start_sample',
    'end_sample', 'frames'}`` per wildcard in time order, from its first frame to the end of its
    last.  ``after_word`` is the index (among `words_on_samples`' words) of the word before it,
    -1 for a wildcard before the first word."""
    path = np.asarray(path)
    labels = [int(v) for v in labels]
    if path.size == 0 or (path < 0).all():
        return []
    frames = np.nonzero((path & 1) == 1)[0]
    seen, where, times = np.unique(path[frames] >> 1, return_index=True, return_counts=True)
    first = dict(zip(seen.tolist(), frames[where].tolist()))
    last = dict(zip(seen.tolist(), frames[where + times - 1].tolist()))
    skipped, word, inside = [], -1, False
    for k, label in enumerate(labels):
        if label == ALIGN_WILDCARD:
            a, b = first[k], last[k]
            skipped.append({'after_word': word,
                            'start': round(int(frame_begin[a]) / sampling_rate, 6),
                            'end': round(int(frame_end[b]) / sampling_rate, 6),
                            'start_sample': int(frame_begin[a]), 'end_sample': int(frame_end[b]),
                            'frames': b - a + 1})
        if label == ALIGN_WILDCARD or label == alignment.SPACE_ID:
            inside = False
        elif not inside:
            inside, word = True, word + 1
    return skipped


def align_recording(model, wav_path, text, settings=None, batch_size=None, report=None,
                    wildcard='', free_ends=False):
    """Place ``text`` on the recording ``wav_path``.  Returns ``{'status', 'score',
    'score_per_frame', 'words', 'pieces', 'audio_seconds', 'speech_seconds'}``: ``status`` one of
    `alignment.STATUS_NAMES` ('infeasible': the speech found is too short for the text),
    ``score`` the log-probability of the best path (None unless ok), ``words`` as
    `words_on_samples` gives them (none unless ok).  ``report``: a dict that receives the table
    of pieces ('start', 'length' in samples, 'frames' kept and 'offset' of each), the
    concatenated 'logits' [T, C], the normalised 'text' and its 'labels', 'path', 'frame_logp',
    'frame_begin' / 'frame_end' in samples, 'hop_samples' and the recording itself ('audio',
    int16 on the host).

    ``wildcard`` / ``free_ends``: the text goes through `parse_transcript` in place of
    `normalize_transcript`.  When that leaves a wildcard among the labels, the alignment is
    `CTCModel.align_partial_fn`'s and the result also holds ``skipped`` (`skipped_on_samples`),
    ``wildcard_frames``, ``covered_frames`` and ``score_per_covered_frame`` - the float64 sum of
    ``frame_logp`` over the frames outside the wildcards, added in time order, over their number
    (None without such a frame).  ``words`` holds words only; ``score`` and
    ``score_per_frame`` run over all frames, wildcard frames included."""
    settings = vad.VadSettings.from_flags(FLAGS) if settings is None else settings
    batch_size = FLAGS.batch_size if batch_size is None else int(batch_size)
    feature_type, normalization = _check_feature_args(None, None)
    if wildcard or free_ends:
        text, labels = parse_transcript(text, wildcard, free_ends)
    else:
        text = normalize_transcript(text)
        labels = encode(text)
    partial = ALIGN_WILDCARD in labels
    pcm, _ = transcribe.upload_recording(model, wav_path)
    start, length, _ = vad.segment(pcm, settings)
    drop = FLAGS.features_drop_every_second_frame
    frames = np.array([model.cfg.output_time(num_frames(int(n), drop)) for n in length],
                      dtype=np.int64)
    kept = [None] * len(start)
    for rows, logits, _ in transcribe.forward_pieces(model, pcm, start, length, batch_size,
                                                     feature_type, normalization):
        for b, row in enumerate(rows):
            kept[row] = logits[:int(frames[row]), b, :]
    classes = model.cfg.num_classes
    logits = torch.cat(kept, dim=0).contiguous() if kept else \
        torch.empty((0, classes), dtype=torch.float32, device=model.device)
    align_fn = model.align_partial_fn if partial else model.align_long_fn
    path, score, frame_logp, _, status = align_fn(logits, labels)
    code = int(status.cpu().numpy()[0])
    path, frame_logp = path.cpu().numpy(), frame_logp.cpu().numpy()
    hop = hop_samples(model.cfg, drop)
    frame_begin, frame_end = frame_samples(start, length, frames, hop)
    value = float(score.cpu().numpy()[0])
    ok = code == 0 and math.isfinite(value)
    words = words_on_samples(path, labels, frame_begin, frame_end, frame_logp,
                             FLAGS.sampling_rate) if ok else []
    if report is not None:
        offset = np.concatenate([[0], np.cumsum(frames)[:-1]]).astype(np.int64) \
            if len(frames) else np.zeros(0, dtype=np.int64)
        report.update(start=start, length=length, frames=frames, offset=offset, logits=logits,
                      text=text, labels=labels, path=path, frame_logp=frame_logp,
                      frame_begin=frame_begin, frame_end=frame_end, hop_samples=hop,
                      audio=pcm.cpu().numpy())
    total = int(logits.shape[0])
    result = {'status': alignment.STATUS_NAMES[code],
              'score': value if ok else None,
              'score_per_frame': value / total if ok and total > 0 else None,
              'words': words,
              'pieces': len(start),
              'audio_seconds': int(pcm.numel()) / FLAGS.sampling_rate,
              'speech_seconds': int(sum(int(v) for v in length)) / FLAGS.sampling_rate}
    if partial:
        result.update(partial_summary(path, labels, frame_logp) if ok else
                      {'wildcard_frames': 0, 'covered_frames': 0,
                       'score_per_covered_frame': None})
        result['skipped'] = skipped_on_samples(path, labels, frame_begin, frame_end,
                                               FLAGS.sampling_rate) if ok else []
    return result


def partial_summary(path, labels, frame_logp):
    """``{'wildcard_frames', 'covered_frames', 'score_per_covered_frame'}`` of a path over labels
    that hold wildcards: the last is the float64 sum of ``frame_logp`` over the frames outside
    the wildcards, added one by one in time order, over their number."""
    path = np.asarray(path)
    ids = np.asarray([int(v) for v in labels] + [0], dtype=np.int64)
    wild = ((path & 1) == 1) & (ids[np.where(path >= 0, path >> 1, len(ids) - 1)] == ALIGN_WILDCARD)
    covered = np.asarray(frame_logp, dtype=np.float64)[~wild]
    return {'wildcard_frames': int(wild.sum()), 'covered_frames': int(covered.size),
            'score_per_covered_frame':
                float(np.cumsum(covered)[-1]) / covered.size if covered.size else None}


def cut_utterances(words, num_samples, max_seconds=15, min_gap_ms=200, pad_ms=100,
                   min_confidence=None, sampling_rate=16000, barriers=None):
    """Group aligned words into utterances; integer arithmetic on sample positions throughout
    (``words``: 'word', 'start_sample', 'end_sample', 'confidence', 'frames', in time order).

    1. a cut candidate lies after word k when ``start[k+1] - end[k] >= min_gap``, and one after
       the last word;
    2. from word a, ``reach`` is the largest k with ``end[k] - start[a] + 2 pad <= max``: the cut
       is made at the largest candidate ``k <= reach``;
    3. without one, after the k in ``[a, reach]`` with the largest gap behind it (the later on a
       tie), and the utterance is marked ``forced``;
    4. a word that does not fit alone is an utterance of its own, status ``too_long``;
    5. an utterance takes ``pad`` before its first and after its last word, but no more than up
       to the midpoint of the gap to its neighbour, and nothing outside the recording;
    6. status: ``too_long``, else ``short`` (below MIN_EXAMPLE_LENGTH), else ``low_confidence``
       (the mean ``frame_logp`` over its label frames below ``min_confidence``), else ``ok``;
    7. the label is its words joined by one space.

    ``barriers``: the word indices after which a wildcard lies (`skipped_on_samples`'
    ``after_word``; -1: before the first word).  A cut after such a word is mandatory - it is a
    candidate whatever the gap, and ``reach`` never passes it - so no utterance holds audio the
    text does not cover between two of its words.  Rule 5 stands: the gap between the two words
    holds the wildcard's span, and an utterance takes at most ``pad`` of it, never more than half.
    (It may reach into the span at all because the wildcard's border is known to one label frame
    only: the tie rule lets a wildcard take the later frames of the label before it.)  Every
    utterance then carries ``'beside_wildcard'``: its first or its last word borders a wildcard.

    Returns ``{'index', 'first_word', 'last_word', 'start_sample', 'end_sample', 'label',
    'status', 'forced', 'confidence'}`` per utterance, in time order."""
    rate = int(sampling_rate)
    limit = int(max_seconds) * rate
    min_gap = int(min_gap_ms) * rate // 1000
    pad = int(pad_ms) * rate // 1000
    shortest = int(round(MIN_EXAMPLE_LENGTH * rate))
    count = len(words)
    begin = [int(w['start_sample']) for w in words]
    end = [int(w['end_sample']) for w in words]
    gap = [begin[k + 1] - end[k] for k in range(count - 1)]
    candidate = [g >= min_gap for g in gap] + [True]
    barrier = set() if barriers is None else set(int(k) for k in barriers)
    for k in barrier:
        if 0 <= k < count:
            candidate[k] = True
    groups, a = [], 0
    while a < count:
        if end[a] - begin[a] + 2 * pad > limit:
            groups.append((a, a, False, True))
            a += 1
            continue
        reach = a
        while reach + 1 < count and reach not in barrier and \
                end[reach + 1] - begin[a] + 2 * pad <= limit:
            reach += 1
        cuts = [k for k in range(a, reach + 1) if candidate[k]]
        if cuts:
            b, forced = cuts[-1], False
        else:                         # (reach < count - 1: the last word is a candidate)
            widest = max(gap[k] for k in range(a, reach + 1))
            b = max(k for k in range(a, reach + 1) if gap[k] == widest)
            forced = True
        groups.append((a, b, forced, False))
        a = b + 1
    utterances = []
    for index, (a, b, forced, too_long) in enumerate(groups):
        low, high = begin[a] - pad, end[b] + pad
        if a > 0:
            low = max(low, end[a - 1] + (begin[a] - end[a - 1]) // 2)
        if b + 1 < count:
            high = min(high, end[b] + (begin[b + 1] - end[b]) // 2)
        low, high = max(low, 0), min(high, int(num_samples))
        frames = sum(int(w['frames']) for w in words[a:b + 1])
        confidence = None
        if frames > 0 and all(w['confidence'] is not None for w in words[a:b + 1]):
            confidence = sum(w['confidence'] * int(w['frames']) for w in words[a:b + 1]) / frames
        if too_long:
            status = 'too_long'
        elif high - low < shortest:
            status = 'short'
        elif min_confidence is not None and confidence is not None and \
                confidence < min_confidence:
            status = 'low_confidence'
        else:
            status = 'ok'
        utterances.append({'index': index, 'first_word': a, 'last_word': b,
                           'start_sample': low, 'end_sample': high,
                           'label': ' '.join(w['word'] for w in words[a:b + 1]),
                           'status': status, 'forced': forced, 'confidence': confidence})
        if barriers is not None:
            utterances[-1]['beside_wildcard'] = a - 1 in barrier or b in barrier
    return utterances


def report_path(csv_path):
    return os.path.splitext(csv_path)[0] + '.report.jsonl'


def write_corpus(audio, utterances, corpus_out_dir, corpus_out_csv, stem, sampling_rate=16000):
    """The ``ok`` utterances as ``<corpus_out_dir>/<stem>_<index:05d>.wav`` - the recording's own
    int16 samples - and their rows in the manifest ``corpus_out_csv`` (``path;label;length``,
    paths relative to ``corpus_out_dir``, lengths ``'{:.4f}'`` seconds), sorted by length
    ascending, ties in time order, the last row written twice as `synth.write_corpus` does (the
    training reader drops the last row).  `report_path` (next to the CSV) lists EVERY utterance,
    one JSON line each, with its status, span, confidence and ``forced`` (and
    ``beside_wildcard`` where `cut_utterances` set it).  Returns the rows."""
    audio = np.asarray(audio)
    if audio.dtype != np.int16 or audio.ndim != 1:
        raise ValueError('write_corpus: the recording must be int16 mono samples.')
    os.makedirs(corpus_out_dir, exist_ok=True)
    os.makedirs(os.path.dirname(os.path.abspath(corpus_out_csv)), exist_ok=True)
    rows, lines = [], []
    for utt in utterances:
        low, high = int(utt['start_sample']), int(utt['end_sample'])
        line = {'index': utt['index'], 'status': utt['status'], 'forced': utt['forced'],
                'start': round(low / sampling_rate, 6), 'end': round(high / sampling_rate, 6),
                'start_sample': low, 'end_sample': high, 'confidence': utt['confidence'],
                'first_word': utt['first_word'], 'last_word': utt['last_word'],
                'label': utt['label'], 'path': None}
        if 'beside_wildcard' in utt:
            line['beside_wildcard'] = bool(utt['beside_wildcard'])
        if utt['status'] == 'ok':
            name = '{}_{:05d}.wav'.format(stem, utt['index'])
            wavfile.write(os.path.join(corpus_out_dir, name), sampling_rate,
                          np.ascontiguousarray(audio[low:high]))
            line['path'] = name
            rows.append((high - low, utt['index'], name, utt['label']))
        lines.append(line)
    rows.sort(key=lambda row: (row[0], row[1]))
    rows = [(name, label, '{:.4f}'.format(samples / sampling_rate))
            for samples, _, name, label in rows]
    if rows:
        rows.append(rows[-1])
    with open(corpus_out_csv, 'w', encoding='utf-8') as handle:
        handle.write(CSV_DELIMITER.join(CSV_FIELDNAMES) + '\n')
        for row in rows:
            handle.write(CSV_DELIMITER.join(row) + '\n')
    with open(report_path(corpus_out_csv), 'w', encoding='utf-8') as handle:
        for line in lines:
            handle.write(json.dumps(line) + '\n')
    return rows


def check_flags():
    """What the driver needs of the flags, checked before anything is loaded."""
    if FLAGS.nbest:
        raise ValueError('ctc_asr_amd.align_long does not serve --nbest.')
    if not os.path.isfile(FLAGS.input):
        raise ValueError('The input file "{}" does not exist.'.format(FLAGS.input))
    if not os.path.isfile(FLAGS.transcript):
        raise ValueError('The transcript file "{}" does not exist.'.format(FLAGS.transcript))
    if bool(FLAGS.corpus_out_dir) != bool(FLAGS.corpus_out_csv):
        raise ValueError('--corpus_out_dir and --corpus_out_csv go together.')
    if not FLAGS.align_output and not FLAGS.corpus_out_csv:
        raise ValueError('ctc_asr_amd.align_long needs --align_output, or --corpus_out_dir and '
                         '--corpus_out_csv.')


def main(argv=None):
    FLAGS.parse(sys.argv[1:] if argv is None else argv)
    check_flags()
    partial = bool(FLAGS.transcript_wildcard) or FLAGS.align_free_ends
    with open(FLAGS.transcript, 'r', encoding='utf-8') as handle:
        text = handle.read()
    if partial:                # (checked here, before anything is loaded; parsed again below)
        parse_transcript(text, FLAGS.transcript_wildcard, FLAGS.align_free_ends)
    else:
        text = normalize_transcript(text)
    if not torch.cuda.is_available():
        raise SystemExit('ctc_asr_amd.align_long needs an MI355X; no GPU is visible.')
    model = CTCModel(ModelConfig.from_flags(FLAGS), 'cuda', seed=FLAGS.random_seed or 1)
    latest = storage.latest_checkpoint(FLAGS.train_dir)
    if latest is None:
        raise SystemExit('No checkpoint found in {}.'.format(FLAGS.train_dir))
    storage.restore_checkpoint(latest, model, weights='ema' if FLAGS.eval_ema else 'param')
    print('Inputs: {} / {}'.format(FLAGS.input, FLAGS.transcript))
    report = {}
    if partial:
        result = align_recording(model, FLAGS.input, text, report=report,
                                 wildcard=FLAGS.transcript_wildcard,
                                 free_ends=FLAGS.align_free_ends)
    else:
        result = align_recording(model, FLAGS.input, text, report=report)
    print('status {}, {} words on {} pieces, audio {:.2f} s, speech {:.2f} s, score per frame {}'
          .format(result['status'], len(result['words']), result['pieces'],
                  result['audio_seconds'], result['speech_seconds'], result['score_per_frame']))
    skipped = result.get('skipped')
    if skipped is not None:
        print('{} wildcard spans on {} frames, {} frames covered, score per covered frame {}'
              .format(len(skipped), result['wildcard_frames'], result['covered_frames'],
                      result['score_per_covered_frame']))
    if FLAGS.align_output:
        with open(FLAGS.align_output, 'w', encoding='utf-8') as handle:
            for word in result['words']:
                handle.write(json.dumps(word) + '\n')
            for span in skipped or []:
                handle.write(json.dumps(dict({'skipped': True}, **span)) + '\n')
        print('{} words -> {}'.format(len(result['words']), FLAGS.align_output))
    if result['status'] != 'ok':
        return 1
    if FLAGS.corpus_out_csv:
        utterances = cut_utterances(result['words'], len(report['audio']), FLAGS.cut_max_seconds,
                                    FLAGS.cut_min_gap_ms, FLAGS.cut_pad_ms,
                                    parse_cut_min_confidence(FLAGS.cut_min_confidence),
                                    FLAGS.sampling_rate,
                                    None if skipped is None else
                                    [span['after_word'] for span in skipped])
        stem = os.path.splitext(os.path.basename(FLAGS.input))[0]
        rows = write_corpus(report['audio'], utterances, FLAGS.corpus_out_dir,
                            FLAGS.corpus_out_csv, stem, FLAGS.sampling_rate)
        counts = {}
        for utt in utterances:
            counts[utt['status']] = counts.get(utt['status'], 0) + 1
        print('{} utterances ({}) -> {} rows in {}'.format(
            len(utterances), ', '.join('{} {}'.format(v, k) for k, v in sorted(counts.items())),
            max(len(rows) - 1, 0), FLAGS.corpus_out_csv))
    return 0


if __name__ == '__main__':
    sys.exit(main())
