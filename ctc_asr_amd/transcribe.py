"""Transcribe a long recording: ``python -m ctc_asr_amd.transcribe --input long.wav
[--timestamps] [--lm_path ...] [--eval_ema] [--transcribe_output pieces.jsonl]``.

`predict` runs one utterance that fits the model; a lecture or a meeting does not.  Here the
recording is uploaded once, cut at its pauses (`vad.segment`: one pass over the PCM on the
MI355X, the decision on the host), and the pieces go through the model in batches:

1. ``read_wav``, one upload of the PCM (under ``--resample_input``: any WAV, uploaded in its own
   layout and converted to 16 kHz mono int16 by ``hip.resample``; every length and time below is
   then counted on the converted recording, and times stay seconds of the recording);
2. ``vad.segment`` -> the table of pieces ``(start, length)`` in samples, in time order;
3. pieces ordered by length, longest first (ties in time order), ``--batch_size`` to a batch, so
   that a batch pads little;
4. per batch ``hip.gather_segments`` (one launch lays the pieces out as rows) -> ``hip.features``
   with the flags' feature settings -> ``inference_fn(training=False)``;
5. the logits of several batches are decoded in one launch (`CTCModel.decode_many`, as
   `evaluate` does), with the language model of ``--lm_path`` when given;
6. with ``--timestamps`` each batch's texts are aligned to its logits (`CTCModel.align_fn`) and
   the word times shifted by the piece's start.

Nothing augments here, whatever the flags say.  ``--nbest`` is refused: a list per piece is not
a list for the recording.
"""

import json
import os
import sys
import time

import numpy as np
import torch

from ctc_asr_amd import alignment, hip, lm, storage, vad
from ctc_asr_amd.input_functions import _check_feature_args, load_audio, read_wav, upload_audio
from ctc_asr_amd.model import CTCModel, ModelConfig
from ctc_asr_amd.params import FLAGS


def batch_order(lengths, batch_size):
    """Lists of piece indices, one per batch: longest first, ties in time order."""
    order = sorted(range(len(lengths)), key=lambda i: (-int(lengths[i]), i))
    return [order[i:i + batch_size] for i in range(0, len(order), batch_size)]


def assemble(start, length, texts, num_samples, words=None, sampling_rate=16000):
    """The result of `transcribe` from per-piece results in TIME order: ``start`` / ``length`` in
    samples, ``texts`` one string per piece, ``words`` (optional) one `alignment.segments` list per
    piece with times counted from the piece's start."""
    segments = []
    for i in range(len(texts)):
        begin = int(start[i]) / sampling_rate
        piece = {'start': round(begin, 6),
                 'end': round((int(start[i]) + int(length[i])) / sampling_rate, 6),
                 'plaintext': texts[i]}
        if words is not None:
            piece['words'] = [dict(word, start=round(word['start'] + begin, 6),
                                   end=round(word['end'] + begin, 6)) for word in words[i]]
        segments.append(piece)
    return {'plaintext': ' '.join(text for text in texts if text),
            'segments': segments,
            'audio_seconds': num_samples / sampling_rate,
            'speech_seconds': int(sum(int(v) for v in length)) / sampling_rate}


class _Clock:
    """Wall time per stage, device work included (a synchronisation per reading): only kept when
    the caller asks for timings."""

    def __init__(self, timings):
        self.timings, self.last = timings, None
        if timings is not None:
            torch.cuda.synchronize()
            self.last = time.perf_counter()

    def lap(self, stage):
        if self.timings is None:
            return
        torch.cuda.synchronize()
        now = time.perf_counter()
        self.timings[stage] = self.timings.get(stage, 0.0) + now - self.last
        self.last = now


def upload_recording(model, wav_path, timings=None):
    """(int16 device tensor of the recording, the `_Clock` started after the file was read):
    ``read_wav`` and one upload, or under ``--resample_input`` any WAV, uploaded in its own layout
    and converted on the device ('upload' holds both)."""
    if FLAGS.resample_input:
        rate, audio = load_audio(wav_path)
        clock = _Clock(timings)
        pcm = upload_audio(rate, audio, model.device, wav_path)
    else:
        audio = read_wav(wav_path)
        clock = _Clock(timings)
        pcm = torch.from_numpy(np.ascontiguousarray(audio)).to(model.device)
    clock.lap('upload')
    return pcm, clock


def forward_pieces(model, pcm, start, length, batch_size, feature_type, normalization):
    """The pieces ``(start, length)`` of `vad.segment` through the model, a batch at a time in
    `batch_order`: yields ``(rows, logits [T, B, C], seq_len)`` per batch, ``rows`` the indices
    of the batch's pieces.  Per batch one `hip.gather_segments`, `hip.features` with the flags'
    feature settings and ``inference_fn(training=False)``: `transcribe` and
    `align_long.align_recording` launch the same work in the same order."""
    if not len(start):
        return
    seg_start = torch.from_numpy(start).to(model.device)
    seg_len = torch.from_numpy(length).to(model.device)
    for rows in batch_order(length, batch_size):
        index = torch.tensor(rows, dtype=torch.int64, device=model.device)
        batch, num = hip.gather_segments(pcm, seg_start[index], seg_len[index],
                                         max_samples=int(length[rows[0]]))
        feats, lengths = hip.features(batch, num, feature_type, normalization,
                                      FLAGS.features_drop_every_second_frame,
                                      FLAGS.sampling_rate)
        logits, seq_len = model.inference_fn(feats, lengths, training=False)
        model.check_rnn_error()
        yield rows, logits, seq_len


def transcribe(model, wav_path, timestamps=False, scorer=None, nbest=0, settings=None,
               batch_size=None, timings=None, report=None):
    """{'plaintext', 'segments', 'audio_seconds', 'speech_seconds'} of one recording.
    ``segments``: one ``{'start', 'end', 'plaintext'[, 'words']}`` per piece in time order, in
    seconds of the recording; ``plaintext``: the non-empty piece texts joined by one space.  A
    recording without speech has no segments and an empty text.  ``settings``: a
    `vad.VadSettings` (default: from the flags); ``timings``: a dict that receives the seconds
    spent in 'upload', 'segmentation', 'forward', 'decode' and 'alignment'; ``report``: a dict
    that receives the table in samples ('start', 'length'), the 'threshold' and the 'decoded'
    label list of every piece, in time order."""
    if nbest:
        raise ValueError('transcribe: --nbest is not served for long recordings (an n-best list '
                         'per piece is no list for the recording); use predict on one piece.')
    settings = vad.VadSettings.from_flags(FLAGS) if settings is None else settings
    batch_size = FLAGS.batch_size if batch_size is None else int(batch_size)
    feature_type, normalization = _check_feature_args(None, None)
    pcm, clock = upload_recording(model, wav_path, timings)
    start, length, threshold = vad.segment(pcm, settings)
    clock.lap('segmentation')
    count = len(start)
    texts, words, labels = [''] * count, [[] for _ in range(count)], [[] for _ in range(count)]
    hop = alignment.frame_seconds(model.cfg, FLAGS.features_drop_every_second_frame)
    pending = []

    def decode_pending():
        results = model.decode_many([(logits, seq_len, None) for _, logits, seq_len in pending],
                                    scorer=scorer)
        clock.lap('decode')
        for (rows, logits, seq_len), (decoded, plaintext, _) in zip(pending, results):
            for b, row in enumerate(rows):
                texts[row], labels[row] = str(plaintext[b]), decoded[b]
            if timestamps:
                ids = [[v for v in row if v != 0] for row in decoded]   # (id 0 is no label)
                path, _, frame_logp, _ = model.align_fn(logits, seq_len, ids)
                path, frame_logp = path.cpu().numpy(), frame_logp.cpu().numpy()
                # a decode the alignment cannot place (status != 0) leaves a path of -1: no words
                for b, row in enumerate(rows):
                    words[row] = alignment.segments(path[b], ids[b], hop, frame_logp[b])
        clock.lap('alignment')
        del pending[:]

    for rows, logits, seq_len in forward_pieces(model, pcm, start, length, batch_size,
                                                feature_type, normalization):
        pending.append((rows, logits, seq_len))
        clock.lap('forward')
        # (the longest pieces bound the prefix-tree pool: size the group on them)
        group = model.decode_group_size(max(int(item[1].shape[0]) for item in pending),
                                        int(logits.shape[1]), scorer=scorer)
        if len(pending) >= group:
            decode_pending()
    if pending:
        decode_pending()
    if report is not None:
        report.update(start=start, length=length, threshold=threshold, decoded=labels)
    return assemble(start, length, texts, int(pcm.numel()), words if timestamps else None,
                    FLAGS.sampling_rate)


def main(argv=None):
    FLAGS.parse(sys.argv[1:] if argv is None else argv)
    if not os.path.isfile(FLAGS.input):
        raise ValueError('The input file "{}" does not exist.'.format(FLAGS.input))
    if FLAGS.nbest:
        raise ValueError('ctc_asr_amd.transcribe does not serve --nbest.')
    if not torch.cuda.is_available():
        raise SystemExit('ctc_asr_amd.transcribe needs an MI355X; no GPU is visible.')
    model = CTCModel(ModelConfig.from_flags(FLAGS), 'cuda', seed=FLAGS.random_seed or 1)
    latest = storage.latest_checkpoint(FLAGS.train_dir)
    if latest is None:
        raise SystemExit('No checkpoint found in {}.'.format(FLAGS.train_dir))
    storage.restore_checkpoint(latest, model, weights='ema' if FLAGS.eval_ema else 'param')
    print('Inputs: {}'.format(FLAGS.input))
    began = time.perf_counter()
    result = transcribe(model, FLAGS.input, FLAGS.timestamps,
                        lm.from_flags(model.cfg.num_classes))
    wall = time.perf_counter() - began
    lines = [json.dumps(piece) for piece in result['segments']]
    if FLAGS.transcribe_output:
        with open(FLAGS.transcribe_output, 'w', encoding='utf-8') as handle:
            for line in lines:
                handle.write(line + '\n')
        print('{} pieces -> {}'.format(len(lines), FLAGS.transcribe_output))
    else:
        for line in lines:
            print(line)
    print(result['plaintext'])
    print('audio {:.2f} s, speech {:.2f} s, wall {:.2f} s'.format(
        result['audio_seconds'], result['speech_seconds'], wall))
    return 0


if __name__ == '__main__':
    sys.exit(main())
