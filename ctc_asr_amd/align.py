"""Corpus aligner: ``python -m ctc_asr_amd.align --align_csv X.csv --align_output Y.jsonl
[model flags]``.

Restores the latest checkpoint in ``train_dir``, runs the model in evaluation mode over a
``path;label;length`` manifest and aligns each row's transcript to its logits on the MI355X
(`CTCModel.align_fn`).  The manifest is read in file order, header dropped and every other row
kept: this is not the training reader, so it has no ``[1:-1]`` quirk that drops the last row.
Rows go through the model ``batch_size`` at a time.  A transcript with a character outside the
alphabet raises ``ValueError``, as training does.  ``--resample_input`` takes recordings of any
sampling rate, channel count and sample format (`input_functions.read_audio`); word times are in
seconds either way.

Output: one JSON object per manifest row, in manifest order::

    {"path": "<as in the manifest>", "status": "ok" | "infeasible" | "bad_row" | "non_finite",
     "score": <log-probability of the best path, null unless ok>,
     "score_per_frame": <score / logit frames, null unless ok and frames > 0>,
     "words": [{"word": "...", "start": <s>, "end": <s>, "confidence": <mean log-prob>}, ...]}

``infeasible``: the audio is too short for the transcript; ``bad_row``: a transcript longer than
the lattice allows; ``non_finite``: the logits hold NaN / inf.  Rows that are not ``ok`` have no
words.
"""

import json
import math
import os
import sys

import torch

from ctc_asr_amd import alignment, storage
from ctc_asr_amd.csv_helper import read_csv_rows
from ctc_asr_amd.input_functions import features_from_files
from ctc_asr_amd.labels import encode
from ctc_asr_amd.model import CTCModel, ModelConfig
from ctc_asr_amd.params import CSV_HEADER_LABEL, CSV_HEADER_PATH, FLAGS


def align_rows(model, rows, corpus_dir, batch_size, drop_every_second_frame=False):
    """Yield one result dict per manifest row (dicts with 'path' and 'label'), in order."""
    hop = alignment.frame_seconds(model.cfg, drop_every_second_frame)
    for start in range(0, len(rows), batch_size):
        chunk = rows[start:start + batch_size]
        labels = [encode(row[CSV_HEADER_LABEL]) for row in chunk]
        paths = [os.path.join(corpus_dir, row[CSV_HEADER_PATH]) for row in chunk]
        feats, lengths = features_from_files(paths, model.device)
        logits, seq_len = model.inference_fn(feats, lengths, training=False)
        model.check_rnn_error()
        path, score, frame_logp, status = model.align_fn(logits, seq_len, labels)
        path, score = path.cpu().numpy(), score.cpu().numpy()
        frame_logp, status = frame_logp.cpu().numpy(), status.cpu().numpy()
        frames = seq_len.cpu().numpy()
        for b, row in enumerate(chunk):
            ok = int(status[b]) == 0
            value = float(score[b]) if ok and math.isfinite(float(score[b])) else None
            yield {'path': row[CSV_HEADER_PATH],
                   'status': alignment.STATUS_NAMES[int(status[b])],
                   'score': value,
                   'score_per_frame': value / int(frames[b]) if value is not None and
                   int(frames[b]) > 0 else None,
                   'words': alignment.segments(path[b], labels[b], hop, frame_logp[b])
                   if ok else []}


def main(argv=None):
    FLAGS.parse(sys.argv[1:] if argv is None else argv)
    if not FLAGS.align_csv or not FLAGS.align_output:
        raise ValueError('ctc_asr_amd.align needs --align_csv and --align_output.')
    if not torch.cuda.is_available():
        raise SystemExit('ctc_asr_amd.align needs an MI355X; no GPU is visible.')
    rows = read_csv_rows(FLAGS.align_csv)[1:]
    model = CTCModel(ModelConfig.from_flags(FLAGS), 'cuda', seed=FLAGS.random_seed or 1)
    latest = storage.latest_checkpoint(FLAGS.train_dir)
    if latest is None:
        raise SystemExit('No checkpoint found in {}.'.format(FLAGS.train_dir))
    storage.restore_checkpoint(latest, model, weights='ema' if FLAGS.eval_ema else 'param')
    count = 0
    with open(FLAGS.align_output, 'w', encoding='utf-8') as handle:
        for result in align_rows(model, rows, FLAGS.corpus_dir, FLAGS.batch_size,
                                 FLAGS.features_drop_every_second_frame):
            handle.write(json.dumps(result) + '\n')
            count += 1
    print('Aligned {} rows of {} -> {}'.format(count, FLAGS.align_csv, FLAGS.align_output))
    return 0


if __name__ == '__main__':
    sys.exit(main())
