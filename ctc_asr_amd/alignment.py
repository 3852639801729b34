"""CTC forced alignment on the host side: frame times, and states -> labels -> timed words.

The alignment itself runs on the MI355X (``ctcasr_ctc_align``, `CTCModel.align_fn`): per
utterance it gives the state of the best path at every logit frame (even state: blank, odd state
2k + 1: label position k), the path's log-probability and the log-softmax of the class it emits
at each frame.  This module turns one such row into word spans.
"""

import numpy as np

from ctc_asr_amd.labels import decode
from ctc_asr_amd.params import WIN_STEP

SPACE_ID = 1          # labels.ALPHABET[0]
STATUS_NAMES = {0: 'ok', 1: 'infeasible', 2: 'bad_row', 3: 'non_finite'}


def frame_seconds(cfg, drop_every_second_frame):
    """Seconds per logit frame: the feature hop (WIN_STEP), x 2 for 'ds2' (the time stride of
    `ModelConfig.output_time`), x 2 when every second feature frame is dropped."""
    step = WIN_STEP * (2 if cfg.used_model == 'ds2' else 1)
    return step * (2 if drop_every_second_frame else 1)


def label_spans(path_row, num_labels):
    """[(first frame, last frame)] per label position: the frames of its odd state."""
    path_row = np.asarray(path_row)
    spans = []
    for k in range(num_labels):
        frames = np.nonzero(path_row == 2 * k + 1)[0]
        spans.append((int(frames[0]), int(frames[-1])) if frames.size else None)
    return spans


def segments(path_row, labels_row, frame_seconds, frame_logp_row=None):
    """Words of one aligned row: a list of ``{'word', 'start', 'end', 'confidence'}``.

    Words are the runs of labels between space labels (id 1).  ``start`` is the first frame of
    the word's first label times ``frame_seconds``, ``end`` the last frame of its last label plus
    one, times ``frame_seconds``; ``confidence`` is the mean ``frame_logp`` over the frames of
    the word's labels (None without ``frame_logp_row``).  A row without a path (all -1) has no
    words."""
    labels_row = [int(v) for v in labels_row]
    path_row = np.asarray(path_row)
    if path_row.size == 0 or (path_row < 0).all():
        return []
    spans = label_spans(path_row, len(labels_row))
    words, current = [], []

    def close():
        if not current:
            return
        first, last = spans[current[0]][0], spans[current[-1]][1]
        confidence = None
        if frame_logp_row is not None:
            odd = np.isin(path_row, [2 * k + 1 for k in current])
            confidence = float(np.mean(np.asarray(frame_logp_row, dtype=np.float64)[odd]))
        words.append({'word': decode([labels_row[k] for k in current]),
                      'start': round(first * frame_seconds, 6),
                      'end': round((last + 1) * frame_seconds, 6),
                      'confidence': confidence})
        current.clear()

    for k, label in enumerate(labels_row):
        if label == SPACE_ID:
            close()
        else:
            current.append(k)
    close()
    return words
