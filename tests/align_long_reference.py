"""Reference for ``ctcasr_ctc_align_long`` (K21): `tests.align_reference.viterbi` on the DEVICE'S
OWN fp32 log-softmax table.

Given that table, `viterbi` performs the kernel's additions and comparisons one for one: one fp64
add of an fp32 value per cell, and numpy's ``argmax`` keeps the first maximum in the order s,
s - 1, s - 2, which is the kernel's strict ``>`` in that order.  So path, fp64 score and
frame_logp must be EQUAL, bit for bit: no margin rule, no tolerance.
"""

import numpy as np

from oracle import ctc as octc
from tests import align_reference as ref


def required_time(label):
    return octc.required_time([int(v) for v in label])


def expected_status(logits, label, blank):
    """K11's codes for one sequence: 2 before 1 before 3."""
    num_steps, classes = logits.shape
    if any(v < 0 or v >= classes or v == blank for v in label):
        return 2
    if num_steps < required_time(label):
        return 1
    if not np.isfinite(logits).all():
        return 3
    return 0


def on_table(table, label, blank):
    """(score float64, path int32[T], frame_logp float32[T]) of the best path on ``table``
    float32 [T, C]; the sequence must have a path."""
    table = np.asarray(table)
    assert table.dtype == np.float32
    label = [int(v) for v in label]
    score, path = ref.viterbi(None, label, blank, logp=table.astype(np.float64))
    assert path is not None
    ext = np.asarray(octc.extended_labels(label, blank))
    path = np.asarray(path, dtype=np.int32).reshape(-1)
    frame_logp = table[np.arange(len(path)), ext[path]] if len(path) else \
        np.zeros(0, dtype=np.float32)
    return np.float64(score), path, frame_logp.astype(np.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
