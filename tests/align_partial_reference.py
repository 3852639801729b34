"""Reference for ``ctcasr_ctc_align_partial`` (K25): the wildcard is one more class.

Append to the device's own fp32 log-softmax table [T, C] a column C that holds the row maximum
(``fill``: what the greedy path emits) and give the wildcard the id C: the result is
`tests.align_reference.viterbi` on that table of C + 1 classes, for the same reasons
`tests.align_long_reference.on_table` equals K21 - one fp64 add of an fp32 value per cell, the
first maximum in the order s, s - 1, s - 2.  The maximum of finite floats does not depend on the
order it is taken in, so ``fill`` is exact however the kernel walks the row.  Path, fp64 score and
frame_logp must be EQUAL, bit for bit.

Also here: the status rules with wildcards, and a restatement of `align_long.parse_transcript`
written from its contract, not from its code.
"""

import itertools
import re

import numpy as np

from oracle import ctc as octc
from tests import align_reference as ref

WILDCARD = -1


def augmented(table, label):
    """(table with the fill column appended, float64 [T, C + 1]; label with C for a wildcard)."""
    table = np.asarray(table)
    classes = table.shape[1]
    fill = table.max(axis=1, keepdims=True) if table.shape[0] else table[:, :1]
    wide = np.concatenate([table, fill], axis=1).astype(np.float64)
    return wide, [classes if int(v) == WILDCARD else int(v) for v in label]


def required_time(label):
    """L + adjacent repeats; a wildcard is a label and never a repeat (two side by side are
    refused before this counts)."""
    label = [int(v) for v in label]
    return len(label) + sum(1 for a, b in zip(label, label[1:]) if a == b and a != WILDCARD)


def expected_status(logits, label, blank):
    """2 (a label that is neither the wildcard nor a valid non-blank class, or two wildcards
    side by side) before 1 (T < L + repeats) before 3 (a non-finite logit)."""
    num_steps, classes = logits.shape
    label = [int(v) for v in label]
    if any(v != WILDCARD and (v < 0 or v >= classes or v == blank) for v in label):
        return 2
    if any(a == WILDCARD and b == WILDCARD for a, b in zip(label, label[1:])):
        return 2
    if num_steps < required_time(label):
        return 1
    if not np.isfinite(logits).all():
        return 3
    return 0


def on_table(table, label, blank):
    """(score float64, path int32[T], frame_logp float32[T]) of the best path on ``table``
    float32 [T, C] for a label row that may hold wildcards; the sequence must have a path."""
    table = np.asarray(table)
    assert table.dtype == np.float32
    wide, ids = augmented(table, label)
    score, path = ref.viterbi(None, ids, blank, logp=wide)
    assert path is not None
    ext = np.asarray(octc.extended_labels(ids, blank))
    path = np.asarray(path, dtype=np.int32).reshape(-1)
    wide32 = np.concatenate([table, table.max(axis=1, keepdims=True)], axis=1) \
        if len(path) else table
    frame_logp = wide32[np.arange(len(path)), ext[path]] if len(path) else \
        np.zeros(0, dtype=np.float32)
    return np.float64(score), path, frame_logp.astype(np.float32)


def wildcard_frames(path, label):
    """bool [T]: the frames the path spends in a wildcard."""
    path = np.asarray(path)
    ids = np.asarray([int(v) for v in label] + [0])
    return ((path & 1) == 1) & (ids[np.where(path >= 0, path >> 1, len(ids) - 1)] == WILDCARD)


def brute_force(table, label, blank):
    """(best score, the state paths that reach it) over EVERY legal state path of the lattice of
    ``label`` with wildcards, scored on the augmented table by a sequential float64 sum; (-inf,
    []) when there is none.  Exponential: T <= 6."""
    wide, ids = augmented(np.asarray(table, dtype=np.float32), label)
    ext = octc.extended_labels(ids, blank)
    size, num_steps = len(ext), wide.shape[0]
    best, winners = -np.inf, []
    # every monotone walk with moves 0, 1, 2 from state 0 or 1; `is_valid_path` keeps the legal
    walks = itertools.product((0, 1), *[range(3)] * max(num_steps - 1, 0))
    for path in (list(itertools.accumulate(walk)) for walk in walks):
        if path[-1] >= size or ref.is_valid_path(path, ids, blank, num_steps) is not None:
            continue
        score = 0.0
        for t, s in enumerate(path):
            score = wide[t, ext[s]] if t == 0 else score + wide[t, ext[s]]
        if score > best:
            best, winners = score, [list(path)]
        elif score == best:
            winners.append(list(path))
    return best, winners


def parse_transcript(text, wildcard='', free_ends=False):
    """`align_long.parse_transcript`, restated: returns (text, label ids) or raises ValueError.
    Alphabet of ctc_asr_amd.labels: space 1, a..z 2..27."""
    tokens = [(m.group(0), m.start()) for m in re.finditer(r'\S+', text)]
    pieces, current = [], []              # pieces: lists of words, None for a wildcard
    for token, start in tokens:
        if wildcard and token == wildcard:
            pieces.extend([current, None])
            current = []
            continue
        for offset, char in enumerate(token, start):
            if char.isdigit():
                raise ValueError('digit at offset {}'.format(offset))
        spelled = ''.join(c.lower() if 'a' <= c.lower() <= 'z' and len(c.lower()) == 1 else
                          ('' if c in "'’" else ' ') for c in token)
        current.extend(spelled.split())
    pieces.append(current)
    merged = []                           # drop empty runs, then merge neighbouring wildcards
    for piece in pieces:
        if piece is None:
            if not merged or merged[-1] is not None:
                merged.append(None)
        elif piece:
            merged.append(piece)
    if not any(piece for piece in merged):
        raise ValueError('nothing is left')
    shown = [wildcard if piece is None else ' '.join(piece) for piece in merged]
    if free_ends and merged[0] is not None:
        merged.insert(0, None)
        shown.insert(0, '*')
    if free_ends and merged[-1] is not None:
        merged.append(None)
        shown.append('*')
    labels = []
    for piece in merged:
        if piece is None:
            labels.append(WILDCARD)
        else:
            labels.extend(1 if c == ' ' else ord(c) - ord('a') + 2 for c in ' '.join(piece))
    return ' '.join(shown), labels
