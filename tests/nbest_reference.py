"""Numpy restatement of the n-best CTC beam search, for the tests of
``ctcasr_ctc_beam_decode_nbest``: the search of ``tests/lm_beam_reference.py``, line for line,
returning EVERY leaf of the final beam as ``(path, total)`` in the order ``(-total, serial)`` -
total descending, the older tree node first among equal totals (include/ctcasr.h, K10).  A zero
one-state scorer stands in for the plain search: with it the fused search is the plain one bit
for bit.

Slow (every insertion scans the beam): keep cases at T <= 60 and width <= 32.
"""

import itertools

import numpy as np

from oracle.ctc import NEG_INF, _f32, _lse32
from tests.lm_beam_reference import _Beam


def zero_scorer(num_classes):
    """(next, score) of the one-state automaton that scores every label 0."""
    return (np.zeros((1, num_classes), dtype=np.int32),
            np.zeros((1, num_classes), dtype=np.float32))


def nbest_single(logits, beam_width, lm_next=None, lm_score=None, lm_final=None, blank=None,
                 normalization='max'):
    """One utterance: ``logits`` [T, C]; the scorer as `lm_beam_reference` takes it, or None for
    the plain search.  Returns [(labels list, float32 total), ...] for every leaf of the final
    beam, in the order (-total, serial)."""
    logits = np.asarray(logits, dtype=np.float32)
    if lm_next is None:
        lm_next, lm_score = zero_scorer(logits.shape[1])
    lm_next = np.asarray(lm_next)
    lm_score = np.asarray(lm_score, dtype=np.float32)
    lm_final = None if lm_final is None else np.asarray(lm_final, dtype=np.float32)
    num_steps, num_classes = logits.shape
    blank = num_classes - 1 if blank is None else blank
    serial = itertools.count()
    root = _Beam(None, -1, next(serial), 0, _f32(0.0))
    root.new = [_f32(0.0), _f32(0.0), NEG_INF]
    leaves = [root]

    def order(nodes):
        return sorted(nodes, key=lambda n: (-n.new[0], n.serial))

    for t in range(num_steps):
        frame = logits[t]
        peak = np.max(frame)
        if normalization == 'log_softmax':
            offset = _f32(peak + _f32(np.log(np.sum(np.exp(frame - peak), dtype=np.float32))))
        else:
            offset = peak
        x = (frame - offset).astype(np.float32)

        branches = order(leaves)
        leaves = []
        for b in branches:
            b.old = list(b.new)
        for b in branches:
            if b.parent is not None:
                if b.parent.active():
                    prev = b.parent.old[1] if b.label == b.parent.label else b.parent.old[0]
                    b.new[2] = _lse32(b.new[2], _f32(prev + b.e))
                b.new[2] = _f32(b.new[2] + x[b.label])
            b.new[1] = _f32(b.old[0] + x[blank])
            b.new[0] = _lse32(b.new[1], b.new[2])
            leaves.append(b)

        def bottom():
            # lowest total; among equal totals the youngest tree node is evicted first
            return min(leaves, key=lambda n: (n.new[0], -n.serial))

        def is_candidate(total):
            if total == NEG_INF:
                return False
            return len(leaves) < beam_width or total > bottom().new[0]

        for b in branches:
            if not is_candidate(b.old[0]):
                continue
            for c_label in range(num_classes):
                if c_label == blank:
                    continue
                edge = lm_score[b.state, c_label]
                if edge == NEG_INF:
                    continue
                child = b.children.get(c_label)
                if child is None:
                    child = _Beam(b, c_label, next(serial), int(lm_next[b.state, c_label]), edge)
                    b.children[c_label] = child
                if child.active():
                    continue
                child.new[1] = NEG_INF
                prev = b.old[1] if c_label == b.label else b.old[0]
                child.new[2] = _f32(x[c_label] + _f32(prev + edge))
                child.new[0] = child.new[2]
                if is_candidate(child.new[0]):
                    if len(leaves) == beam_width:
                        worst = bottom()
                        worst.new = [NEG_INF, NEG_INF, NEG_INF]
                        leaves.remove(worst)
                    leaves.append(child)
                else:
                    child.old = [NEG_INF, NEG_INF, NEG_INF]
                    child.new = [NEG_INF, NEG_INF, NEG_INF]

    if lm_final is not None:
        for leaf in leaves:
            leaf.new[0] = _f32(leaf.new[0] + lm_final[leaf.state])
    return [(leaf.path(), np.float32(leaf.new[0])) for leaf in order(leaves)]


def nbest(logits, seq_len, beam_width, lm_next=None, lm_score=None, lm_final=None, blank=None,
          normalization='max'):
    """Batch form: ``logits`` [T, B, C]; returns one `nbest_single` list per utterance."""
    logits = np.asarray(logits, dtype=np.float32)
    return [nbest_single(logits[:int(seq_len[b]), b], beam_width, lm_next, lm_score, lm_final,
                         blank, normalization) for b in range(logits.shape[1])]
