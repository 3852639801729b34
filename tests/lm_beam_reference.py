"""Numpy restatement of the CTC beam search with a language model fused in, for the tests of
``ctcasr_ctc_beam_decode_lm``.

The structure, the float32 arithmetic and the tie rule (lowest total first, the youngest node
evicted first) are those of ``oracle/ctc.py::beam_search_decode_single``; added are the three
scorer calls of TensorFlow's ``CTCBeamSearchDecoder`` for a scorer that is a deterministic
weighted automaton over label ids (include/ctcasr.h, K10):

* ``ExpandState``: a child of a node in state ``s`` under label ``c`` is in state ``next[s, c]``
  and carries ``e = score[s, c]``, both for good; the root is in state 0 with ``e = 0``;
* ``GetStateExpansionScore(state, previous) = previous + e``: in the first loop
  ``new.label = lse(new.label, prev + e)`` before ``+ x[label]``, in the second a child's value
  is ``x[c] + (prev + score[s, c])``, in float32 and in that order; an edge of ``-inf`` is no
  candidate and creates no node;
* ``GetStateEndExpansionScore``: ``final[state]`` joins every leaf's total before the best leaf
  is chosen; the returned log-probability is that fused total.

Slow (every insertion scans the beam): keep cases at T <= 60 and width <= 32.
"""

import itertools

import numpy as np

from oracle.ctc import NEG_INF, _f32, _lse32


class _Beam:
    __slots__ = ('parent', 'label', 'children', 'old', 'new', 'serial', 'state', 'e')

    def __init__(self, parent, label, serial, state, e):
        self.parent, self.label, self.serial = parent, label, serial
        self.state, self.e = state, e
        self.children = {}
        self.old = [NEG_INF, NEG_INF, NEG_INF]  # total, blank, label
        self.new = [NEG_INF, NEG_INF, NEG_INF]

    def active(self):
        return self.new[0] != NEG_INF

    def path(self):
        labels, node = [], self
        while node.parent is not None:
            labels.append(node.label)
            node = node.parent
        return labels[::-1]


def beam_search_decode_single(logits, beam_width, lm_next, lm_score, lm_final=None, blank=None,
                              normalization='max'):
    """One utterance: ``logits`` [T, C]; ``lm_next`` int [S, C], ``lm_score`` float [S, C] and
    ``lm_final`` float [S] or None as the kernel takes them (read as float32).  Returns (labels
    list, fused log-probability of the top path)."""
    logits = np.asarray(logits, dtype=np.float32)
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
    best = order(leaves)[0]
    return best.path(), float(best.new[0])


def beam_search_decode(logits, seq_len, beam_width, lm_next, lm_score, lm_final=None, blank=None,
                       normalization='max'):
    """Batch form: ``logits`` [T, B, C]; returns (list of B label lists, logp f32[B])."""
    logits = np.asarray(logits, dtype=np.float32)
    batch = logits.shape[1]
    paths, scores = [], np.zeros(batch, dtype=np.float32)
    for b in range(batch):
        path, score = beam_search_decode_single(logits[:int(seq_len[b]), b], beam_width, lm_next,
                                                lm_score, lm_final, blank, normalization)
        paths.append(path)
        scores[b] = score
    return paths, scores


def automaton_score(label, lm_next, lm_score, lm_final=None):
    """Sum of the edge scores of ``label`` from state 0 plus ``lm_final`` of the end state, in
    float64 - what the fused search adds to ln p_ctc(label)."""
    state, total = 0, 0.0
    for c in label:
        total += float(lm_score[state, c])
        state = int(lm_next[state, c])
    return total + (0.0 if lm_final is None else float(lm_final[state]))
