"""Language models for the fused CTC beam search (`hip.ctc_beam_decode_lm`; no counterpart in
the reference).

The search takes a **deterministic weighted automaton over label ids** - TensorFlow's
``BeamScorer`` with an integer state:

* ``next  int32 [S, C]``: the state after label ``c`` in state ``s``; state 0 is the start state;
* ``score float [S, C]``: the expansion score of that edge; ``-inf`` forbids it;
* ``final float [S]``, optional: the end score of a hypothesis that ends in ``s``.

The blank's column is never read.  `LmScorer` holds and validates such tables,
`build_char_ngram` compiles an interpolated Witten-Bell character n-gram to one (back-off resolved
at build time: every edge has its score, no back-off arcs at decode time), and

    python -m ctc_asr_amd.lm --lm_corpus_csv train.csv --lm_order 5 --lm_path out.npz

builds one from the transcripts of a ``path;label;length`` manifest (header row dropped, every
other row kept, characters through `labels.ctoi`: a character outside the alphabet raises
``ValueError`` as in training).  The drivers load it with ``--lm_path`` and scale it with
``--lm_weight`` / ``--lm_bonus``.
"""

import sys

import numpy as np


class LmScorer:
    """Validated automaton tables.  ``score`` / ``final`` keep the precision they come in
    (float64 log-probabilities from `build_char_ngram`); `scaled` folds weight and bonus in and
    rounds to the float32 the kernel reads.  ``order`` is carried for `save` (None: not an
    n-gram).  Raises ``ValueError`` for wrong shapes, a ``next`` entry outside [0, S), NaN or
    +inf - before anything is uploaded."""

    def __init__(self, next, score, final=None, order=None):
        next_, score = np.asarray(next), np.asarray(score)
        if next_.ndim != 2 or next_.shape[0] < 1 or next_.shape[1] < 2:
            raise ValueError('LmScorer: next must be [S >= 1, C >= 2] (got shape {}).'
                             .format(next_.shape))
        if not np.issubdtype(next_.dtype, np.integer):
            raise ValueError('LmScorer: next must hold integers (got {}).'.format(next_.dtype))
        if score.shape != next_.shape:
            raise ValueError('LmScorer: score has shape {}, next {}.'
                             .format(score.shape, next_.shape))
        states = next_.shape[0]
        if next_.min() < 0 or next_.max() >= states:
            raise ValueError('LmScorer: next holds states outside [0, {}).'.format(states))
        score = self._floats('score', score)
        if final is not None:
            final = np.asarray(final)
            if final.shape != (states,):
                raise ValueError('LmScorer: final has shape {}, expected ({},).'
                                 .format(final.shape, states))
            final = self._floats('final', final)
        self.next = np.ascontiguousarray(next_, dtype=np.int32)
        self.score, self.final = score, final
        self.order = None if order is None else int(order)
        self._device = {}

    @staticmethod
    def _floats(name, values):
        if values.dtype != np.float32:
            values = values.astype(np.float64)
        # (what the kernel reads is the float32 rounding: a finite float64 must stay finite)
        with np.errstate(over='ignore'):
            rounded = values.astype(np.float32)
        if np.isnan(values).any() or np.isposinf(rounded).any():
            raise ValueError('LmScorer: {} holds NaN or +inf.'.format(name))
        return np.ascontiguousarray(values)

    @property
    def num_states(self):
        return self.next.shape[0]

    @property
    def num_classes(self):
        return self.next.shape[1]

    def scaled(self, weight=1.0, bonus=0.0):
        """The scorer the kernel takes: ``score = f32(weight * lnP + bonus)`` and ``final =
        f32(weight * lnP_eos)``, computed in float64 and rounded once.  A forbidden edge (-inf)
        stays forbidden at every weight, 0 included."""
        weight, bonus = float(weight), float(bonus)
        if not (np.isfinite(weight) and np.isfinite(bonus)):
            raise ValueError('LmScorer.scaled: weight and bonus must be finite.')

        def scale(values, add):
            values = values.astype(np.float64)
            safe = np.where(np.isneginf(values), 0.0, values)
            return np.where(np.isneginf(values), -np.inf, weight * safe + add).astype(np.float32)

        return LmScorer(self.next, scale(self.score, bonus),
                        None if self.final is None else scale(self.final, 0.0), self.order)

    def sequence_scores(self, rows):
        """float64 [len(rows)]: for each label row the sum of its edge scores from state 0 plus
        ``final`` of the state it ends in - what the fused search adds to a hypothesis, and
        what a second-pass model gives one of an n-best list.  ``-inf`` (a forbidden edge or
        end) passes through.  Raises ``ValueError`` for a label outside [0, C)."""
        totals = np.zeros(len(rows), dtype=np.float64)
        for i, row in enumerate(rows):
            state, total = 0, 0.0
            for c in row:
                c = int(c)
                if not 0 <= c < self.num_classes:
                    raise ValueError('LmScorer.sequence_scores: label {} outside [0, {}).'
                                     .format(c, self.num_classes))
                total += float(self.score[state, c])
                state = int(self.next[state, c])
            if self.final is not None:
                total += float(self.final[state])
            totals[i] = total
        return totals

    def to(self, device):
        """(next int32 [S, C], score f32 [S, C], final f32 [S] or None) on ``device``; uploaded
        once per device and cached."""
        import torch
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if device not in self._device:
            self._device[device] = (
                torch.from_numpy(self.next).to(device),
                torch.from_numpy(self.score.astype(np.float32)).to(device),
                None if self.final is None
                else torch.from_numpy(self.final.astype(np.float32)).to(device))
        return self._device[device]

    def save(self, path):
        """``.npz`` of the arrays plus ``order`` (0: none) and ``num_classes``; no pickle."""
        arrays = {'next': self.next, 'score': self.score,
                  'order': np.int64(self.order or 0), 'num_classes': np.int64(self.num_classes)}
        if self.final is not None:
            arrays['final'] = self.final
        with open(path, 'wb') as handle:
            np.savez(handle, **arrays)


def load(path, num_classes=None):
    """The `LmScorer` of a `save`d file; ``num_classes`` (the model's) must match the file's."""
    with np.load(path, allow_pickle=False) as data:
        stored = int(data['num_classes'])
        if num_classes is not None and stored != int(num_classes):
            raise ValueError('{}: built for {} classes, the model has {}.'
                             .format(path, stored, int(num_classes)))
        scorer = LmScorer(data['next'], data['score'],
                          data['final'] if 'final' in data.files else None,
                          int(data['order']) or None)
    if scorer.num_classes != stored:
        raise ValueError('{}: num_classes {} does not match its tables.'.format(path, stored))
    return scorer


def from_flags(num_classes):
    """The scaled scorer of ``--lm_path`` / ``--lm_weight`` / ``--lm_bonus`` for a model of
    ``num_classes``; None when ``--lm_path`` is unset."""
    from ctc_asr_amd.params import FLAGS
    if not FLAGS.lm_path:
        return None
    return load(FLAGS.lm_path, num_classes).scaled(FLAGS.lm_weight, FLAGS.lm_bonus)


def rescorer_from_flags(num_classes):
    """The scaled scorer of ``--rescore_lm_path`` / ``--rescore_lm_weight`` /
    ``--rescore_lm_bonus``, which re-ranks the n-best list on the host; None when unset."""
    from ctc_asr_amd.params import FLAGS
    if not FLAGS.rescore_lm_path:
        return None
    return load(FLAGS.rescore_lm_path, num_classes).scaled(FLAGS.rescore_lm_weight,
                                                           FLAGS.rescore_lm_bonus)


def build_char_ngram(label_rows, order, num_classes, blank=None):
    """Interpolated Witten-Bell n-gram of ``order`` over label ids (the space is a label like any
    other), with an end-of-sentence event, in float64.  The blank is ``num_classes - 1`` unless ``blank`` names another id.

    Counts: every row, with the end event appended, gives one (context, event) observation per
    position and context length 0 .. order - 1 (shorter at the start of a row: no start padding).
    With c(h, w) those counts, c(h) their sum over w and n(h) the number of distinct w after h,

        P(w | h) = (c(h, w) + n(h) * P(w | h')) / (c(h) + n(h)),    h' = h less its oldest label,

    and below the empty context the uniform distribution over the num_classes - 1 labels and the
    end event.  States are the observed contexts - suffix-closed by construction -, the empty one
    first; ``next[s, c]`` is the longest suffix of ``context(s) + c`` that is a state.  Returns an
    `LmScorer` with ``score[s, c] = ln P(c | s)`` (blank column: -inf) and ``final[s] =
    ln P(end | s)``: each state's row and its end event sum to one."""
    order, classes = int(order), int(num_classes)
    if order < 1:
        raise ValueError('build_char_ngram: order must be >= 1.')
    if classes < 2:
        raise ValueError('build_char_ngram: num_classes must be >= 2.')
    blank, end = classes - 1 if blank is None else int(blank), classes
    if not 0 <= blank < classes:
        raise ValueError('build_char_ngram: blank outside [0, {}).'.format(classes))
    counts = {(): np.zeros(classes + 1)}
    for row in label_rows:
        row = [int(v) for v in row]
        if any(v < 0 or v >= classes or v == blank for v in row):
            raise ValueError('build_char_ngram: label outside [0, {}) or the blank.'
                             .format(classes))
        events = row + [end]
        for i, event in enumerate(events):
            for m in range(min(order - 1, i) + 1):
                context = tuple(row[i - m:i])
                if context not in counts:
                    counts[context] = np.zeros(classes + 1)
                counts[context][event] += 1.0
    contexts = sorted(counts, key=lambda h: (len(h), h))       # shorter first: () is state 0
    index = {h: s for s, h in enumerate(contexts)}
    uniform = np.full(classes + 1, 1.0 / classes)
    uniform[blank] = 0.0
    prob = np.empty((len(contexts), classes + 1))
    for s, h in enumerate(contexts):
        lower = prob[index[h[1:]]] if h else uniform
        seen = float(np.count_nonzero(counts[h]))
        total = float(counts[h].sum())
        prob[s] = (counts[h] + seen * lower) / (total + seen) if total > 0 else lower
    next_ = np.zeros((len(contexts), classes), dtype=np.int32)
    for s, h in enumerate(contexts):
        for c in range(classes):
            if c == blank:
                next_[s, c] = s
                continue
            target = (h + (c,))[-(order - 1):] if order > 1 else ()
            while target not in index:
                target = target[1:]
            next_[s, c] = index[target]
    with np.errstate(divide='ignore'):
        log_prob = np.log(prob)
    return LmScorer(next_, log_prob[:, :classes], log_prob[:, end], order)


def corpus_label_rows(csv_path):
    """Label-id rows of a manifest's transcripts, in file order."""
    from ctc_asr_amd.csv_helper import read_csv_rows
    from ctc_asr_amd.labels import ctoi
    from ctc_asr_amd.params import CSV_HEADER_LABEL
    return [[ctoi(ch) for ch in row[CSV_HEADER_LABEL]] for row in read_csv_rows(csv_path)[1:]]


def main(argv=None):
    from ctc_asr_amd.params import FLAGS
    FLAGS.parse(sys.argv[1:] if argv is None else argv)
    if not FLAGS.lm_corpus_csv or not FLAGS.lm_path:
        raise ValueError('ctc_asr_amd.lm needs --lm_corpus_csv and --lm_path.')
    rows = corpus_label_rows(FLAGS.lm_corpus_csv)
    scorer = build_char_ngram(rows, FLAGS.lm_order, FLAGS.num_classes)
    scorer.save(FLAGS.lm_path)
    print('Order-{} character model of {} transcripts, {} states -> {}'.format(
        FLAGS.lm_order, len(rows), scorer.num_states, FLAGS.lm_path))
    return 0


if __name__ == '__main__':
    sys.exit(main())
