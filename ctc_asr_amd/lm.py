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

A **word** n-gram does not fit that dense form: its decode-time automaton is the composition of
a lexicon trie with the n-gram's contexts.  `build_word_ngram` keeps it implicit (`WordLmScorer`:
a trie over label ids plus back-off tables; `hip.ctc_beam_decode_wordlm` looks a word's score up
on the device when a hypothesis closes the word), and ``--lm_unit word`` builds one from the same
manifest and / or the plain text lines of ``--lm_corpus_text``.  `load` tells the two kinds of
file apart; every driver that takes ``--lm_path`` takes either.
"""

import sys

import numpy as np


class LmScorer:
    """Validated automaton tables.  ``score`` / ``final`` keep the precision they come in
    (float64 log-probabilities from `build_char_ngram`); `scaled` folds weight and bonus in and
    rounds to the float32 the kernel reads.  ``order`` is carried for `save` (None: not an
    n-gram).  Raises ``ValueError`` for wrong shapes, a ``next`` entry outside [0, S), NaN or
    +inf - before anything is uploaded."""

    kind = 'dense'      # what `hip.ctc_beam_search` launches for this scorer

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
    """The `LmScorer` or `WordLmScorer` of a `save`d file (a file without ``kind`` is a character
    model); ``num_classes`` (the model's) must match the file's."""
    with np.load(path, allow_pickle=False) as data:
        stored = int(data['num_classes'])
        if num_classes is not None and stored != int(num_classes):
            raise ValueError('{}: built for {} classes, the model has {}.'
                             .format(path, stored, int(num_classes)))
        kind = str(data['kind']) if 'kind' in data.files else 'char_ngram'
        if kind == WORD_KIND:
            for name in WORD_ARRAYS + ('order', 'space', 'vocab_offsets', 'vocab_labels'):
                if name not in data.files:
                    raise ValueError('{}: the word model lacks the array {}.'.format(path, name))
            offsets, flat = data['vocab_offsets'], data['vocab_labels']
            vocab = [flat[offsets[i]:offsets[i + 1]].tolist() for i in range(len(offsets) - 1)]
            scorer = WordLmScorer(*[data[name] for name in WORD_ARRAYS], order=int(data['order']),
                                  space=int(data['space']), vocab=vocab)
            if scorer.num_classes != stored:
                raise ValueError('{}: num_classes {} does not match trie_next.'
                                 .format(path, stored))
            return scorer
        if kind != 'char_ngram':
            raise ValueError('{}: unknown kind of model "{}".'.format(path, kind))
        scorer = LmScorer(data['next'], data['score'],
                          data['final'] if 'final' in data.files else None,
                          int(data['order']) or None)
    if scorer.num_classes != stored:
        raise ValueError('{}: num_classes {} does not match its tables.'.format(path, stored))
    return scorer


WORD_KIND = 'word_ngram'
WORD_ARRAYS = ('trie_next', 'trie_word', 'ctx_begin', 'succ_word', 'succ_lp', 'succ_ctx',
               'ctx_backoff', 'ctx_parent')
WORD_MAX_ORDER = 5
UNK, EOS = 0, 1          # word ids; real words follow from 2


class WordLmScorer:
    """A word n-gram in back-off form over a lexicon trie - the implicit scorer of
    `hip.ctc_beam_decode_wordlm` (include/ctcasr.h, K24, pins what it scores).

    ==============  ==========  =======  =========================================================
    ``trie_next``   [N, C]      int32    -1: no edge; node 0 the root, node 1 the OOV sink
    ``trie_word``   [N]         int32    word id that ends at this node, or -1
    ``ctx_begin``   [H + 1]     int64    start of each context's successor range
    ``succ_word``   [M]         int32    strictly ascending inside a range; context 0 lists all
    ``succ_lp``     [M]         float64  log-probability of the successor
    ``succ_ctx``    [M]         int32    context after (h, w)
    ``ctx_backoff`` [H]         float64  ln bo(h)
    ``ctx_parent``  [H]         int32    h less its oldest word; < h for h > 0
    ==============  ==========  =======  =========================================================

    Word id 0 is ``<unk>``, 1 is ``</s>``.  ``bonus`` and ``oov_score`` (-inf: closed vocabulary)
    are what `scaled` sets.  Everything is validated before anything is uploaded: a violation is a
    ``ValueError`` that names the array.

    ``lookahead`` is None, or the float64 [N] look-ahead table of the scaled arrays
    (`lookahead_table`; ``scaled(..., lookahead=True)`` sets it): the scorer then scores by K26 -
    entering a trie node charges the best score a word below it can still get, the space settles
    the difference - in `step`, `end_score`, `sequence_scores` and on the device.  Complete
    hypotheses are worth what they are worth without it; only pruning changes."""

    kind = 'word'       # what `hip.ctc_beam_search` launches for this scorer

    def __init__(self, trie_next, trie_word, ctx_begin, succ_word, succ_lp, succ_ctx, ctx_backoff,
                 ctx_parent, order, space, vocab=None, bonus=0.0, oov_score=-np.inf):
        def fail(name, what):
            raise ValueError('WordLmScorer: {} {}.'.format(name, what))

        def ints(name, values, ndim):
            values = np.asarray(values)
            if values.ndim != ndim:
                fail(name, 'must have {} dimension(s) (got shape {})'.format(ndim, values.shape))
            if not np.issubdtype(values.dtype, np.integer):
                fail(name, 'must hold integers (got {})'.format(values.dtype))
            return values

        def floats(name, values, length):
            values = np.asarray(values)
            if values.shape != (length,):
                fail(name, 'has shape {}, expected ({},)'.format(values.shape, length))
            values = values.astype(np.float64)
            with np.errstate(over='ignore'):
                rounded = values.astype(np.float32)
            if np.isnan(values).any():
                fail(name, 'holds NaN')
            if np.isposinf(rounded).any():
                fail(name, 'holds +inf')
            return np.ascontiguousarray(values)

        def within(name, values, low, high):
            if values.size and (values.min() < low or values.max() >= high):
                fail(name, 'holds values outside [{}, {})'.format(low, high))

        order, space = int(order), int(space)
        if not 1 <= order <= WORD_MAX_ORDER:
            raise ValueError('WordLmScorer: order must be 1..{} (got {}).'
                             .format(WORD_MAX_ORDER, order))
        trie_next = ints('trie_next', trie_next, 2)
        nodes, classes = trie_next.shape
        if nodes < 2 or classes < 2:
            fail('trie_next', 'must be [N >= 2, C >= 2] (got shape {})'.format(trie_next.shape))
        if not 0 <= space < classes:
            raise ValueError('WordLmScorer: space {} outside [0, {}).'.format(space, classes))
        trie_word = ints('trie_word', trie_word, 1)
        if trie_word.shape != (nodes,):
            fail('trie_word', 'has shape {}, expected ({},)'.format(trie_word.shape, nodes))
        ctx_begin = ints('ctx_begin', ctx_begin, 1)
        if ctx_begin.shape[0] < 2:
            fail('ctx_begin', 'must hold H + 1 >= 2 entries')
        contexts = ctx_begin.shape[0] - 1
        succ_word = ints('succ_word', succ_word, 1)
        total = succ_word.shape[0]
        succ_ctx = ints('succ_ctx', succ_ctx, 1)
        if succ_ctx.shape != (total,):
            fail('succ_ctx', 'has shape {}, expected ({},)'.format(succ_ctx.shape, total))
        ctx_parent = ints('ctx_parent', ctx_parent, 1)
        if ctx_parent.shape != (contexts,):
            fail('ctx_parent', 'has shape {}, expected ({},)'.format(ctx_parent.shape, contexts))
        succ_lp = floats('succ_lp', succ_lp, total)
        ctx_backoff = floats('ctx_backoff', ctx_backoff, contexts)
        if ctx_begin[0] != 0 or ctx_begin[-1] != total or (np.diff(ctx_begin) < 0).any():
            fail('ctx_begin', 'must rise from 0 to M = {}'.format(total))
        words = int(ctx_begin[1])
        if words < 2 or not np.array_equal(succ_word[:words], np.arange(words)):
            fail('succ_word', 'must list every word id (<unk>, </s>, ...) in context 0')
        within('succ_word', succ_word, 0, words)
        rising = np.diff(succ_word) > 0
        rising[ctx_begin[1:-1][(ctx_begin[1:-1] > 0) & (ctx_begin[1:-1] < total)] - 1] = True
        if not rising.all():
            fail('succ_word', 'must be strictly ascending inside every context')
        within('succ_ctx', succ_ctx, 0, contexts)
        within('ctx_parent', ctx_parent, 0, contexts)
        if ctx_parent[0] != 0 or (ctx_parent[1:] >= np.arange(1, contexts)).any():
            fail('ctx_parent', 'must be below its context (ctx_parent[h] < h for h > 0)')
        within('trie_next', trie_next, -1, nodes)
        closing = trie_word[trie_word != -1]
        within('trie_word', closing, 2, words)
        if trie_word[0] != -1 or trie_word[1] != -1:
            fail('trie_word', 'must be -1 at the root and at the OOV sink')
        bonus, oov_score = float(bonus), float(oov_score)
        if not np.isfinite(bonus):
            raise ValueError('WordLmScorer: bonus must be finite.')
        if np.isnan(oov_score) or np.isposinf(oov_score):
            raise ValueError('WordLmScorer: oov_score must be finite or -inf.')
        self.trie_next = np.ascontiguousarray(trie_next, dtype=np.int32)
        self.trie_word = np.ascontiguousarray(trie_word, dtype=np.int32)
        self.ctx_begin = np.ascontiguousarray(ctx_begin, dtype=np.int64)
        self.succ_word = np.ascontiguousarray(succ_word, dtype=np.int32)
        self.succ_lp = succ_lp
        self.succ_ctx = np.ascontiguousarray(succ_ctx, dtype=np.int32)
        self.ctx_backoff = ctx_backoff
        self.ctx_parent = np.ascontiguousarray(ctx_parent, dtype=np.int32)
        self.order, self.space = order, space
        self.bonus, self.oov_score = bonus, oov_score
        self.vocab = None if vocab is None else [[int(v) for v in row] for row in vocab]
        if self.vocab is not None and len(self.vocab) != words - 2:
            raise ValueError('WordLmScorer: vocab holds {} words, the tables {}.'
                             .format(len(self.vocab), words - 2))
        self.lookahead = None
        self._device = {}
        self._device_lookahead = {}

    num_nodes = property(lambda self: self.trie_next.shape[0])
    num_classes = property(lambda self: self.trie_next.shape[1])
    num_contexts = property(lambda self: self.ctx_parent.shape[0])
    num_successors = property(lambda self: self.succ_word.shape[0])
    num_words = property(lambda self: int(self.ctx_begin[1]))     # <unk> and </s> included
    oov = property(lambda self: np.isfinite(self.oov_score))

    def scaled(self, weight=1.0, bonus=0.0, oov_score=-np.inf, lookahead=False):
        """The scorer the kernel takes: ``succ_lp`` and ``ctx_backoff`` times ``weight`` in
        float64 (-inf stays -inf at every weight, 0 included); ``bonus`` and ``oov_score`` are
        kept as float64 - the device adds them in float64 and rounds each score once.
        ``lookahead``: the scorer carries the `lookahead_table` of its scaled arrays (K26)."""
        weight = float(weight)
        if not np.isfinite(weight):
            raise ValueError('WordLmScorer.scaled: weight must be finite.')

        def scale(values):
            safe = np.where(np.isneginf(values), 0.0, values)
            return np.where(np.isneginf(values), -np.inf, weight * safe)

        scorer = WordLmScorer(self.trie_next, self.trie_word, self.ctx_begin, self.succ_word,
                              scale(self.succ_lp), self.succ_ctx, scale(self.ctx_backoff),
                              self.ctx_parent, self.order, self.space, self.vocab, bonus,
                              oov_score)
        if lookahead:
            scorer.lookahead = scorer.lookahead_table()
        return scorer

    def _trie_levels(self):
        """The nodes of the trie level by level from the root, as (parents, children) arrays per
        level - after checking that ``trie_next`` is a tree rooted at node 0: every node >= 2 the
        target of exactly one edge, nodes 0 and 1 of none, every node but the sink reached from
        the root.  Anything else is a ``ValueError`` that names ``trie_next``."""
        nodes = self.num_nodes
        targets = self.trie_next[self.trie_next >= 0]
        reached = np.bincount(targets, minlength=nodes)
        if reached[0] or reached[1]:
            raise ValueError('WordLmScorer: trie_next is no tree: an edge leads into node {}.'
                             .format(0 if reached[0] else 1))
        if (reached[2:] != 1).any():
            node = 2 + int(np.flatnonzero(reached[2:] != 1)[0])
            raise ValueError('WordLmScorer: trie_next is no tree: node {} is the target of {} '
                             'edges.'.format(node, int(reached[node])))
        levels, frontier, seen = [], np.zeros(1, dtype=np.int64), 1
        while frontier.size:
            rows = self.trie_next[frontier]
            at = rows >= 0
            parents = np.broadcast_to(frontier[:, None], rows.shape)[at]
            children = rows[at].astype(np.int64)
            if children.size:
                levels.append((parents, children))
            seen += children.size
            frontier = children
        if seen != nodes - 1:
            raise ValueError('WordLmScorer: trie_next is no tree: {} nodes are not reached from '
                             'the root.'.format(nodes - 1 - seen))
        return levels

    def lookahead_table(self):
        """float64 [N], K26's table of these (scaled) arrays: for a node n >= 2 the best unigram
        score ``succ_lp[w]`` (context 0 lists every word) of a word at or below n, -inf entries
        not counting; with OOV on never below ``oov_score + succ_lp[0]``, which is the sink's
        entry; 0.0 where nothing is finite, and 0.0 at the root.  ``trie_next`` must be a tree
        (``ValueError``).  Level by level, no recursion."""
        levels = self._trie_levels()
        unigram = self.succ_lp[:self.num_words]
        table = np.full(self.num_nodes, -np.inf)
        closing = self.trie_word >= 0
        table[closing] = unigram[self.trie_word[closing]]
        table[:2] = -np.inf
        for parents, children in reversed(levels):
            np.maximum.at(table, parents, table[children])
        unk = self.oov_score + float(unigram[UNK])
        if self.oov and np.isfinite(unk):
            table[2:] = np.maximum(table[2:], unk)
            table[1] = unk
        else:
            table[1] = -np.inf
        table[~np.isfinite(table)] = 0.0
        table[0] = 0.0
        return table

    def word_score(self, context, word):
        """(Wd(h, w) in float64, next context): the pinned back-off walk - search h's range for
        w; found: add ``succ_lp`` and stop; else add ``ctx_backoff[h]``, go to ``ctx_parent[h]``.
        At most ``order`` searches: tables that would run longer give (-inf, 0)."""
        h, acc = int(context), 0.0
        for _ in range(self.order):
            low, high = int(self.ctx_begin[h]), int(self.ctx_begin[h + 1])
            at = low + int(np.searchsorted(self.succ_word[low:high], word))
            if at < high and self.succ_word[at] == word:
                return acc + float(self.succ_lp[at]), int(self.succ_ctx[at])
            acc += float(self.ctx_backoff[h])
            h = int(self.ctx_parent[h])
        return -np.inf, 0

    def _close(self, node, context):
        """(score of the word that ``node`` closes in ``context``, no bonus; next context).  With
        a look-ahead table the word's full cost: the sink's word carries ``oov_score`` too."""
        if node == 0:
            return -np.inf, 0
        word = -1 if node == 1 else int(self.trie_word[node])
        if word >= 0:
            return self.word_score(context, word)
        if not self.oov:
            return -np.inf, 0
        score, after = self.word_score(context, UNK)
        if node == 1 and self.lookahead is None:
            return score, after
        return score + self.oov_score, after

    def step(self, node, context, label):
        """((next node, next context), float32 score) of the edge ``label`` out of the state
        (node, context); a forbidden edge gives (None, -inf)."""
        forbidden = (None, np.float32(-np.inf))
        la = self.lookahead
        if label != self.space:
            if node == 1:
                return (1, context), np.float32(self.bonus)
            target = int(self.trie_next[node, label])
            if target >= 0:
                if la is not None:
                    return (target, context), np.float32((la[target] - la[node]) + self.bonus)
                return (target, context), np.float32(self.bonus)
            if self.oov:
                if la is not None:
                    return (1, context), np.float32((la[1] - la[node]) + self.bonus)
                return (1, context), np.float32(self.oov_score + self.bonus)
            return forbidden
        score, after = self._close(node, context)
        if np.isneginf(score):       # nothing closes here (or the tables forbid the word)
            return forbidden
        if la is not None:
            return (0, after), np.float32((score - la[node]) + self.bonus)
        return (0, after), np.float32(score + self.bonus)

    def end_score(self, node, context):
        """float32 end score of a hypothesis in (node, context); no bonus at the end."""
        if node == 0:
            return np.float32(self.word_score(context, EOS)[0])
        score, after = self._close(node, context)
        if np.isneginf(score):
            return np.float32(-np.inf)
        if self.lookahead is not None:
            return np.float32((score - self.lookahead[node]) + self.word_score(after, EOS)[0])
        return np.float32(score + self.word_score(after, EOS)[0])

    def sequence_scores(self, rows):
        """float64 [len(rows)]: for each label row the sum of the float32 edge scores from the
        start state (0, 0) plus the end score of the state it ends in - what the fused search
        adds to a hypothesis.  ``-inf`` (a forbidden edge or end) passes through.  Raises
        ``ValueError`` for a label outside [0, C)."""
        totals = np.zeros(len(rows), dtype=np.float64)
        for i, row in enumerate(rows):
            state, total = (0, 0), 0.0
            for c in row:
                c = int(c)
                if not 0 <= c < self.num_classes:
                    raise ValueError('WordLmScorer.sequence_scores: label {} outside [0, {}).'
                                     .format(c, self.num_classes))
                if state is not None:
                    state, score = self.step(state[0], state[1], c)
                    total += float(score)
            if state is None:
                total = -np.inf
            else:
                total += float(self.end_score(*state))
            totals[i] = total
        return totals

    def to(self, device):
        """The eight arrays on ``device``, in the order of `WORD_ARRAYS`; uploaded once per device
        and cached."""
        import torch
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if device not in self._device:
            self._device[device] = tuple(torch.from_numpy(getattr(self, name)).to(device)
                                         for name in WORD_ARRAYS)
        return self._device[device]

    def lookahead_to(self, device):
        """The look-ahead table on ``device`` (float64 [N]); uploaded once per device and
        cached, like the arrays of `to`."""
        import torch
        if self.lookahead is None:
            raise ValueError('WordLmScorer.lookahead_to: the scorer carries no look-ahead table.')
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        cached = self._device_lookahead.get(device)
        if cached is None or cached[0] is not self.lookahead:
            table = np.ascontiguousarray(self.lookahead, dtype=np.float64)
            cached = (self.lookahead, torch.from_numpy(table).to(device))
            self._device_lookahead[device] = cached
        return cached[1]

    def save(self, path):
        """``.npz`` of the arrays plus ``kind``, ``order``, ``num_classes``, ``space`` and the
        vocabulary as flat label rows with offsets; no pickle.  Scaling is not stored: save the
        model `build_word_ngram` returned.  Nor is a look-ahead table: it is derived."""
        vocab = self.vocab or []
        arrays = {name: getattr(self, name) for name in WORD_ARRAYS}
        arrays.update(kind=np.array(WORD_KIND), order=np.int64(self.order),
                      num_classes=np.int64(self.num_classes), space=np.int64(self.space),
                      vocab_labels=np.array([v for row in vocab for v in row], dtype=np.int32),
                      vocab_offsets=np.cumsum([0] + [len(row) for row in vocab]).astype(np.int64))
        with open(path, 'wb') as handle:
            np.savez(handle, **arrays)


def split_words(row, space):
    """The words of a label row: runs of labels between spaces (empty runs dropped)."""
    words, word = [], []
    for c in row:
        if c == space:
            if word:
                words.append(tuple(word))
            word = []
        else:
            word.append(c)
    if word:
        words.append(tuple(word))
    return words


def build_word_ngram(word_rows, order, num_classes, space, vocab_size=0, blank=None):
    """Interpolated Witten-Bell n-gram of ``order`` (1..5) over the *words* of label rows (runs of
    labels between ``space``), in float64 and in back-off form - the estimate of
    `build_char_ngram` with words for labels.  Events are the vocabulary, ``</s>`` and ``<unk>``;
    below the empty context the distribution is uniform over all events, so every event has mass
    in every context.  ``vocab_size`` > 0 keeps the most frequent words (ties: the smaller label
    row); every other word counts as ``<unk>``.  Word ids: 0 ``<unk>``, 1 ``</s>``, real words from
    2 in ascending order of their label rows.

    With c(h, w) the counts, c(h) their sum and n(h) the number of distinct w after h,
    P(w | h) = (c(h, w) + n(h) P(w | h')) / (c(h) + n(h)): a seen pair stores ln P(w | h), an
    unseen one costs ln bo(h) + (the same question asked of h'), bo(h) = n(h) / (c(h) + n(h)) -
    exact for Witten-Bell.  Contexts are the observed histories, suffix-closed, shorter first."""
    order, classes, space, vocab_size = int(order), int(num_classes), int(space), int(vocab_size)
    if not 1 <= order <= WORD_MAX_ORDER:
        raise ValueError('build_word_ngram: order must be 1..{}.'.format(WORD_MAX_ORDER))
    if classes < 2:
        raise ValueError('build_word_ngram: num_classes must be >= 2.')
    blank = classes - 1 if blank is None else int(blank)
    if not 0 <= blank < classes:
        raise ValueError('build_word_ngram: blank outside [0, {}).'.format(classes))
    if not 0 <= space < classes or space == blank:
        raise ValueError('build_word_ngram: space outside [0, {}) or the blank.'.format(classes))
    if vocab_size < 0:
        raise ValueError('build_word_ngram: vocab_size must be >= 0.')
    sentences, frequency = [], {}
    for row in word_rows:
        row = [int(v) for v in row]
        if any(v < 0 or v >= classes or v == blank for v in row):
            raise ValueError('build_word_ngram: label outside [0, {}) or the blank.'
                             .format(classes))
        sentences.append(split_words(row, space))
        for word in sentences[-1]:
            frequency[word] = frequency.get(word, 0) + 1
    kept = sorted(frequency, key=lambda word: (-frequency[word], word))
    vocab = sorted(kept[:vocab_size] if vocab_size > 0 else kept)
    word_id = {word: 2 + i for i, word in enumerate(vocab)}
    events = len(vocab) + 2

    counts = {(): {}}
    for sentence in sentences:
        ids = [word_id.get(word, UNK) for word in sentence]
        for i, event in enumerate(ids + [EOS]):
            for m in range(min(order - 1, i) + 1):
                seen = counts.setdefault(tuple(ids[i - m:i]), {})
                seen[event] = seen.get(event, 0) + 1
    contexts = sorted(counts, key=lambda h: (len(h), h))        # shorter first: () is context 0
    index = {h: i for i, h in enumerate(contexts)}
    prob, backoff = {}, np.zeros(len(contexts))
    for i, h in enumerate(contexts):
        seen, total = float(len(counts[h])), float(sum(counts[h].values()))
        lower = prob[h[1:]] if h else None
        if h:
            prob[h] = {w: (c + seen * lower[w]) / (total + seen) for w, c in counts[h].items()}
        else:
            # context 0 lists every event: the unseen ones at their back-off value
            uniform = 1.0 / events
            prob[h] = {w: (counts[h].get(w, 0) + seen * uniform) / (total + seen)
                       if total > 0 else uniform for w in range(events)}
        with np.errstate(divide='ignore'):
            backoff[i] = np.log(seen / (total + seen)) if total > 0 else 0.0

    def after(h, w):
        target = (h + (w,))[-(order - 1):] if order > 1 else ()
        while target not in index:
            target = target[1:]
        return index[target]

    begin, succ_word, succ_lp, succ_ctx = [0], [], [], []
    for h in contexts:
        for w in sorted(prob[h]):
            succ_word.append(w)
            succ_lp.append(np.log(prob[h][w]))
            succ_ctx.append(after(h, w))
        begin.append(len(succ_word))
    parent = [index[h[1:]] if h else 0 for h in contexts]

    edges, ends = [{}, {}], [-1, -1]
    for word in vocab:
        node = 0
        for c in word:
            if c not in edges[node]:
                edges[node][c] = len(edges)
                edges.append({})
                ends.append(-1)
            node = edges[node][c]
        ends[node] = word_id[word]
    trie_next = np.full((len(edges), classes), -1, dtype=np.int32)
    for node, row in enumerate(edges):
        for c, target in row.items():
            trie_next[node, c] = target
    return WordLmScorer(trie_next, np.array(ends, dtype=np.int32),
                        np.array(begin, dtype=np.int64), np.array(succ_word, dtype=np.int32),
                        np.array(succ_lp, dtype=np.float64), np.array(succ_ctx, dtype=np.int32),
                        backoff, np.array(parent, dtype=np.int32), order, space,
                        [list(word) for word in vocab])



def from_flags(num_classes):
    """The scaled scorer of ``--lm_path`` / ``--lm_weight`` / ``--lm_bonus`` for a model of
    ``num_classes``; None when ``--lm_path`` is unset."""
    from ctc_asr_amd.params import FLAGS
    if not FLAGS.lm_path:
        return None
    scorer = load(FLAGS.lm_path, num_classes)
    if isinstance(scorer, WordLmScorer):
        check_word_space('--lm_path', scorer)
        return scorer.scaled(FLAGS.lm_weight, FLAGS.lm_bonus, FLAGS.lm_oov_score,
                             lookahead=FLAGS.lm_lookahead)
    return scorer.scaled(FLAGS.lm_weight, FLAGS.lm_bonus)


def rescorer_from_flags(num_classes):
    """The scaled scorer of ``--rescore_lm_path`` / ``--rescore_lm_weight`` /
    ``--rescore_lm_bonus``, which re-ranks the n-best list on the host; None when unset."""
    from ctc_asr_amd.params import FLAGS
    if not FLAGS.rescore_lm_path:
        return None
    scorer = load(FLAGS.rescore_lm_path, num_classes)
    if isinstance(scorer, WordLmScorer):
        check_word_space('--rescore_lm_path', scorer)
        return scorer.scaled(FLAGS.rescore_lm_weight, FLAGS.rescore_lm_bonus,
                             FLAGS.rescore_lm_oov_score)
    return scorer.scaled(FLAGS.rescore_lm_weight, FLAGS.rescore_lm_bonus)


def check_word_space(flag, scorer):
    """A word model ends its words at the label it was built with: refuse one whose ``space`` is
    not the space of the model's alphabet."""
    _check_space(flag, scorer.space)


def _check_space(flag, space):
    from ctc_asr_amd.labels import ctoi
    if space != ctoi(' '):
        raise ValueError('{}: the word model\'s space is label {}, the model\'s {}.'
                         .format(flag, space, ctoi(' ')))


def check_file(flag, path, num_classes):
    """The parse-time check of ``--lm_path`` / ``--rescore_lm_path``: the file exists, is a model
    of either kind for ``num_classes`` classes and, if a word model, ends its words at the
    alphabet's space.  Reads the file's scalars only: the tables are validated when the model is
    loaded for use.  Every refusal is a ``ValueError`` that names the flag.  Returns the file's
    ``kind``."""
    import zipfile
    try:
        with np.load(path, allow_pickle=False) as data:
            named = set(data.files)
            stored = int(data['num_classes']) if 'num_classes' in named else None
            kind = str(data['kind']) if 'kind' in named else 'char_ngram'
            space = int(data['space']) if kind == WORD_KIND and 'space' in named else None
    except (OSError, ValueError, zipfile.BadZipFile) as error:
        raise ValueError('{}: {}: {}'.format(flag, path, error))
    if stored is None:
        raise ValueError('{}: {} is no model of ctc_asr_amd.lm.'.format(flag, path))
    if stored != int(num_classes):
        raise ValueError('{}: {}: built for {} classes, the model has {}.'
                         .format(flag, path, stored, int(num_classes)))
    if kind == WORD_KIND:
        if space is None:
            raise ValueError('{}: {}: the word model lacks the array space.'.format(flag, path))
        _check_space(flag, space)
    return kind


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


def text_label_rows(text_path):
    """Label-id rows of a plain text file, one per non-empty line, each through
    `align_long.normalize_transcript`; a digit is refused with its line number."""
    from ctc_asr_amd.align_long import normalize_transcript
    from ctc_asr_amd.labels import ctoi
    rows = []
    with open(text_path, encoding='utf-8') as handle:
        for number, line in enumerate(handle, 1):
            if not line.strip():
                continue
            try:
                rows.append([ctoi(ch) for ch in normalize_transcript(line)])
            except ValueError as error:
                raise ValueError('{}, line {}: {}'.format(text_path, number, error))
    return rows


def main(argv=None):
    from ctc_asr_amd.params import FLAGS
    FLAGS.parse(sys.argv[1:] if argv is None else argv)
    if FLAGS.lm_unit == 'word':
        return _main_word(FLAGS)
    if not FLAGS.lm_corpus_csv or not FLAGS.lm_path:
        raise ValueError('ctc_asr_amd.lm needs --lm_corpus_csv and --lm_path.')
    rows = corpus_label_rows(FLAGS.lm_corpus_csv)
    scorer = build_char_ngram(rows, FLAGS.lm_order, FLAGS.num_classes)
    scorer.save(FLAGS.lm_path)
    print('Order-{} character model of {} transcripts, {} states -> {}'.format(
        FLAGS.lm_order, len(rows), scorer.num_states, FLAGS.lm_path))
    return 0


def _main_word(flags):
    from ctc_asr_amd.labels import ctoi
    if not (flags.lm_corpus_csv or flags.lm_corpus_text) or not flags.lm_path:
        raise ValueError('ctc_asr_amd.lm --lm_unit word needs --lm_corpus_csv or '
                         '--lm_corpus_text, and --lm_path.')
    rows = corpus_label_rows(flags.lm_corpus_csv) if flags.lm_corpus_csv else []
    if flags.lm_corpus_text:
        rows = rows + text_label_rows(flags.lm_corpus_text)
    scorer = build_word_ngram(rows, flags.lm_order, flags.num_classes, ctoi(' '),
                              vocab_size=flags.lm_vocab_size)
    scorer.save(flags.lm_path)
    print('Order-{} word model of {} transcripts, {} words, {} trie nodes, {} contexts, {} '
          'successors -> {}'.format(flags.lm_order, len(rows), scorer.num_words - 2,
                                    scorer.num_nodes, scorer.num_contexts, scorer.num_successors,
                                    flags.lm_path))
    return 0


if __name__ == '__main__':
    sys.exit(main())
