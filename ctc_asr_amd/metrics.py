"""Scoring helpers: text rendering, Levenshtein distance, WER and label edit distance.

Behavioural mirror of ``asr/util/metrics.py:9-141`` (``dense_to_text``, ``wer``, ``wer_batch``,
``levenshtein``) and of the ``tf.edit_distance(decoded, labels)`` call in
``asr/model.py:338`` (normalised Levenshtein over integer labels).  Host-side Python like the
reference's ``tf.py_func`` bodies; nothing here is on the GPU hot path.

`error_counts` scores a whole batch in one launch of the edit-distance kernel
(``ctcasr_edit_distance``) and the ``*_from_counts`` helpers turn its integer distances into the
rates above, with the same host expressions.
"""

import itertools

import numpy as np
import torch

from ctc_asr_amd import hip
from ctc_asr_amd.labels import itoc
from ctc_asr_amd.params import NP_FLOAT


def levenshtein(a, b):
    """Edit distance between two sequences (strings or lists of words / ints).

    Single-row dynamic programme; unit costs for insert / delete / substitute, as in
    ``asr/util/metrics.py:110-141``.
    """
    if len(a) < len(b):
        a, b = b, a
    # `b` is now the shorter sequence; one row of len(b)+1 cells.
    row = list(range(len(b) + 1))
    for i, item_a in enumerate(a, start=1):
        diagonal, row[0] = row[0], i
        for j, item_b in enumerate(b, start=1):
            substitute = diagonal + (item_a != item_b)
            diagonal = row[j]
            row[j] = min(substitute, row[j] + 1, row[j - 1] + 1)
    return row[len(b)]


def wer(original, result):
    """Word error rate = word-level Levenshtein / number of words in ``original``
    (``asr/util/metrics.py:52-76``).  Raises ``ZeroDivisionError`` for an empty original, like the
    reference."""
    if isinstance(original, bytes):
        original = original.decode('utf-8')
    if isinstance(result, bytes):
        result = result.decode('utf-8')
    original_words = original.split()
    result_words = result.split()
    return np.array(levenshtein(original_words, result_words) / float(len(original_words)),
                    dtype=NP_FLOAT)


def wer_batch(originals, results):
    """Per-sample WER ``f32[B]`` and their mean ``f32[]`` (``asr/util/metrics.py:81-105``)."""
    if len(originals) != len(results):
        raise AssertionError('wer_batch(): originals and results differ in length.')
    rates = np.array([wer(o, r) for o, r in zip(originals, results)], dtype=NP_FLOAT)
    mean = np.array(float(np.sum(rates.astype(np.float64))) / float(len(originals)),
                    dtype=NP_FLOAT)
    return rates, mean


def dense_to_text(decoded, originals):
    """Render dense integer rows as strings (0 -> '') and stack them with the originals.

    Returns ``(decoded_strings object[B], summary object[2, B])`` like
    ``asr/util/metrics.py:9-47``; ``originals`` may be empty, giving ``'n/a'`` placeholders.
    (The reference uses the removed ``np.object`` alias; plain ``object`` is the same dtype.)
    """
    decoded_strings = [''.join(itoc(int(i)) for i in row) for row in decoded]
    if len(originals) > 0:
        original_strings = [o.decode('utf-8') if isinstance(o, bytes) else str(o)
                            for o in originals]
    else:
        original_strings = ['n/a'] * len(decoded_strings)
    decoded_arr = np.array(decoded_strings, dtype=object)
    summary = np.vstack([decoded_arr, np.array(original_strings, dtype=object)])
    return decoded_arr, summary


def edit_distance(hypothesis, truth, normalize=True):
    """``tf.edit_distance`` for one pair of integer sequences: Levenshtein(hyp, truth), divided
    by ``len(truth)`` when ``normalize``.  An empty truth gives ``inf`` for a non-empty
    hypothesis and 0 for an empty one (TensorFlow's convention)."""
    hypothesis, truth = list(hypothesis), list(truth)
    dist = float(levenshtein(hypothesis, truth))
    if not normalize:
        return dist
    if len(truth) == 0:
        return float('inf') if dist != 0.0 else 0.0
    return dist / float(len(truth))


def edit_distance_batch(hypotheses, truths, normalize=True):
    """Batch form: ``f32[B]`` of per-utterance distances and their mean (``asr/model.py:338-339``)."""
    if len(hypotheses) != len(truths):
        raise ValueError('edit_distance_batch(): batch sizes differ.')
    dists = np.array([edit_distance(h, t, normalize) for h, t in zip(hypotheses, truths)],
                     dtype=NP_FLOAT)
    return dists, np.array(np.mean(dists.astype(np.float64)) if len(dists) else 0.0,
                           dtype=NP_FLOAT)


def word_ids(originals, results):
    """Both sides of a batch of transcripts as lists of integer word ids, split exactly as `wer`
    splits them (bytes decoded as UTF-8, then ``str.split()``).  One dictionary serves the whole
    call, so equal words get equal ids on both sides.  Returns (original ids, result ids)."""
    table = {}

    def ids(text):
        if isinstance(text, bytes):
            text = text.decode('utf-8')
        return [table.setdefault(word, len(table)) for word in text.split()]

    return [ids(o) for o in originals], [ids(r) for r in results]


def _packed(sequences):
    lengths = np.fromiter((len(s) for s in sequences), dtype=np.int64, count=len(sequences))
    flat = np.fromiter(itertools.chain.from_iterable(sequences), dtype=np.int32,
                       count=int(lengths.sum()))
    return flat, np.cumsum(lengths) - lengths, lengths


def error_counts(hyps, refs, device):
    """Edit distance and error breakdown of ``B`` pairs of integer sequences in ONE kernel launch
    (`hip.edit_distance`): int32 numpy ``[B, 4]`` of (distance, substitutions, deletions,
    insertions).  One upload, one download.  Raises on a non-zero status."""
    if len(hyps) != len(refs):
        raise ValueError('error_counts(): batch sizes differ.')
    batch = len(hyps)
    if batch == 0:
        return np.zeros((0, 4), dtype=np.int32)
    hyp, hyp_off, hyp_len = _packed(hyps)
    ref, ref_off, ref_len = _packed(refs)
    # one host buffer, one copy: symbols (at least one int each, never a null pointer), then the
    # four vectors of B
    sizes = [max(hyp.size, 1), max(ref.size, 1), batch, batch, batch, batch]
    starts = np.cumsum([0] + sizes)
    host = np.zeros(int(starts[-1]), dtype=np.int32)
    for start, part in zip(starts, (hyp, ref, hyp_off, hyp_len, ref_off, ref_len)):
        host[start:start + part.size] = part
    packed = torch.from_numpy(host).to(device)
    views = [packed[start:stop] for start, stop in zip(starts[:-1], starts[1:])]
    out = torch.empty((5, batch), dtype=torch.int32, device=device)
    hip.edit_distance(views[0], views[2], views[3], views[1], views[4], views[5],
                      max_hyp_len=int(hyp_len.max()), max_ref_len=int(ref_len.max()), out=out)
    out = out.cpu().numpy()
    if out[4].any():
        raise hip.CtcAsrError('error_counts(): status {} for pair {}.'.format(
            int(out[4][np.flatnonzero(out[4])[0]]), int(np.flatnonzero(out[4])[0])))
    return np.ascontiguousarray(out[:4].T)


def edit_distance_batch_from_counts(distances, truth_lengths, normalize=True):
    """`edit_distance_batch` from integer Levenshtein distances and the lengths of the truths:
    the same host expressions, so the same bits."""
    if len(distances) != len(truth_lengths):
        raise ValueError('edit_distance_batch_from_counts(): batch sizes differ.')

    def one(distance, truth_length):
        dist = float(int(distance))
        if not normalize:
            return dist
        if int(truth_length) == 0:
            return float('inf') if dist != 0.0 else 0.0
        return dist / float(int(truth_length))

    dists = np.array([one(d, n) for d, n in zip(distances, truth_lengths)], dtype=NP_FLOAT)
    return dists, np.array(np.mean(dists.astype(np.float64)) if len(dists) else 0.0,
                           dtype=NP_FLOAT)


def wer_batch_from_counts(distances, original_lengths):
    """`wer_batch` from integer word-level distances and the word counts of the originals: the
    same host expressions, ``ZeroDivisionError`` for an empty original included."""
    if len(distances) != len(original_lengths):
        raise AssertionError('wer_batch_from_counts(): distances and lengths differ in length.')
    rates = np.array([np.array(int(d) / float(int(n)), dtype=NP_FLOAT)
                      for d, n in zip(distances, original_lengths)], dtype=NP_FLOAT)
    mean = np.array(float(np.sum(rates.astype(np.float64))) / float(len(original_lengths)),
                    dtype=NP_FLOAT)
    return rates, mean


def oracle_errors(distances, group_sizes):
    """The fewest errors among each utterance's hypotheses: ``distances`` holds one edit
    distance per hypothesis, utterance after utterance, ``group_sizes`` how many each utterance
    has.  Returns int64 ``[len(group_sizes)]``; an utterance without hypotheses raises
    ``ValueError`` (its oracle is undefined)."""
    distances = np.asarray(distances, dtype=np.int64).reshape(-1)
    sizes = np.asarray(group_sizes, dtype=np.int64).reshape(-1)
    if (sizes < 1).any():
        raise ValueError('oracle_errors(): an utterance has no hypothesis.')
    if int(sizes.sum()) != distances.size:
        raise ValueError('oracle_errors(): {} distances for groups of {} in all.'
                         .format(distances.size, int(sizes.sum())))
    starts = np.cumsum(sizes) - sizes
    return np.minimum.reduceat(distances, starts) if sizes.size else np.zeros(0, dtype=np.int64)


def corpus_rate(errors, reference_length):
    """Total errors over total reference length, the corpus-level form of
    ``corpus_*_error_rate``; NaN for an empty reference."""
    return int(errors) / int(reference_length) if int(reference_length) else float('nan')
