"""Evaluation driver: ``python -m ctc_asr_amd.evaluate [--dev] [--flag=value ...]``.

Counterpart of ``asr/evaluate.py:18-43``: one pass over dev.csv (``--dev``) or test.csv with the
model in evaluation mode; reports the CTC loss and the two ``eval_metric_ops`` of
``asr/model.py:111-118`` — mean edit distance and word error rate, each the unweighted mean over
batches of the per-batch mean.  Decoding is the CTC beam search of width ``FLAGS.beam_width``,
with the language model of ``--lm_path`` fused in when that flag is set.  ``--nbest N`` also
reads the N best hypotheses off each final beam and reports the oracle error rates of the beam
and, with ``--rescore_lm_path``, the rates of the re-ranked hypotheses.
"""

import sys

import numpy as np
import torch

from ctc_asr_amd import lm, metrics, storage, summaries
from ctc_asr_amd.input_functions import input_fn_generator
from ctc_asr_amd.model import CTCModel, ModelConfig
from ctc_asr_amd.params import FLAGS


def evaluate_dataset(model, target, rank=0, world=1, max_batches=None, report_samples=True,
                     scorer=None, nbest=0, rescorer=None):
    """{'loss', 'mean_edit_distance', 'word_error_rate', 'batches'} for one pass over
    ``target`` ('dev' or 'test'); with ``world > 1`` every rank scores its shard and the
    per-batch means are averaged over ranks.  ``scorer``: a scaled `lm.LmScorer` to decode
    with.  When the decodes are scored on the GPU (``CTCASR_GPU_METRICS``, the default) the
    result also holds the error breakdown summed over the set - 'label_errors' and
    'word_errors', each {'substitutions', 'deletions', 'insertions', 'reference'} - and the
    corpus-level 'corpus_label_error_rate' and 'corpus_word_error_rate': total errors over
    total reference length.
    ``nbest`` > 0 decodes with `CTCModel.nbest_many` (rank 0 is the top-1 decode, so every value
    above is what it is without it) and adds 'oracle_label_error_rate' /
    'oracle_word_error_rate' - per utterance the fewest errors over its hypotheses, summed, over
    the total reference length -, 'nbest_mean_paths' and, with a ``rescorer`` (a scaled
    `lm.LmScorer` that re-ranks the lists), 'rescored_label_error_rate' /
    'rescored_word_error_rate', the same corpus-level rates of the selected hypotheses."""
    input_fn = input_fn_generator(target, device=model.device, rank=rank, world_size=world,
                                  seed=(FLAGS.random_seed or 1) if world > 1 else None)
    losses, meds, wers = [], [], []
    # Decoding is deferred: the beam search runs one workgroup per utterance, so the logits of
    # several batches are decoded in ONE launch (`CTCModel.decode_many`) - same results, and a
    # group costs about what a single batch does.  The metrics stay per-batch means.
    pending, group, samples = [], None, None
    # (S, D, I, reference length) summed over the set: labels, then words
    totals = np.zeros((2, 4), dtype=np.int64)
    # n-best: oracle errors (labels, words), rescored errors (labels, words), reference lengths
    # (labels, words), hypotheses, utterances
    listed_totals = np.zeros(8, dtype=np.int64)

    def score_lists(lists, labels, texts):
        label_dist, word_dist, sizes = model.nbest_error_counts(lists, labels, texts)
        listed_totals[0] += metrics.oracle_errors(label_dist, sizes).sum()
        listed_totals[1] += metrics.oracle_errors(word_dist, sizes).sum()
        picked = np.cumsum(sizes) - sizes + np.array([r['selected'] for r in lists])
        listed_totals[2] += label_dist[picked].sum()
        listed_totals[3] += word_dist[picked].sum()
        truths = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else labels
        listed_totals[4] += sum(int(np.count_nonzero(np.asarray(row))) for row in truths)
        listed_totals[5] += sum(len(text.split()) for text in texts)
        listed_totals[6] += sizes.sum()
        listed_totals[7] += len(sizes)

    def score_pending():
        nonlocal samples
        batches = [(logits, seq_len, originals) for logits, seq_len, originals, _, _ in pending]
        if nbest:
            lists = model.nbest_many(batches, nbest, scorer=scorer, rescorer=rescorer)
            results = [model.nbest_top(listed, originals)
                       for listed, (_, _, originals) in zip(lists, batches)]
            for listed, (_, _, _, labels, texts) in zip(lists, pending):
                score_lists(listed, labels, texts)
        else:
            results = model.decode_many(batches, scorer=scorer)
        for (decoded, plaintext, summary), (_, _, _, labels, texts) in zip(results, pending):
            if model.gpu_metrics:
                _, mean_ed, _, wer, label_counts, word_counts, reference = \
                    model.error_counts_fn(labels, texts, decoded, plaintext)
                totals[0, :3] += label_counts[:, 1:].sum(axis=0, dtype=np.int64)
                totals[1, :3] += word_counts[:, 1:].sum(axis=0, dtype=np.int64)
                totals[:, 3] += reference.sum(axis=0)
            else:
                _, mean_ed, _, wer = model.error_rates_fn(labels, texts, decoded, plaintext)
            meds.append(float(mean_ed))
            wers.append(float(wer))
            if samples is None:
                samples = summary
        del pending[:]

    for index, batch in enumerate(input_fn()):
        if max_batches is not None and index >= max_batches:
            break
        features, labels = batch
        logits, seq_len = model.inference_fn(features['spectrogram'],
                                             features['spectrogram_length'], training=False)
        loss = model.loss_fn(logits, seq_len, labels)
        model.check_rnn_error()       # a timed-out persistent recurrence would score garbage
        losses.append(float(loss))
        originals = np.array([t.encode('utf-8') for t in features['label_plaintext']],
                             dtype=object)
        pending.append((logits, seq_len, originals, labels, features['label_plaintext']))
        # (the longest utterances bound the prefix-tree pool: size the group on them)
        group = model.decode_group_size(max(int(item[0].shape[0]) for item in pending),
                                        int(logits.shape[1]), scorer=scorer)
        if len(pending) >= group:
            score_pending()
    if pending:
        score_pending()
    if report_samples and rank == 0 and samples is not None:
        for dec, orig in list(zip(samples[0], samples[1]))[:FLAGS.num_samples_to_report]:
            print('  decoded: "{}"\n  original: "{}"'.format(dec, orig))
    # (the integer sums ride in the same float64 all_reduce: exact below 2^53)
    stats = torch.tensor([np.sum(losses), np.sum(meds), np.sum(wers), len(losses)] +
                         totals.reshape(-1).tolist() + listed_totals.tolist(),
                         dtype=torch.float64, device=model.device)
    if world > 1:
        torch.distributed.all_reduce(stats)
    count = max(float(stats[3]), 1.0)
    result = {'loss': float(stats[0]) / count, 'mean_edit_distance': float(stats[1]) / count,
              'word_error_rate': float(stats[2]) / count, 'batches': int(stats[3])}
    if model.gpu_metrics:
        for name, row in (('label', stats[4:8].tolist()), ('word', stats[8:12].tolist())):
            subs, dels, ins, reference = (int(v) for v in row)
            result[name + '_errors'] = {'substitutions': subs, 'deletions': dels,
                                        'insertions': ins, 'reference': reference}
            result['corpus_{}_error_rate'.format(name)] = \
                (subs + dels + ins) / reference if reference else float('nan')
    if nbest:
        listed = [int(v) for v in stats[12:20].tolist()]
        result['oracle_label_error_rate'] = metrics.corpus_rate(listed[0], listed[4])
        result['oracle_word_error_rate'] = metrics.corpus_rate(listed[1], listed[5])
        result['nbest_mean_paths'] = listed[6] / listed[7] if listed[7] else float('nan')
        if rescorer is not None:
            result['rescored_label_error_rate'] = metrics.corpus_rate(listed[2], listed[4])
            result['rescored_word_error_rate'] = metrics.corpus_rate(listed[3], listed[5])
    return result


def main(argv=None):
    FLAGS.parse(sys.argv[1:] if argv is None else argv)
    if not torch.cuda.is_available():
        raise SystemExit('ctc_asr_amd.evaluate needs an MI355X; no GPU is visible.')
    model = CTCModel(ModelConfig.from_flags(FLAGS), 'cuda', seed=FLAGS.random_seed or 1)
    latest = storage.latest_checkpoint(FLAGS.train_dir)
    if latest is None:
        raise SystemExit('No checkpoint found in {}.'.format(FLAGS.train_dir))
    storage.restore_checkpoint(latest, model, weights='ema' if FLAGS.eval_ema else 'param')
    target = 'dev' if FLAGS.dev else 'test'
    print('Evaluating checkpoint {} on the {} set.'.format(latest, target))
    result = evaluate_dataset(model, target, scorer=lm.from_flags(model.cfg.num_classes),
                              nbest=FLAGS.nbest,
                              rescorer=lm.rescorer_from_flags(model.cfg.num_classes))
    writer = summaries.SummaryWriter(FLAGS.train_dir, 'eval_' + target)
    for tag in ('loss', 'mean_edit_distance', 'word_error_rate'):       # eval_metric_ops + loss
        writer.scalar(tag, result[tag], model.step_count)
    print('Evaluation result: {}'.format(result))
    return 0


if __name__ == '__main__':
    sys.exit(main())
