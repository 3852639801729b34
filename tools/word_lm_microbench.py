#!/usr/bin/env python
"""Times ctcasr_ctc_beam_decode_wordlm next to ctcasr_ctc_beam_decode_lm (character 5-gram) and
the plain search, all three on the same logits in one process, and ctcasr_wordlm_lookup alone.

A synthetic language, nothing downloaded: 20 000 seeded pseudo-words, sentences by a Zipf draw,
word n-grams of orders 2 and 3.  The logits spell sentences of that language (peaked, with noise)
at the evaluation group's shape: T' = 500, 176 utterances, widths 64 and 1024.  Also printed: the
word lookups actually performed per utterance against the branches expanded (the kernel's
`stats`).  Then the search with look-ahead scores inside a word (K26) beside the plain word search
at equal widths, 4 to 1024: the time per launch and the mean exact fused total of the returned
hypothesis - `hip.ctc_score` of it plus the model's `sequence_scores` of it, the quantity the search
maximises, comparable across both forms because the look-ahead sums telescope.  The models are
cached as .npz under the directory given (building them is host work):
python tools/word_lm_microbench.py [cache_dir [T B [build-only | lookahead-only]]]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ctc_asr_amd import hip, lm  # noqa: E402
from ctc_asr_amd.labels import ctoi  # noqa: E402

WORDS, SENTENCES, CLASSES = 20000, 40000, 29


def language(rng):
    """(pseudo-words as label rows, sentences as lists of word indices)."""
    letters = [ctoi(ch) for ch in 'abcdefghijklmnopqrstuvwxyz']
    words = set()
    while len(words) < WORDS:
        words.add(tuple(letters[int(i)] for i in rng.integers(0, 26, size=int(rng.integers(2, 10)))))
    words = sorted(words)
    order = rng.permutation(WORDS)                     # rank -> word, so that rank is not length
    sentences = [[int(order[min(int(r), WORDS) - 1]) for r in rng.zipf(1.2, size=int(n))]
                 for n in rng.integers(4, 20, size=SENTENCES)]
    return words, sentences


def label_rows(words, sentences):
    space = ctoi(' ')
    rows = []
    for sentence in sentences:
        row = []
        for index in sentence:
            row += ([space] if row else []) + list(words[index])
        rows.append(row)
    return rows


def cached(path, build):
    if path and os.path.isfile(path):
        return lm.load(path, CLASSES)
    start = time.time()
    model = build()
    print('  built {} in {:.1f} s'.format(os.path.basename(path or 'model'), time.time() - start))
    if path:
        model.save(path)
    return model


def spelled_logits(rng, rows, num_steps, batch):
    """Row b spells as much of sentence b as fits at one label per three frames."""
    logits = rng.normal(size=(num_steps, batch, CLASSES)).astype(np.float32)
    logits[:, :, CLASSES - 1] += 4.0
    for b in range(batch):
        for i, c in enumerate(rows[b % len(rows)][:(num_steps - 1) // 3]):
            logits[3 * i + 1, b, c] += 6.0
            logits[3 * i + 1, b, CLASSES - 1] -= 4.0
    return logits


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def fused_total(logits, seq_len, out, out_len, scorer):
    """Mean over the utterances of ctc_score(hypothesis) + sequence_scores(hypothesis), float64;
    and how many hypotheses the exact scorer placed (status 0) with a finite model score."""
    lengths = out_len[:, 0].cpu().numpy()
    rows = [out[b, 0, :lengths[b]].cpu().tolist() for b in range(out.shape[0])]
    labels = torch.as_tensor([c for row in rows for c in row] or [0], dtype=torch.int32,
                             device='cuda')
    offsets = torch.as_tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32,
                              device='cuda')
    utt = torch.arange(len(rows), dtype=torch.int32, device='cuda')
    score, status = hip.ctc_score(logits, seq_len, labels, offsets, utt)
    total = score.double().cpu().numpy() + scorer.sequence_scores(rows)
    good = (status.cpu().numpy() == 0) & np.isfinite(total)
    return (float(total[good].mean()) if good.any() else float('nan')), int(good.sum())


def lookahead_table(logits, seq_len, name, model):
    """Per width, the plain word search and the look-ahead search: ms per launch, mean fused
    total, hypotheses counted."""
    plain = model.scaled(1.0, 0.0, -8.0)
    start = time.time()
    ahead = model.scaled(1.0, 0.0, -8.0, lookahead=True)
    print('{}: look-ahead table of {} nodes in {:.2f} s'.format(name, model.num_nodes,
                                                                time.time() - start))
    print('  {:>5s} {:>11s} {:>13s} {:>6s} {:>11s} {:>13s} {:>6s}'.format(
        'width', 'plain ms', 'plain total', 'n', 'ahead ms', 'ahead total', 'n'))
    for width in (4, 16, 64, 256, 1024):
        reps = 3 if width <= 64 else 1
        line = '  {:5d}'.format(width)
        for scorer in (plain, ahead):
            ms = timed(lambda: hip.ctc_beam_decode_wordlm(logits, seq_len, width, scorer), reps)
            out, out_len, _, _ = hip.ctc_beam_decode_wordlm(logits, seq_len, width, scorer)
            # the total under the plain scorer: the same number for both forms, to rounding
            total, count = fused_total(logits, seq_len, out, out_len, plain)
            line += ' {:11.1f} {:13.4f} {:6d}'.format(ms, total, count)
        print(line, flush=True)


def main():
    cache = sys.argv[1] if len(sys.argv) >= 2 else ''
    T, B = (int(v) for v in sys.argv[2:4]) if len(sys.argv) >= 4 else (500, 176)
    if cache:
        os.makedirs(cache, exist_ok=True)
    rng = np.random.default_rng(0)
    words, sentences = language(rng)
    rows = label_rows(words, sentences)
    space = ctoi(' ')
    models = [('word order {}'.format(order),
               cached(cache and os.path.join(cache, 'word{}.npz'.format(order)),
                      lambda order=order: lm.build_word_ngram(rows, order, CLASSES, space)))
              for order in (2, 3)]
    chars = cached(cache and os.path.join(cache, 'char5.npz'),
                   lambda: lm.build_char_ngram(rows[:2000], 5, CLASSES))
    for name, model in models:
        print('{}: {} words, {} trie nodes, {} contexts, {} successors, {:.1f} MB of tables'.format(
            name, model.num_words - 2, model.num_nodes, model.num_contexts, model.num_successors,
            sum(getattr(model, a).nbytes for a in lm.WORD_ARRAYS) / 1e6))
    print('character order 5: {} states'.format(chars.num_states))
    if len(sys.argv) >= 5 and sys.argv[4] == 'build-only':
        return
    chars = chars.scaled(1.0, 0.0)
    chars.to('cuda')
    scaled = [(name, model.scaled(1.0, 0.0, -8.0)) for name, model in models]
    logits = torch.as_tensor(spelled_logits(rng, rows, T, B)).cuda()
    seq_len = torch.full((B,), T, dtype=torch.int32, device='cuda')
    stats = torch.zeros((B, 2), dtype=torch.int64, device='cuda')
    if len(sys.argv) >= 5 and sys.argv[4] == 'lookahead-only':
        lookahead_table(logits, seq_len, *models[0])
        return
    print('T={} B={}: ms per launch'.format(T, B))
    print('  {:>5s} {:>9s} {:>9s}'.format('width', 'plain', 'char 5') +
          ''.join(' {:>13s} {:>20s}'.format(name, 'lookups / branches') for name, _ in scaled))
    for width in (64, 1024):
        reps = 3 if width <= 64 else 1
        line = '  {:5d} {:9.1f} {:9.1f}'.format(
            width, timed(lambda: hip.ctc_beam_decode(logits, seq_len, width), reps),
            timed(lambda: hip.ctc_beam_decode_lm(logits, seq_len, width, chars), reps))
        for _, scorer in scaled:
            ms = timed(lambda: hip.ctc_beam_decode_wordlm(logits, seq_len, width, scorer,
                                                          stats=stats), reps)
            per_utt = stats.double().mean(dim=0).tolist()
            line += ' {:13.1f} {:>20s}'.format(ms, '{:.0f} / {:.0f}'.format(per_utt[1], per_utt[0]))
        print(line)
    # the lookup alone: random (context, word) pairs, most of which back off
    for name, scorer in scaled:
        pairs = 1 << 20
        ctx = torch.as_tensor(rng.integers(0, scorer.num_contexts, size=pairs), dtype=torch.int32,
                              device='cuda')
        word = torch.as_tensor(rng.integers(0, scorer.num_words, size=pairs), dtype=torch.int32,
                               device='cuda')
        ms = timed(lambda: hip.wordlm_lookup(scorer, ctx, word), 3)
        print('wordlm_lookup, {}: {} pairs in {:.2f} ms ({:.1f} ns per pair)'.format(
            name, pairs, ms, ms * 1e6 / pairs))
    lookahead_table(logits, seq_len, *models[0])


if __name__ == '__main__':
    main()
