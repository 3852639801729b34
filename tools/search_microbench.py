#!/usr/bin/env python
"""Times ctcasr_ctc_search (K22) on a transcribe-shaped load - 64 pieces x 750 frames x 29
classes against 1, 32 and 256 phrases of 8 and 40 labels, all pieces x phrases pairs grouped by
piece - next to ctcasr_ctc_score (K14) on the same pairs in the same run, and the numpy
reference (tests/search_reference.py) on a few pairs, whose results are compared exactly:
python tools/search_microbench.py [--json out.json]

Times are HIP events around whole entry-point calls on logits already in HBM and a workspace
allocated once: each includes the log-softmax of the batch (both kernels) and the filler
pre-pass (K22).  Every configuration is warmed up, then timed in WINDOWS windows of ITERS calls;
the median window and the spread are printed."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ctc_asr_amd import hip  # noqa: E402
from tests import search_reference as sref  # noqa: E402

PIECES, FRAMES, CLASSES = 64, 750, 29
WINDOWS, ITERS = 5, 20
REFERENCE_PAIRS = 4


def windows(fn):
    """ms per call: (median, lowest, highest) over WINDOWS windows of ITERS calls."""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(WINDOWS):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(ITERS):
            fn()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop) / ITERS)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def traffic(pairs, label_len, max_hits):
    """Bytes the launch sequence needs to move, from the shapes: the log-softmax reads the
    logits and writes the table, the pre-pass reads the table and writes the filler, and every
    pair reads one emission per state and frame and one filler per frame (served by the caches
    where pairs share an utterance), its labels, and writes its hit rows and summary."""
    rows = FRAMES * PIECES
    states = 2 * label_len - 1
    return {'table_bytes': 2 * rows * CLASSES * 4, 'fill_bytes': rows * CLASSES * 4 + rows * 4,
            'pair_read_bytes': pairs * (FRAMES * (states + 1) * 4 + label_len * 4),
            'pair_write_bytes': pairs * (max_hits * 16 + 4 + 8 + 8 + 4)}


def main():
    out_path = sys.argv[sys.argv.index('--json') + 1] if '--json' in sys.argv else None
    rng = np.random.default_rng(0)
    blank = CLASSES - 1
    # trained-like: a decisive blank, labels in between
    logits = (rng.normal(size=(FRAMES, PIECES, CLASSES)) * 3.0).astype(np.float32)
    logits[:, :, blank] += 4.0
    lg = torch.as_tensor(logits).cuda()
    seq_len = torch.full((PIECES,), FRAMES, dtype=torch.int32, device='cuda')
    search_ws = torch.empty(hip.ctc_search_workspace_bytes(FRAMES, PIECES, CLASSES),
                            dtype=torch.uint8, device='cuda')
    max_hits = 16
    records = []
    for label_len in (8, 40):
        for count in (1, 32, 256):
            phrases = rng.integers(1, blank, size=(count, label_len)).astype(np.int32)
            labels = torch.as_tensor(phrases.reshape(-1)).cuda()
            offsets = torch.arange(count + 1, dtype=torch.int32, device='cuda') * label_len
            min_score = torch.full((count,), -1.0 * label_len, dtype=torch.float64, device='cuda')
            utt = torch.arange(PIECES, dtype=torch.int32, device='cuda') \
                .repeat_interleave(count).contiguous()
            phrase = torch.arange(count, dtype=torch.int32, device='cuda').repeat(PIECES)
            pairs = utt.numel()

            def run_search():
                return hip.ctc_search(lg, seq_len, labels, offsets, utt, phrase, min_score,
                                      max_hits=max_hits, max_label_len=label_len,
                                      workspace=search_ws)

            # K14 on the same pairs: one label row per pair
            score_labels = labels.reshape(count, label_len).repeat(PIECES, 1).reshape(-1) \
                .contiguous()
            score_offsets = torch.arange(pairs + 1, dtype=torch.int32, device='cuda') * label_len
            score_ws = torch.empty(max(hip.ctc_score_workspace_bytes(
                FRAMES, PIECES, CLASSES, pairs, label_len), 256), dtype=torch.uint8,
                device='cuda')

            def run_score():
                return hip.ctc_score(lg, seq_len, score_labels, score_offsets, utt,
                                     max_label_len=label_len, workspace=score_ws)

            # alternate the two, so that a busy neighbour hits both alike
            search_ms = windows(run_search)
            score_ms = windows(run_score)
            search_again = windows(run_search)
            n_hits, status = run_search()[2], run_search()[7]
            record = {'phrases': count, 'labels': label_len, 'pairs': pairs,
                      'states_per_lane': (2 * label_len - 1 + 63) // 64,
                      'search_ms': search_ms, 'search_ms_second_pass': search_again,
                      'score_ms': score_ms, 'ratio_search_over_score': search_ms[0] / score_ms[0],
                      'hits': int(n_hits.sum()), 'status_nonzero': int((status != 0).sum()),
                      'frame_states_per_s': pairs * FRAMES * (2 * label_len - 1) /
                      (search_ms[0] * 1e-3)}
            record.update(traffic(pairs, label_len, max_hits))
            records.append(record)
            print('{:3d} phrases x {:2d} labels ({:5d} pairs): search {:8.3f} ms ({:.3f} .. '
                  '{:.3f}; again {:.3f}), ctc_score {:8.3f} ms ({:.3f} .. {:.3f}), search / '
                  'score {:.2f}, hits {}'.format(count, label_len, pairs, *search_ms,
                                                 search_again[0], *score_ms,
                                                 record['ratio_search_over_score'],
                                                 record['hits']))
    # the numpy reference on a few pairs of the last configuration, and that it agrees
    table = hip.log_softmax_fwd(lg).cpu().numpy()
    got = [v.cpu().numpy() for v in hip.ctc_search(
        lg, seq_len, labels, offsets, utt[:REFERENCE_PAIRS].contiguous(),
        phrase[:REFERENCE_PAIRS].contiguous(), min_score, max_hits=max_hits, per_frame=True)]
    began = time.perf_counter()
    want = sref.search(table, [FRAMES] * PIECES, blank, phrases.tolist(),
                       min_score.cpu().numpy(), utt[:REFERENCE_PAIRS].cpu().numpy(),
                       phrase[:REFERENCE_PAIRS].cpu().numpy(), max_hits)
    reference_s = (time.perf_counter() - began) / REFERENCE_PAIRS
    names = ('hits', 'hit_score', 'n_hits', 'best_score', 'best_span', 'end_score', 'end_start',
             'status')
    equal = all(np.array_equal(a, want[name], equal_nan=True) for a, name in zip(got, names))
    print('numpy reference: {:.3f} s per pair of {} labels x {} frames; equal to the kernel on '
          '{} pairs: {}'.format(reference_s, label_len, FRAMES, REFERENCE_PAIRS, equal))
    if out_path:
        with open(out_path, 'w', encoding='utf-8') as handle:
            json.dump({'pieces': PIECES, 'frames': FRAMES, 'classes': CLASSES,
                       'windows': WINDOWS, 'iters': ITERS, 'configurations': records,
                       'reference_seconds_per_pair': reference_s, 'reference_equal': equal},
                      handle, indent=1)
    return 0 if equal else 1


if __name__ == '__main__':
    sys.exit(main())
