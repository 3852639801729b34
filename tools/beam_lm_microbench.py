#!/usr/bin/env python
"""Times ctcasr_ctc_beam_decode and ctcasr_ctc_beam_decode_lm side by side, in one process, on
the shapes of tools/beam_microbench.py (flat and peaked logits, C = 29), with an order-3 and an
order-5 character n-gram built from `synth.random_label` transcripts:
python tools/beam_lm_microbench.py [T B]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ctc_asr_amd import hip, lm, synth  # noqa: E402
from ctc_asr_amd.labels import encode  # noqa: E402


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def main():
    T, B = (int(v) for v in sys.argv[1:3]) if len(sys.argv) >= 3 else (500, 16)
    C = 29
    rng = np.random.default_rng(0)
    rows = [encode(synth.random_label(rng, int(rng.integers(20, 200)))) for _ in range(2000)]
    # a scorer that scores nothing runs the very search of the unfused kernel - same insertions,
    # same result -, so its column is the cost of the fused kernel itself; an n-gram changes the
    # search as well (it prices every emitted label, fewer children beat the beam's bottom)
    zero = lm.LmScorer(np.zeros((1, C), dtype=np.int32), np.zeros((1, C), dtype=np.float32))
    scorers = [('zero scorer', zero)]
    for order in (3, 5):
        scorer = lm.build_char_ngram(rows, order, C).scaled(1.0, 0.0)
        scorer.to('cuda')
        scorers.append(('order {} ({} states)'.format(order, scorer.num_states), scorer))
    for name, scale, blank_bias in (('untrained (flat)', 0.3, 0.0),
                                    ('trained-like (peaked)', 3.0, 4.0)):
        logits = (rng.normal(size=(T, B, C)) * scale).astype(np.float32)
        logits[:, :, -1] += blank_bias
        lg = torch.as_tensor(logits).cuda()
        sl = torch.full((B,), T, dtype=torch.int32, device='cuda')
        print('{}: T={} B={}, us per frame'.format(name, T, B))
        print('  {:>5s} {:>9s}'.format('width', 'unfused') +
              ''.join(' {:>24s}'.format(label) for label, _ in scorers))
        for width in (16, 64, 256, 1024):
            line = '  {:5d} {:9.1f}'.format(
                width, timed(lambda: hip.ctc_beam_decode(lg, sl, width), reps=2) * 1e3 / T)
            for _, scorer in scorers:
                ms = timed(lambda: hip.ctc_beam_decode_lm(lg, sl, width, scorer), reps=2)
                line += ' {:24.1f}'.format(ms * 1e3 / T)
            print(line)


if __name__ == '__main__':
    main()
