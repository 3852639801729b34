#!/usr/bin/env python
"""Times ctcasr_ctc_align_partial (K25) beside ctcasr_ctc_align_long (K21) on the hour-like shape
of tools/align_long_microbench.py (T = 180 000 logit frames, 54 000 labels, C = 29): K21 on the
labels as they are, K25 on the same labels (no wildcard: its outputs must equal K21's) and with
2 and 50 of them replaced by wildcards.  The four take turns window by window in one process, on
one workspace.  Prints one JSON line; nothing is gated on the numbers.  ``--small`` runs a shape
of milliseconds (T = 6000, L = 1800) for a check of the tool itself; ``--counts 50`` times K21 and
one wildcard count only (under a kernel trace the two then show as the <false> and the <true>
instantiations of each kernel)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import align_long_microbench as base  # noqa: E402
from ctc_asr_amd import hip  # noqa: E402


def with_wildcards(labels, count):
    """``count`` wildcards spread evenly, the first label and the last among them."""
    out = labels.copy()
    if count:
        out[np.linspace(0, len(out) - 1, count).round().astype(np.int64)] = hip.ALIGN_WILDCARD
    return out


def run(name, T, L, C, iters, counts=(0, 2, 50)):
    rng = np.random.default_rng(0)
    logits = torch.tensor((rng.normal(size=(T, C)) * 2).astype(np.float32), device='cuda')
    plain = rng.integers(0, C - 1, size=L).astype(np.int32)
    info = base.sizes(T, L, C)
    ws = torch.empty(info['workspace_bytes'], dtype=torch.uint8, device='cuda')
    rows = [torch.tensor(with_wildcards(plain, n), device='cuda') for n in counts]
    plain = torch.tensor(plain, device='cuda')
    want = hip.ctc_align_long(logits, plain, workspace=ws)
    assert int(want[4][0]) == 0
    want = [None if v is None else v.clone() for v in want]
    scores, wild_frames = [], []
    for n, row in zip(counts, rows):
        path, score, flp, _, status = hip.ctc_align_partial(logits, row, workspace=ws)
        torch.cuda.synchronize()
        assert int(status[0]) == 0, (n, status)
        base.check_path(path, 2 * L + 1)
        if n == 0:
            assert torch.equal(path, want[0]) and torch.equal(score, want[1]) and \
                torch.equal(flp, want[2]), 'K25 without a wildcard differs from K21'
        else:
            assert float(score[0]) >= float(want[1][0])
        on_label = (path & 1) == 1
        ids = row[(path >> 1).clamp(max=L - 1).long()]
        wild_frames.append(int((on_label & (ids == hip.ALIGN_WILDCARD)).sum()))
        scores.append(float(score[0]))
    fns = [lambda: hip.ctc_align_long(logits, plain, workspace=ws)]
    fns += [lambda row=row: hip.ctc_align_partial(logits, row, workspace=ws) for row in rows]
    times = base.time_ms(fns, iters)
    line = dict(shape=name, T=T, L=L, C=C, tile_frames=hip.ALIGN_LONG_TILE_FRAMES, iters=iters,
                windows=base.REPEATS, align_long_ms=base.spread(times[0], 4),
                align_long_score=float(want[1][0]), launches=info['launches'],
                live_tiles=info['live_tiles'], cells=info['cells'])
    for n, t, score, frames in zip(counts, times[1:], scores, wild_frames):
        line['align_partial_{}_wildcards'.format(n)] = dict(
            ms=base.spread(t, 4), score=score, wildcard_frames=frames,
            over_k21=round(t[len(t) // 2] / times[0][len(times[0]) // 2], 4))
    print(json.dumps(line), flush=True)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--small', action='store_true')
    parser.add_argument('--counts', default='0,2,50')
    args = parser.parse_args()
    counts = tuple(int(v) for v in args.counts.split(','))
    if args.small:
        run('small', 6000, 1800, 29, 5, counts)
    else:
        run('hour', 180000, 54000, 29, 3, counts)


if __name__ == '__main__':
    main()
