#!/usr/bin/env python
"""Times ctcasr_ctc_align_long (K21): an hour-like shape (T = 180 000 logit frames, 54 000
labels, C = 29 - an hour of audio at the ds2 frame rate against its text), and K11's ceiling
shape (T = 1150, L = 575) through both kernels, K11 being the yardstick there.  Prints the
derived sizes (cells, back-pointer and boundary bytes, launches) and one JSON line per shape;
nothing is gated on the numbers.  ``--tile_frames N`` times another tile height as well."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ctc_asr_amd import hip  # noqa: E402


def sizes(T, L, C, tile_frames=0):
    """The layout of csrc/ctc_align_long.hip, restated."""
    ts = hip.ALIGN_LONG_TILE_STATES
    tf = min(tile_frames or hip.ALIGN_LONG_TILE_FRAMES, T)
    states = 2 * L + 1
    rows, cols = -(-T // tf), -(-states // ts)
    live = 0
    for i in range(rows):
        t_first, t_last = i * tf, min(T, (i + 1) * tf) - 1
        for j in range(cols):
            s_min, s_max = j * ts, min(states, (j + 1) * ts) - 1
            live += s_min <= 2 * t_last + 1 and s_max + 2 * (T - 1 - t_first) >= states - 2
    return {'cells': T * states, 'rows': rows, 'cols': cols, 'tiles': rows * cols,
            'live_tiles': live, 'launches': rows + cols - 1 + 4,
            'backpointer_bytes': cols * T * ts // 4, 'row_boundary_bytes': rows * cols * ts * 8,
            'column_halo_bytes': cols * T * 8, 'table_bytes': T * C * 4,
            'workspace_bytes': hip.ctc_align_long_workspace_bytes(T, C, L, tile_frames)}


REPEATS = 5


def time_ms(fns, iters, warmup=1):
    """Per function: the ms per call of REPEATS windows of ``iters`` calls each, the functions
    taking turns window by window (what else runs on the host moves both alike)."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    out = [[] for _ in fns]
    for _ in range(REPEATS):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            start = torch.cuda.Event(enable_timing=True)
            stop = torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(iters):
                fn()
            stop.record()
            torch.cuda.synchronize()
            out[k].append(start.elapsed_time(stop) / iters)
    return [sorted(v) for v in out]


def spread(values, digits):
    return {'median': round(values[len(values) // 2], digits), 'min': round(values[0], digits),
            'max': round(values[-1], digits)}


def check_path(path, states):
    """A legal monotone path from {0, 1} to {S - 1, S - 2} (on the device: one reduction)."""
    step = path[1:] - path[:-1]
    ok = bool(((step >= 0) & (step <= 2)).all()) and int(path[0]) in (0, 1) and \
        int(path[-1]) in (states - 1, states - 2)
    assert ok, 'not a path'


def run(name, T, L, C, tile_frames, iters, with_k11=False):
    rng = np.random.default_rng(0)
    logits = torch.tensor((rng.normal(size=(T, C)) * 2).astype(np.float32), device='cuda')
    labels = torch.tensor(rng.integers(0, C - 1, size=L).astype(np.int32), device='cuda')
    info = sizes(T, L, C, tile_frames)
    ws = torch.empty(info['workspace_bytes'], dtype=torch.uint8, device='cuda')
    path, score, _, _, status = hip.ctc_align_long(logits, labels, tile_frames=tile_frames,
                                                   workspace=ws)
    torch.cuda.synchronize()
    assert int(status[0]) == 0, status
    check_path(path, 2 * L + 1)
    fns = [lambda: hip.ctc_align_long(logits, labels, tile_frames=tile_frames, workspace=ws)]
    if with_k11:
        offsets = torch.tensor([0, L], dtype=torch.int32, device='cuda')
        seq = torch.tensor([T], dtype=torch.int32, device='cuda')
        x = logits.reshape(T, 1, C)
        k_ws = torch.empty(hip.ctc_align_workspace_bytes(T, 1, C, L), dtype=torch.uint8,
                           device='cuda')
        k_path, k_score, _, k_status = hip.ctc_align(x, labels, offsets, seq, L, workspace=k_ws)
        assert int(k_status[0]) == 0 and torch.equal(k_path[0], path)
        fns.append(lambda: hip.ctc_align(x, labels, offsets, seq, L, workspace=k_ws))
    times = time_ms(fns, iters)
    ms = times[0][len(times[0]) // 2]
    line = dict(shape=name, T=T, L=L, C=C, tile_frames=tile_frames or hip.ALIGN_LONG_TILE_FRAMES,
                iters=iters, windows=REPEATS, align_long_ms=spread(times[0], 4),
                score=float(score[0]), gcell_per_s=round(info['cells'] / ms / 1e6, 2),
                us_per_launch=round(ms * 1e3 / info['launches'], 2), **info)
    if with_k11:
        line['k11_ms'] = spread(times[1], 4)
        line['k11_score'] = float(k_score[0])
    print(json.dumps(line), flush=True)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--tile_frames', type=int, default=0)
    parser.add_argument('--skip_hour', action='store_true')
    args = parser.parse_args()
    heights = [0] + ([args.tile_frames] if args.tile_frames else [])
    for tile_frames in heights:
        run('k11_ceiling', 1150, 575, 29, tile_frames, 300, with_k11=True)
    if not args.skip_hour:
        for tile_frames in heights:
            run('hour', 180000, 54000, 29, tile_frames, 5)


if __name__ == '__main__':
    main()
