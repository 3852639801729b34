#!/usr/bin/env python
"""Times ctcasr_ctc_align alone, next to ctcasr_ctc_loss_fwd_bwd at the same shape, on the
C3 shape (T' = 500, B = 32, 150 labels: slab and table in LDS; and with max_label_len 575: the
back-pointer slab in the workspace) and the C5 ceiling (T' = 1700, B = 16, 575 labels: table and
slab in the workspace).  Prints one JSON line per shape; nothing is gated on the numbers."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ctc_asr_amd import hip  # noqa: E402

SHAPES = (('c3', 500, 32, 150, 150), ('c3_max_label_len_575', 500, 32, 150, 575),
          ('c5_ceiling', 1700, 16, 575, 575))
LDS_MAX = 150 * 1024


def tier(T, C, max_label_len):
    """The launcher's choice (csrc/ctc_align.hip)."""
    s_pad = 2 * max_label_len + 1
    fixed = 2 * s_pad * 8 + (s_pad * 4 + 15) // 16 * 16 + 64 + 256 + 64 * 3 * 16
    if fixed + T * C * 4 + T * ((s_pad + 63) // 64) * 16 <= LDS_MAX:
        return 'slab+table in LDS'
    return 'table in LDS' if fixed + T * C * 4 <= LDS_MAX else 'both in workspace'


def time_ms(fn, iters=20):
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    C = 29
    for name, T, B, L, max_label_len in SHAPES:
        rng = np.random.default_rng(0)
        logits = torch.tensor((rng.normal(size=(T, B, C)) * 2).astype(np.float32), device='cuda')
        flat = torch.tensor(rng.integers(0, C - 1, size=B * L).astype(np.int32), device='cuda')
        offsets = torch.arange(0, (B + 1) * L, L, dtype=torch.int32, device='cuda')
        seq = torch.full((B,), T, dtype=torch.int32, device='cuda')
        ws = torch.empty(hip.ctc_align_workspace_bytes(T, B, C, max_label_len),
                         dtype=torch.uint8, device='cuda')
        path, score, frame_logp, status = hip.ctc_align(logits, flat, offsets, seq,
                                                        max_label_len, workspace=ws)
        torch.cuda.synchronize()
        assert (status == 0).all(), status
        align_ms = time_ms(lambda: hip.ctc_align(logits, flat, offsets, seq, max_label_len,
                                                 path=path, score=score,
                                                 frame_logp=frame_logp, status=status,
                                                 workspace=ws))
        loss_ws = torch.empty(hip.ctc_loss_workspace_bytes(T, B, C, max_label_len),
                              dtype=torch.uint8, device='cuda')
        loss_ms = time_ms(lambda: hip.ctc_loss_fwd_bwd(logits, flat, offsets, seq,
                                                       max_label_len, workspace=loss_ws))
        print(json.dumps({'shape': name, 'T': T, 'B': B, 'L': L, 'max_label_len': max_label_len,
                          'tier': tier(T, C, max_label_len), 'align_ms': round(align_ms, 4),
                          'align_us_per_step': round(align_ms * 1e3 / T, 4),
                          'loss_fwd_bwd_ms': round(loss_ms, 4)}))


if __name__ == '__main__':
    main()
