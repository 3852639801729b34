#!/usr/bin/env python
"""Times the n-best entry point next to the top-1 one, and ctcasr_ctc_score next to the only
route to exact hypothesis scores that existed before it - the logits replicated per hypothesis
and fed to ctcasr_ctc_loss_fwd_bwd, in chunks of CHUNK hypotheses so that the lattices fit - on
the shapes of tools/beam_microbench.py (flat and peaked logits, C = 29):
python tools/nbest_microbench.py [T B]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ctc_asr_amd import hip  # noqa: E402

CHUNK = 200          # hypotheses per ctc_loss_fwd_bwd launch of the old route
TOP_PATHS = 100      # hypotheses per utterance scored in (c)


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


def pack(out, out_len, n_paths):
    """(labels, offsets, utt, longest) of every listed hypothesis, on the device."""
    batch, top_paths, num_steps = out.shape
    listed = torch.arange(top_paths, device=out.device)[None, :] < n_paths[:, None]
    lengths = torch.where(listed, out_len, torch.zeros_like(out_len))[listed]
    rows = out[listed]
    utt = torch.arange(batch, device=out.device, dtype=torch.int32)[:, None] \
        .expand(-1, top_paths)[listed].contiguous()
    offsets = torch.zeros(lengths.numel() + 1, dtype=torch.int32, device=out.device)
    offsets[1:] = torch.cumsum(lengths, 0)
    keep = torch.arange(num_steps, device=out.device)[None, :] < lengths[:, None]
    return rows[keep].contiguous(), offsets, utt, int(lengths.max())


def main():
    T, B = (int(v) for v in sys.argv[1:3]) if len(sys.argv) >= 3 else (500, 16)
    C = 29
    rng = np.random.default_rng(0)
    for name, scale, blank_bias in (('untrained (flat)', 0.3, 0.0),
                                    ('trained-like (peaked)', 3.0, 4.0)):
        logits = (rng.normal(size=(T, B, C)) * scale).astype(np.float32)
        logits[:, :, -1] += blank_bias
        lg = torch.as_tensor(logits).cuda()
        sl = torch.full((B,), T, dtype=torch.int32, device='cuda')
        print('{}: T={} B={}'.format(name, T, B))
        # (b) the n-best entry point next to the top-1 one
        for width in (64, 1024):
            line = '  width {:5d}: top-1 {:9.3f} ms'.format(
                width, timed(lambda: hip.ctc_beam_decode(lg, sl, width), reps=2))
            for top_paths in (1, 16, 100):
                if top_paths > width:
                    line += ' | N={:3d} (above the width)'.format(top_paths)
                    continue
                ms = timed(lambda: hip.ctc_beam_decode_nbest(lg, sl, width, top_paths), reps=2)
                line += ' | N={:3d} {:9.3f} ms'.format(top_paths, ms)
            print(line)
        # (c) exact scores of B x TOP_PATHS hypotheses of the width-1024 search
        out, out_len, _, n_paths = hip.ctc_beam_decode_nbest(lg, sl, 1024, TOP_PATHS,
                                                             normalization='log_softmax')
        labels, offsets, utt, longest = pack(out, out_len, n_paths)
        hyps = utt.numel()
        score, status = hip.ctc_score(lg, sl, labels, offsets, utt, max_label_len=longest)
        new_ms = timed(lambda: hip.ctc_score(lg, sl, labels, offsets, utt,
                                             max_label_len=longest))

        def old_route():
            losses = []
            for first in range(0, hyps, CHUNK):
                last = min(first + CHUNK, hyps)
                rows = utt[first:last].long()
                part = (offsets[first:last + 1] - offsets[first]).contiguous()
                flat = labels[int(offsets[first]):int(offsets[last])].contiguous()
                if flat.numel() == 0:
                    flat = torch.zeros(1, dtype=torch.int32, device='cuda')
                loss, _, _ = hip.ctc_loss_fwd_bwd(lg[:, rows].contiguous(), flat, part,
                                                  sl[rows].contiguous(), longest)
                losses.append(loss)
            return torch.cat(losses)

        old_ms = timed(old_route, reps=2)
        worst = float((score + old_route()).abs().max())
        print('  ctc_score over {} hypotheses (longest {} labels, status != 0: {}): {:.3f} ms; '
              'replicated logits through ctc_loss_fwd_bwd in chunks of {}: {:.3f} ms; ratio '
              '{:.1f}; max |score + loss| {:.3g}'.format(
                  hyps, longest, int((status != 0).sum()), new_ms, CHUNK, old_ms,
                  old_ms / new_ms, worst))


if __name__ == '__main__':
    main()
