#!/usr/bin/env python
"""Times minimum word error rate training (include/ctcasr.h, K23):
(a) ctcasr_ctc_mwer beside ctcasr_ctc_loss_fwd_bwd and ctcasr_ctc_score on the same logits, at
    B = 32, T = 500, C = 29 with the N = 8 / 16 best hypotheses of a width-64 search (HIP events),
    with the workspace bytes and the bytes the kernels move;
(b) the training step of the C3 workload (bench.py: 2 convs, 5 x BiLSTM-1024, batch 32, 10 s) with
    the flag off and on, for both risks (host clock around steps that end in a synchronise).
python tools/mwer_microbench.py [kernel|step|all]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ctc_asr_amd import hip  # noqa: E402

T, B, C = 500, 32, 29


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def kernel():
    rng = np.random.default_rng(0)
    # trained-like logits: a transcript of 150 labels (15 per second) spread over the frames,
    # peaked, so that the hypotheses of the list are as long as a training step's
    logits = (rng.normal(size=(T, B, C)) * 0.5).astype(np.float32)
    logits[:, :, -1] += 4.0
    for b in range(B):
        frames = np.sort(rng.choice(T, size=150, replace=False))
        logits[frames, b, rng.integers(1, 28, size=150)] += 8.0
    lg = torch.as_tensor(logits).cuda()
    sl = torch.full((B,), T, dtype=torch.int32, device='cuda')
    for nbest in (8, 16):
        out, out_len, _, n_paths = hip.ctc_beam_decode_nbest(lg, sl, 64, nbest)
        lengths = out_len.reshape(-1)
        offsets = torch.zeros(B * nbest + 1, dtype=torch.int32, device='cuda')
        offsets[1:] = torch.cumsum(lengths, 0)
        keep = torch.arange(T, device='cuda')[None, :] < lengths[:, None]
        labels = out.reshape(-1, T)[keep].contiguous()
        longest = int(lengths.max())
        utt = torch.arange(B, device='cuda', dtype=torch.int32).repeat_interleave(nbest)
        risk = torch.as_tensor(rng.integers(0, 6, size=B * nbest).astype(np.float32)).cuda()
        # the references of the CTC loss: rank 0 of every list
        top = out[:, 0]
        top_len = out_len[:, 0]
        ref_offsets = torch.zeros(B + 1, dtype=torch.int32, device='cuda')
        ref_offsets[1:] = torch.cumsum(top_len, 0)
        ref = top[torch.arange(T, device='cuda')[None, :] < top_len[:, None]].contiguous()
        grad = torch.zeros_like(lg)
        need = hip.ctc_mwer_workspace_bytes(T, B, C, nbest, longest)
        workspace = torch.empty(need, dtype=torch.uint8, device='cuda')
        score_ws = torch.empty(max(hip.ctc_score_workspace_bytes(T, B, C, B * nbest, longest),
                                   256), dtype=torch.uint8, device='cuda')
        loss_ws = torch.empty(hip.ctc_loss_workspace_bytes(T, B, C, int(top_len.max())),
                              dtype=torch.uint8, device='cuda')
        mwer_ms = timed(lambda: hip.ctc_mwer(lg, sl, labels, offsets, n_paths, risk,
                                             max_label_len=longest, scale=1.0 / B,
                                             accumulate=True, grad=grad, workspace=workspace))
        score_ms = timed(lambda: hip.ctc_score(lg, sl, labels, offsets, utt,
                                               max_label_len=longest, workspace=score_ws))
        loss_ms = timed(lambda: hip.ctc_loss_fwd_bwd(lg, ref, ref_offsets, sl,
                                                     int(top_len.max()), grad=grad,
                                                     workspace=loss_ws))
        search_ms = timed(lambda: hip.ctc_beam_decode_nbest(lg, sl, 64, nbest), reps=2)
        status = hip.ctc_mwer(lg, sl, labels, offsets, n_paths, risk, max_label_len=longest,
                              workspace=workspace)[4]
        # bytes: both lattices of every listed hypothesis written once and read once (the rows
        # below seq_len, at the padded row of 64 * states-per-lane fp64), the table written once
        # and read by every sweep, the gradient read and written
        per_lane = (2 * longest + 1 + 63) // 64
        per_lane = per_lane if per_lane <= 3 else (6 if per_lane <= 6 else 18)
        listed = int(n_paths.clamp(min=0).sum())
        lattice = 2 * listed * T * per_lane * 64 * 8
        moved = 2 * lattice + T * B * C * 4 * 4
        print('N = {:2d}: {} hypotheses listed (longest {} labels, {} states per lane, status != '
              '0: {}); ctc_mwer {:.3f} ms, ctc_score {:.3f} ms, ctc_loss_fwd_bwd (B rows) {:.3f} '
              'ms, the width-64 n-best search {:.3f} ms; workspace {:.1f} MB, lattice bytes '
              'written + read {:.1f} MB -> {:.3f} ms at 6.3 TB/s'.format(
                  nbest, listed, longest, per_lane, int(((status != 0) & (status != -1)).sum()),
                  mwer_ms, score_ms, loss_ms, search_ms, need / 1e6, moved / 1e6,
                  moved / 6.3e12 * 1e3))


def step():
    from ctc_asr_amd.engine import Trainer
    from ctc_asr_amd.model import CTCModel, ModelConfig
    from ctc_asr_amd.synth import synthetic_batch
    cfg = ModelConfig(used_model='ds2', conv_filters=(32, 32), num_units_dense=2048,
                      num_layers_rnn=5, num_units_rnn=1024, rnn_cell='lstm', cudnn=True,
                      dense_dropout_rate=0.1)
    feats, lengths, labels, texts = synthetic_batch(32, 10.0, seed=1234)
    for name, kwargs in (('off', {}),
                         ('label risk', {'mwer_nbest': 8, 'mwer_risk': 'label'}),
                         ('word risk', {'mwer_nbest': 8, 'mwer_risk': 'word'})):
        trainer = Trainer(cfg, device='cuda', seed=0, conv_autotune=True, **kwargs)
        feats_d = torch.tensor(feats, device='cuda')
        len_d = torch.tensor(lengths, device='cuda')
        packed = CTCModel.pack_labels(labels, trainer.model.device)
        for _ in range(3):
            trainer.train_step(feats_d, len_d, packed, originals=texts)
        torch.cuda.synchronize()
        steps = 8
        t0 = time.perf_counter()
        for _ in range(steps):
            trainer.train_step(feats_d, len_d, packed, originals=texts)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        trainer.drain_checks()
        extra = ''
        if trainer.mwer:
            extra = ' (nbest 8, beam width 64; lists of {:.1f}, expected risk {:.2f})'.format(
                float(trainer.last_mwer_paths.float().mean()),
                float(trainer.last_expected_risk.mean()))
        print('C3 step, mwer {}: {:.1f} ms{}'.format(name, ms, extra))
        del trainer
        torch.cuda.empty_cache()


if __name__ == '__main__':
    what = sys.argv[1] if len(sys.argv) > 1 else 'all'
    if what in ('kernel', 'all'):
        kernel()
    if what in ('step', 'all'):
        step()
