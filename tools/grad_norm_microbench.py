#!/usr/bin/env python
"""Times ctcasr_grad_norm alone on the gradient arena of the C3 model (BASELINE.json configs[2]:
its layer slices are the segments), next to ctcasr_absmax over the same bytes - an existing
one-read kernel, the yardstick - and then C3 training steps with clipping off and on.

    python tools/grad_norm_microbench.py [--launches 50] [--steps 20] [--blocks 0,1024,4096]

Kernel times: one HIP event pair per launch (for grad_norm: both of its launches), the median and
the extremes of `--launches` launches after warm-up.  Steps: `--steps` steps per leg, the legs
alternated off / on / off / on on ONE trainer, host clock around a device synchronise.
`--steps 0` skips the training part."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from ctc_asr_amd import hip  # noqa: E402
from ctc_asr_amd.model import CTCModel, ModelConfig, param_spec  # noqa: E402


def c3_config(dropout=0.1):
    filters, layers, hidden, dense, batch, seconds, cell = bench.WORKLOADS['c3']
    cfg = ModelConfig(used_model='ds2', conv_filters=filters, num_units_dense=dense,
                      num_layers_rnn=layers, num_units_rnn=hidden, rnn_cell=cell, cudnn=True,
                      dense_dropout_rate=dropout)
    return cfg, batch, seconds


def arena_layout(cfg):
    """(n, [offsets], [layer names]) of `model.ParamArena` without building a model."""
    offsets, names, cursor = [0], [], 0
    for name, shape in param_spec(cfg):
        layer = name.split('/')[0]
        if names and layer != names[-1]:
            offsets.append(cursor)
        if not names or layer != names[-1]:
            names.append(layer)
        cursor += (int(np.prod(shape)) + 3) // 4 * 4
    return cursor, offsets + [cursor], names


def time_launches(fn, launches, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(launches):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        pairs.append((start, stop))
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in pairs)
    return statistics.median(ms), ms[0], ms[-1]


def kernels(args):
    cfg, _, _ = c3_config()
    n, table, names = arena_layout(cfg)
    print('C3 arena: {:,d} floats = {:.3f} GB in {} segments {}'.format(
        n, n * 4 / 1e9, len(names), names))
    grad = torch.randn(n, device='cuda') * 0.01
    offsets = torch.tensor(table, dtype=torch.int64, device='cuda')
    out = torch.zeros(len(names) + 2, device='cuda')
    workspace = torch.empty(hip.grad_norm_workspace_bytes(n, len(names)), dtype=torch.uint8,
                            device='cuda')
    word = torch.zeros(1, dtype=torch.int32, device='cuda')
    rows = []
    for rounds in range(2):         # twice, alternated: the spread between the two is the noise
        rows.append(('absmax', time_launches(lambda: hip.absmax(grad, word), args.launches)))
        for blocks in args.blocks:
            hip.set_option('grad_norm_blocks', blocks)
            rows.append(('grad_norm blocks={}'.format(blocks or 'default'), time_launches(
                lambda: hip.grad_norm(grad, offsets, 1.0, 1.0, out=out, workspace=workspace),
                args.launches)))
        hip.set_option('grad_norm_blocks', 0)
    for name, (median, low, high) in rows:
        print('{:28s} median {:.4f} ms  (min {:.4f}, max {:.4f})  {:.2f} TB/s'.format(
            name, median, low, high, n * 4 / median / 1e9))
    want = float(grad.double().pow(2).sum().sqrt())
    print('global norm {:.6f} (torch float64: {:.6f}), factor {:.6f}'.format(
        float(out[-2]), want, float(out[-1])))


def steps(args):
    from ctc_asr_amd.engine import Trainer
    from ctc_asr_amd.synth import random_pcm, synthetic_batch
    cfg, batch, seconds = c3_config()
    trainer = Trainer(cfg, device='cuda:0', seed=0, conv_autotune=True)
    _, _, labels, _ = synthetic_batch(batch, seconds, seed=1234, frames=1)
    rng = np.random.default_rng(4321)
    num_samples = int(round(seconds * 16000))
    pcm = torch.from_numpy(np.stack([random_pcm(rng, num_samples) for _ in range(batch)])).cuda()
    nsamp = torch.full((batch,), num_samples, dtype=torch.int32, device='cuda')
    packed = CTCModel.pack_labels(labels, trainer.model.device)

    def step():
        feats, lengths = hip.features(pcm, nsamp, 'mel', 'local', False, 16000)
        return trainer.train_step(feats, lengths, packed)

    def leg(max_norm):
        trainer.max_grad_norm = max_norm
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for _ in range(5):
        step()
    trainer.drain_checks()
    for max_norm in (0.0, args.max_grad_norm, 0.0, args.max_grad_norm):
        ms = leg(max_norm)
        trainer.drain_checks()
        print('C3 step, max_grad_norm {:g}: {:.3f} ms per step ({} steps){}'.format(
            max_norm, ms, args.steps, '' if not max_norm else
            '; last global norm {:.4g}, factor {:.4g}, clipped steps so far {}'.format(
                float(trainer.last_grad_norms[-1]), float(trainer.last_clip_factor),
                trainer.clipped_step_count())))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--launches', type=int, default=50)
    parser.add_argument('--steps', type=int, default=20)
    parser.add_argument('--max_grad_norm', type=float, default=100.0)
    parser.add_argument('--blocks', type=lambda s: [int(v) for v in s.split(',')], default=[0])
    args = parser.parse_args()
    hip.load(os.environ.get('CTCASR_LIB'))
    kernels(args)
    if args.steps > 0:
        steps(args)


if __name__ == '__main__':
    main()
