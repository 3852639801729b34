#!/usr/bin/env python
"""Times the three entry points of the sequence-wise batch normalisation (ctcasr_seq_bn_fwd /
_infer / _bwd) alone on [500, 32, 2048] (a C3 inter-layer tensor) and [500, 32, 4096], prints the
bytes each moves and its time next to the roof, and then runs C3 training steps with
--rnn_batch_norm off and on.

    python tools/batch_norm_microbench.py [--launches 30] [--steps 20] [--blocks 0,1024]

Bytes: forward 3 x the tensor (two reads, one write), inference 2 x, backward 5 x (dy and x twice
each, dx once); the roof is those bytes over the 6.3 TB/s that profiles/grad_norm.md records as
what the part sustains - a second read that hits the 256 MB last-level cache may beat it.
Kernel times: one HIP event pair per call (all launches of the call), the median and the extremes
of `--launches` calls after warm-up; the list is measured twice, alternating.  Steps: `--steps`
steps per leg on two trainers (the flag changes the parameter layout), legs alternated off / on /
off / on, host clock around a device synchronise.

Every part runs in a child process of its own under a time limit (`--limit` seconds); the first
part that fails or runs out of time ends the run with its status."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF_TBS = 6.3
SHAPES = ((500, 32, 2048), (500, 32, 4096))
EPS = 1e-5


def time_calls(fn, launches, warmup=5):
    import torch
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
    import torch
    from ctc_asr_amd import hip
    hip.load(os.environ.get('CTCASR_LIB'))
    for steps, batch, channels in SHAPES:
        x = torch.randn((steps, batch, channels), device='cuda')
        dy = torch.randn_like(x)
        gamma = torch.rand(channels, device='cuda') + 0.5
        beta = torch.randn(channels, device='cuda')
        state = torch.stack([torch.zeros(channels), torch.ones(channels)]).cuda()
        dgamma, dbeta = torch.zeros_like(gamma), torch.zeros_like(gamma)
        workspace = torch.empty(hip.seq_bn_workspace_bytes(steps * batch, channels),
                                dtype=torch.uint8, device='cuda')
        _, mean, rstd = hip.seq_bn_fwd(x, None, gamma, beta, state[0], state[1], 0.99, EPS,
                                       workspace=workspace)
        tensor_bytes = x.numel() * 4
        print('[{}, {}, {}]: {:.1f} MB, {} chunks of {} rows, workspace {:.1f} MB'.format(
            steps, batch, channels, tensor_bytes / 1e6, -(-steps * batch // hip.SEQ_BN_ROWS),
            hip.SEQ_BN_ROWS, workspace.numel() / 1e6))
        calls = (
            ('seq_bn_fwd', 3, lambda: hip.seq_bn_fwd(x, None, gamma, beta, state[0], state[1],
                                                     0.99, EPS, workspace=workspace)),
            ('seq_bn_infer', 2, lambda: hip.seq_bn_infer(x, None, gamma, beta, state[0],
                                                         state[1], EPS)),
            ('seq_bn_bwd', 5, lambda: hip.seq_bn_bwd(dy, x, None, mean, rstd, gamma, dgamma,
                                                     dbeta, workspace=workspace)))
        rows = []
        for _ in range(2):          # twice, alternated: the spread between the two is the noise
            for blocks in args.blocks:
                hip.set_option('seq_bn_blocks', blocks)
                for name, passes, fn in calls:
                    rows.append(('{} blocks={}'.format(name, blocks or 'default'), passes,
                                 time_calls(fn, args.launches)))
            hip.set_option('seq_bn_blocks', 0)
        for name, passes, (median, low, high) in rows:
            moved = passes * tensor_bytes
            print('  {:30s} {:6.1f} MB  median {:.4f} ms (min {:.4f}, max {:.4f})  roof {:.4f} ms'
                  '  {:.2f} TB/s'.format(name, moved / 1e6, median, low, high,
                                         moved / (ROOF_TBS * 1e9), moved / median / 1e9))


def steps(args):
    import numpy as np
    import torch
    import bench
    from ctc_asr_amd import hip
    from ctc_asr_amd.engine import Trainer
    from ctc_asr_amd.model import CTCModel, ModelConfig
    from ctc_asr_amd.synth import random_pcm, synthetic_batch
    hip.load(os.environ.get('CTCASR_LIB'))
    filters, layers, hidden, dense, batch, seconds, cell = bench.WORKLOADS['c3']
    trainers = {}
    for flag in (False, True):
        cfg = ModelConfig(used_model='ds2', conv_filters=filters, num_units_dense=dense,
                          num_layers_rnn=layers, num_units_rnn=hidden, rnn_cell=cell, cudnn=True,
                          dense_dropout_rate=0.1, rnn_batch_norm=flag)
        trainers[flag] = Trainer(cfg, device='cuda:0', seed=0, conv_autotune=True)
    _, _, labels, _ = synthetic_batch(batch, seconds, seed=1234, frames=1)
    rng = np.random.default_rng(4321)
    num_samples = int(round(seconds * 16000))
    pcm = torch.from_numpy(np.stack([random_pcm(rng, num_samples) for _ in range(batch)])).cuda()
    nsamp = torch.full((batch,), num_samples, dtype=torch.int32, device='cuda')
    packed = CTCModel.pack_labels(labels, trainers[False].model.device)

    def step(trainer):
        feats, lengths = hip.features(pcm, nsamp, 'mel', 'local', False, 16000)
        return trainer.train_step(feats, lengths, packed)

    def leg(trainer):
        for _ in range(3):
            step(trainer)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss = step(trainer)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3, float(loss)

    for trainer in trainers.values():
        for _ in range(5):
            step(trainer)
        trainer.drain_checks()
    for flag in (False, True, False, True):
        ms, loss = leg(trainers[flag])
        trainers[flag].drain_checks()
        print('C3 step, rnn_batch_norm {}: {:.3f} ms per step ({} steps), last loss {:.3f}'.format(
            'on ' if flag else 'off', ms, args.steps, loss))
    print('arithmetic with the flag on: {}'.format(
        {k: v for k, v in trainers[True].model.arithmetic().items() if k.startswith('rnn')}))


PARTS = {'kernels': kernels, 'steps': steps}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--launches', type=int, default=30)
    parser.add_argument('--steps', type=int, default=20, help='0 skips the training steps')
    parser.add_argument('--blocks', default='0', help='seq_bn_blocks values, comma separated')
    parser.add_argument('--limit', type=int, default=240, help='seconds per part')
    parser.add_argument('--part', choices=sorted(PARTS), help='(internal) run one part here')
    args = parser.parse_args()
    if args.part:
        args.blocks = [int(v) for v in args.blocks.split(',')]
        PARTS[args.part](args)
        return 0
    for part in ('kernels', 'steps'):
        if part == 'steps' and args.steps <= 0:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), '--part', part, '--launches',
               str(args.launches), '--steps', str(args.steps), '--blocks', args.blocks]
        try:
            code = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            print('{}: no result within {} s; stopping.'.format(part, args.limit))
            return 124
        if code != 0:
            print('{}: exit status {}; stopping.'.format(part, code))
            return code
    return 0


if __name__ == '__main__':
    sys.exit(main())
