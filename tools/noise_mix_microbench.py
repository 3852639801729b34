#!/usr/bin/env python
"""Times `ctcasr_noise_mix` - both launches and the memset before them, as one call - on a
C3-shaped batch (32 x 10 s: int16 [32, 160000] PCM), next to ctcasr_features on the same batch in
the same run, and then C3-shaped training steps from a corpus on disk through
`input_fn_generator('train_batch')` with the noise flags off and on.

    python tools/noise_mix_microbench.py [--launches 50] [--steps 6] [--legs 2]

Kernel times: one HIP event pair per call, the median and the extremes of `--launches` calls after
warm-up; the rows are taken twice, alternated, and the spread between the two is the noise.  Bytes:
what the code moves - speech and noise read twice, one store - over the median.  Banks: short clips
(401 samples: 399 wraps per row, one group in fifty walks its samples one by one), long clips
(30 s: no wrap) and an hour-sized bank whose reads miss every cache.  Pipeline: every leg is one
epoch over the same manifest, host clock around a device synchronise, legs alternated off / on on
ONE trainer.  `--steps 0` skips the pipeline part."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from ctc_asr_amd import hip  # noqa: E402


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


def _bank(rng, clip, clips):
    bank = torch.from_numpy(rng.integers(-1000, 1000, size=clip * clips).astype(np.int16)).cuda()
    offsets = torch.arange(clips + 1, dtype=torch.int64, device='cuda') * clip
    return bank, offsets


def kernels(args):
    from ctc_asr_amd.synth import random_pcm
    batch, samples = 32, 160000
    rng = np.random.default_rng(4321)
    pcm = torch.from_numpy(np.stack([random_pcm(rng, samples) for _ in range(batch)])).cuda()
    nsamp = torch.full((batch,), samples, dtype=torch.int32, device='cuda')
    out = torch.empty_like(pcm)
    scratch = pcm.clone()
    banks = (('short clips (64 x 401)', _bank(rng, 401, 64)),
             ('long clips (8 x 480000)', _bank(rng, 480000, 8)),
             ('an hour (225 x 256000)', _bank(rng, 256000, 225)))
    moved = batch * samples * 2 * 5           # speech and noise twice, one store
    print('batch {} x {} samples = {:.1f} MB of PCM; a call that mixes every row moves {:.1f} MB'
          .format(batch, samples, pcm.numel() * 2 / 1e6, moved / 1e6))
    rows = []
    for _ in range(2):
        rows.append(('features (mel, local)', 0, time_launches(
            lambda: hip.features(pcm, nsamp, 'mel', 'local', False, 16000), args.launches)))
        for name, (bank, offsets) in banks:
            rows.append(('noise_mix ' + name, moved, time_launches(
                lambda: hip.noise_mix(pcm, nsamp, bank, offsets, 7, 10, 30, 1000, out=out),
                args.launches)))
        bank, offsets = banks[1][1]
        rows.append(('noise_mix long clips, in place', moved, time_launches(
            lambda: hip.noise_mix(scratch, nsamp, bank, offsets, 7, 10, 30, 1000, out=scratch),
            args.launches)))
        rows.append(('noise_mix long clips, permille 500, in place', 0, time_launches(
            lambda: hip.noise_mix(scratch, nsamp, bank, offsets, 7, 10, 30, 500, out=scratch),
            args.launches)))
        rows.append(('noise_mix permille 0 (a copy)', batch * samples * 4, time_launches(
            lambda: hip.noise_mix(pcm, nsamp, bank, offsets, 7, 10, 30, 0, out=out),
            args.launches)))
    for name, nbytes, (median, low, high) in rows:
        rate = '  {:.2f} TB/s'.format(nbytes / median / 1e9) if nbytes else ''
        print('{:46s} median {:.4f} ms  (min {:.4f}, max {:.4f}){}'.format(name, median, low,
                                                                          high, rate))


def pipeline(args):
    from ctc_asr_amd import synth
    from ctc_asr_amd.engine import Trainer
    from ctc_asr_amd.input_functions import input_fn_generator
    from ctc_asr_amd.model import ModelConfig
    from ctc_asr_amd.params import CSV_DELIMITER, CSV_FIELDNAMES, FLAGS
    filters, layers, hidden, dense, batch, seconds, rnn_cell = bench.WORKLOADS['c3']
    with tempfile.TemporaryDirectory() as tmp:
        corpus, csv = os.path.join(tmp, 'corpus'), os.path.join(tmp, 'train.csv')
        rows = synth.write_corpus(corpus, csv, [seconds] * batch, seed=78, subdir='train',
                                  sacrificial_row=False)
        with open(csv, 'w', encoding='utf-8') as handle:
            handle.write(CSV_DELIMITER.join(CSV_FIELDNAMES) + '\n')
            for row in [r for _ in range(args.steps) for r in rows] + [rows[-1]]:
                handle.write(CSV_DELIMITER.join(row) + '\n')
        noise_csv = os.path.join(tmp, 'noise.csv')
        synth.write_corpus(os.path.join(tmp, 'noise'), noise_csv, [30.0] * 8, seed=79,
                           subdir='n', sacrificial_row=False)
        FLAGS.reset()
        FLAGS.update(corpus_dir=corpus, train_csv=csv, batch_size=batch, feature_type='mel',
                     feature_normalization='local', random_seed=5,
                     noise_dir=os.path.join(tmp, 'noise'))
        cfg = ModelConfig(used_model='ds2', conv_filters=filters, num_units_dense=dense,
                          num_layers_rnn=layers, num_units_rnn=hidden, rnn_cell=rnn_cell,
                          cudnn=True, dense_dropout_rate=0.1)
        trainer = Trainer(cfg, device='cuda:0', seed=0)

        def epoch(**flags):
            FLAGS.update(noise_csv='', noise_permille=500)
            FLAGS.update(**flags)
            steps, audio, mixed = 0, 0.0, 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for item in input_fn_generator('train_batch', device='cuda:0', seed=11)():
                trainer.train_step(item.features['spectrogram'],
                                   item.features['spectrogram_length'], item.packed_labels)
                steps += 1
                audio += item.audio_seconds
                if item.noise_draws is not None:
                    mixed += 1
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            trainer.drain_checks()
            return wall / steps * 1e3, audio / wall, steps, mixed

        kinds = (('off', {}), ('noise, permille 500', {'noise_csv': noise_csv}),
                 ('noise, permille 1000', {'noise_csv': noise_csv, 'noise_permille': 1000}))
        epoch()                      # untimed: allocator, page cache, autotuning
        epoch(noise_csv=noise_csv)   # ... and the upload of the bank
        for leg in range(args.legs):
            for name, flags in kinds:
                ms, rate, steps, mixed = epoch(**flags)
                print('leg {} {:22s} {:.3f} ms per step, {:.1f} audio-s/s, {} steps, {} of them '
                      'through noise_mix'.format(leg, name, ms, rate, steps, mixed))
        FLAGS.reset()


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--launches', type=int, default=50)
    parser.add_argument('--steps', type=int, default=6)
    parser.add_argument('--legs', type=int, default=2)
    args = parser.parse_args()
    hip.load(os.environ.get('CTCASR_LIB'))
    kernels(args)
    if args.steps > 0:
        pipeline(args)


if __name__ == '__main__':
    main()
