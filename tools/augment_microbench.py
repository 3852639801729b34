#!/usr/bin/env python
"""Times the augmentation kernels alone on a C3-shaped batch (32 x 10 s: int16 [32, 160000] PCM,
float32 [32, 999, 80] features), next to ctcasr_features on the same batch - the kernel they sit
around, the yardstick - and then one bucket sequence of `bench.py --workload c5`'s shape from a
corpus on disk through `input_fn_generator('train_bucket')` into training steps, with the
augmentation flags off and on.

    python tools/augment_microbench.py [--launches 50] [--files 96] [--repeat 4] [--legs 2]

Kernel times: one HIP event pair per launch, the median and the extremes of `--launches` launches
after warm-up.  Pipeline: every leg is one epoch over the same manifest with the same shuffle
seed, host clock around a device synchronise, the legs alternated off / on / off / on on ONE
trainer; the difference between the legs of one kind is the run-to-run spread the other difference
has to be read against.  audio-s/s counts SOURCE seconds; `frames` is what the steps processed.
`--files 0` skips the pipeline part."""
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


def kernels(args):
    from ctc_asr_amd.synth import random_pcm
    batch, samples = 32, 160000
    rng = np.random.default_rng(4321)
    pcm = torch.from_numpy(np.stack([random_pcm(rng, samples) for _ in range(batch)])).cuda()
    nsamp = torch.full((batch,), samples, dtype=torch.int32, device='cuda')
    feats, lengths = hip.features(pcm, nsamp, 'mel', 'local', False, 16000)
    print('batch {} x {} samples = {:.1f} MB of PCM, features {} = {:.1f} MB'.format(
        batch, samples, pcm.numel() * 2 / 1e6, tuple(feats.shape), feats.numel() * 4 / 1e6))
    rows = []
    for _ in range(2):              # twice, alternated: the spread between the two is the noise
        rows.append(('features (mel, local)', time_launches(
            lambda: hip.features(pcm, nsamp, 'mel', 'local', False, 16000), args.launches)))
        for name, percents in (('all 90', [90]), ('all 110', [110]), ('90/100/110', [90, 100, 110]),
                               ('all 97 (100 phases)', [97]), ('all 200 (52 taps)', [200])):
            percent = torch.tensor([percents[i % len(percents)] for i in range(batch)],
                                   dtype=torch.int32, device='cuda')
            width = max(hip.resample_num_samples(samples, p) for p in percents)
            rows.append(('speed_perturb ' + name, time_launches(
                lambda: hip.speed_perturb(pcm, nsamp, percent, width), args.launches)))
        for name, setting in (('2 x 27 + 2 x 100', (2, 27, 2, 100, 1000)),
                              ('16 x 27 + 16 x 100', (16, 27, 16, 100, 1000))):
            rows.append(('spec_augment ' + name, time_launches(
                lambda: hip.spec_augment(feats, lengths, 7, *setting), args.launches)))
    for name, (median, low, high) in rows:
        print('{:36s} median {:.4f} ms  (min {:.4f}, max {:.4f})'.format(name, median, low, high))
    masked = float((feats == 0).float().mean())
    print('share of feature cells masked after the runs above: {:.1%}'.format(masked))


def pipeline(args):
    from ctc_asr_amd import synth
    from ctc_asr_amd.engine import Trainer
    from ctc_asr_amd.input_functions import input_fn_generator
    from ctc_asr_amd.model import ModelConfig
    from ctc_asr_amd.params import CSV_DELIMITER, CSV_FIELDNAMES, FLAGS
    filters, layers, hidden, dense, batch, _, rnn_cell = bench.WORKLOADS['c5']
    with tempfile.TemporaryDirectory() as tmp:
        corpus, csv = os.path.join(tmp, 'corpus'), os.path.join(tmp, 'train.csv')
        rng = np.random.default_rng(77)
        rows = synth.write_corpus(corpus, csv,
                                  synth.librispeech_like_durations(rng, args.files, drop=True),
                                  seed=78, subdir='train', sacrificial_row=False)
        with open(csv, 'w', encoding='utf-8') as handle:
            handle.write(CSV_DELIMITER.join(CSV_FIELDNAMES) + '\n')
            for row in [r for r in rows for _ in range(args.repeat)] + [rows[-1]]:
                handle.write(CSV_DELIMITER.join(row) + '\n')
        FLAGS.reset()
        FLAGS.update(corpus_dir=corpus, train_csv=csv, batch_size=batch, num_buckets=8,
                     feature_type='mel', feature_normalization='local', random_seed=5)
        cfg = ModelConfig(used_model='ds2', conv_filters=filters, num_units_dense=dense,
                          num_layers_rnn=layers, num_units_rnn=hidden, rnn_cell=rnn_cell,
                          cudnn=True, dense_dropout_rate=0.1)
        trainer = Trainer(cfg, device='cuda:0', seed=0)

        def epoch(**flags):
            FLAGS.update(spec_augment=False, speed_perturb='')
            FLAGS.update(**flags)
            steps, audio, frames = 0, 0.0, 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for item in input_fn_generator('train_bucket', device='cuda:0', seed=11)():
                trainer.train_step(item.features['spectrogram'],
                                   item.features['spectrogram_length'], item.packed_labels)
                steps += 1
                audio += item.audio_seconds
                frames += item.features['spectrogram'].shape[0] * \
                    item.features['spectrogram'].shape[1]
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            trainer.drain_checks()
            return wall / steps * 1e3, audio / wall, steps, frames

        kinds = (('off', {}), ('spec_augment', {'spec_augment': True}),
                 ('speed 90,100,110', {'speed_perturb': '90,100,110'}),
                 ('both', {'spec_augment': True, 'speed_perturb': '90,100,110'}),
                 ('both, all 90', {'spec_augment': True, 'speed_perturb': '90'}))
        epoch()                      # untimed: allocator, page cache, autotuning
        epoch(spec_augment=True, speed_perturb='90,100,110')
        for leg in range(args.legs):
            for name, flags in kinds:
                ms, rate, steps, frames = epoch(**flags)
                print('leg {} {:18s} {:.3f} ms per step, {:.1f} audio-s/s (source seconds), '
                      '{} steps, {:,d} padded frames'.format(leg, name, ms, rate, steps, frames))
        FLAGS.reset()


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--launches', type=int, default=50)
    parser.add_argument('--files', type=int, default=96)
    parser.add_argument('--repeat', type=int, default=4)
    parser.add_argument('--legs', type=int, default=2)
    args = parser.parse_args()
    hip.load(os.environ.get('CTCASR_LIB'))
    kernels(args)
    if args.files > 0:
        pipeline(args)


if __name__ == '__main__':
    main()
