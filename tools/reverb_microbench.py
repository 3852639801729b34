#!/usr/bin/env python
"""Times `ctcasr_reverb` on a C3-shaped batch (32 x 10 s: int16 [32, 160000] PCM) with banks of
about 1000-tap and about 8000-tap responses at permille 500 and 1000, next to ctcasr_features on
the same batch in the same run, and then C3-shaped training steps from a corpus on disk through
`input_fn_generator('train_batch')` with --rir_csv off and on.

    python tools/reverb_microbench.py [--launches 30] [--steps 6] [--legs 2]

Kernel times: one HIP event pair per call, the median and the extremes of `--launches` calls after
warm-up; the rows are taken twice, alternated, and the spread between the two is the noise.
Multiply-adds: rows that status 1 was drawn for x samples x taps (the padded length the kernel
walks), over the median, beside the derived roof of the dot instructions (256 CUs x 4 SIMDs x 16
lanes x 2 per instruction x 2.4 GHz = 78.6 T/s).  Pipeline: every leg is one epoch over the same
manifest, host clock around a device synchronise, legs alternated off / on on ONE trainer.
`--steps 0` skips the pipeline part."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from scipy.io import wavfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from ctc_asr_amd import hip  # noqa: E402

ROOF = 256 * 4 * 16 * 2 * 2.4e9          # multiply-adds per second


def time_launches(fn, launches, warmup=3):
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


def synthetic_rir(rng, t60, taps, pre_delay=40, peak=20000):
    """A direct path and an exponentially decaying noise tail (60 dB in ``t60`` seconds)."""
    t = np.arange(taps) / 16000.0
    tail = rng.normal(size=taps) * np.exp(-6.907755 * t / t60) * 0.3
    tail[0] = 1.0
    h = np.concatenate([np.zeros(pre_delay), tail]) * peak
    return np.clip(np.rint(h), -32768, 32767).astype(np.int16)


def _bank(rng, t60, taps, rooms=8):
    from ctc_asr_amd.reverb import quantise_rir
    parts = [quantise_rir(synthetic_rir(rng, t60, taps)) for _ in range(rooms)]
    lengths = [len(p[0]) for p in parts]
    to = lambda a, dtype: torch.from_numpy(np.asarray(a, dtype=dtype)).cuda()    # noqa: E731
    return (to(np.concatenate([p[0] for p in parts]), np.int16),
            to(np.concatenate([[0], np.cumsum(lengths)]), np.int64),
            to([p[1] for p in parts], np.int32), to([p[2] for p in parts], np.float32)), lengths


def kernels(args):
    from ctc_asr_amd.synth import random_pcm
    batch, samples = 32, 160000
    rng = np.random.default_rng(4321)
    pcm = torch.from_numpy(np.stack([random_pcm(rng, samples) for _ in range(batch)])).cuda()
    nsamp = torch.full((batch,), samples, dtype=torch.int32, device='cuda')
    out = torch.empty_like(pcm)
    draws = torch.zeros((batch, 2), dtype=torch.int32, device='cuda')
    banks = (('about 1000 taps (T60 0.07 s)', _bank(rng, 0.07, 1500)),
             ('about 8000 taps (T60 0.9 s)', _bank(rng, 0.9, 12000)))
    print('batch {} x {} samples = {:.1f} MB of PCM, read once and stored once per call'
          .format(batch, samples, pcm.numel() * 2 / 1e6))
    rows = []
    for _ in range(2):
        rows.append(('features (mel, local)', 0, time_launches(
            lambda: hip.features(pcm, nsamp, 'mel', 'local', False, 16000), args.launches)))
        for name, (bank, lengths) in banks:
            for permille in (500, 1000):
                hip.reverb(pcm, nsamp, *bank, 7, permille, out=out, draws=draws)
                got = draws.cpu().numpy()
                macs = sum(samples * lengths[r] for status, r in got if status == 1)
                rows.append(('reverb {}, permille {} ({} rows, {:.1f} G)'.format(
                    name, permille, int((got[:, 0] == 1).sum()), macs / 1e9), macs, time_launches(
                        lambda: hip.reverb(pcm, nsamp, *bank, 7, permille, out=out),
                        args.launches)))
        bank = banks[0][1][0]
        rows.append(('reverb permille 0 (a copy)', 0, time_launches(
            lambda: hip.reverb(pcm, nsamp, *bank, 7, 0, out=out), args.launches)))
    for name, macs, (median, low, high) in rows:
        rate = ''
        if macs:
            per_s = macs / (median * 1e-3)
            rate = '  {:.1f} T/s = {:.0f} % of the roof'.format(per_s / 1e12, 100 * per_s / ROOF)
        print('{:62s} median {:.4f} ms  (min {:.4f}, max {:.4f}){}'.format(name, median, low,
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
        rng = np.random.default_rng(80)
        rir_dir, rir_csv = os.path.join(tmp, 'rir'), os.path.join(tmp, 'rir.csv')
        os.makedirs(rir_dir)
        with open(rir_csv, 'w', encoding='utf-8') as handle:
            handle.write(CSV_DELIMITER.join(CSV_FIELDNAMES) + '\n')
            for i, t60 in enumerate((0.1, 0.2, 0.3, 0.5, 0.7, 0.9)):
                wavfile.write(os.path.join(rir_dir, 'r{}.wav'.format(i)), 16000,
                              synthetic_rir(rng, t60, 16000))
                handle.write('r{}.wav;;1.0\n'.format(i))
        FLAGS.reset()
        FLAGS.update(corpus_dir=corpus, train_csv=csv, batch_size=batch, feature_type='mel',
                     feature_normalization='local', random_seed=5, rir_dir=rir_dir)
        cfg = ModelConfig(used_model='ds2', conv_filters=filters, num_units_dense=dense,
                          num_layers_rnn=layers, num_units_rnn=hidden, rnn_cell=rnn_cell,
                          cudnn=True, dense_dropout_rate=0.1)
        trainer = Trainer(cfg, device='cuda:0', seed=0)

        def epoch(**flags):
            FLAGS.update(rir_csv='', rir_permille=500)
            FLAGS.update(**flags)
            steps, audio, wet = 0, 0.0, 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for item in input_fn_generator('train_batch', device='cuda:0', seed=11)():
                trainer.train_step(item.features['spectrogram'],
                                   item.features['spectrogram_length'], item.packed_labels)
                steps += 1
                audio += item.audio_seconds
                if item.reverb_draws is not None:
                    wet += 1
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            trainer.drain_checks()
            return wall / steps * 1e3, audio / wall, steps, wet

        kinds = (('off', {}), ('reverb, permille 500', {'rir_csv': rir_csv}),
                 ('reverb, permille 1000', {'rir_csv': rir_csv, 'rir_permille': 1000}))
        epoch()                      # untimed: allocator, page cache, autotuning
        epoch(rir_csv=rir_csv)       # ... and the upload of the bank
        for leg in range(args.legs):
            for name, flags in kinds:
                ms, rate, steps, wet = epoch(**flags)
                print('leg {} {:22s} {:.3f} ms per step, {:.1f} audio-s/s, {} steps, {} of them '
                      'through reverb'.format(leg, name, ms, rate, steps, wet))
        FLAGS.reset()


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--launches', type=int, default=30)
    parser.add_argument('--steps', type=int, default=6)
    parser.add_argument('--legs', type=int, default=2)
    args = parser.parse_args()
    hip.load(os.environ.get('CTCASR_LIB'))
    kernels(args)
    if args.steps > 0:
        pipeline(args)


if __name__ == '__main__':
    main()
