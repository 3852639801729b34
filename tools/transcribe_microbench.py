#!/usr/bin/env python
"""Times the device side of long-recording transcription (K18) and one whole `transcribe` call.

    python tools/transcribe_microbench.py [--launches 30] [--minutes 10] [--beam_width 64]

1. `ctcasr_vad_energy` on 10 minutes and on 1 hour of synthetic audio, beside its derived roof
   (bytes moved / 8.0 TB/s, the HBM3E rate of the data sheet; bytes = 2 per sample read + 8 per
   hop of 160 samples stored) and beside the numpy form of the same pass on this host (int64
   squares, sum per hop).  One hour of PCM (115 MB) fits the 256 MiB last-level cache, so a loop
   over ONE buffer is not an HBM measurement: every row is taken twice, on one buffer ('warm') and
   rotating over copies that add up to more than 600 MB ('rotating').  The 2-byte aligned path (a
   view one sample into the buffer) is timed the same way.
2. `ctcasr_gather_segments` for a batch of 32 pieces of about 10 s, beside the slice-and-pad form
   in torch (one zero fill and B slice copies).
3. One `transcribe` call on `--minutes` of synthetic audio (a floor of rms 30, bursts of rms 3000
   of 0.3 .. 20 s with pauses of 0.5 .. 3 s, about a seventh of the recording: the default floor
   percentile needs a tenth) with the C3-shaped model of bench.py at random weights, split into
   upload, segmentation, forward, decode and alignment (host clock around a device synchronise
   per stage).  Random weights emit far more labels than speech does, so decode and alignment
   are upper bounds, not what a trained model costs.

Kernel times: one HIP event pair per call, median and extremes of `--launches` calls after
warm-up."""
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

HBM_BYTES_PER_S = 8.0e12
RATE = 16000


def time_launches(fn, launches, warmup=3):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    pairs = []
    for i in range(launches):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn(i)
        stop.record()
        pairs.append((start, stop))
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in pairs)
    return statistics.median(ms), ms[0], ms[-1]


def show(name, timing, note=''):
    print('{:58s} median {:.4f} ms  (min {:.4f}, max {:.4f}){}'.format(name, *timing, note))


def energy_pass(args):
    rng = np.random.default_rng(17)
    for label, seconds in (('10 minutes', 600), ('1 hour', 3600)):
        n = seconds * RATE
        host = rng.integers(-3000, 3001, size=n + 8).astype(np.int16)
        nbytes = 2 * n + 8 * (-(-n // hip.VAD_HOP))
        roof_ms = nbytes / HBM_BYTES_PER_S * 1e3
        copies = max(2, -(-600_000_000 // (2 * n)))
        buffers = [torch.from_numpy(host).cuda() for _ in range(copies)]
        print('{}: {:,d} samples, {:.1f} MB moved, roof {:.4f} ms; {} copies for the rotating rows'
              .format(label, n, nbytes / 1e6, roof_ms, copies))
        for path, offset in (('16-byte aligned', 0), ('2-byte aligned view', 1)):
            for kind, pick in (('warm', lambda i: 0), ('rotating', lambda i: i % copies)):
                timing = time_launches(
                    lambda i: hip.vad_energy(buffers[pick(i)][offset:offset + n]), args.launches)
                show('vad_energy {}, {}, {}'.format(label, path, kind), timing,
                     '  {:.2f} TB/s = {:.0f} % of the roof'.format(
                         nbytes / (timing[0] * 1e-3) / 1e12, 100 * roof_ms / timing[0]))
        del buffers
        torch.cuda.empty_cache()
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            x = host[:n].astype(np.int64)
            energy = (x * x).reshape(-1, hip.VAD_HOP).sum(axis=1)
            walls.append((time.perf_counter() - t0) * 1e3)
        got, _ = hip.vad_energy(torch.from_numpy(host[:n]).cuda())
        assert np.array_equal(got.cpu().numpy(), energy)
        print('{:58s} median {:.1f} ms  (min {:.1f}, max {:.1f}) on this host'.format(
            'numpy form, ' + label, statistics.median(walls), min(walls), max(walls)))


def gather(args):
    rng = np.random.default_rng(18)
    n, batch = 3600 * RATE, 32
    pcm = torch.from_numpy(rng.integers(-3000, 3001, size=n).astype(np.int16)).cuda()
    lengths = (rng.integers(800, 1001, size=batch) * hip.VAD_HOP).astype(np.int32)
    starts = (np.sort(rng.choice(n // hip.VAD_HOP - 1000, size=batch, replace=False)) *
              hip.VAD_HOP).astype(np.int64)
    width = int(lengths.max())
    seg_start, seg_len = torch.from_numpy(starts).cuda(), torch.from_numpy(lengths).cuda()
    moved = 2 * int(lengths.sum()) + 2 * batch * width
    print('gather: {} pieces of {:.1f} .. {:.1f} s into [{}, {}], {:.1f} MB moved'.format(
        batch, lengths.min() / RATE, lengths.max() / RATE, batch, width, moved / 1e6))

    def slices(_):
        out = torch.zeros((batch, width), dtype=torch.int16, device='cuda')
        for b in range(batch):
            out[b, :lengths[b]] = pcm[starts[b]:starts[b] + lengths[b]]
        return out

    ours = hip.gather_segments(pcm, seg_start, seg_len, width)[0]
    assert torch.equal(ours, slices(0))
    for _ in range(2):
        show('gather_segments (one launch)', time_launches(
            lambda i: hip.gather_segments(pcm, seg_start, seg_len, width), args.launches))
        show('torch zeros + {} slice copies'.format(batch), time_launches(slices, args.launches))


def synthetic_recording(seconds, seed=19):
    rng = np.random.default_rng(seed)
    n = int(seconds * RATE)
    rms = np.full(n, 30.0, dtype=np.float32)
    at = int(rng.uniform(0.5, 3.0) * RATE)
    while at < n:
        stop = at + int(rng.uniform(0.3, 20.0) * RATE)
        rms[at:stop] = 3000.0
        at = stop + int(rng.uniform(0.5, 3.0) * RATE)
    return np.clip(rng.standard_normal(n, dtype=np.float32) * rms, -32768, 32767).astype(np.int16)


def whole_call(args):
    from ctc_asr_amd import transcribe
    from ctc_asr_amd.model import CTCModel, ModelConfig
    from ctc_asr_amd.params import FLAGS
    filters, layers, hidden, dense, batch, _, rnn_cell = bench.WORKLOADS['c3']
    FLAGS.reset()
    FLAGS.update(feature_type='mel', feature_normalization='local', batch_size=batch)
    cfg = ModelConfig(used_model='ds2', conv_filters=filters, num_units_dense=dense,
                      num_layers_rnn=layers, num_units_rnn=hidden, rnn_cell=rnn_cell, cudnn=True,
                      dense_dropout_rate=0.0, beam_width=args.beam_width)
    model = CTCModel(cfg, 'cuda', seed=1)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'long.wav')
        wavfile.write(path, RATE, synthetic_recording(args.minutes * 60))
        for leg, timestamps in ((0, False), (1, False), (2, True)):
            timings = {}
            t0 = time.perf_counter()
            result = transcribe.transcribe(model, path, timestamps=timestamps, timings=timings)
            wall = time.perf_counter() - t0
            pieces = result['segments']
            print('transcribe leg {} ({}): {:.1f} s of audio, {:.1f} s in {} pieces (longest '
                  '{:.2f} s), wall {:.3f} s'.format(
                      leg, 'timestamps' if timestamps else 'text only', result['audio_seconds'],
                      result['speech_seconds'], len(pieces),
                      max([p['end'] - p['start'] for p in pieces] + [0.0]), wall))
            print('    ' + ', '.join('{} {:.1f} ms'.format(k, v * 1e3) for k, v in timings.items())
                  + ', WAV read and the rest {:.1f} ms'.format(
                      (wall - sum(timings.values())) * 1e3))
    FLAGS.reset()


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--launches', type=int, default=30)
    parser.add_argument('--minutes', type=float, default=10.0)
    parser.add_argument('--beam_width', type=int, default=64)
    args = parser.parse_args()
    hip.load(os.environ.get('CTCASR_LIB'))
    energy_pass(args)
    gather(args)
    if args.minutes > 0:
        whole_call(args)


if __name__ == '__main__':
    main()
