#!/usr/bin/env python
"""Times `ctcasr_resample` - the memset of the status word and the one launch behind it - on ten
minutes and on an hour of 48 kHz stereo int16 and of 44.1 kHz mono int16, to 16 kHz, next to
`scipy.signal.resample_poly` on the host over the same samples.

    python tools/resample_microbench.py [--launches 20] [--no_host_hour]

Device times: one HIP event pair per call of `hip.resample_launch` (no read-back of the status
word), the median and the extremes of `--launches` calls after warm-up; the rows are taken twice,
alternated, and the spread between the two is the noise.  The table of weights is built before the
clock starts (once per pair of rates); its launch is timed by itself.  Bytes: the input read once
and the output stored once, over the median.  The recordings are uniform noise made on the
device: an hour of 48 kHz stereo is 691 MB in and 115 MB out, far beyond the 256 MB Infinity
Cache; ten minutes (134 MB in and out) fit it, yet run at a lower rate than the hour - the stage
is bound by its LDS reads, not by HBM, and the tail of the shorter grid counts
(profiles/resample.md).  Host: ONE run each of `resample_poly` (its own Kaiser
window, float64, channels averaged first) on all cores numpy gives it; `--no_host_hour` leaves out
the hour, which needs about 6 GB of host memory."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ctc_asr_amd import hip  # noqa: E402


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


def host_seconds(samples, rate):
    from scipy import signal
    m, l, _, _ = hip.resample_plan(rate)
    x = samples.cpu().numpy()
    began = time.perf_counter()
    mono = x.astype(np.float64).mean(axis=1) if x.ndim == 2 else x.astype(np.float64)
    y = signal.resample_poly(mono, l, m)
    np.clip(np.rint(y), -32768, 32767).astype(np.int16)
    return time.perf_counter() - began


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--launches', type=int, default=20)
    parser.add_argument('--no_host_hour', action='store_true')
    args = parser.parse_args()
    hip.load(os.environ.get('CTCASR_LIB'))
    cases = []
    for rate, channels in ((48000, 2), (44100, 1)):
        for seconds in (600, 3600):
            shape = (rate * seconds, channels) if channels > 1 else (rate * seconds,)
            cases.append((rate, channels, seconds, shape))
    for rate in (48000, 44100):
        hip._RESAMPLE_TABLES.clear()
        median, low, high = time_launches(
            lambda: (hip._RESAMPLE_TABLES.clear(), hip.resample_table(rate, 16000, 'cuda')), 10)
        m, l, radius, taps = hip.resample_plan(rate)
        print('table {} -> 16000 ({} x {} weights, allocation included): median {:.4f} ms '
              '(min {:.4f}, max {:.4f})'.format(rate, l, taps, median, low, high))
    rows = []
    for leg in range(2):
        for rate, channels, seconds, shape in cases:
            samples = torch.randint(-32768, 32768, shape, dtype=torch.int16, device='cuda')
            hip.resample(samples[:rate], rate)             # (the table, and a check of the status)
            n_out = hip.resample_out_samples(shape[0], rate)
            moved = samples.numel() * 2 + n_out * 2
            taps = hip.resample_plan(rate)[3]
            stats = time_launches(lambda: hip.resample_launch(samples, rate), args.launches)
            host = None
            if leg == 0 and not (seconds == 3600 and args.no_host_hour):
                host = host_seconds(samples, rate)
            rows.append((leg, rate, channels, seconds, moved, n_out * taps, stats, host))
            del samples
            torch.cuda.empty_cache()
    for leg, rate, channels, seconds, moved, fma, (median, low, high), host in rows:
        line = ('leg {} {:6d} Hz x {} ch, {:4d} s: median {:.4f} ms (min {:.4f}, max {:.4f})  '
                '{:.2f} TB/s  {:.2f} Tfma/s  {:.0f} x real time'
                .format(leg, rate, channels, seconds, median, low, high, moved / median / 1e9,
                        fma / median / 1e9, seconds / (median / 1e3)))
        if host is not None:
            line += '   host resample_poly {:.2f} s ({:.0f} x real time)'.format(host,
                                                                                seconds / host)
        print(line)


if __name__ == '__main__':
    main()
