"""numpy restatement of `ctcasr_resample` (include/ctcasr.h, K19): the plan and the output count in
integers, the weight table in float64 rounded once to float32, the frame values of the four
sample formats and the tap sum in the fp32 arithmetic the header pins - and, beside it, an
independent form of the same filter that is float64 from end to end.  Nothing here looks at the
library."""

import math

import numpy as np

from tests.augment_reference import fma_f32, tap_weight

MAX_TABLE = 16640
RATES = (4000, 192000)
S16, U8, S32, F32 = 0, 1, 2, 3
FORMAT_OF = {np.dtype(np.int16): S16, np.dtype(np.uint8): U8, np.dtype(np.int32): S32,
             np.dtype(np.float32): F32}

# (M, L, R, taps) to 16 000 Hz, as the issue and the header list them
PLANS_TO_16K = {
    8000: (1, 2, 12, 26), 11025: (441, 640, 12, 26), 12000: (3, 4, 12, 26),
    22050: (441, 320, 17, 36), 24000: (3, 2, 18, 38), 32000: (2, 1, 25, 52),
    44100: (441, 160, 34, 70), 48000: (3, 1, 37, 76), 88200: (441, 80, 69, 140),
    96000: (6, 1, 75, 152), 192000: (12, 1, 151, 304),
}


def plan(rate_in, rate_out=16000):
    """(M, L, R, taps), or None for a pair that is not served."""
    if not (RATES[0] <= rate_in <= RATES[1] and RATES[0] <= rate_out <= RATES[1]):
        return None
    g = math.gcd(rate_in, rate_out)
    m, l = rate_in // g, rate_out // g
    s = max(m, l)
    radius = (1200 * s) // (95 * l)
    taps = 2 * radius + 2
    if l * taps > MAX_TABLE:
        return None
    return m, l, radius, taps


def out_samples(n, rate_in, rate_out=16000):
    p = plan(rate_in, rate_out)
    if p is None or n < 1 or n > 2 ** 31 - 1:
        return 0
    return max(1, n * p[1] // p[0])


def cutoff(m, l):
    return (95.0 * l) / (100.0 * max(m, l))


def table(rate_in, rate_out=16000):
    """float32 [L, taps]: entry (p, i) = h(p / L - (i - R)) in float64, rounded once."""
    m, l, radius, taps = plan(rate_in, rate_out)
    p = np.arange(l, dtype=np.float64)[:, None] / float(l)
    i = (np.arange(taps) - radius).astype(np.float64)[None, :]
    return tap_weight(cutoff(m, l), p - i).astype(np.float32)


def frame_values(samples):
    """float32 [n]: the sum over channels, in ascending order and in fp32, of every sample on the
    int16 scale.  ``samples``: [n] or [n, C] of int16, uint8, int32 or float32."""
    x = np.asarray(samples)
    if x.ndim == 1:
        x = x[:, None]
    fmt = FORMAT_OF[x.dtype]
    if fmt == S16:
        v = x.astype(np.float32)
    elif fmt == U8:
        v = ((x.astype(np.int32) - 128) * 256).astype(np.float32)
    elif fmt == S32:
        v = x.astype(np.float32) * np.float32(2.0 ** -16)
    else:
        v = x * np.float32(32768.0)
    s = v[:, 0].copy()
    for c in range(1, x.shape[1]):
        s = (s + v[:, c]).astype(np.float32)
    return s


def gain(channels):
    return np.float32(1.0 / channels)


def _finish(acc, channels):
    """sat16(rintf(acc * gain)) from a float32 accumulator."""
    scaled = (acc.astype(np.float32) * gain(channels)).astype(np.float32)
    return np.clip(np.rint(scaled), -32768, 32767).astype(np.int16)


def resample_f32(samples, rate_in, rate_out=16000):
    """The arithmetic the header pins -> (int16 [n_out], float32 [n_out] accumulator times gain,
    before the rounding to an integer).  The fused multiply-add is `fma_f32` of
    tests/augment_reference.py: the product of two fp32 values is exact in float64, its sum
    with the fp32 accumulator is rounded to odd there and then once to fp32."""
    x = np.asarray(samples)
    channels = 1 if x.ndim == 1 else x.shape[1]
    s = frame_values(x)
    n = len(s)
    m, l, radius, taps = plan(rate_in, rate_out)
    n_out = out_samples(n, rate_in, rate_out)
    if m == l:
        acc = s[:n_out].copy()
    else:
        w = table(rate_in, rate_out).astype(np.float64)
        pos = np.arange(n_out, dtype=np.int64) * m
        t0, phase = pos // l, pos % l
        s64 = s.astype(np.float64)
        acc = np.zeros(n_out, dtype=np.float64)
        for i in range(taps):
            k = t0 - radius + i
            valid = (k >= 0) & (k < n)
            # a tap outside the recording adds a zero: the accumulator keeps its value
            acc = np.where(valid, fma_f32(s64[np.clip(k, 0, n - 1)], w[phase, i], acc), acc)
        acc = acc.astype(np.float32)
    scaled = (acc * gain(channels)).astype(np.float32)
    return _finish(acc, channels), scaled


def resample_float64(samples, rate_in, rate_out=16000):
    """Independent form, float64 throughout: y[j] = mean over channels of
    sum_k x[k] h(j M / L - k), weights never rounded to fp32, no table, the taps walked a superset
    of the filter's support.  -> float64 [n_out], before rounding."""
    x = np.asarray(samples)
    if x.ndim == 1:
        x = x[:, None]
    fmt = FORMAT_OF[x.dtype]
    v = x.astype(np.float64)
    if fmt == U8:
        v = (v - 128.0) * 256.0
    elif fmt == S32:
        v = v / 65536.0
    elif fmt == F32:
        v = v * 32768.0
    mono = v.mean(axis=1)
    n = len(mono)
    m, l, _, _ = plan(rate_in, rate_out)
    n_out = out_samples(n, rate_in, rate_out)
    if m == l:
        return mono[:n_out]
    c = cutoff(m, l)
    reach = int(np.ceil(12.0 / c)) + 2
    pos = np.arange(n_out, dtype=np.int64) * m
    t0, frac = pos // l, (pos % l) / float(l)
    y = np.zeros(n_out, dtype=np.float64)
    for d in range(-reach, reach + 1):
        k = t0 + d
        valid = (k >= 0) & (k < n)
        y += np.where(valid, mono[np.clip(k, 0, n - 1)], 0.0) * tap_weight(c, frac - d)
    return y


def to_int16(y):
    return np.clip(np.rint(y), -32768, 32767).astype(np.int16)


def compare(got, want):
    """(largest difference in counts, share of samples that differ)."""
    diff = np.abs(np.asarray(got, dtype=np.int64) - np.asarray(want, dtype=np.int64))
    return int(diff.max()), float((diff != 0).mean())
