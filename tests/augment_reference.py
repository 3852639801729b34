"""numpy restatement of the augmentation kernels (include/ctcasr.h, K15): the integer draws and
mask intervals of `ctcasr_spec_augment`, exact, and the resampler of `ctcasr_speed_perturb` in
float64 and, tap for tap, in the fp32 arithmetic the header pins.  Nothing here looks at the
library."""

import numpy as np

MASK64 = (1 << 64) - 1
COLS = 80


def r24(seed, idx):
    """Top 24 bits of the splitmix64 finaliser over (seed, idx)."""
    z = (seed + 0x9E3779B97F4A7C15 * (idx + 1)) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return z >> 40


def below(seed, idx, n):
    assert 1 <= n <= 1 << 24
    return (r24(seed, idx) * n) >> 24


def mask_intervals(seed, lengths, out_frames, n_freq, freq_width, n_time, time_width,
                   time_permille):
    """int32 [B, n_freq + n_time, 2]: (start, width), frequency masks first."""
    out = np.zeros((len(lengths), n_freq + n_time, 2), dtype=np.int32)
    for b, length in enumerate(lengths):
        length = min(max(int(length), 0), out_frames)
        if length == 0:
            continue
        for i in range(n_freq):
            w = below(seed, 64 * b + 2 * i, min(freq_width, COLS) + 1)
            out[b, i] = below(seed, 64 * b + 2 * i + 1, COLS - w + 1), w
        for i in range(n_time):
            cap = min(time_width, length * time_permille // 1000)
            w = below(seed, 64 * b + 32 + 2 * i, cap + 1)
            out[b, n_freq + i] = below(seed, 64 * b + 32 + 2 * i + 1, length - w + 1), w
    return out


def mask_cells(intervals, lengths, out_frames, n_freq):
    """bool [B, out_frames, 80]: the cells the masks of ``intervals`` cover."""
    mask = np.zeros((len(lengths), out_frames, COLS), dtype=bool)
    for b, length in enumerate(lengths):
        length = min(max(int(length), 0), out_frames)
        for i, (start, width) in enumerate(intervals[b]):
            if i < n_freq:
                mask[b, :length, start:start + width] = True
            else:
                assert start + width <= length
                mask[b, start:start + width, :] = True
    return mask


# Seeds whose single mask lands on an edge, found by search with `mask_intervals` and re-asserted
# in tests/test_augment_host.py: seed -> (start, width) of row 0.
# One time mask, time_width 200, permille 1000, L = out_frames = 129 (tiles of 64, 64 and 1 frame):
TIME_SEAM_SEEDS = {
    74: (64, 3),            # starts on a tile seam
    1263: (22, 42),         # ends on frame 64
    6: (6, 123),            # spans three tiles
    125: (0, 129),          # the whole row
    46192: (128, 1),        # the last frame alone, in a tile of one frame
    454: (80, 0),           # zero width
}
# One frequency mask, freq_width 27, L = out_frames = 5:
FREQ_EDGE_SEEDS = {
    38: (0, 25),            # touches column 0
    45: (53, 27),           # ends at column 80
    10: (59, 0),            # zero width
}


def resample_num_samples(n, percent):
    if n < 1 or not 50 <= percent <= 200:
        return 0
    return max(1, n * 100 // percent)


def tap_weight(c, d):
    """h(d) = c sinc(c d) 0.5 (1 + cos(pi c d / 12)) inside |c d| < 12, float64, vectorised."""
    u = c * np.asarray(d, dtype=np.float64)
    safe = np.where(u == 0.0, 1.0, u)
    sinc = np.where(u == 0.0, 1.0, np.sin(np.pi * safe) / (np.pi * safe))
    return np.where(np.abs(u) < 12.0, c * sinc * 0.5 * (1.0 + np.cos(np.pi * u / 12.0)), 0.0)


def resample_float64(x, percent):
    """y[j] = sum_k x[k] h(j P / 100 - k), k in [0, n), all in float64, before rounding.  The
    position is split into integer part and phase in integers; the taps walked are a superset of
    the filter's support, whose edge `tap_weight` decides."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    n_out = resample_num_samples(n, percent)
    pos = np.arange(n_out, dtype=np.int64) * percent
    t0, phase = pos // 100, (pos % 100) / 100.0
    c = 95.0 / max(percent, 100)
    reach = int(np.ceil(12.0 / c)) + 2
    y = np.zeros(n_out, dtype=np.float64)
    for m in range(-reach, reach + 1):
        k = t0 + m
        valid = (k >= 0) & (k < n)
        y += np.where(valid, x[np.clip(k, 0, n - 1)], 0.0) * tap_weight(c, phase - m)
    return y


def speed_perturb(x, percent):
    """int16 result of one row: rounded to nearest even, saturated; a bit copy at 100."""
    if percent == 100:
        return np.asarray(x, dtype=np.int16).copy()
    return np.clip(np.rint(resample_float64(x, percent)), -32768, 32767).astype(np.int16)


def tap_radius(percent):
    """R of the header: the kernel's taps are m in [-R, R + 1]."""
    return 12 * max(percent, 100) // 95


def fma_f32(a, b, acc):
    """fp32(a * b + acc), one rounding, for float64 arrays that hold an int16 (``a``) and fp32
    values (``b``, ``acc``).  The product of 16 and 24 significant bits is exact in float64.  Its
    sum with ``acc`` is not always, so the sum is taken with Knuth's error-free two-sum (s + e is
    the exact sum, s its float64 rounding) and s is then moved to the neighbouring float64 with an
    odd last bit wherever e != 0 (rounding to odd).  A value rounded to odd at 53 bits rounds to
    the same fp32 as the exact value, since 53 >= 24 + 2 (Boldo and Melquiond, "Emulation of FMA
    and correctly rounded sums: proved algorithms using rounding to odd", 2008); a plain float64
    sum would round twice and can land on the wrong side of an fp32 tie.  fp32 overflow and
    underflow are out of reach: |sum| < 2^22 and no product is below 2^-149 unless it is 0."""
    p = a * b
    s = p + acc
    bb = s - p
    e = (p - (s - bb)) + (acc - bb)
    even = (s.view(np.int64) & 1) == 0
    away = np.nextafter(s, np.where(e > 0.0, np.inf, -np.inf))
    s = np.where((e != 0.0) & even, away, s)
    return s.astype(np.float32).astype(np.float64)


def speed_perturb_f32(x, percent):
    """The arithmetic include/ctcasr.h pins for `ctcasr_speed_perturb`, literally: taps
    k = t0 + m for m in [-R, R + 1] that fall into [0, n), weights h(p / 100 - m) evaluated in
    float64 and rounded once to fp32, one fused multiply-add per tap in ascending k from +0.0f
    (`fma_f32`: exact, by two-sum and rounding to odd, because this interpreter may have no
    `math.fma`), then round to nearest even and saturate.  Vectorised over the output samples,
    a loop over the <= 52 taps.  -> (int16 [n_out], float32 [n_out] accumulator before rounding);
    at 100 % the copy and its values."""
    x = np.asarray(x, dtype=np.int16)
    n = len(x)
    if percent == 100:
        return x.copy(), x.astype(np.float32)
    n_out = resample_num_samples(n, percent)
    pos = np.arange(n_out, dtype=np.int64) * percent
    t0, phase = pos // 100, pos % 100
    c = 95.0 / max(percent, 100)
    radius = tap_radius(percent)
    xf = x.astype(np.float64)
    acc = np.zeros(n_out, dtype=np.float64)
    for m in range(-radius, radius + 2):
        k = t0 + m
        valid = (k >= 0) & (k < n)
        w = tap_weight(c, phase / 100.0 - m).astype(np.float32).astype(np.float64)
        # a tap outside the row is skipped, not added as zero: -0.0 + +0.0 aside, the same sum
        acc = np.where(valid, fma_f32(xf[np.clip(k, 0, n - 1)], w, acc), acc)
    y = np.clip(np.rint(acc), -32768, 32767).astype(np.int16)
    return y, acc.astype(np.float32)


def tie_eligible(acc):
    """Where the accumulator before rounding lies within 2^-6 of a half-integer: the only
    samples at which a kernel whose fp64 sin / cos differ from the host's in the last place may
    round the other way (tests/test_gpu_augment_edges.py)."""
    a = np.asarray(acc, dtype=np.float64)
    return np.abs(np.abs(a - np.floor(a)) - 0.5) <= 2.0 ** -6
