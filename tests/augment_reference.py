"""numpy restatement of the augmentation kernels (include/ctcasr.h, K15): the integer draws and
mask intervals of `ctcasr_spec_augment`, exact, and the resampler of `ctcasr_speed_perturb` in
float64.  Nothing here looks at the library."""

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
