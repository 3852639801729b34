"""numpy restatement of `ctcasr_noise_mix` (include/ctcasr.h, K16): the integer draws through
`augment_reference.below`, the exact integer powers, the gain in float64 and the mix before
rounding, `y64 = x + f64(g) * v`.  Nothing here looks at the library."""

import numpy as np

from tests.augment_reference import below

MAX_CLIP = 1 << 24


def draw_row(seed, b, n, max_samples, clip_offsets, snr_lo, snr_hi, permille):
    """(status, k, o, snr) before the powers are known: status 1 = to be mixed unless a power is
    zero, 2 = the drawn clip's length is not served, 0 = not drawn or a bad row."""
    if n < 1 or n > max_samples or below(seed, 8 * b, 1000) >= permille:
        return 0, 0, 0, 0
    k = below(seed, 8 * b + 1, len(clip_offsets) - 1)
    snr = snr_lo + below(seed, 8 * b + 3, snr_hi - snr_lo + 1)
    length = int(clip_offsets[k + 1]) - int(clip_offsets[k])
    if length < 1 or length > MAX_CLIP:
        return 2, k, 0, snr
    return 1, k, below(seed, 8 * b + 2, length), snr


def noise_under(bank, clip_offsets, k, o, n):
    """v[i] = clip_k[(o + i) mod len_k] for i < n, int64."""
    clip = np.asarray(bank[int(clip_offsets[k]):int(clip_offsets[k + 1])], dtype=np.int64)
    return clip[(o + np.arange(n, dtype=np.int64)) % len(clip)]


def gain64(ps, pn, snr):
    """sqrt(Ps / Pn) * 10^(-snr / 20) in float64 (the integers converted as Python converts them:
    correctly rounded)."""
    return float(np.sqrt(float(ps) / float(pn)) * 10.0 ** (-snr / 20.0))


def mix(pcm, num_samples, bank, clip_offsets, seed, snr_lo, snr_hi, permille=1000, gains=None):
    """The whole call on the host.  Returns a dict:
    draws int32 [B, 4], powers int64 [B, 2], gain float64 [B] (0 where not mixed),
    y64: per row None (a bit copy) or the float64 mix of the first n samples, computed with
    ``gains[b]`` (the gain the library reported, a float32) where ``gains`` is given and with the
    float64 gain itself otherwise."""
    pcm = np.asarray(pcm)
    batch, max_samples = pcm.shape
    draws = np.zeros((batch, 4), dtype=np.int32)
    powers = np.zeros((batch, 2), dtype=np.int64)
    gain = np.zeros(batch, dtype=np.float64)
    y64 = [None] * batch
    for b in range(batch):
        n = int(num_samples[b])
        status, k, o, snr = draw_row(seed, b, n, max_samples, clip_offsets, snr_lo, snr_hi,
                                     permille)
        if status == 1:
            x = pcm[b, :n].astype(np.int64)
            v = noise_under(bank, clip_offsets, k, o, n)
            ps, pn = int((x * x).sum()), int((v * v).sum())
            powers[b] = ps, pn
            if ps == 0 or pn == 0:
                status = 2
            else:
                gain[b] = gain64(ps, pn, snr)
                g = gain[b] if gains is None else np.float32(gains[b])
                y64[b] = x.astype(np.float64) + np.float64(g) * v.astype(np.float64)
        draws[b] = status, k, o, snr
    return {'draws': draws, 'powers': powers, 'gain': gain, 'y64': y64}


def rounded(y64):
    """clamp(rint(y64)) as int16: round to nearest even, saturated."""
    return np.clip(np.rint(y64), -32768, 32767).astype(np.int16)


def expected_pcm(pcm, num_samples, result):
    """int16 [B, N]: the mix rounded from float64 where a row is mixed, the input elsewhere."""
    out = np.array(pcm, dtype=np.int16, copy=True)
    for b, y in enumerate(result['y64']):
        if y is not None:
            out[b, :len(y)] = rounded(y)
    return out


def snr_db(x, y64):
    """10 log10(sum x^2 / sum (y64 - x)^2) in float64."""
    x = np.asarray(x, dtype=np.float64)
    d = np.asarray(y64, dtype=np.float64) - x
    return 10.0 * np.log10((x * x).sum() / (d * d).sum())


def find_seed(predicate, start=1, tries=200000):
    """The first seed >= start for which ``predicate(seed)`` holds (a search on the host)."""
    for seed in range(start, start + tries):
        if predicate(seed):
            return seed
    raise AssertionError('no seed found')
