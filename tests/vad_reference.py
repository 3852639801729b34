"""The rules of K18 (include/ctcasr.h) and ctc_asr_amd/vad.py, restated slowly and obviously: plain
Python integers, one hop and one loop at a time.  Nothing here is shared with the code under test
but the numbers the header pins."""

import numpy as np

HOP = 160
LEVELS = 160
CHUNK = 40960


def level(e):
    e = int(e)
    b = e.bit_length()
    if b <= 2:
        return e
    return 4 * (b - 2) + ((e >> (b - 3)) & 3)


def level_floor(lvl):
    lvl = int(lvl)
    if lvl < 4:
        return lvl
    return (4 + (lvl & 3)) << ((lvl >> 2) - 1)


def energy(pcm):
    """int64[F]: the sum of squares of every hop, the last one as long as it is."""
    pcm = np.asarray(pcm)
    out = []
    for first in range(0, len(pcm), HOP):
        total = 0
        for x in pcm[first:first + HOP].tolist():
            total += x * x
        out.append(total)
    return np.array(out, dtype=np.int64)


def histogram(energies):
    hist = [0] * LEVELS
    for e in energies:
        hist[level(e)] += 1
    return np.array(hist, dtype=np.int64)


def gather(pcm, seg_start, seg_len, max_samples):
    """(int16[B, max_samples], int32[B]) of ctcasr_gather_segments."""
    pcm = np.asarray(pcm)
    n = len(pcm)
    out = np.zeros((len(seg_start), max_samples), dtype=np.int16)
    counts = np.zeros(len(seg_start), dtype=np.int32)
    for b, (start, length) in enumerate(zip(seg_start, seg_len)):
        start, length = int(start), int(length)
        if start < 0 or start >= n or length < 1:
            continue
        length = min(length, n - start, max_samples)
        out[b, :length] = pcm[start:start + length]
        counts[b] = length
    return out, counts


def threshold(hist, margin_db=9, floor_permille=100, min_rms=16, rms=0):
    if rms > 0:
        return HOP * rms * rms
    frames = sum(int(v) for v in hist)
    cumulative, noise = 0, None
    for lvl in range(LEVELS):
        cumulative += int(hist[lvl])
        if cumulative * 1000 >= frames * floor_permille:
            noise = lvl
            break
    levels = (margin_db * 1000 + 376) // 753
    top = min(noise + levels, 159)
    return max(level_floor(top), HOP * min_rms * min_rms, 1)


def mark(energies, thr, pad):
    raw = [int(e) >= thr for e in energies]
    speech = []
    for f in range(len(raw)):
        speech.append(any(raw[g] for g in range(max(f - pad, 0), min(f + pad, len(raw) - 1) + 1)))
    return raw, speech


def regions(raw, speech, min_raw):
    found, f = [], 0
    while f < len(speech):
        if not speech[f]:
            f += 1
            continue
        a = f
        while f < len(speech) and speech[f]:
            f += 1
        if sum(raw[a:f]) >= min_raw and f - a >= 3:
            found.append((a, f))
    return found


def split(energies, a, b, max_segment):
    pieces = []
    while b - a > max_segment:
        best = None
        for f in range(a + max_segment // 2, min(a + max_segment, b - 3) + 1):
            if best is None or int(energies[f]) < int(energies[best]):
                best = f
        pieces.append((a, best))
        a = best
    pieces.append((a, b))
    return pieces


def pieces(energies, hist, margin_db=9, floor_permille=100, min_rms=16, rms=0, pad=20, min_raw=5,
           max_segment=1500):
    """[(a, b)] in hops, the threshold, the raw marks and the kept regions."""
    thr = threshold(hist, margin_db, floor_permille, min_rms, rms)
    raw, speech = mark(energies, thr, pad)
    kept = regions(raw, speech, min_raw)
    out = []
    for a, b in kept:
        out.extend(split(energies, a, b, max_segment))
    return out, thr, raw, kept


def table(energies, hist, n, **settings):
    """(start int64[S], length int32[S]) in samples and the threshold."""
    found, thr, _, _ = pieces(energies, hist, **settings)
    start = np.array([HOP * a for a, _ in found], dtype=np.int64)
    length = np.array([min(HOP * b, n) - HOP * a for a, b in found], dtype=np.int32)
    return start, length, thr
