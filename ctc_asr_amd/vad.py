"""Speech segmentation of a long recording: where to cut it into pieces the model can take.

The device makes the one pass over the PCM (``ctcasr_vad_energy``: the energy of every 10 ms hop
as an exact integer, and the histogram of the hops' quarter-octave levels); everything here works
on that one value per hop, on the host, in exact integers - the host has to wait for the table in
any case to size the batches.  The rules, in order (pinned; tests/vad_reference.py restates them
hop by hop):

threshold   ``Ln``: the smallest level whose cumulative count ``c`` has
            ``c * 1000 >= F * floor_permille``; ``Lt = min(Ln + (margin_db * 1000 + 376) // 753,
            159)`` (a level is 0.753 dB); ``thr = max(level_floor(Lt), 160 * min_rms^2, 1)``.
            With ``rms > 0`` the threshold is ``160 * rms^2`` and the histogram is not consulted.
marking     ``raw[f] = energy[f] >= thr``; ``speech[f]``: any raw hop within ``pad`` hops (pads
            both edges of a run and closes gaps of up to ``2 pad`` hops).
regions     the maximal runs of ``speech``; dropped when they hold fewer than ``min_raw`` raw
            hops (clicks) or are shorter than 3 hops.
splitting   a region ``[a, b)`` longer than ``M = max_segment`` hops is cut, while ``b - a > M``,
            at the hop of smallest energy in ``[a + M // 2, min(a + M, b - 3)]`` (both ends
            included, the lowest hop on a tie): every piece has 3..M hops.
table       ``(start, length)`` in samples, ascending: ``start = 160 a``,
            ``length = min(160 b, n) - 160 a``.
"""

import numpy as np
import torch

from ctc_asr_amd import hip

HOP = hip.VAD_HOP
LEVELS = hip.VAD_LEVELS
MIN_PIECE = 3                   # hops: no piece is shorter
DB_PER_LEVEL_MILLI = 753        # 10 log10(2) / 4 dB, in thousandths


def level(energy):
    """The quarter-octave level of ``ctcasr_vad_energy`` (include/ctcasr.h) of non-negative
    integers below 2^53, as an int64 array."""
    energy = np.asarray(energy, dtype=np.int64)
    bits = np.frexp(energy.astype(np.float64))[1].astype(np.int64)      # the bit length, exact
    return np.where(bits <= 2, energy, 4 * (bits - 2) + ((energy >> np.maximum(bits - 3, 0)) & 3))


def level_floor(lvl):
    """The smallest energy of a level: ``level(level_floor(L)) == L``."""
    lvl = np.asarray(lvl, dtype=np.int64)
    return np.where(lvl < 4, lvl, (4 + (lvl & 3)) << np.maximum((lvl >> 2) - 1, 0))


class VadSettings:
    """The knobs of the segmentation, in the units the rules use (hops of 10 ms)."""

    def __init__(self, margin_db=9, floor_permille=100, min_rms=16, rms=0, pad=20, min_raw=5,
                 max_segment=1500):
        if max_segment < 2 * MIN_PIECE:         # (a cut at a + M // 2 must leave 3 hops before it)
            raise ValueError('vad: max_segment is {} hops, at least {} needed.'
                             .format(max_segment, 2 * MIN_PIECE))
        if pad < 0 or min_raw < 0:
            raise ValueError('vad: pad and min_raw count hops and cannot be negative.')
        self.margin_db, self.floor_permille = int(margin_db), int(floor_permille)
        self.min_rms, self.rms = int(min_rms), int(rms)
        self.pad, self.min_raw, self.max_segment = int(pad), int(min_raw), int(max_segment)

    @classmethod
    def from_flags(cls, flags):
        return cls(flags.vad_margin_db, flags.vad_floor_permille, flags.vad_min_rms,
                   flags.vad_rms, flags.vad_pad_ms // 10, flags.vad_min_speech_ms // 10,
                   flags.max_segment_seconds * 100)


def threshold(hist, settings):
    """The energy a hop must reach to count as raw speech."""
    if settings.rms > 0:
        return HOP * settings.rms * settings.rms
    cumulative = np.cumsum(np.asarray(hist, dtype=np.int64))
    frames = int(cumulative[-1])
    noise = int(np.argmax(cumulative * 1000 >= frames * settings.floor_permille))
    steps = (settings.margin_db * 1000 + DB_PER_LEVEL_MILLI // 2) // DB_PER_LEVEL_MILLI
    top = min(noise + steps, LEVELS - 1)
    return max(int(level_floor(top)), HOP * settings.min_rms * settings.min_rms, 1)


def dilate(raw, pad):
    """``speech[f]``: any ``raw[g]`` with ``|g - f| <= pad``, by one prefix sum."""
    raw = np.asarray(raw, dtype=bool)
    total = np.concatenate([[0], np.cumsum(raw, dtype=np.int64)])
    index = np.arange(raw.size)
    return total[np.minimum(index + pad + 1, raw.size)] - total[np.maximum(index - pad, 0)] > 0


def regions(energy, thr, settings):
    """[(a, b)] in hops: the runs of padded speech that pass the two size rules."""
    energy = np.asarray(energy, dtype=np.int64)
    raw = energy >= thr
    speech = dilate(raw, settings.pad)
    edges = np.diff(np.concatenate([[0], speech.astype(np.int8), [0]]))
    starts, stops = np.nonzero(edges == 1)[0], np.nonzero(edges == -1)[0]
    raw_total = np.concatenate([[0], np.cumsum(raw, dtype=np.int64)])
    keep = (raw_total[stops] - raw_total[starts] >= settings.min_raw) & \
        (stops - starts >= MIN_PIECE)
    return [(int(a), int(b)) for a, b in zip(starts[keep], stops[keep])]


def split(energy, a, b, max_segment):
    """The pieces of region ``[a, b)``, none longer than ``max_segment`` hops."""
    pieces = []
    while b - a > max_segment:
        low, high = a + max_segment // 2, min(a + max_segment, b - MIN_PIECE)
        cut = low + int(np.argmin(energy[low:high + 1]))      # (argmin: the first of equal minima)
        pieces.append((a, cut))
        a = cut
    pieces.append((a, b))
    return pieces


def segment_table(energy, hist, num_samples, settings):
    """(start int64[S], length int32[S]) in samples, ascending, and the threshold used."""
    energy = np.asarray(energy, dtype=np.int64)
    thr = threshold(hist, settings)
    pieces = [piece for a, b in regions(energy, thr, settings)
              for piece in split(energy, a, b, settings.max_segment)]
    start = np.array([HOP * a for a, _ in pieces], dtype=np.int64)
    stop = np.array([min(HOP * b, num_samples) for _, b in pieces], dtype=np.int64)
    return start, (stop - start).astype(np.int32), thr


def segment(pcm, settings):
    """``pcm``: a recording as an int16 device tensor -> (start, length, thr) as `segment_table`
    gives them.  One launch pair on the device, one copy back."""
    energy, hist = hip.vad_energy(pcm)
    host = torch.cat([energy, hist.to(torch.int64)]).cpu().numpy()
    return segment_table(host[:energy.numel()], host[energy.numel():], pcm.numel(), settings)
