"""The bank of room impulse responses of `hip.reverb`: every recording of a ``path;label;length``
manifest, trimmed and quantised to the int16 taps the kernel serves, back to back in one array
that is uploaded once and stays in HBM.  Which response a row gets is drawn inside the kernel, so
nothing here runs per batch.

Per recording ``h`` (int16, read with `input_functions.read_wav`'s checks), all in float64 or exact
integers:

1. ``p`` is the first index of ``max |h|``.  An all-zero recording is refused.
2. The propagation delay is cut: ``start = max(0, p - 32)`` (``p - (max_taps - 1)`` where
   ``max_taps`` is below 33, so that the peak is always kept).
3. The inaudible tail is cut: ``end = 1 +`` the last ``k`` with ``1000 |h[k]| >= |h[p]|``, capped
   at ``start + max_taps``.
4. ``delay = p - start`` and ``K = end - start``.
5. ``q = min(32767 / |h[p]|, (65535 - K / 2) / sum |h|)`` over ``h[start:end]``.
6. ``hq = rint(h q)``, half to even.  Rounding moves a tap by at most 1/2, so
   ``sum |hq| <= q sum |h| + K / 2 <= 65535``: no sum of the kernel can leave 32 bits.
7. ``scale = float32(1 / sqrt(sum hq^2))``, rounded once: a response of unit energy, so white
   input keeps its power (and the kernel's clamp takes care of peaks).
8. ``hq`` is padded with zero taps to a multiple of 8; the padded length is the ``K`` the kernel
   sees, and every response starts 16-byte aligned in the bank.

Rule 5 trades precision for the 32-bit sum: a long response gets a small peak tap (a few hundred
at T60 = 0.9 s), and the quantisation error is 33 to 45 dB below the response's energy on synthetic
responses - below the noise that is mixed in right after."""

import os

import numpy as np
import torch

from ctc_asr_amd.csv_helper import read_csv_rows
from ctc_asr_amd.params import CSV_HEADER_PATH, FLAGS

TAP_ALIGN = 8            # CTCASR_REVERB_TAP_ALIGN
MAX_TAPS = 8192          # CTCASR_REVERB_MAX_TAPS
PRE_DELAY = 32           # samples kept in front of the direct path
TAIL_RATIO = 1000        # the tail ends where |h| stays below peak / 1000
TAP_SUM = 65535          # sum |hq| of a response, at most


def quantise_rir(h, max_taps=MAX_TAPS, name='impulse response'):
    """Rules 1 to 8 on one recording: (int16 taps, padded to a multiple of 8; delay; float32
    scale)."""
    if not TAP_ALIGN <= max_taps <= MAX_TAPS:
        raise ValueError('max_taps is {}, {}..{} needed.'.format(max_taps, TAP_ALIGN, MAX_TAPS))
    mag = np.abs(np.asarray(h, dtype=np.int64))
    if mag.size == 0 or mag.max() == 0:
        raise ValueError('"{}" is silent: no impulse response.'.format(name))
    p = int(np.argmax(mag))
    peak = int(mag[p])
    start = max(0, p - min(PRE_DELAY, max_taps - 1))
    last = int(np.flatnonzero(TAIL_RATIO * mag >= peak)[-1])
    end = min(last + 1, start + max_taps)
    delay, num_taps = p - start, end - start
    cut = np.asarray(h[start:end], dtype=np.float64)
    q = min(32767.0 / peak, (TAP_SUM - num_taps / 2.0) / float(mag[start:end].sum()))
    hq = np.rint(cut * q).astype(np.int64)
    assert int(np.abs(hq).sum()) <= TAP_SUM and np.abs(hq).max() <= 32767
    energy = int((hq * hq).sum())       # (the peak tap is at least (65535 - K / 2) / K >= 7)
    scale = np.float32(1.0 / np.sqrt(np.float64(energy)))
    padded = np.zeros(-(-num_taps // TAP_ALIGN) * TAP_ALIGN, dtype=np.int16)
    padded[:num_taps] = hq
    return padded, delay, scale


def load_rirs(csv_path, rir_dir, max_taps=MAX_TAPS, device='cuda'):
    """(int16 taps of all responses back to back, int64 offsets [R + 1], int32 delay [R],
    float32 scale [R]).

    Every row after the header is read (labels and lengths are ignored), in file order, with
    `input_functions.read_wav` and its checks (16 kHz, mono, int16); paths are relative to
    ``rir_dir``.  Under ``--resample_input`` a response of any rate, channel count and format is
    converted on ``device`` (`input_functions.read_audio`) and copied back for the quantisation
    here, once per run.  A manifest without a row and a silent recording are refused."""
    from ctc_asr_amd.input_functions import read_pcm_host
    pieces, offsets, delays, scales = [], [0], [], []
    for row in read_csv_rows(csv_path)[1:]:
        path = os.path.join(rir_dir, row[CSV_HEADER_PATH])
        taps, delay, scale = quantise_rir(read_pcm_host(path, device), max_taps, path)
        pieces.append(taps)
        offsets.append(offsets[-1] + len(taps))
        delays.append(delay)
        scales.append(scale)
    if not pieces:
        raise ValueError('Impulse response manifest "{}" holds no recording.'.format(csv_path))
    return (np.concatenate(pieces), np.array(offsets, dtype=np.int64),
            np.array(delays, dtype=np.int32), np.array(scales, dtype=np.float32))


_BANKS = {}       # (manifest, directory, max_taps, device) -> RirBank: epochs share the upload


class RirBank:
    """``taps`` int16[*], ``offsets`` int64[R + 1], ``delay`` int32[R] and ``scale`` float32[R] in
    HBM: the bank arguments of `hip.reverb`."""

    def __init__(self, taps, offsets, delay, scale, device):
        self.taps = torch.from_numpy(taps).to(device)
        self.offsets = torch.from_numpy(offsets).to(device)
        self.delay = torch.from_numpy(delay).to(device)
        self.scale = torch.from_numpy(scale).to(device)

    @classmethod
    def get(cls, csv_path, rir_dir, max_taps, device):
        device = torch.device(device)
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        key = (os.path.abspath(csv_path), os.path.abspath(rir_dir), int(max_taps), str(device))
        if key not in _BANKS:
            _BANKS[key] = cls(*load_rirs(csv_path, rir_dir, max_taps, device), device)
        return _BANKS[key]

    @classmethod
    def from_flags(cls, device):
        """The bank of ``--rir_csv`` / ``--rir_dir`` / ``--rir_max_taps``."""
        return cls.get(FLAGS.rir_csv, FLAGS.rir_dir or FLAGS.corpus_dir, FLAGS.rir_max_taps,
                       device)
