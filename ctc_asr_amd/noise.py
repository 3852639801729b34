"""The noise bank of `hip.noise_mix`: every recording of a ``path;label;length`` manifest, cut into
clips the kernel serves, back to back in one int16 array that is uploaded once and stays in HBM
(an hour of 16 kHz audio is 115 MB).  Which clip a row gets, where in it and at how many dB is
drawn inside the kernel, so nothing here runs per batch."""

import os

import numpy as np
import torch

from ctc_asr_amd.csv_helper import read_csv_rows
from ctc_asr_amd.params import CSV_HEADER_PATH, FLAGS

MAX_CLIP_SAMPLES = 1 << 24       # the longest clip ctcasr_noise_mix serves (its offset draw)


def load_clips(csv_path, noise_dir, max_seconds, device='cuda'):
    """(int16 ndarray of all clips back to back, int64 offsets [clips + 1]).

    Every row after the header is read (labels and lengths are ignored), in file order, with
    `input_functions.read_wav` and its checks (16 kHz, mono, int16); paths are relative to
    ``noise_dir``.  Under ``--resample_input`` a recording of any rate, channel count and format
    is converted on ``device`` (`input_functions.read_audio`) and copied back for the assembly
    here, once per run; ``max_seconds`` counts converted audio.  A recording longer than
    `MAX_CLIP_SAMPLES` becomes several clips.  Reading stops once ``max_seconds`` of audio are
    held; the recording that crosses the mark is cut at it.  A manifest that yields no sample is
    refused."""
    from ctc_asr_amd.input_functions import read_pcm_host
    if max_seconds < 1:
        raise ValueError('load_clips: max_seconds is {}, at least 1 needed.'.format(max_seconds))
    budget = int(max_seconds) * int(FLAGS.sampling_rate)
    pieces, offsets = [], [0]
    for row in read_csv_rows(csv_path)[1:]:
        if budget <= 0:
            break
        audio = read_pcm_host(os.path.join(noise_dir, row[CSV_HEADER_PATH]), device)[:budget]
        budget -= len(audio)
        for start in range(0, len(audio), MAX_CLIP_SAMPLES):
            piece = audio[start:start + MAX_CLIP_SAMPLES]
            pieces.append(piece)
            offsets.append(offsets[-1] + len(piece))
    if not pieces:
        raise ValueError('Noise manifest "{}" holds no recording.'.format(csv_path))
    return np.concatenate(pieces).astype(np.int16, copy=False), np.array(offsets, dtype=np.int64)


_BANKS = {}       # (manifest, directory, seconds, device) -> NoiseBank: epochs share the upload


class NoiseBank:
    """``bank`` int16[*] and ``clip_offsets`` int64[clips + 1] in HBM."""

    def __init__(self, bank, clip_offsets, device):
        self.bank = torch.from_numpy(bank).to(device)
        self.clip_offsets = torch.from_numpy(clip_offsets).to(device)

    @classmethod
    def get(cls, csv_path, noise_dir, max_seconds, device):
        device = torch.device(device)
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        key = (os.path.abspath(csv_path), os.path.abspath(noise_dir), int(max_seconds), str(device))
        if key not in _BANKS:
            _BANKS[key] = cls(*load_clips(csv_path, noise_dir, max_seconds, device), device)
        return _BANKS[key]

    @classmethod
    def from_flags(cls, device):
        """The bank of ``--noise_csv`` / ``--noise_dir`` / ``--noise_max_seconds``."""
        return cls.get(FLAGS.noise_csv, FLAGS.noise_dir or FLAGS.corpus_dir,
                       FLAGS.noise_max_seconds, device)
