"""What of the noise mixing can be checked without a GPU: the flags, the loader of the noise bank,
the argument checks of the C ABI and of the wrapper, and the reference itself
(tests/noise_reference.py)."""

import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from tests import noise_reference as ref

BAD_FLAGS = [
    '--noise_snr_db=30,10', '--noise_snr_db=-21,10', '--noise_snr_db=10,61', '--noise_snr_db=61',
    '--noise_snr_db=loud', '--noise_snr_db=10,20,30', '--noise_snr_db=', '--noise_snr_db=10.5',
    '--noise_permille=-1', '--noise_permille=1001', '--noise_permille=half',
    '--noise_max_seconds=0', '--noise_max_seconds=-3',
    '--eval_noise_snr_db=61', '--eval_noise_snr_db=-21', '--eval_noise_snr_db=10,20',
    '--eval_noise_snr_db=quiet',
]


@pytest.fixture()
def flags():
    from ctc_asr_amd.params import FLAGS
    FLAGS.reset()
    yield FLAGS
    FLAGS.reset()


@pytest.mark.parametrize('bad', BAD_FLAGS)
def test_bad_flag_values_are_refused_when_parsed(flags, bad):
    with pytest.raises(ValueError):
        flags.parse(['--noise_csv=noise.csv', bad])


def test_flags(flags):
    from ctc_asr_amd import params
    assert (flags.noise_csv, flags.noise_dir, flags.noise_snr_db, flags.noise_permille,
            flags.noise_max_seconds, flags.eval_noise_snr_db) == ('', '', '10,30', 500, 3600, '')
    plain = params.get_parameters()
    # the evaluation SNR needs a bank to draw from - whatever the order on the command line
    for argv in (['--eval_noise_snr_db=10'], ['--eval_noise_snr_db', '10', '--noise_csv=']):
        flags.reset()
        with pytest.raises(ValueError, match='noise_csv'):
            flags.parse(argv)
    flags.reset()
    assert flags.parse(['--eval_noise_snr_db=10', '--noise_csv', 'n.csv', '--noise_snr_db=15',
                        '--noise_permille=1000', '--noise_max_seconds=1', '--noise_dir=/x']) == []
    assert params.parse_noise_snr_db(flags.noise_snr_db) == (15, 15)
    assert params.parse_eval_noise_snr_db(flags.eval_noise_snr_db) == 10
    shown = params.get_parameters()
    assert shown.startswith(plain) and 'noise_csv=n.csv' in shown and 'eval_snr_db=10' in shown
    assert params.parse_noise_snr_db('-20 60') == (-20, 60)
    assert params.parse_noise_snr_db('10,30') == (10, 30)
    assert params.parse_eval_noise_snr_db('') is None
    with pytest.raises(ValueError):
        flags.noise_snr_db = '40,30'                   # assignments are checked like the parser's
    with pytest.raises(ValueError):
        flags.update(noise_permille=2000)
    assert flags.noise_snr_db == '15' and flags.noise_permille == 1000


# ------------------------------------------------------------------------------------------
def _write_noise(tmp_path, lengths, seed=1, rate=16000):
    rng = np.random.default_rng(seed)
    folder = tmp_path / 'noise'
    folder.mkdir(exist_ok=True)
    clips = []
    with open(tmp_path / 'noise.csv', 'w', encoding='utf-8') as handle:
        handle.write('path;label;length\n')
        for i, n in enumerate(lengths):
            clip = rng.integers(-2000, 2000, size=n).astype(np.int16)
            wavfile.write(str(folder / 'n{}.wav'.format(i)), rate, clip)
            handle.write('n{}.wav;whatever it says;{:.3f}\n'.format(i, n / rate))
            clips.append(clip)
    return str(tmp_path / 'noise.csv'), str(folder), clips


def test_load_clips(flags, tmp_path):
    from ctc_asr_amd import noise
    csv, folder, clips = _write_noise(tmp_path, [401, 16000, 5000])
    bank, offsets = noise.load_clips(csv, folder, 3600)
    assert bank.dtype == np.int16 and offsets.dtype == np.int64
    assert list(offsets) == [0, 401, 16401, 21401]            # every row, the last one included
    assert np.array_equal(bank, np.concatenate(clips))
    # the cap: reading stops at the mark, in the middle of a recording where it falls there
    bank, offsets = noise.load_clips(csv, folder, 1)
    assert list(offsets) == [0, 401, 16000] and np.array_equal(bank, np.concatenate(clips)[:16000])
    csv2, folder2, clips2 = _write_noise(tmp_path, [16000, 16000, 16000], seed=2)
    bank, offsets = noise.load_clips(csv2, folder2, 2)
    assert list(offsets) == [0, 16000, 32000]                  # the third file is not opened
    with pytest.raises(ValueError):
        noise.load_clips(csv2, folder2, 0)


def test_load_clips_cuts_a_long_recording(flags, tmp_path):
    from ctc_asr_amd import noise
    long = noise.MAX_CLIP_SAMPLES + 1000
    assert noise.MAX_CLIP_SAMPLES == 1 << 24 == ref.MAX_CLIP
    csv, folder, clips = _write_noise(tmp_path, [500, long, 600])
    bank, offsets = noise.load_clips(csv, folder, 3600)
    assert list(offsets) == [0, 500, 500 + (1 << 24), 500 + long, 500 + long + 600]
    assert np.diff(offsets).max() == 1 << 24
    assert np.array_equal(bank[500:500 + long], clips[1]) and np.array_equal(bank[-600:], clips[2])


def test_load_clips_refuses_an_empty_bank_and_bad_files(flags, tmp_path):
    from ctc_asr_amd import noise
    with open(tmp_path / 'empty.csv', 'w', encoding='utf-8') as handle:
        handle.write('path;label;length\n')
    with pytest.raises(ValueError, match='no recording'):
        noise.load_clips(str(tmp_path / 'empty.csv'), str(tmp_path), 3600)
    csv, folder, _ = _write_noise(tmp_path, [8000], rate=8000)       # read_wav's checks
    with pytest.raises(RuntimeError, match='Sampling rate'):
        noise.load_clips(csv, folder, 3600)
    with open(csv, 'a', encoding='utf-8') as handle:
        handle.write('missing.wav;x;1.0\n')
    flags.sampling_rate = 8000
    with pytest.raises(ValueError, match='does not exist'):
        noise.load_clips(csv, folder, 3600)


# ------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from ctc_asr_amd import build, hip
    build.build(verbose=False)
    return hip.load()


def test_the_abi_refuses_bad_arguments_before_any_launch(lib):
    """No GPU here: every call below has to return before it touches the device.  The pointers
    are made-up addresses."""
    good = dict(pcm=0x1000, num=0x2000, B=2, max_samples=64, bank=0x3000, off=0x4000, num_clips=2,
                seed=1, lo=10, hi=30, permille=500, out=0x5000, draws=None, powers=None,
                gain=None, ws=0x6000, ws_bytes=256, stream=None)

    def call(**change):
        return lib.ctcasr_noise_mix(*{**good, **change}.values())

    for name in ('pcm', 'num', 'bank', 'off', 'out'):
        assert call(**{name: None}) == -1, name
    for change in (dict(B=0), dict(B=-1), dict(max_samples=0), dict(num_clips=0),
                   dict(lo=31, hi=30), dict(lo=-21), dict(hi=61), dict(lo=61, hi=61),
                   dict(lo=-21, hi=-21), dict(permille=-1), dict(permille=1001)):
        assert call(**change) == -1, change
    assert call(max_samples=(1 << 30) + 1) == -2 and call(num_clips=(1 << 24) + 1) == -2
    assert call(ws=None) == -3 and call(ws_bytes=31) == -3 and call(ws=0x6004) == -3
    assert lib.ctcasr_noise_mix_workspace_bytes(2) == 32
    assert lib.ctcasr_noise_mix_workspace_bytes(0) == lib.ctcasr_noise_mix_workspace_bytes(-4) == 0


def test_the_wrapper_refuses_cpu_tensors_and_wrong_shapes(lib):
    from ctc_asr_amd import hip
    pcm = torch.zeros((2, 64), dtype=torch.int16)
    num = torch.full((2,), 64, dtype=torch.int32)
    bank, off = torch.ones(100, dtype=torch.int16), torch.tensor([0, 40, 100])
    with pytest.raises(hip.CtcAsrError, match='HBM'):
        hip.noise_mix(pcm, num, bank, off, 1, 10, 30)
    with pytest.raises(hip.CtcAsrError, match='3 entries for a batch of 2'):
        hip.noise_mix(pcm, torch.zeros(3, dtype=torch.int32), bank, off, 1, 10, 30)
    with pytest.raises(hip.CtcAsrError, match='draws holds 6 elements, 8 expected'):
        hip.noise_mix(pcm, num, bank, off, 1, 10, 30, draws=torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(hip.CtcAsrError, match='at least 2'):
        hip.noise_mix(pcm, num, bank, off[:1], 1, 10, 30)
    with pytest.raises(hip.CtcAsrError, match='2 dimensions|dimensions'):
        hip.noise_mix(pcm[0], num[:1], bank, off, 1, 10, 30)
    assert hip.NOISE_MIX_SNR_DB == (-20, 60) and hip.NOISE_MIX_CHUNK == 8192


# ------------------------------------------------------------------------------------------
def test_reference_offsets_stay_inside_their_clip():
    lengths = [1, 2, 5, 401, 4096, 50000, 1 << 24]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    seen = set()
    for seed in range(300):
        for b in range(8):
            status, k, o, snr = ref.draw_row(seed, b, 100, 100, offsets, -20, 60, 1000)
            assert status == 1 and 0 <= k < len(lengths) and 0 <= o < lengths[k]
            assert -20 <= snr <= 60
            seen.add(k)
    assert seen == set(range(len(lengths)))
    # the last offset of a clip is reached (below() never returns n, and does return n - 1)
    assert ref.find_seed(lambda s: ref.draw_row(s, 0, 9, 9, offsets[:4], 0, 0, 1000)[1:3] == (2, 4))
    assert ref.draw_row(7, 0, 0, 100, offsets, 0, 0, 1000) == (0, 0, 0, 0)
    assert ref.draw_row(7, 0, 101, 100, offsets, 0, 0, 1000) == (0, 0, 0, 0)
    assert ref.draw_row(7, 0, 50, 100, offsets, 0, 0, 0) == (0, 0, 0, 0)
    empty = np.array([0, 0], dtype=np.int64)
    assert ref.draw_row(7, 0, 50, 100, empty, 3, 3, 1000) == (2, 0, 0, 3)


def test_reference_mix_has_the_drawn_snr():
    """In float64 the mix has the drawn SNR to 1e-9 dB; rounded to integers, at the synthetic
    corpus's scale of 3000, it is still within 1e-3 dB (the rounding error has power 1/12 beside
    a noise power of about 3000^2 / 1000 at 30 dB, and is not correlated with the noise)."""
    rng = np.random.default_rng(2)
    lengths = [5, 401, 50000]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    bank = np.clip(rng.normal(size=int(offsets[-1])) * 3000, -32768, 32767).astype(np.int16)
    nums = np.array([14400, 16000, 20000, 9000, 0, 16001], dtype=np.int32)
    pcm = np.zeros((6, 20000), dtype=np.int16)
    for b, n in enumerate(nums):
        pcm[b, :n] = np.clip(rng.normal(size=n) * 3000, -32768, 32767)
    pcm[3, :9000] = 0
    got = ref.mix(pcm, nums, bank, offsets, 99, 10, 30)
    assert list(got['draws'][:, 0]) == [1, 1, 1, 2, 0, 1]
    assert len(set(got['draws'][:, 3])) > 2
    for b in (0, 1, 2, 5):
        n, snr = int(nums[b]), int(got['draws'][b, 3])
        assert 10 <= snr <= 30
        assert abs(ref.snr_db(pcm[b, :n], got['y64'][b]) - snr) < 1e-9
        assert abs(ref.snr_db(pcm[b, :n], ref.rounded(got['y64'][b])) - snr) < 1e-3
    assert got['y64'][3] is None and got['y64'][4] is None
    out = ref.expected_pcm(pcm, nums, got)
    assert np.array_equal(out[3], pcm[3]) and np.array_equal(out[4], pcm[4])
    assert np.array_equal(out[0, 14400:], pcm[0, 14400:]) and not np.array_equal(out[0], pcm[0])
