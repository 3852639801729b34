"""What of the rate conversion (include/ctcasr.h, K19) can be checked without a GPU: the plan and
the output count through the C ABI, the numpy restatement (tests/resample_reference.py) against
its independent float64 form and against ideal tones, the flag, the readers that must not
change, and the argument checks of every new export."""

import ctypes
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from tests import resample_reference as ref


@pytest.fixture()
def flags():
    from ctc_asr_amd.params import FLAGS
    FLAGS.reset()
    yield FLAGS
    FLAGS.reset()


@pytest.fixture(scope='module')
def lib():
    from ctc_asr_amd import build, hip
    build.build(verbose=False)
    return hip.load()


# ---- 1. plan and count ------------------------------------------------------------------------
def test_plan_through_the_abi_equals_the_table(lib):
    from ctc_asr_amd import hip
    for rate, want in ref.PLANS_TO_16K.items():
        assert hip.resample_plan(rate) == want == ref.plan(rate), rate
        assert want[1] * want[3] <= hip.RESAMPLE_MAX_TABLE == ref.MAX_TABLE
        assert lib.ctcasr_resample_table_bytes(rate, 16000) == -(-want[1] * want[3] // 4) * 16
        assert hip.resample_chunk(rate) in (256, 512, 1024, 2048)
    # the largest table served is the one the limit is named after
    assert ref.PLANS_TO_16K[11025][1] * ref.PLANS_TO_16K[11025][3] == 16640
    # the speed kernel's rule is the case L = 100, M = P
    for percent in (50, 90, 100, 110, 200):
        m, l, radius, taps = ref.plan(160 * percent, 16000)
        speed_radius = 12 * max(percent, 100) // 95
        assert (radius, taps) == (speed_radius, 2 * speed_radius + 2)
        assert (m * 100, ref.cutoff(m, l)) == (l * percent, 95.0 / max(percent, 100))
    out = [ctypes.c_int(-7) for _ in range(4)]
    refs = [ctypes.byref(v) for v in out]
    assert lib.ctcasr_resample_plan(16001, 16000, *refs) == -2       # 416 000 weights
    assert ref.plan(16001) is None and 16000 * (2 * (1200 * 16001 // (95 * 16000)) + 2) == 416000
    assert lib.ctcasr_resample_plan(3999, 16000, *refs) == -1
    assert lib.ctcasr_resample_plan(16000, 192001, *refs) == -1
    assert [v.value for v in out] == [-7] * 4                         # nothing written on refusal
    for bad in (16001, 3999):
        with pytest.raises(hip.CtcAsrError):
            hip.resample_plan(bad)
        assert hip.resample_out_samples(1000, bad) == 0
        assert hip.resample_chunk(bad) == 0
        assert lib.ctcasr_resample_table_bytes(bad, 16000) == 0
    assert hip.resample_plan(16000) == (1, 1, 12, 26)                # equal rates: M == L
    assert hip.resample_plan(16000, 48000) == (1, 3, 12, 26)         # upwards, any target
    assert hip.resample_plan(192000, 4000) == (48, 1, 606, 1214)     # the longest filter served
    assert hip.resample_chunk(192000, 4000) == 256


def test_out_sample_counts(lib):
    from ctc_asr_amd import hip
    for rate, (m, l, _, _) in ref.PLANS_TO_16K.items():
        for n in sorted({1, max(m - 1, 1), m, m + 1, 12345, 2 ** 31 - 1}):
            want = max(1, n * l // m)
            assert hip.resample_out_samples(n, rate) == want == ref.out_samples(n, rate), (rate, n)
        for n in (0, -1, 2 ** 31):
            assert hip.resample_out_samples(n, rate) == 0 == ref.out_samples(n, rate)
    assert hip.resample_out_samples(2 ** 31 - 1, 8000) == 2 ** 32 - 2      # a 64-bit count
    assert hip.resample_out_samples(48000, 48000) == 16000
    assert hip.resample_out_samples(777, 16000) == 777


# ---- 2. the restatement against the float64 form ---------------------------------------------
@pytest.mark.parametrize('rate', [8000, 44100, 48000])
def test_restatement_against_float64(rate):
    rng = np.random.default_rng(rate)
    x = rng.integers(-32768, 32768, size=20000).astype(np.int16)
    got, _ = ref.resample_f32(x, rate)
    want = ref.to_int16(ref.resample_float64(x, rate))
    worst, share = ref.compare(got, want)
    print('rate {}: max difference {}, share differing {:.4%}'.format(rate, worst, share))
    assert len(got) == ref.out_samples(20000, rate)
    assert worst <= 1
    assert share <= 0.01


def test_restatement_formats_and_channels():
    """The four formats carry one signal: the same frame values, so the same output; channels
    are averaged."""
    rng = np.random.default_rng(5)
    x16 = (rng.integers(-128, 128, size=(3000, 2)) * 256).astype(np.int16)
    as_u8 = (x16 // 256 + 128).astype(np.uint8)
    as_s32 = x16.astype(np.int32) * 65536
    as_f32 = (x16 / 32768.0).astype(np.float32)
    want = ref.frame_values(x16)
    for other in (as_u8, as_s32, as_f32):
        assert np.array_equal(ref.frame_values(other), want)
    assert np.array_equal(want, x16.astype(np.float32).sum(axis=1))
    base, _ = ref.resample_f32(x16, 48000)
    for other in (as_u8, as_s32, as_f32):
        assert np.array_equal(ref.resample_f32(other, 48000)[0], base)
    worst, share = ref.compare(base, ref.to_int16(ref.resample_float64(x16, 48000)))
    assert worst <= 1 and share <= 0.01
    # equal rates: a copy for mono int16, the rounded mean (ties to even) for stereo
    mono = rng.integers(-32768, 32768, size=1000).astype(np.int16)
    assert np.array_equal(ref.resample_f32(mono, 16000)[0], mono)
    pair = np.array([[1, 2], [3, 4], [-1, -2], [32767, 32767], [-32768, -32768]], dtype=np.int16)
    assert list(ref.resample_f32(pair, 16000)[0]) == [2, 4, -2, 32767, -32768]


# ---- 3. tones ----------------------------------------------------------------------------------
def _tone(rate, hertz, seconds=0.5, amplitude=20000.0):
    t = np.arange(int(rate * seconds), dtype=np.float64) / rate
    return np.clip(np.rint(amplitude * np.sin(2.0 * np.pi * hertz * t)), -32768, 32767) \
        .astype(np.int16)


def _rms(v):
    return float(np.sqrt(np.mean(np.square(np.asarray(v, dtype=np.float64)))))


@pytest.mark.parametrize('rate', [8000, 22050, 44100, 48000, 96000])
def test_a_passband_tone_comes_through(rate):
    _, y = ref.resample_f32(_tone(rate, 1000.0), rate)
    t = np.arange(len(y), dtype=np.float64) / 16000.0
    ideal = 20000.0 * np.sin(2.0 * np.pi * 1000.0 * t)
    error = _rms((y - ideal)[200:-200])
    print('1 kHz from {}: rms error {:.3f} counts'.format(rate, error))
    assert len(y) == 8000
    assert error <= 2.0


@pytest.mark.parametrize('rate', [44100, 48000, 96000])
@pytest.mark.parametrize('hertz,bound', [(12000.0, 4.0), (20000.0, 1.0)])
def test_a_tone_above_the_band_is_removed(rate, hertz, bound):
    _, y = ref.resample_f32(_tone(rate, hertz), rate)
    left = _rms(y[200:-200])
    print('{:.0f} Hz from {}: rms {:.3f} counts'.format(hertz, rate, left))
    assert left <= bound


# ---- 4. the flag -------------------------------------------------------------------------------
def test_flag(flags):
    from ctc_asr_amd import params
    assert flags.resample_input is False
    plain = params.get_parameters()
    assert flags.parse(['--resample_input']) == [] and flags.resample_input is True
    assert params.get_parameters() == plain
    assert flags.parse(['--noresample_input']) == [] and flags.resample_input is False
    assert flags.parse(['--resample_input=true', '--input', 'a.wav']) == []
    assert flags.resample_input is True and flags.sampling_rate == 16000
    with pytest.raises(ValueError):
        flags.parse(['--resample_input=perhaps'])
    flags.reset()
    assert flags.resample_input is False


# ---- 5. / 6. the readers that do not change ----------------------------------------------------
def _write(path, rate, samples):
    wavfile.write(str(path), rate, samples)
    return str(path)


@pytest.mark.parametrize('on', [False, True])
def test_read_wav_and_probe_wav_are_unchanged(flags, tmp_path, on):
    """Same results and the same messages, with the flag and without: the corpus readers never
    convert."""
    from ctc_asr_amd import input_functions as inp
    flags.resample_input = on
    rng = np.random.default_rng(3)
    mono = rng.integers(-3000, 3000, size=1600).astype(np.int16)
    good = _write(tmp_path / 'good.wav', 16000, mono)
    assert np.array_equal(inp.read_wav(good), mono) and inp.read_wav(good).dtype == np.int16
    assert inp.probe_wav(good) == 1600
    fast = _write(tmp_path / 'fast.wav', 48000, mono)
    for reader in (inp.read_wav, inp.probe_wav):
        with pytest.raises(RuntimeError, match=r'^Sampling rate is 48,000, expected 16,000\.$'):
            reader(fast)
    stereo = _write(tmp_path / 'stereo.wav', 16000, np.stack([mono, mono], axis=1))
    floats = _write(tmp_path / 'floats.wav', 16000, (mono / 32768.0).astype(np.float32))
    for path in (stereo, floats):
        for reader in (inp.read_wav, inp.probe_wav):
            with pytest.raises(RuntimeError, match='Only mono 16-bit PCM WAV files are supported'):
                reader(path)
    short = _write(tmp_path / 'short.wav', 16000, mono[:400])
    for reader in (inp.read_wav, inp.probe_wav):
        with pytest.raises(RuntimeError, match='to short'):
            reader(short)
        with pytest.raises(ValueError, match='does not exist'):
            reader(str(tmp_path / 'missing.wav'))


def _manifest(tmp_path, name, rate, samples):
    _write(tmp_path / (name + '.wav'), rate, samples)
    with open(tmp_path / (name + '.csv'), 'w', encoding='utf-8') as handle:
        handle.write('path;label;length\n{}.wav;x;1.0\n'.format(name))
    return str(tmp_path / (name + '.csv'))


def test_without_the_flag_the_banks_refuse_other_rates(flags, tmp_path):
    from ctc_asr_amd import noise, reverb
    clip = np.random.default_rng(4).integers(-2000, 2000, size=4410).astype(np.int16)
    assert flags.resample_input is False
    with pytest.raises(RuntimeError, match='Sampling rate is 44,100, expected 16,000'):
        noise.load_clips(_manifest(tmp_path, 'noise', 44100, clip), str(tmp_path), 3600)
    with pytest.raises(RuntimeError, match='Sampling rate is 48,000, expected 16,000'):
        reverb.load_rirs(_manifest(tmp_path, 'rir', 48000, clip), str(tmp_path))
    # and serve what they always served
    bank, offsets = noise.load_clips(_manifest(tmp_path, 'plain', 16000, clip), str(tmp_path),
                                     3600)
    assert np.array_equal(bank, clip) and list(offsets) == [0, 4410]


def test_read_audio_refuses_by_name_before_the_device(flags, tmp_path, lib):
    from ctc_asr_amd import input_functions as inp
    rng = np.random.default_rng(6)
    x = rng.normal(size=2000) * 0.1
    with pytest.raises(RuntimeError, match='float64'):
        inp.read_audio(_write(tmp_path / 'f64.wav', 48000, x.astype(np.float64)))
    nine = (rng.normal(size=(2000, 9)) * 1000).astype(np.int16)
    with pytest.raises(RuntimeError, match='More than 8 channels'):
        inp.read_audio(_write(tmp_path / 'nine.wav', 48000, nine))
    with pytest.raises(RuntimeError, match='16,001'):
        inp.read_audio(_write(tmp_path / 'odd.wav', 16001, nine[:, 0]))
    with pytest.raises(RuntimeError, match='2,000'):
        inp.read_audio(_write(tmp_path / 'slow.wav', 2000, nine[:, 0]))
    # the 401-sample minimum applies to the converted length: 1200 frames at 48 kHz are 400
    with pytest.raises(RuntimeError, match='Sample length 400 to short'):
        inp.read_audio(_write(tmp_path / 'brief.wav', 48000, nine[:1200, 0]))
    with pytest.raises(ValueError, match='does not exist'):
        inp.read_audio(str(tmp_path / 'missing.wav'))


# ---- 7. argument errors of every new export ----------------------------------------------------
def test_the_abi_refuses_bad_arguments_before_any_launch(lib):
    """No GPU here: every call below has to return before it touches the device.  The pointers
    are made-up addresses."""
    a, t, o, s = 0x10000, 0x20000, 0x30000, 0x40000
    good = dict(src=a, fmt=0, ch=2, n=4800, rate_in=48000, rate_out=16000, table=t, out=o,
                n_out=1600, status=s)

    def call(**change):
        v = dict(good, **change)
        return lib.ctcasr_resample(v['src'], v['fmt'], v['ch'], v['n'], v['rate_in'],
                                   v['rate_out'], v['table'], v['out'], v['n_out'], v['status'],
                                   None)

    for name in ('src', 'table', 'out', 'status'):
        assert call(**{name: None}) == -1, name
    for change in (dict(fmt=-1), dict(fmt=4), dict(ch=0), dict(ch=9), dict(n=0), dict(n=-5),
                   dict(rate_in=3999), dict(rate_in=192001), dict(rate_out=3999),
                   dict(rate_out=192001), dict(n_out=1599), dict(n_out=1601), dict(n_out=0),
                   dict(src=a + 1), dict(table=t + 4), dict(out=o + 1), dict(status=s + 2),
                   dict(fmt=2, src=a + 2), dict(fmt=3, src=a + 2)):
        assert call(**change) == -1, change
    assert call(rate_in=16001, n_out=4799) == -2
    assert call(n=2 ** 31, n_out=(2 ** 31) // 3) == -2
    assert lib.ctcasr_resample_table(48000, 16000, None, None) == -1
    assert lib.ctcasr_resample_table(48000, 16000, t + 4, None) == -1
    assert lib.ctcasr_resample_table(3999, 16000, t, None) == -1
    assert lib.ctcasr_resample_table(16001, 16000, t, None) == -2
    out = [ctypes.c_int(0) for _ in range(4)]
    refs = [ctypes.byref(v) for v in out]
    for hole in range(4):
        args = list(refs)
        args[hole] = None
        assert lib.ctcasr_resample_plan(48000, 16000, *args) == -1
    assert lib.ctcasr_abi_version() == 8


def test_the_wrapper_refuses_before_the_device(lib):
    from ctc_asr_amd import hip
    with pytest.raises(hip.CtcAsrError, match='CPU tensor'):
        hip.resample(torch.zeros(100, dtype=torch.int16), 48000)
    with pytest.raises(hip.CtcAsrError, match='no GPU'):
        hip.resample_table(48000, 16000, 'cpu')
    for bad in (torch.zeros((10, 2, 2), dtype=torch.int16), torch.zeros((), dtype=torch.int16)):
        with pytest.raises(hip.CtcAsrError, match='dimensions'):
            hip.resample(bad, 48000)
    with pytest.raises(hip.CtcAsrError, match='float64'):
        hip.resample(torch.zeros(100, dtype=torch.float64), 48000)
    with pytest.raises(hip.CtcAsrError, match='9 channels'):
        hip.resample(torch.zeros((100, 9), dtype=torch.int16), 48000)
    with pytest.raises(hip.CtcAsrError, match='empty'):
        hip.resample(torch.zeros((0, 2), dtype=torch.int16), 48000)
    assert os.path.exists(hip.LIB_PATH)
