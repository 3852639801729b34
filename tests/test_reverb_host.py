"""What of the reverberation can be checked without a GPU: the loader of the impulse responses
against hand-made WAVs, the flags, the argument checks of the C ABI and of the wrapper, and the
reference itself (tests/reverb_reference.py)."""

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from tests import reverb_reference as ref

BAD_FLAGS = ['--rir_permille=-1', '--rir_permille=1001', '--rir_permille=half',
             '--rir_max_taps=7', '--rir_max_taps=8193', '--rir_max_taps=0', '--rir_max_taps=long']


@pytest.fixture()
def flags():
    from ctc_asr_amd.params import FLAGS
    FLAGS.reset()
    yield FLAGS
    FLAGS.reset()


@pytest.mark.parametrize('bad', BAD_FLAGS)
def test_bad_flag_values_are_refused_when_parsed(flags, bad):
    with pytest.raises(ValueError):
        flags.parse(['--rir_csv=rir.csv', bad])


def test_flags(flags):
    from ctc_asr_amd import params
    assert (flags.rir_csv, flags.rir_dir, flags.rir_permille, flags.rir_max_taps) == \
        ('', '', 500, 8192)
    plain = params.get_parameters()
    assert flags.parse(['--rir_csv', 'r.csv', '--rir_permille=1000', '--rir_max_taps=8',
                        '--rir_dir=/x']) == []
    shown = params.get_parameters()
    assert shown.startswith(plain) and 'rir_csv=r.csv' in shown and 'max_taps=8' in shown
    with pytest.raises(ValueError):
        flags.rir_max_taps = 9000                      # assignments are checked like the parser's
    with pytest.raises(ValueError):
        flags.update(rir_permille=2000)
    assert flags.rir_max_taps == 8 and flags.rir_permille == 1000


def test_without_rir_csv_the_augmenter_is_off(flags):
    from ctc_asr_amd import input_functions
    augment = input_functions._Augmenter(5)
    assert not augment and augment.reverb is None
    assert input_functions._Augmenter(5, training=False).reverb is None
    # a sequence of its own: neither the masks' nor the noise's, and stepped per call
    first, second = augment.next_reverb_seed(), augment.next_reverb_seed()
    twin = input_functions._Augmenter(5)
    assert first != second and first == twin.next_reverb_seed()
    assert len({first, twin.next_seed(), twin.next_noise_seed()}) == 3
    assert input_functions._Augmenter(5, rank=1).next_reverb_seed() != first
    batch = input_functions.Batch(None, None, [], None, 0.0)
    assert batch.reverb_draws is None and batch.noise_draws is None


# ------------------------------------------------------------------------------------------
def _write_rirs(tmp_path, responses, rate=16000, name='rir'):
    folder = tmp_path / name
    folder.mkdir(exist_ok=True)
    csv = tmp_path / (name + '.csv')
    with open(csv, 'w', encoding='utf-8') as handle:
        handle.write('path;label;length\n')
        for i, h in enumerate(responses):
            wavfile.write(str(folder / 'h{}.wav'.format(i)), rate, np.asarray(h, dtype=np.int16))
            handle.write('h{}.wav;a room;{:.3f}\n'.format(i, len(h) / rate))
    return str(csv), str(folder)


def _response(length, peak_at, peak=20000):
    h = np.zeros(length, dtype=np.int16)
    h[peak_at] = peak
    return h


def test_loader_cuts_the_delay_and_the_tail_and_pads(flags, tmp_path):
    from ctc_asr_amd import reverb
    a = _response(1000, 100)                 # direct path at 100; a tail that ends at 500
    a[101:501] = 30                          # 30 * 1000 >= 20000: audible
    a[501:] = 19                             # 19 * 1000 <  20000: inaudible
    a[60] = -20000                           # an equal peak earlier: the first one counts
    b = _response(450, 10, peak=-32768)      # a peak nearer than 32 samples to the start
    b[11:45] = 700
    c = _response(450, 40, peak=5)           # a tiny recording: scaled up to the full range
    c[41] = -3
    csv, folder = _write_rirs(tmp_path, [a, b, c])
    taps, offsets, delay, scale = reverb.load_rirs(csv, folder, 8192)
    assert taps.dtype == np.int16 and offsets.dtype == np.int64
    assert delay.dtype == np.int32 and scale.dtype == np.float32
    # a: p = 60, start = 28, end = 501 -> 473 taps, padded to 480; b: start 0, end 45 -> 48
    # c: p = 40, start = 8, end = 42 -> 34 taps, padded to 40
    assert list(offsets) == [0, 480, 528, 568] and list(delay) == [32, 10, 32]
    assert not (offsets % 8).any()
    ha, hb, hc = taps[:480], taps[480:528], taps[528:]
    assert not ha[473:].any() and ha[472] != 0 and not hb[45:].any() and not hc[34:].any()
    assert ha[32] == -ha[72] and ha[32] < 0 and hb[10] < 0 and list(hc[32:34]) == [32767, -19660]
    for h, (start, end), got, s in ((a, (28, 501), ha, scale[0]), (b, (0, 45), hb, scale[1]),
                                    (c, (8, 42), hc, scale[2])):
        cut = h[start:end].astype(np.float64)
        num = end - start
        q = min(32767.0 / np.abs(cut).max(), (65535.0 - num / 2.0) / np.abs(cut).sum())
        want = np.rint(cut * q)
        assert np.array_equal(got[:num], want)
        assert np.abs(got.astype(np.int64)).sum() <= 65535
        assert s == np.float32(1.0 / np.sqrt((want * want).sum()))     # float64, rounded once
    # ... and the reference restates the same rules
    for h, r in zip((a, b, c), range(3)):
        want_taps, want_delay, want_scale = ref.quantise_rir(h)
        assert np.array_equal(taps[offsets[r]:offsets[r + 1]], want_taps)
        assert (delay[r], scale[r]) == (want_delay, want_scale)


def test_loader_caps_a_response_at_max_taps(flags, tmp_path):
    from ctc_asr_amd import reverb
    h = _response(9000, 50)
    h[51:] = 100                                        # audible to the end
    equal = np.full(8192, 7, dtype=np.int16)            # 8192 equal taps: the sum rule binds
    csv, folder = _write_rirs(tmp_path, [h, equal])
    taps, offsets, delay, scale = reverb.load_rirs(csv, folder, 8192)
    assert list(offsets) == [0, 8192, 16384] and list(delay) == [32, 0]
    assert np.abs(taps[:8192].astype(np.int64)).sum() <= 65535
    # the sum rule gives q = (65535 - 4096) / 57344: taps of 7.4998..., rounded to 7 (a q that
    # let them reach 7.5 could round every one of them up)
    assert set(taps[8192:]) == {7} and np.abs(taps[8192:].astype(np.int64)).sum() <= 65535
    assert scale[1] == np.float32(1.0 / np.sqrt(8192 * 49.0))
    taps, offsets, delay, _ = reverb.load_rirs(csv, folder, 100)
    assert list(offsets) == [0, 104, 208] and list(delay) == [32, 0]    # 100 taps, padded
    assert not taps[100:104].any() and taps[99] != 0
    taps, offsets, delay, _ = reverb.load_rirs(csv, folder, 8)          # the peak is kept
    assert list(offsets) == [0, 8, 16] and list(delay) == [7, 0] and taps[7] == 32767
    for bad in (7, 0, 8193):
        with pytest.raises(ValueError, match='max_taps'):
            reverb.load_rirs(csv, folder, bad)


def test_loader_refuses_silence_an_empty_bank_and_bad_files(flags, tmp_path):
    from ctc_asr_amd import reverb
    with open(tmp_path / 'empty.csv', 'w', encoding='utf-8') as handle:
        handle.write('path;label;length\n')
    with pytest.raises(ValueError, match='no recording'):
        reverb.load_rirs(str(tmp_path / 'empty.csv'), str(tmp_path), 8192)
    csv, folder = _write_rirs(tmp_path, [_response(500, 5), np.zeros(500, dtype=np.int16)])
    with pytest.raises(ValueError, match='h1.wav'):
        reverb.load_rirs(csv, folder, 8192)
    csv, folder = _write_rirs(tmp_path, [_response(500, 5)], rate=8000, name='slow')
    with pytest.raises(RuntimeError, match='Sampling rate'):
        reverb.load_rirs(csv, folder, 8192)
    with pytest.raises(ValueError):
        ref.quantise_rir(np.zeros(10, dtype=np.int16))


def test_synthetic_responses_keep_the_sum_rule(flags, tmp_path):
    from ctc_asr_amd import reverb
    rng = np.random.default_rng(4)
    responses = [ref.synthetic_rir(rng, t60, taps) for t60, taps in
                 ((0.05, 900), (0.2, 4000), (0.9, 16000))]
    csv, folder = _write_rirs(tmp_path, responses)
    taps, offsets, delay, scale = reverb.load_rirs(csv, folder, 8192)
    assert list(delay) == [32, 32, 32] and offsets[-1] == len(taps)
    for r, h in enumerate(responses):
        got = taps[offsets[r]:offsets[r + 1]].astype(np.int64)
        assert 8 <= len(got) <= 8192 and len(got) % 8 == 0
        assert np.abs(got).sum() <= 65535 and got[32] == got.max() > 0
        want_taps, want_delay, want_scale = ref.quantise_rir(h)
        assert np.array_equal(got, want_taps) and scale[r] == want_scale
        # unit energy: white input keeps its power to within the rounding of the scale
        assert abs(float(scale[r]) ** 2 * float((got * got).sum()) - 1.0) < 1e-6
    assert offsets[3] - offsets[2] == 8192                   # the long one hits the cap


# ------------------------------------------------------------------------------------------
def test_reference_sum_is_the_float64_convolution():
    """The integer sum against a float64 `np.convolve` of the same taps: exact (every partial sum
    is an integer below 2^53), for every delay, and wrapping only where a bank breaks the rule."""
    rng = np.random.default_rng(11)
    x = rng.integers(-32768, 32768, size=700).astype(np.int16)
    x[100:140], x[300:330] = -32768, 32767
    for taps, delay in ((8, 0), (8, 7), (64, 31), (1000, 999), (1000, 0)):
        h = rng.integers(-60, 61, size=taps).astype(np.int16)
        assert np.abs(h.astype(np.int64)).sum() <= 65535
        acc = ref.accumulate(x, h, delay)
        full = np.convolve(x.astype(np.float64), h.astype(np.float64))
        assert acc.dtype == np.int64 and np.array_equal(acc.astype(np.float64),
                                                        full[delay:delay + len(x)])
        assert np.abs(acc).max() < 2 ** 31 and np.array_equal(ref.wrap32(acc), acc)
        direct = sum(int(h[k]) * int(x[5 + delay - k]) for k in range(taps)
                     if 0 <= 5 + delay - k < len(x))
        assert acc[5] == direct
    assert list(ref.wrap32(np.array([2 ** 31, -2 ** 31 - 1, 2 ** 32 + 5, -7]))) == \
        [-2 ** 31, 2 ** 31 - 1, 5, -7]
    assert list(ref.finish(np.array([3, 5, -3, 10 ** 9, -10 ** 9], dtype=np.int32), 0.5)) == \
        [2, 2, -2, 32767, -32768]                            # half to even, and the clamp


def test_reference_draws_and_copies():
    rng = np.random.default_rng(3)
    good = (rng.integers(-50, 50, size=16), 3, 0.01)
    bank = ref.Bank.of([good, (np.ones(4), 0, 1.0), (np.ones(12), 0, 1.0), good,
                        (np.ones(16), 16, 1.0), (np.ones(16), -1, 1.0)])
    assert list(bank.offsets) == [0, 16, 20, 32, 48, 64, 80]
    seen = {}
    for seed in range(200):
        for b in range(4):
            status, r = ref.draw_row(seed, b, 100, 100, bank, 1000)
            seen[r] = status
    # response 3 is sound but starts at 32: served; 1 and 2 have bad lengths; 2's successor (3)
    # starts on a multiple of 8 again; 4 and 5 have a delay outside [0, K)
    assert seen == {0: 1, 1: 2, 2: 2, 3: 1, 4: 2, 5: 2}
    assert ref.draw_row(7, 0, 0, 100, bank, 1000) == (0, 0)
    assert ref.draw_row(7, 0, 101, 100, bank, 1000) == (0, 0)
    assert ref.draw_row(7, 0, 50, 100, bank, 0) == (0, 0)
    shifted = ref.Bank(np.ones(20), [4, 12, 20], [0, 0], [1.0, 1.0])      # offsets off the grid
    assert {ref.draw_row(s, 0, 9, 9, shifted, 1000)[0] for s in range(50)} == {2}
    pcm = rng.integers(-3000, 3000, size=(4, 50)).astype(np.int16)
    nums = np.array([50, 20, 0, 51], dtype=np.int32)
    seed = ref.find_seed(lambda s: [ref.draw_row(s, b, 50, 50, bank, 1000)[1] for b in (0, 1)]
                         == [0, 1])
    out, draws = ref.reverb_rows(pcm, nums, bank, seed)
    assert draws.tolist()[:2] == [[1, 0], [2, 1]] and draws.tolist()[2:] == [[0, 0], [0, 0]]
    assert not np.array_equal(out[0], pcm[0]) and np.array_equal(out[1:], pcm[1:])


# ------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from ctc_asr_amd import build, hip
    build.build(verbose=False)
    return hip.load()


def test_the_abi_refuses_bad_arguments_before_any_launch(lib):
    """No GPU here: every call below has to return before it touches the device.  The pointers
    are made-up addresses."""
    good = dict(pcm=0x1000, num=0x2000, B=2, max_samples=64, taps=0x3000, off=0x4000,
                delay=0x5000, scale=0x6000, num_rirs=2, seed=1, permille=500, out=0x7000,
                draws=None, stream=None)

    def call(**change):
        return lib.ctcasr_reverb(*{**good, **change}.values())

    for name in ('pcm', 'num', 'taps', 'off', 'delay', 'scale', 'out'):
        assert call(**{name: None}) == -1, name
    for change in (dict(out=0x1000), dict(B=0), dict(B=-1), dict(max_samples=0),
                   dict(num_rirs=0), dict(permille=-1), dict(permille=1001)):
        assert call(**change) == -1, change
    assert call(max_samples=(1 << 30) + 1) == -2 and call(num_rirs=(1 << 24) + 1) == -2
    assert call(B=1 << 22, max_samples=1 << 30) == -2            # more workgroups than a grid holds


def test_the_wrapper_refuses_cpu_tensors_and_wrong_shapes(lib):
    from ctc_asr_amd import hip
    pcm = torch.zeros((2, 64), dtype=torch.int16)
    num = torch.full((2,), 64, dtype=torch.int32)
    taps, off = torch.ones(16, dtype=torch.int16), torch.tensor([0, 8, 16])
    delay, scale = torch.zeros(2, dtype=torch.int32), torch.ones(2)
    with pytest.raises(hip.CtcAsrError, match='HBM'):
        hip.reverb(pcm, num, taps, off, delay, scale, 1)
    with pytest.raises(hip.CtcAsrError, match='3 entries for a batch of 2'):
        hip.reverb(pcm, torch.zeros(3, dtype=torch.int32), taps, off, delay, scale, 1)
    with pytest.raises(hip.CtcAsrError, match='draws holds 6 elements, 4 expected'):
        hip.reverb(pcm, num, taps, off, delay, scale, 1,
                   draws=torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(hip.CtcAsrError, match='rir_delay holds 3 elements, 2 expected'):
        hip.reverb(pcm, num, taps, off, torch.zeros(3, dtype=torch.int32), scale, 1)
    with pytest.raises(hip.CtcAsrError, match='rir_scale holds 1 elements, 2 expected'):
        hip.reverb(pcm, num, taps, off, delay, scale[:1], 1)
    with pytest.raises(hip.CtcAsrError, match='at least 2'):
        hip.reverb(pcm, num, taps, off[:1], delay, scale, 1)
    with pytest.raises(hip.CtcAsrError, match='dimensions'):
        hip.reverb(pcm[0], num[:1], taps, off, delay, scale, 1)
    assert (hip.REVERB_CHUNK, hip.REVERB_TAP_ALIGN, hip.REVERB_MAX_TAPS) == (2048, 8, 8192)
    assert hip.REVERB_TAP_BLOCK % 8 == 0 and 16 <= hip.REVERB_TAP_BLOCK <= 4096
    header = open(hip._PKG_DIR + '/../include/ctcasr.h').read()
    for name in ('CHUNK', 'TAP_BLOCK', 'TAP_ALIGN', 'MAX_TAPS'):
        assert '#define CTCASR_REVERB_{} {}\n'.format(name, getattr(hip, 'REVERB_' + name)) \
            in header
