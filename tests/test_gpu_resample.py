"""`ctcasr_resample` on the MI355X against its numpy restatement (tests/resample_reference.py).

The kernel and the restatement do the same fp32 operations in the same order on weights that are
rounded once from float64; the one thing that may differ is the last place of the device's and
the host's float64 sine and cosine, which moves a weight by one fp32 place at most and an output
across a rounding tie.  So: no sample may differ by more than one count, and over each case at
most 1 % of the samples may differ at all (the restatement itself stays near 0.1 % against an
all-float64 filter, tests/test_resample_host.py) - a bias could hide behind "at most one count",
not behind both.  A case of fewer than 100 outputs therefore has to be exact: the shortest
recordings, where every output reaches past both ends.

Every call here goes through the C ABI with a sentinel behind ``out[n_out]`` that must
survive."""

import numpy as np
import pytest
import torch

from tests import resample_reference as ref

pytestmark = pytest.mark.gpu

SENTINEL = 0x3A5C
PAD = 64


def _tensor(samples, offset=0):
    """``samples`` on the device, its base pointer ``offset`` elements behind an aligned one."""
    x = torch.from_numpy(np.ascontiguousarray(samples))
    flat = torch.empty(x.numel() + 16, dtype=x.dtype, device='cuda')
    assert flat.data_ptr() % 16 == 0
    view = flat[offset:offset + x.numel()].view(x.shape)
    view.copy_(x)
    return view


def _run(hip, samples, rate_in, rate_out=16000, offset=0, out_offset=0):
    """int16 ndarray [n_out] and the status word, through the C ABI."""
    x = _tensor(samples, offset)
    n = x.shape[0]
    channels = x.shape[1] if x.dim() == 2 else 1
    n_out = hip.resample_out_samples(n, rate_in, rate_out)
    assert n_out == ref.out_samples(n, rate_in, rate_out) >= 1
    table = hip.resample_table(rate_in, rate_out, x.device)
    buf = torch.full((out_offset + n_out + PAD,), SENTINEL, dtype=torch.int16, device='cuda')
    status = torch.full((1,), -1, dtype=torch.int32, device='cuda')
    code = hip.load().ctcasr_resample(
        x.data_ptr(), hip.RESAMPLE_FORMATS[x.dtype], channels, n, rate_in, rate_out,
        table.data_ptr(), buf.data_ptr() + 2 * out_offset, n_out, status.data_ptr(),
        torch.cuda.current_stream().cuda_stream)
    assert code == 0
    got = buf.cpu().numpy()
    assert (got[:out_offset] == SENTINEL).all() and (got[out_offset + n_out:] == SENTINEL).all()
    return got[out_offset:out_offset + n_out], int(status.item())


def _agree(got, want, what):
    worst, share = ref.compare(got, want)
    differing = int(round(share * len(want)))
    print('{}: {} outputs, max difference {}, {} differ ({:.4%})'.format(
        what, len(want), worst, differing, share))
    assert got.shape == want.shape, what
    assert worst <= 1, what
    assert share <= 0.01, what


def _check(hip, samples, rate, what, **kwargs):
    got, status = _run(hip, samples, rate, **kwargs)
    want, _ = ref.resample_f32(samples, rate)
    assert status == 0, what
    _agree(got, want, what)
    return got, want


def _frames_for(hip, rate, chunks=3.3):
    """Input frames that come to a little over ``chunks`` workgroups of outputs."""
    m, l, _, _ = ref.plan(rate)
    return min(50000, int(chunks * hip.resample_chunk(rate)) * m // l + 5)


def _noise(rng, shape, dtype):
    if dtype == np.int16:
        return rng.integers(-32768, 32768, size=shape).astype(np.int16)
    if dtype == np.uint8:
        return rng.integers(0, 256, size=shape).astype(np.uint8)
    if dtype == np.int32:        # 24 bits left-justified, as a 24-bit file is read
        return (rng.integers(-2 ** 23, 2 ** 23, size=shape) * 256).astype(np.int32)
    return rng.uniform(-1.0, 1.0, size=shape).astype(np.float32)


def _frames_to_reach(target, rate):
    """The fewest input frames that come to ``target`` outputs; None where no length does (going
    up, 8000 -> 16 000, only even counts occur)."""
    m, l, _, _ = ref.plan(rate)
    n = -(-target * m // l)
    return n if ref.out_samples(n, rate) == target else None


# ---- the table ----------------------------------------------------------------------------------
@pytest.mark.parametrize('rate', sorted(ref.PLANS_TO_16K))
def test_table(hip, rate):
    """Weights evaluated in float64 and rounded once: the host's, but for the last place of
    sin / cos in float64, which can move an fp32 weight by one place."""
    m, l, radius, taps = ref.plan(rate)
    got = hip.resample_table(rate, 16000, 'cuda').cpu().numpy()
    want = ref.table(rate)
    assert got.size == -(-l * taps // 4) * 4 and not got[l * taps:].any()      # the pad is zero
    got = got[:l * taps].reshape(l, taps)
    apart = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    apart[(got == 0) & (want == 0)] = 0                                        # (+0 and -0)
    print('rate {}: {} of {} weights differ'.format(rate, int((apart != 0).sum()), got.size))
    assert apart.max() <= 1
    assert (apart != 0).mean() <= 0.01
    assert hip.resample_table(rate, 16000, 'cuda') is hip.resample_table(rate, 16000, 'cuda:0')


# ---- cases ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('rate', sorted(ref.PLANS_TO_16K))
def test_every_listed_rate_mono(hip, rate):
    rng = np.random.default_rng(rate)
    _check(hip, _noise(rng, _frames_for(hip, rate), np.int16), rate, 'mono {}'.format(rate))


@pytest.mark.parametrize('rate', [44100, 48000])
@pytest.mark.parametrize('channels', [2, 3, 8])
def test_channels(hip, rate, channels):
    rng = np.random.default_rng(rate + channels)
    x = _noise(rng, (_frames_for(hip, rate, 2.2), channels), np.int16)
    _check(hip, x, rate, '{} channels at {}'.format(channels, rate))


@pytest.mark.parametrize('dtype', [np.int16, np.uint8, np.int32, np.float32])
def test_formats_at_48k_stereo(hip, dtype):
    rng = np.random.default_rng(7)
    x = _noise(rng, (_frames_for(hip, 48000, 2.2), 2), dtype)
    _check(hip, x, 48000, '{} stereo at 48000'.format(np.dtype(dtype).name))


def test_upwards_and_to_another_target(hip):
    rng = np.random.default_rng(8)
    x = _noise(rng, 3000, np.int16)
    got, _ = _run(hip, x, 16000, 48000)
    want, _ = ref.resample_f32(x, 16000, 48000)
    _agree(got, want, '16000 -> 48000')
    x = _noise(rng, (30000, 2), np.float32)
    got, _ = _run(hip, x, 192000, 4000)            # the longest filter served: 1214 taps
    want, _ = ref.resample_f32(x, 192000, 4000)
    _agree(got, want, '192000 -> 4000')


# ---- edges ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('rate', [8000, 11025, 44100, 48000, 192000])
def test_shortest_recordings(hip, rate):
    rng = np.random.default_rng(rate + 1)
    taps = ref.plan(rate)[3]
    for n in (1, 2, taps - 1, taps, taps + 1):
        for channels in (1, 3):
            shape = n if channels == 1 else (n, channels)
            _check(hip, _noise(rng, shape, np.int16), rate,
                   '{} frames x {} at {}'.format(n, channels, rate))


@pytest.mark.parametrize('rate', [8000, 44100, 48000, 88200])
def test_around_the_seam_of_two_workgroups(hip, rate):
    """Just short of, at and past one workgroup's run of outputs, and the same around the second
    seam; the samples on both sides of each seam are compared by themselves as well."""
    rng = np.random.default_rng(rate + 2)
    chunk = hip.resample_chunk(rate)
    assert chunk in (256, 512, 1024, 2048)
    reached = 0
    for target in (chunk - 1, chunk, chunk + 1, chunk + 2, 2 * chunk - 1, 2 * chunk,
                   2 * chunk + 1):
        frames = _frames_to_reach(target, rate)
        if frames is None:
            continue
        reached += 1
        x = _noise(rng, (frames, 2), np.int16)
        got, want = _check(hip, x, rate, '{} outputs at {}'.format(target, rate))
        assert len(got) == target
        for seam in range(chunk, target, chunk):
            near = slice(max(seam - 8, 0), seam + 8)
            assert np.abs(got[near].astype(np.int32) - want[near]).max() <= 1
            assert (got[near] != want[near]).sum() <= 1
    assert reached >= 3


@pytest.mark.parametrize('rate', [11025, 44100, 48000])
def test_zero_extension_at_both_ends(hip, rate):
    """The first and last R + 1 outputs reach past the recording: a loud constant makes every
    missing tap count."""
    radius = ref.plan(rate)[2]
    x = np.full((_frames_for(hip, rate, 1.5), 2), 30000, dtype=np.int16)
    got, want = _check(hip, x, rate, 'constant at {}'.format(rate))
    for part in (slice(0, radius + 1), slice(-(radius + 1), None)):
        assert np.abs(got[part].astype(np.int32) - want[part]).max() <= 1
        assert (got[part] != want[part]).sum() <= 1
    # (away from the ends the constant comes through: the filter's gain at 0 Hz is 1 to 1e-3)
    assert abs(int(got[len(got) // 2]) - 30000) <= 30 and got[0] != got[len(got) // 2]


@pytest.mark.parametrize('rate', [44100, 48000])
def test_full_scale_square_wave_saturates(hip, rate):
    n = _frames_for(hip, rate, 1.5)
    x = np.where((np.arange(n) // 40) % 2 == 0, 32767, -32768).astype(np.int16)
    got, want = _check(hip, np.stack([x, x], axis=1), rate, 'square at {}'.format(rate))
    assert (want == 32767).sum() > 10 and (want == -32768).sum() > 10      # the overshoot clips
    assert ((got == 32767) == (want == 32767)).mean() > 0.99


@pytest.mark.parametrize('rate,channels,dtype', [(48000, 2, np.int16), (44100, 3, np.int16),
                                                 (48000, 3, np.uint8), (44100, 2, np.float32),
                                                 (48000, 1, np.int32), (16000, 2, np.int16)])
def test_any_base_pointer(hip, rate, channels, dtype):
    """A base 1, 3 and 7 elements behind a 16-byte boundary - a slice - gives the bits of the
    aligned call (6-byte frames among them), and so does an output that starts off a boundary."""
    rng = np.random.default_rng(rate + channels)
    x = _noise(rng, (_frames_for(hip, rate, 1.2), channels), dtype)
    base, _ = _check(hip, x, rate, 'aligned')
    for offset in (1, 3, 7):
        got, status = _run(hip, x, rate, offset=offset, out_offset=offset)
        assert status == 0 and np.array_equal(got, base), offset


def test_two_calls_agree(hip):
    rng = np.random.default_rng(11)
    x = _noise(rng, (20000, 2), np.float32)
    first, _ = _run(hip, x, 44100)
    again, _ = _run(hip, x, 44100)
    moved, _ = _run(hip, x, 44100, offset=5)
    assert np.array_equal(first, again) and np.array_equal(first, moved)


# ---- equal rates ---------------------------------------------------------------------------------
def test_equal_rates_copy_and_mean(hip):
    rng = np.random.default_rng(12)
    mono = _noise(rng, 5000, np.int16)                         # more than two workgroups
    for offset in (0, 1, 7):
        got, status = _run(hip, mono, 16000, offset=offset)
        assert status == 0 and np.array_equal(got, mono)
    assert torch.equal(hip.resample(torch.from_numpy(mono).cuda(), 16000).cpu(),
                       torch.from_numpy(mono))
    stereo = _noise(rng, (5000, 2), np.int16)
    stereo[:4] = [[1, 2], [3, 4], [-1, -2], [32767, 32767]]   # ties go to the even neighbour
    got, _ = _run(hip, stereo, 16000)
    mean = np.rint((stereo[:, 0].astype(np.float64) + stereo[:, 1]) * 0.5).astype(np.int16)
    assert list(got[:4]) == [2, 4, -2, 32767] and np.array_equal(got, mean)
    for dtype, channels in ((np.uint8, 3), (np.int32, 2), (np.float32, 8)):
        x = _noise(rng, (3000, channels), dtype)
        got, _ = _run(hip, x, 22050, 22050)
        assert np.array_equal(got, ref.resample_f32(x, 22050, 22050)[0]), dtype


# ---- the status word -----------------------------------------------------------------------------
@pytest.mark.parametrize('poison', [np.nan, np.inf, -np.inf])
def test_a_non_finite_sample_raises_the_status_bit(hip, poison):
    rng = np.random.default_rng(13)
    clean = _noise(rng, (9000, 2), np.float32)
    m, l, radius, _ = ref.plan(48000)
    _, status = _run(hip, clean, 48000)
    assert status == 0
    bad = clean.copy()
    at = 4321
    bad[at, 1] = poison
    got, status = _run(hip, bad, 48000)
    assert status == 1
    with pytest.raises(ValueError, match='non-finite sample'):
        hip.resample(torch.from_numpy(bad).cuda(), 48000)
    assert hip.resample(torch.from_numpy(clean).cuda(), 48000).shape == (3000,)
    # outputs farther than R + 1 inputs from it are what they are without it
    t0 = np.arange(len(got), dtype=np.int64) * m // l
    far = np.abs(t0 - at) > radius + 1
    assert 0 < (~far).sum() <= 2 * (radius + 2) * l // m + 2
    want, _ = ref.resample_f32(clean, 48000)
    _agree(got[far], want[far], 'far from the {}'.format(poison))
    # a wrapper call on other samples afterwards starts from a cleared word
    out, word = hip.resample_launch(torch.from_numpy(clean).cuda(), 48000)
    assert int(word.item()) == 0 and out.dtype == torch.int16
