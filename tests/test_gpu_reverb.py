"""`ctcasr_reverb` on the GPU against tests/reverb_reference.py, bit for bit: the draws, the
reverberated samples (an exact 32-bit integer sum, one float32 product, one rounding) and every
sample that must come through as a copy - rows that drew nothing, bad rows, rows whose response
is not served, and in every row the columns at or beyond n, filled with 1234 here, not zero, so
that padding leaking into a sum or a store of padding would show."""

import numpy as np
import pytest
import torch

from tests import reverb_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FILL = 1234
CHUNK = 2048                # hip.REVERB_CHUNK (asserted below): output samples per workgroup
BLOCK = 32                  # hip.REVERB_TAP_BLOCK (asserted below): taps per inner round
TAP_COUNTS = [8, 16, BLOCK - 8, BLOCK, BLOCK + 8, 8192]


def _taps(rng, count):
    """Random taps that keep the bank's rule, sum |h| <= 65535, as large as that allows."""
    most = max(1, min(32767, 65535 // count))
    return rng.integers(-most, most + 1, size=count).astype(np.int16)


def _audio(rng, lengths, max_samples):
    """Random int16 over the whole range with runs of both extremes; FILL at and beyond n."""
    pcm = np.full((len(lengths), max_samples), FILL, dtype=np.int16)
    for row, n in enumerate(lengths):
        if 0 < n <= max_samples:
            x = rng.integers(-32768, 32768, size=n).astype(np.int16)
            for start, value in ((n // 5, -32768), (n // 2, 32767), (n - n // 7 - 1, -32768)):
                x[start:start + max(1, n // 9)] = value
            pcm[row, :n] = x
    return pcm, np.array(lengths, dtype=np.int32)


def _run(hip, pcm, nums, bank, seed, permille=1000, out=None, with_draws=True):
    x = torch.from_numpy(pcm).to(DEV)
    draws = torch.full((len(nums), 2), -7, dtype=torch.int32, device=DEV) if with_draws else None
    got = hip.reverb(x, torch.from_numpy(nums).to(DEV), torch.from_numpy(bank.taps).to(DEV),
                     torch.from_numpy(bank.offsets).to(DEV), torch.from_numpy(bank.delay).to(DEV),
                     torch.from_numpy(bank.scale).to(DEV), seed, permille, out=out, draws=draws)
    assert got is not x and got.shape == x.shape and got.dtype == torch.int16
    assert out is None or got is out
    assert np.array_equal(x.cpu().numpy(), pcm)                  # the input is only read
    return got.cpu().numpy(), (draws.cpu().numpy() if with_draws else None)


def _check(hip, pcm, nums, bank, seed, permille=1000):
    got, draws = _run(hip, pcm, nums, bank, seed, permille)
    want, want_draws = ref.reverb_rows(pcm, nums, bank, seed, permille)
    assert np.array_equal(draws, want_draws)
    assert got.tobytes() == want.tobytes()
    return got, draws


def test_constants(hip):
    assert (hip.REVERB_CHUNK, hip.REVERB_TAP_BLOCK) == (CHUNK, BLOCK)
    assert (hip.REVERB_TAP_ALIGN, hip.REVERB_MAX_TAPS) == (ref.TAP_ALIGN, ref.MAX_TAPS) == (8, 8192)


@pytest.mark.parametrize('count', [8, 8192])
def test_rows_shorter_than_the_response(hip, count):
    rng = np.random.default_rng(count)
    for lengths, delay in (([1, 2, 7, 8], 0), ([9, 1, 8, 7], count - 1), ([9, 2, 7, 8], 5)):
        bank = ref.Bank.of([(_taps(rng, count), delay, 2.0 ** -9)])
        pcm, nums = _audio(rng, lengths, 11)
        got, draws = _check(hip, pcm, nums, bank, 3)
        assert (draws[:, 0] == 1).all() and (got[:, 9:] == FILL).all()


@pytest.mark.parametrize('delay', [0, 1, 31, -1])
@pytest.mark.parametrize('count', TAP_COUNTS)
def test_chunk_seams_tap_block_seams_and_delays(hip, count, delay):
    """Rows that end just before, on and just behind a workgroup's seam, in a batch whose rows
    are an odd number of samples apart (every second row starts off a 4-byte boundary); a delay
    of 31 is outside a response of 8 or 16 taps, which is then not served."""
    delay = count - 1 if delay < 0 else delay
    rng = np.random.default_rng(1000 * count + delay)
    lengths = [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
    max_samples = 2 * CHUNK + 5
    bank = ref.Bank.of([(_taps(rng, count), delay, 2.0 ** -7)])
    pcm, nums = _audio(rng, lengths, max_samples)
    for row, n in enumerate(lengths):
        pcm[row, n - 1], pcm[row, n], pcm[row, n + 1] = 32767, -32768, 32767
    got, draws = _check(hip, pcm, nums, bank, 5)
    assert (draws[:, 0] == (1 if delay < count else 2)).all()
    for row, n in enumerate(lengths):
        assert np.array_equal(got[row, n:], pcm[row, n:])        # (part of the check above)


@pytest.mark.parametrize('count', [16, BLOCK + 8])
def test_a_single_tap_shifts_the_input(hip, count):
    rng = np.random.default_rng(count)
    n = CHUNK + 77
    pcm, nums = _audio(rng, [n, n - 1], n + 2)
    for position in (0, 1, 7, 8, count - 1):
        h = np.zeros(count, dtype=np.int16)
        h[position] = 1
        for delay in (0, position):
            got, _ = _check(hip, pcm, nums, ref.Bank.of([(h, delay, 1.0)]), 1)
            shift = position - delay                              # out[i] = x[i - shift]
            for row, m in enumerate(nums):
                assert not got[row, :shift].any()
                assert np.array_equal(got[row, shift:m], pcm[row, :m - shift])


def test_extremes(hip):
    """Audio that sits on one end of the range under 8192 taps of +7, and under 6144 taps of +10,
    which a row of 3 CHUNK + 5 samples covers whole: the accumulator reaches -10 * 6144 * 32768 =
    -0.94 * 2^31 (and +0.94 * 2^31 less a bit, where the int-to-float conversion rounds) and the
    result is still exact; a scale of 1 drives both clamps; scales of 0 and of a denormal give
    silence."""
    n = 3 * CHUNK + 5
    pcm = np.full((2, n + 2), FILL, dtype=np.int16)
    pcm[0, :n], pcm[1, :n] = -32768, 32767
    nums = np.array([n, n], dtype=np.int32)
    sevens, tens = np.full(8192, 7, dtype=np.int16), np.full(6144, 10, dtype=np.int16)
    got, _ = _check(hip, pcm, nums, ref.Bank.of([(sevens, 0, 2.0 ** -16)]), 1)
    # -3.5, -7, -10.5 and 3.4999, 6.9998, 10.4997: half to even
    assert got[0, :3].tolist() == [-4, -7, -10] and got[1, :3].tolist() == [3, 7, 10]
    assert ref.accumulate(pcm[0, :n], tens, 3000).min() == -10 * 6144 * 32768 < -0.93 * 2 ** 31
    assert ref.accumulate(pcm[1, :n], tens, 3000).max() == 10 * 6144 * 32767 > 0.93 * 2 ** 31
    for h, delay in ((tens, 3000), (sevens, 4000), (sevens, 8191)):
        got, _ = _check(hip, pcm, nums, ref.Bank.of([(h, delay, 2.0 ** -16)]), 1)
        assert got[0, :n].min() < -21000 and got[1, :n].max() > 21000
        got, _ = _check(hip, pcm, nums, ref.Bank.of([(h, delay, 1.0)]), 1)
        assert (got[0, :n] == -32768).all() and (got[1, :n] == 32767).all()
        for scale in (0.0, 1e-40):
            got, _ = _check(hip, pcm, nums, ref.Bank.of([(h, delay, scale)]), 1)
            assert not got[:, :n].any() and (got[:, n:] == FILL).all()


def test_copies_and_status_words(hip):
    rng = np.random.default_rng(21)
    max_samples = CHUNK + 9
    good = (_taps(rng, 24), 3, 2.0 ** -8)
    bank = ref.Bank.of([good])
    # permille 0: a bit copy and zeroed draws; permille 1000: every row; bad rows: copies
    pcm, nums = _audio(rng, [max_samples, 500, CHUNK, 1], max_samples)
    got, draws = _check(hip, pcm, nums, bank, 9, permille=0)
    assert np.array_equal(got, pcm) and not draws.any()
    got, draws = _check(hip, pcm, nums, bank, 9, permille=1000)
    assert draws.tolist() == [[1, 0]] * 4
    assert all(not np.array_equal(got[row, :n], pcm[row, :n]) for row, n in enumerate(nums[:3]))
    pcm, nums = _audio(rng, [0, -1, max_samples + 1, 700], max_samples)
    got, draws = _check(hip, pcm, nums, bank, 9)
    assert draws.tolist() == [[0, 0], [0, 0], [0, 0], [1, 0]]
    assert np.array_equal(got[:3], pcm[:3]) and (got[:3] == FILL).all()
    # responses that are not served: status 2 and a copy
    pcm, nums = _audio(rng, [max_samples, 500, CHUNK, 1], max_samples)
    room = np.concatenate([np.zeros(4, dtype=np.int16), _taps(rng, 8200)])
    for offsets, delay in (([0, 4], 0), ([0, 12], 0), ([0, 8200], 0), ([4, 12], 0), ([0, 8], -1),
                           ([0, 8], 8), ([8, 8], 0)):
        bad = ref.Bank(room, offsets, [delay], [1.0])
        got, draws = _check(hip, pcm, nums, bad, 9)
        assert draws.tolist() == [[2, 0]] * 4 and np.array_equal(got, pcm)
    # a bank of five, two of them bad, half of the rows drawn: the draws are the reference's
    five = ref.Bank.of([good, (_taps(rng, 8), 7, 0.01), (_taps(rng, 12), 0, 1.0),
                        (_taps(rng, 4), 0, 1.0), (_taps(rng, 8192), 40, 2.0 ** -10)])
    seen = set()
    for seed in (1, 2, 3):
        _, draws = _check(hip, pcm, nums, five, seed, permille=500)
        seen |= {tuple(row) for row in draws.tolist()}
    assert {status for status, _ in seen} == {0, 1, 2}            # (known from the reference)


def test_calls_repeat_and_leave_no_trace(hip):
    rng = np.random.default_rng(33)
    max_samples = 3 * CHUNK + 9
    bank = ref.Bank.of([(_taps(rng, 104), 32, 2.0 ** -8), (_taps(rng, 8), 0, 0.5)])
    pcm, nums = _audio(rng, [max_samples, 3 * CHUNK, 17, 2 * CHUNK + 1], max_samples)
    first, draws = _run(hip, pcm, nums, bank, 77, 700)
    second, again = _run(hip, pcm, nums, bank, 77, 700)
    assert first.tobytes() == second.tobytes() and np.array_equal(draws, again)
    # another batch into the tensor that held a result: nothing of the old one stays
    out = torch.from_numpy(first).to(DEV)
    other, lengths = _audio(rng, [5, max_samples, 0, CHUNK], max_samples)
    got, _ = _run(hip, other, lengths, bank, 78, 700, out=out, with_draws=False)
    want, _ = ref.reverb_rows(other, lengths, bank, 78, 700)
    assert got.tobytes() == want.tobytes()


def test_argument_errors_come_through_the_abi_as_codes(hip):
    lib = hip.load()
    pcm = torch.zeros((2, 64), dtype=torch.int16, device=DEV)
    out = torch.full((2, 64), 5, dtype=torch.int16, device=DEV)
    num = torch.full((2,), 64, dtype=torch.int32, device=DEV)
    taps = torch.ones(8, dtype=torch.int16, device=DEV)
    off = torch.tensor([0, 8], device=DEV)
    delay = torch.zeros(1, dtype=torch.int32, device=DEV)
    scale = torch.ones(1, device=DEV)
    good = dict(pcm=pcm.data_ptr(), num=num.data_ptr(), B=2, max_samples=64, taps=taps.data_ptr(),
                off=off.data_ptr(), delay=delay.data_ptr(), scale=scale.data_ptr(), num_rirs=1,
                seed=1, permille=1000, out=out.data_ptr(), draws=None, stream=None)

    def call(**change):
        return lib.ctcasr_reverb(*{**good, **change}.values())

    assert call(out=pcm.data_ptr()) == -1
    for name in ('pcm', 'num', 'taps', 'off', 'delay', 'scale', 'out'):
        assert call(**{name: None}) == -1, name
    assert call(B=0) == -1 and call(permille=1001) == -1 and call(num_rirs=0) == -1
    torch.cuda.synchronize()
    assert (out == 5).all()                                       # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert not out.any()                                          # silence in, silence out


def test_the_wrapper_refuses_what_the_kernel_cannot_take(hip):
    pcm = torch.zeros((2, 64), dtype=torch.int16, device=DEV)
    num = torch.full((2,), 64, dtype=torch.int32, device=DEV)
    taps = torch.ones(8, dtype=torch.int16, device=DEV)
    off = torch.tensor([0, 8], device=DEV)
    delay = torch.zeros(1, dtype=torch.int32, device=DEV)
    scale = torch.ones(1, device=DEV)
    assert hip.reverb(pcm, num, taps, off, delay, scale, 1).shape == (2, 64)
    with pytest.raises(hip.CtcAsrError, match='out is pcm'):
        hip.reverb(pcm, num, taps, off, delay, scale, 1, out=pcm)
    with pytest.raises(hip.CtcAsrError, match='out is pcm'):
        hip.reverb(pcm, num, taps, off, delay, scale, 1, out=pcm.view(-1))
    for position in range(6):
        args = [pcm, num, taps, off, delay, scale]
        args[position] = args[position].cpu()
        with pytest.raises(hip.CtcAsrError, match='HBM'):
            hip.reverb(*args, 1)
        args[position] = args[position].to(DEV).to(torch.float64)
        with pytest.raises(hip.CtcAsrError, match='must be torch'):
            hip.reverb(*args, 1)
    with pytest.raises(hip.CtcAsrError, match='draws holds 2 elements, 4 expected'):
        hip.reverb(pcm, num, taps, off, delay, scale, 1,
                   draws=torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(hip.CtcAsrError, match='must be torch.int32'):
        hip.reverb(pcm, num, taps, off, delay, scale, 1,
                   draws=torch.zeros((2, 2), dtype=torch.int64, device=DEV))
    with pytest.raises(hip.CtcAsrError, match='out holds'):
        hip.reverb(pcm, num, taps, off, delay, scale, 1,
                   out=torch.zeros((2, 63), dtype=torch.int16, device=DEV))
    with pytest.raises(hip.CtcAsrError, match='failed'):
        hip.reverb(pcm, num, taps, off, delay, scale, 1, prob_permille=1001)
