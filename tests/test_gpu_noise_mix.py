"""`ctcasr_noise_mix` on the GPU against tests/noise_reference.py.

Exact: the draws and the two integer powers.  The gain: within relative 2^-23 (one fp32 ulp) of
the float64 gain.  The samples are judged against y64 = x + f64(g) * v computed from the gain the
KERNEL reported: a sample equals clamp(rint(y64)), or differs from it by 1 while y64 lies within
2^-7 of a half-integer.  (The fp32 value x + g * v is off from y64 by at most two roundings of
magnitude <= 2^16: 2 * 2^-24 * 2^16 = 2^-7 for |y64| <= 65536; beyond that both sides saturate.)
Everything that is not mixed keeps its bits: rows that drew nothing, bad rows, silent rows, and
in every row the columns at or beyond n - filled with 1234 here, not zero, so that a store of
padding would show.  The share of samples that differ at all is printed, not asserted."""

import numpy as np
import pytest
import torch

from tests import noise_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
N = 16001                   # odd: every second row starts on an odd sample
FILL = 1234
CHUNK = 8192                # hip.NOISE_MIX_CHUNK (asserted below): samples per workgroup
LENGTHS = [1, 7, 8, 9, 255, 256, 257, 4095, 4096, 4097, 16001, CHUNK - 1, CHUNK, CHUNK + 1]
CLIPS = [1, 5, 401, 4096, 50000]


def _bank(lengths, seed=7, scale=3000):
    rng = np.random.default_rng(seed)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    bank = np.clip(rng.normal(size=int(offsets[-1])) * scale, -32768, 32767).astype(np.int16)
    bank[bank == 0] = 1                      # (no clip of one sample that is silent by chance)
    return bank, offsets


def _speech(lengths, max_samples=N, seed=9, scale=3000):
    rng = np.random.default_rng(seed)
    pcm = np.full((len(lengths), max_samples), FILL, dtype=np.int16)
    for row, n in enumerate(lengths):
        if 0 < n <= max_samples:
            pcm[row, :n] = np.clip(rng.normal(size=n) * scale, -32768, 32767)
    return pcm, np.array(lengths, dtype=np.int32)


@pytest.fixture(scope='module')
def bank5():
    return _bank(CLIPS)


@pytest.fixture(scope='module')
def speech():
    return _speech(LENGTHS)


class Got:
    pass


def _run(hip, pcm, nums, bank, offsets, seed, lo, hi, permille=1000, in_place=False,
         reports=True):
    batch = len(nums)
    x = torch.from_numpy(pcm).to(DEV)
    got = Got()
    draws = torch.full((batch, 4), -7, dtype=torch.int32, device=DEV) if reports else None
    powers = torch.full((batch, 2), -7, dtype=torch.int64, device=DEV) if reports else None
    gain = torch.full((batch,), -7.0, dtype=torch.float32, device=DEV) if reports else None
    out = hip.noise_mix(x, torch.from_numpy(nums).to(DEV), torch.from_numpy(bank).to(DEV),
                        torch.from_numpy(offsets).to(DEV), seed, lo, hi, permille,
                        out=x if in_place else None, draws=draws, powers=powers, gain=gain)
    assert (out is x) == in_place and out.shape == x.shape and out.dtype == torch.int16
    if not in_place:
        assert np.array_equal(x.cpu().numpy(), pcm)          # the input is only read
    got.out = out.cpu().numpy()
    if reports:
        got.draws, got.powers, got.gain = draws.cpu().numpy(), powers.cpu().numpy(), \
            gain.cpu().numpy()
    return got


def _check(pcm, nums, bank, offsets, seed, lo, hi, permille, got):
    """Everything the header pins; returns (samples that differ from rint(y64), mixed samples)."""
    want = ref.mix(pcm, nums, bank, offsets, seed, lo, hi, permille, gains=got.gain)
    assert np.array_equal(got.draws, want['draws'])
    assert np.array_equal(got.powers, want['powers'])
    differing = total = 0
    for b, y64 in enumerate(want['y64']):
        n = int(nums[b])
        if y64 is None:
            assert got.gain[b] == 0.0
            assert np.array_equal(got.out[b], pcm[b]), b          # a bit copy, every column
            continue
        assert got.draws[b, 0] == 1
        g64 = want['gain'][b]
        assert abs(float(got.gain[b]) - g64) <= 2.0 ** -23 * g64, (b, got.gain[b], g64)
        assert np.array_equal(got.out[b, n:], pcm[b, n:]), b       # the padding keeps its bits
        diff = np.abs(got.out[b, :n].astype(np.int64) - ref.rounded(y64).astype(np.int64))
        off_half = np.abs(y64 - np.floor(y64) - 0.5)
        bad = (diff > 1) | ((diff == 1) & (off_half > 2.0 ** -7))
        assert not bad.any(), (b, int(np.argmax(bad)), int(diff.max()))
        differing += int((diff > 0).sum())
        total += n
    return differing, total


def test_constants(hip):
    assert hip.NOISE_MIX_CHUNK == CHUNK and hip.NOISE_MIX_SNR_DB == (-20, 60)
    assert hip.noise_mix_workspace_bytes(32) >= 32 * 16


def test_each_row_alone(hip, bank5, speech):
    bank, offsets = bank5
    pcm, nums = speech
    clips_seen = set()
    for row in range(len(LENGTHS)):
        seed = 100 + row
        one, n_one = pcm[row:row + 1], nums[row:row + 1]
        got = _run(hip, one, n_one, bank, offsets, seed, 5, 25)
        _check(one, n_one, bank, offsets, seed, 5, 25, 1000, got)
        assert got.draws[0, 0] == 1
        clips_seen.add(int(got.draws[0, 1]))
    assert len(clips_seen) >= 4


def test_all_rows_in_one_batch(hip, bank5, speech):
    bank, offsets = bank5
    pcm, nums = speech
    differing = total = 0
    for seed in (1, 2, 3):
        got = _run(hip, pcm, nums, bank, offsets, seed, 5, 25)
        more = _check(pcm, nums, bank, offsets, seed, 5, 25, 1000, got)
        assert (got.draws[:, 0] == 1).all()
        assert len(set(got.draws[:, 3])) > 1                     # lo < hi: more than one SNR
        differing, total = differing + more[0], total + more[1]
    print('noise_mix: {} of {} mixed samples differ from rint(y64) ({:.4%})'
          .format(differing, total, differing / max(total, 1)))


def _drawn(offsets, n, max_samples=N):
    return lambda seed: ref.draw_row(seed, 0, n, max_samples, offsets, 10, 10, 1000)


# (name, n, what the draw of row 0 has to be); lengths of the clips: 1, 5, 401, 4096, 50 000
WRAPS = [
    ('no_wrap', 16001, lambda k, o: k == 4 and o + 16001 < 50000),
    ('one_wrap', 16001, lambda k, o: k == 4 and o + 16001 > 50000),
    ('many_wraps_len_1', 16001, lambda k, o: k == 0),
    ('many_wraps_len_5', 16001, lambda k, o: k == 1),
    ('many_wraps_len_401', 16001, lambda k, o: k == 2),
    ('four_wraps_len_4096', 16001, lambda k, o: k == 3),
    ('ends_at_the_clips_end', 257, lambda k, o: k == 2 and o + 257 == 401),
    ('ends_at_the_clips_end_8_aligned', 4096 - 8, lambda k, o: k == 3 and o == 8),
    ('starts_at_the_last_sample', 4097, lambda k, o: k == 2 and o == 400),
    ('starts_at_the_last_sample_len_5', 9, lambda k, o: k == 1 and o == 4),
]


@pytest.mark.parametrize('name,n,wanted', WRAPS, ids=[w[0] for w in WRAPS])
def test_wraps(hip, bank5, name, n, wanted):
    bank, offsets = bank5
    draw = _drawn(offsets, n)
    seed = ref.find_seed(lambda s: wanted(*draw(s)[1:3]))
    pcm, nums = _speech([n], seed=11)
    got = _run(hip, pcm, nums, bank, offsets, seed, 10, 10)
    _check(pcm, nums, bank, offsets, seed, 10, 10, 1000, got)
    assert got.draws[0, 0] == 1 and wanted(int(got.draws[0, 1]), int(got.draws[0, 2]))
    assert got.draws[0, 3] == 10                                 # lo == hi
    v = ref.noise_under(bank, offsets, int(got.draws[0, 1]), int(got.draws[0, 2]), n)
    assert got.powers[0, 1] == int((v * v).sum())


def test_a_bank_of_one_clip_and_one_of_300(hip, speech):
    pcm, nums = speech
    bank, offsets = _bank([777], seed=3)
    got = _run(hip, pcm, nums, bank, offsets, 21, 0, 40)
    _check(pcm, nums, bank, offsets, 21, 0, 40, 1000, got)
    assert (got.draws[:, 1] == 0).all() and (got.draws[:, 0] == 1).all()
    rng = np.random.default_rng(5)
    lengths = [int(v) for v in rng.integers(1, 3000, size=300)]
    lengths[::50] = [1, 2, 7, 8, 9, 2999]
    bank, offsets = _bank(lengths, seed=4)
    got = _run(hip, pcm, nums, bank, offsets, 22, -5, 40)
    _check(pcm, nums, bank, offsets, 22, -5, 40, 1000, got)
    assert len(set(got.draws[:, 1])) >= 10 and got.draws[:, 1].max() > 150


def test_permille(hip, bank5):
    bank, offsets = bank5
    pcm, nums = _speech([257 + (i % 5) for i in range(64)], max_samples=301, seed=13)
    statuses = {}
    for permille in (0, 500, 1000):
        got = _run(hip, pcm, nums, bank, offsets, 31, 10, 30, permille)
        _check(pcm, nums, bank, offsets, 31, 10, 30, permille, got)
        statuses[permille] = got.draws[:, 0]
        same = _run(hip, pcm, nums, bank, offsets, 31, 10, 30, permille, in_place=True)
        assert np.array_equal(same.out, got.out) and np.array_equal(same.draws, got.draws)
    assert not statuses[0].any() and (statuses[1000] == 1).all()
    assert 16 <= int(statuses[500].sum()) <= 48 and set(statuses[500]) == {0, 1}
    # permille 0: a bit copy, draws and powers all zero; nothing at all without the reports
    got = _run(hip, pcm, nums, bank, offsets, 31, 10, 30, 0)
    assert np.array_equal(got.out, pcm) and not got.draws.any() and not got.powers.any()
    assert not got.gain.any()
    bare = _run(hip, pcm, nums, bank, offsets, 31, 10, 30, 0, in_place=True, reports=False)
    assert np.array_equal(bare.out, pcm)


def test_silent_speech_and_silent_noise(hip, bank5):
    bank, offsets = bank5
    pcm, nums = _speech([4097, 4097, 300])
    pcm[1, :4097] = 0                                            # a silent utterance
    got = _run(hip, pcm, nums, bank, offsets, 41, 10, 10)
    _check(pcm, nums, bank, offsets, 41, 10, 10, 1000, got)
    assert list(got.draws[:, 0]) == [1, 2, 1] and got.powers[1, 0] == 0 < got.powers[1, 1]
    assert got.gain[1] == 0.0 and np.array_equal(got.out[1], pcm[1])
    quiet = np.zeros(500, dtype=np.int16)                        # a silent clip
    q_off = np.array([0, 500], dtype=np.int64)
    pcm[1, :4097] = 5
    for in_place in (False, True):
        got = _run(hip, pcm, nums, quiet, q_off, 41, 10, 10, in_place=in_place)
        _check(pcm, nums, quiet, q_off, 41, 10, 10, 1000, got)
        assert (got.draws[:, 0] == 2).all() and not got.powers[:, 1].any()
        assert got.powers[:, 0].all() and np.array_equal(got.out, pcm)


def test_a_clip_of_no_samples_is_not_served(hip):
    bank, _ = _bank([100], seed=6)
    offsets = np.array([0, 0, 100, 100], dtype=np.int64)         # clips 0 and 2 are empty
    pcm, nums = _speech([300] * 12, max_samples=333)
    got = _run(hip, pcm, nums, bank, offsets, 51, 10, 20)
    _check(pcm, nums, bank, offsets, 51, 10, 20, 1000, got)
    assert set(got.draws[:, 0]) == {1, 2}
    empty = got.draws[:, 1] != 1
    assert (got.draws[empty, 0] == 2).all() and not got.draws[empty, 2].any()
    assert not got.powers[empty].any() and np.array_equal(got.out[empty], pcm[empty])


def test_saturation(hip):
    """Full-scale square waves at -20 dB: the gain is about ten, both rails are reached, and
    nothing wraps around."""
    n = 4097
    pcm = np.full((1, n + 4), FILL, dtype=np.int16)
    pcm[0, :n] = 32767 * np.where((np.arange(n) // 20) % 2 == 0, 1, -1)
    pcm[0, 5] = -32768
    bank = (32767 * np.where((np.arange(1001) // 7) % 2 == 0, 1, -1)).astype(np.int16)
    bank[3] = -32768
    offsets = np.array([0, 1001], dtype=np.int64)
    nums = np.array([n], dtype=np.int32)
    got = _run(hip, pcm, nums, bank, offsets, 61, -20, -20)
    _check(pcm, nums, bank, offsets, 61, -20, -20, 1000, got)
    assert 9.9 < got.gain[0] < 10.1
    out = got.out[0, :n].astype(np.int64)
    assert out.max() == 32767 and out.min() == -32768
    y64 = pcm[0, :n].astype(np.float64) + float(got.gain[0]) * ref.noise_under(
        bank, offsets, 0, int(got.draws[0, 2]), n)
    assert (out[y64 > 32768] == 32767).all() and (out[y64 < -32769] == -32768).all()
    assert (y64 > 40000).any() and (y64 < -40000).any()


def test_in_place_equals_out_of_place_and_runs_repeat(hip, bank5, speech):
    bank, offsets = bank5
    pcm, nums = speech
    runs = [_run(hip, pcm, nums, bank, offsets, 71, 0, 30, 700, in_place=flag)
            for flag in (False, True, False, True)]
    for other in runs[1:]:
        assert np.array_equal(other.out, runs[0].out)
        assert np.array_equal(other.draws, runs[0].draws)
        assert np.array_equal(other.powers, runs[0].powers)
        assert other.gain.tobytes() == runs[0].gain.tobytes()
    assert set(runs[0].draws[:, 0]) == {0, 1}
    bare = _run(hip, pcm, nums, bank, offsets, 71, 0, 30, 700, reports=False)
    assert np.array_equal(bare.out, runs[0].out)                 # the reports are optional
    other_seed = _run(hip, pcm, nums, bank, offsets, 72, 0, 30, 700)
    assert not np.array_equal(other_seed.out, runs[0].out)


def test_bad_rows_are_copied(hip, bank5):
    bank, offsets = bank5
    pcm, nums = _speech([0, -5, 501, 401], max_samples=500)
    rng = np.random.default_rng(1)
    pcm[:3] = rng.integers(-3000, 3000, size=(3, 500))           # whatever a bad row holds
    for in_place in (False, True):
        got = _run(hip, pcm, nums, bank, offsets, 81, 10, 10, in_place=in_place)
        _check(pcm, nums, bank, offsets, 81, 10, 10, 1000, got)
        assert not got.draws[:3].any() and not got.powers[:3].any() and not got.gain[:3].any()
        assert np.array_equal(got.out[:3], pcm[:3]) and got.draws[3, 0] == 1


def _abi_args(hip):
    t = {'pcm': torch.zeros((2, 64), dtype=torch.int16, device=DEV),
         'num': torch.full((2,), 64, dtype=torch.int32, device=DEV),
         'bank': torch.ones(100, dtype=torch.int16, device=DEV),
         'off': torch.tensor([0, 40, 100], dtype=torch.int64, device=DEV),
         'out': torch.zeros((2, 64), dtype=torch.int16, device=DEV),
         'ws': torch.zeros(256, dtype=torch.uint8, device=DEV)}
    good = dict(pcm=t['pcm'].data_ptr(), num=t['num'].data_ptr(), B=2, max_samples=64,
                bank=t['bank'].data_ptr(), off=t['off'].data_ptr(), num_clips=2, seed=1, lo=10,
                hi=30, permille=500, out=t['out'].data_ptr(), draws=None, powers=None, gain=None,
                ws=t['ws'].data_ptr(), ws_bytes=256, stream=None)
    return t, good


def test_argument_errors_through_the_abi(hip):
    lib = hip.load()
    keep, good = _abi_args(hip)

    def call(**change):
        return lib.ctcasr_noise_mix(*{**good, **change}.values())

    assert call() == 0
    torch.cuda.synchronize()
    for name in ('pcm', 'num', 'bank', 'off', 'out'):
        assert call(**{name: None}) == -1, name
    for change in (dict(B=0), dict(B=-1), dict(max_samples=0), dict(num_clips=0),
                   dict(lo=31, hi=30), dict(lo=-21), dict(hi=61), dict(lo=61, hi=61),
                   dict(lo=-21, hi=-21), dict(permille=-1), dict(permille=1001)):
        assert call(**change) == -1, change
    assert call(max_samples=(1 << 30) + 1) == -2
    assert call(num_clips=(1 << 24) + 1) == -2
    assert call(ws=None) == -3 and call(ws_bytes=31) == -3
    assert call(ws=good['ws'] + 4) == -3                          # not 8-byte aligned
    assert lib.ctcasr_noise_mix_workspace_bytes(2) == 32 and call(ws_bytes=32) == 0
    assert lib.ctcasr_noise_mix_workspace_bytes(0) == 0
    torch.cuda.synchronize()
    del keep


def test_argument_errors_through_the_wrapper(hip):
    keep, _ = _abi_args(hip)
    pcm, num, bank, off = keep['pcm'], keep['num'], keep['bank'], keep['off']
    assert hip.noise_mix(pcm, num, bank, off, 1, 10, 30).shape == pcm.shape
    bad_calls = [
        lambda: hip.noise_mix(pcm, num, bank, off, 1, 31, 30),
        lambda: hip.noise_mix(pcm, num, bank, off, 1, -21, 30),
        lambda: hip.noise_mix(pcm, num, bank, off, 1, 10, 61),
        lambda: hip.noise_mix(pcm, num, bank, off, 1, 10, 30, -1),
        lambda: hip.noise_mix(pcm, num, bank, off, 1, 10, 30, 1001),
        lambda: hip.noise_mix(pcm[:0], num[:0], bank, off, 1, 10, 30),            # B < 1
        lambda: hip.noise_mix(pcm[:, :0].contiguous(), num, bank, off, 1, 10, 30),
        lambda: hip.noise_mix(pcm, num, bank, off[:1], 1, 10, 30),                # no clip
        lambda: hip.noise_mix(pcm, num, bank[:0], off, 1, 10, 30),
        lambda: hip.noise_mix(pcm.cpu(), num, bank, off, 1, 10, 30),              # a CPU tensor
        lambda: hip.noise_mix(pcm, num.cpu(), bank, off, 1, 10, 30),
        lambda: hip.noise_mix(pcm, num, bank.cpu(), off, 1, 10, 30),
        lambda: hip.noise_mix(pcm, num, bank, off.cpu(), 1, 10, 30),
        lambda: hip.noise_mix(pcm.int(), num, bank, off, 1, 10, 30),              # dtypes
        lambda: hip.noise_mix(pcm, num.long(), bank, off, 1, 10, 30),
        lambda: hip.noise_mix(pcm, num, bank.float(), off, 1, 10, 30),
        lambda: hip.noise_mix(pcm, num, bank, off.int(), 1, 10, 30),
        lambda: hip.noise_mix(pcm, num[:1], bank, off, 1, 10, 30),                # counts
        lambda: hip.noise_mix(pcm, num, bank, off, 1, 10, 30, out=keep['out'][:1]),
        lambda: hip.noise_mix(pcm, num, bank, off, 1, 10, 30,
                              draws=torch.zeros((2, 3), dtype=torch.int32, device=DEV)),
        lambda: hip.noise_mix(pcm, num, bank, off, 1, 10, 30,
                              draws=torch.zeros((2, 4), dtype=torch.int64, device=DEV)),
        lambda: hip.noise_mix(pcm, num, bank, off, 1, 10, 30,
                              powers=torch.zeros(2, dtype=torch.int64, device=DEV)),
        lambda: hip.noise_mix(pcm, num, bank, off, 1, 10, 30,
                              gain=torch.zeros(3, dtype=torch.float32, device=DEV)),
        lambda: hip.noise_mix(pcm.t(), num, bank, off, 1, 10, 30),                # not contiguous
        lambda: hip.noise_mix(pcm[0], num[:1], bank, off, 1, 10, 30),             # not [B, N]
    ]
    for i, bad in enumerate(bad_calls):
        with pytest.raises(hip.CtcAsrError):
            bad()
            pytest.fail('call {} was accepted'.format(i))
    torch.cuda.synchronize()
