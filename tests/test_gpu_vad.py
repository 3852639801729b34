"""`ctcasr_vad_energy` and `ctcasr_gather_segments` on the GPU against tests/vad_reference.py, bit
for bit: integer sums and integer atomics, so nothing is left to a tolerance.  The lengths sit on
the seams of a hop (160 samples) and of a workgroup's share (VAD_CHUNK); a view that starts one
sample into a tensor takes the 2-byte aligned path and must give the numbers of the aligned copy.
The gather writes into rows pre-filled with 1234, so that padding it did not store would show."""

import numpy as np
import pytest
import torch

from tests import vad_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FILL = 1234
CHUNK = ref.CHUNK
LENGTHS = [1, 159, 160, 161, 7, 8, 9, 167, 168, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 161]


@pytest.fixture(scope='module')
def audio():
    """Full-range random samples, longer than the longest case by the offsets the views use."""
    rng = np.random.default_rng(21)
    return rng.integers(-32768, 32768, size=max(LENGTHS) + 16).astype(np.int16)


def _energy(hip, pcm_host, offset=0):
    """(energy, hist) of hip.vad_energy on a copy of ``pcm_host`` that starts ``offset`` samples
    into a 16-byte aligned tensor; also checks shapes, dtypes and that the input is only read."""
    n = len(pcm_host)
    base = torch.full((n + offset + 8,), FILL, dtype=torch.int16, device=DEV)
    base[offset:offset + n] = torch.from_numpy(pcm_host).to(DEV)
    before = base.clone()
    view = base[offset:offset + n]
    assert base.data_ptr() % 16 == 0 and view.data_ptr() == base.data_ptr() + 2 * offset
    energy, hist = hip.vad_energy(view)
    assert energy.dtype == torch.int64 and energy.shape == (-(-n // ref.HOP),)
    assert hist.dtype == torch.int32 and hist.shape == (ref.LEVELS,)
    assert torch.equal(base, before)
    return energy.cpu().numpy(), hist.cpu().numpy()


def _check(hip, pcm_host, offsets=(0, 1)):
    want = ref.energy(pcm_host)
    want_hist = ref.histogram(want)
    for offset in offsets:
        energy, hist = _energy(hip, pcm_host, offset)
        assert np.array_equal(energy, want), offset
        assert np.array_equal(hist, want_hist), offset
        assert hist.sum() == len(want)
    return want, want_hist


def test_constants(hip):
    assert (hip.VAD_HOP, hip.VAD_LEVELS, hip.VAD_CHUNK) == (ref.HOP, ref.LEVELS, ref.CHUNK)


@pytest.mark.parametrize('n', LENGTHS)
def test_energy_at_the_seams(hip, audio, n):
    _check(hip, audio[:n])


def test_energy_from_every_misalignment(hip, audio):
    n = CHUNK + 161
    want = ref.energy(audio[3:3 + n])
    for offset in range(8):
        energy, hist = _energy(hip, audio[3:3 + n], offset)
        assert np.array_equal(energy, want) and np.array_equal(hist, ref.histogram(want))


def test_largest_energy_and_silence(hip):
    n = 2 * ref.HOP + 7
    want, hist = _check(hip, np.full(n, -32768, dtype=np.int16))
    assert want.tolist() == [ref.HOP << 30, ref.HOP << 30, 7 << 30]
    assert hist[145] == 2 and ref.level(ref.HOP << 30) == 145
    want, hist = _check(hip, np.zeros(CHUNK + 5, dtype=np.int16))
    assert not want.any() and hist[0] == len(want) == CHUNK // ref.HOP + 1


def test_histogram_is_zeroed_by_the_call_and_is_a_bincount(hip, audio):
    from ctc_asr_amd import vad
    rng = np.random.default_rng(2)
    # every loudness from silence to full scale, so that many bins are in use
    n = 2 * CHUNK + 1000
    scale = np.repeat(2.0 ** rng.uniform(-16, 0, size=-(-n // ref.HOP)), ref.HOP)[:n]
    pcm_host = (audio[:n] * scale).astype(np.int16)
    x = torch.from_numpy(pcm_host).to(DEV)
    energy, hist = hip.vad_energy(x)
    again_energy, again = hip.vad_energy(x)
    levels = vad.level(energy.cpu().numpy())
    assert levels.tolist() == [ref.level(e) for e in energy.cpu().tolist()]
    assert np.array_equal(hist.cpu().numpy(), np.bincount(levels, minlength=ref.LEVELS))
    assert np.count_nonzero(hist.cpu().numpy()) > 40
    assert torch.equal(hist, again) and torch.equal(energy, again_energy)
    # the same buffers a second time, through the C ABI: the counts do not add up
    lib = hip.load()
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(2):
        assert lib.ctcasr_vad_energy(x.data_ptr(), n, energy.data_ptr(), hist.data_ptr(),
                                     stream) == 0
    assert torch.equal(hist, again) and int(hist.sum()) == energy.numel()
    assert np.array_equal(x.cpu().numpy(), pcm_host)


def test_segment_reads_back_what_the_reference_computes(hip, audio):
    from ctc_asr_amd import vad
    rng = np.random.default_rng(4)
    n = 3 * CHUNK + 77
    rms = np.full(-(-n // ref.HOP), 30.0)
    for a, b in ((20, 90), (200, 420), (500, 505), (700, 769)):
        rms[a:b] = 3000.0
    pcm_host = np.clip(rng.normal(size=n) * np.repeat(rms, ref.HOP)[:n], -32768, 32767) \
        .astype(np.int16)
    energies = ref.energy(pcm_host)
    settings = dict(pad=10, min_raw=5, max_segment=100)
    want = ref.table(energies, ref.histogram(energies), n, **settings)
    got = vad.segment(torch.from_numpy(pcm_host).to(DEV), vad.VadSettings(**settings))
    assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist()
    assert got[2] == want[2] and len(got[0]) >= 6 and got[0][-1] + got[1][-1] == n


def test_energy_argument_errors(hip):
    lib = hip.load()
    x = torch.zeros(512, dtype=torch.int16, device=DEV)
    energy = torch.zeros(8, dtype=torch.int64, device=DEV)
    hist = torch.full((ref.LEVELS,), 5, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.ctcasr_vad_energy(None, 512, energy.data_ptr(), hist.data_ptr(), stream) == -1
    assert lib.ctcasr_vad_energy(x.data_ptr(), 512, None, hist.data_ptr(), stream) == -1
    assert lib.ctcasr_vad_energy(x.data_ptr(), 512, energy.data_ptr(), None, stream) == -1
    assert lib.ctcasr_vad_energy(x.data_ptr(), 0, energy.data_ptr(), hist.data_ptr(), stream) == -1
    code = lib.ctcasr_vad_energy(x.data_ptr(), 1 << 31, energy.data_ptr(), hist.data_ptr(), stream)
    assert code == -2 and lib.ctcasr_error_string(code) == b'unsupported configuration'
    torch.cuda.synchronize()
    assert (hist == 5).all() and not energy.any()            # refused before anything was launched


# ------------------------------------------------------------------------------------------
def _gather(hip, pcm_host, starts, lengths, max_samples, offset=0):
    base = torch.full((len(pcm_host) + offset + 8,), FILL, dtype=torch.int16, device=DEV)
    base[offset:offset + len(pcm_host)] = torch.from_numpy(pcm_host).to(DEV)
    before = base.clone()
    batch = len(starts)
    out = torch.full((batch, max_samples), FILL, dtype=torch.int16, device=DEV)
    num = torch.full((batch,), -7, dtype=torch.int32, device=DEV)
    got = hip.gather_segments(base[offset:offset + len(pcm_host)],
                              torch.tensor(starts, dtype=torch.int64, device=DEV),
                              torch.tensor(lengths, dtype=torch.int32, device=DEV),
                              max_samples, out=out, num_samples=num)
    assert got[0] is out and got[1] is num and torch.equal(base, before)
    want, want_num = ref.gather(pcm_host, starts, lengths, max_samples)
    assert np.array_equal(num.cpu().numpy(), want_num)
    assert np.array_equal(out.cpu().numpy(), want)
    return want, want_num


@pytest.mark.parametrize('max_samples', [1, 7, 640, 641, 8191, 8192, 8200, 16391])
def test_gather_rows(hip, audio, max_samples):
    n = 40000
    pcm_host = audio[:n]
    m = max_samples
    starts = [1, 3, 8, 16, 160, 320, 4801, 0, 160, 160,           # odd, x8, x160, repeated
              n - 5, n - 1, n - m, -1, -160, n, n + 9, 8, 1600, 2 ** 40]
    lengths = [1, m - 1, m, m + 1, m + 1000, m, m, m, 1, m,       # 1, m - 1, m, and above: cut
               m, m, m + 3, m, m, m, m, 0, -4, m]                 # past n: clipped; zero rows
    for offset in (0, 1):
        want, num = _gather(hip, pcm_host, starts, lengths, m, offset)
    assert num[13:].tolist() == [0] * 7 and not want[13:].any()
    assert num[10] == min(5, m) and num[11] == 1 and num[2] == m and num[0] == 1
    assert num[1] == m - 1 and num[12] == min(m, n - max(n - m, 0))
    assert np.array_equal(want[9], pcm_host[160:160 + m]) and not want[8, 1:].any()


def test_gather_default_width_and_one_row(hip, audio):
    x = torch.from_numpy(audio[:5000]).to(DEV)
    out, num = hip.gather_segments(x, torch.tensor([160, 0], dtype=torch.int64, device=DEV),
                                   torch.tensor([480, 1601], dtype=torch.int32, device=DEV))
    assert out.shape == (2, 1601) and num.tolist() == [480, 1601]
    want, _ = ref.gather(audio[:5000], [160, 0], [480, 1601], 1601)
    assert np.array_equal(out.cpu().numpy(), want)
    out, num = hip.gather_segments(x, torch.tensor([4990], dtype=torch.int64, device=DEV),
                                   torch.tensor([100], dtype=torch.int32, device=DEV), 100)
    assert num.tolist() == [10] and out[0, :10].cpu().tolist() == audio[4990:5000].tolist()
    assert not out[0, 10:].any()


def test_gather_feeds_the_features_like_slices(hip, audio):
    """A gathered batch is the input `features_from_pcm` builds on the host, bit for bit, so the
    features are the same launches on the same data."""
    from ctc_asr_amd.input_functions import features_from_pcm
    from ctc_asr_amd.params import FLAGS
    FLAGS.reset()
    starts, lengths = [1600, 0, 8000], [3200, 2721, 480]
    x = torch.from_numpy(audio[:20000]).to(DEV)
    batch, num = hip.gather_segments(x, torch.tensor(starts, dtype=torch.int64, device=DEV),
                                     torch.tensor(lengths, dtype=torch.int32, device=DEV), 3200)
    got = hip.features(batch, num, FLAGS.feature_type, FLAGS.feature_normalization)
    want = features_from_pcm([audio[s:s + n] for s, n in zip(starts, lengths)], DEV)
    # (bit patterns: under 'local' a column that is constant over a short piece is NaN in both)
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
    assert torch.equal(got[1], want[1]) and got[1].tolist() == [19, 16, 2]


def test_gather_argument_errors(hip):
    lib = hip.load()
    x = torch.zeros(512, dtype=torch.int16, device=DEV)
    start = torch.zeros(2, dtype=torch.int64, device=DEV)
    length = torch.full((2,), 16, dtype=torch.int32, device=DEV)
    out = torch.full((2, 16), FILL, dtype=torch.int16, device=DEV)
    num = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    good = [x.data_ptr(), 512, start.data_ptr(), length.data_ptr(), 2, 16, out.data_ptr(),
            num.data_ptr(), stream]
    for hole in (0, 2, 3, 6, 7):
        args = list(good)
        args[hole] = None
        assert lib.ctcasr_gather_segments(*args) == -1
    for position, value, code in ((4, 0, -1), (4, -2, -1), (5, 0, -1), (5, -1, -1)):
        args = list(good)
        args[position] = value
        assert lib.ctcasr_gather_segments(*args) == code
    args = list(good)
    args[5] = (1 << 30) + 1
    code = lib.ctcasr_gather_segments(*args)
    assert code == -2 and lib.ctcasr_error_string(code) == b'unsupported configuration'
    torch.cuda.synchronize()
    assert (out == FILL).all() and (num == -7).all()          # refused before anything was launched
    with pytest.raises(hip.CtcAsrError, match='1 entries for a batch of 2'):
        hip.gather_segments(x, start, length[:1])
    with pytest.raises(hip.CtcAsrError, match='16 expected'):
        hip.gather_segments(x, start, length, 8, out=out)
