"""Feature extraction (csrc/features.hip: frame_features_kernel, mfcc_delta_kernel,
normalize_kernel behind ctcasr_features) at the shapes where it goes wrong first: lengths on both
sides of every frame-count seam and of the normaliser's 96-row statistics stride, 1-5 frames
(where the deltas' +-2 edge clamp is the whole result), the every-second-frame drop at odd and
even frame counts, kept counts and out_frames on both sides of the 16 output bands, digital
silence (the eps paths), full-scale and clipped int16, impulses and exact-bin tones, wide ragged
batches, caller buffers and workspaces full of garbage, rows outside [1, max_samples] and
sampling rates other than 16 kHz.

The reference is the float64 oracle (oracle/features.py, pinned in test_oracle_features.py):
log_mel / mfcc_with_delta, cast to float32, drop, then the normalisation done in float64 on those
float32 values.  The oracle's load_sample_from_pcm refuses n < 401 like the reference does; the
ABI serves every n >= 1, so the pieces are called directly.  DESIGN.md's 1e-3 absolute is the
ceiling of every bar; the bars below are derived, see `_raw_bar` and `_normalized`."""

import numpy as np
import pytest
import torch

from oracle import features as ofeat

pytestmark = pytest.mark.gpu
DEV = 'cuda'

FRAME, STEP = 400, 160
NORM_SPLIT = 16                    # normalize_kernel's output bands (grid.y)
STATS_STRIDE = 12 * 8              # its statistics loop: 12 row groups x 8 rows in flight
LOG_EPS = np.float32(np.log(ofeat.EPS))
CEILING = 1e-3

# largest error seen per group, {group: [|error|, |error| / bar]} (read by whoever runs the
# module to report it; the asserts do not depend on it)
MEASURED = {}


def _record(group, err, ratio):
    seen = MEASURED.setdefault(group, [0.0, 0.0])
    seen[0], seen[1] = max(seen[0], float(err)), max(seen[1], float(ratio))


def frames(n):
    return 1 if n <= FRAME else 1 + -(-(n - FRAME) // STEP)


def kept(n, drop):
    return (frames(n) + 1) // 2 if drop else frames(n)


def tight(k):
    """The most samples that make k frames: the last frame ends on the last sample, no padding
    (one sample more makes k + 1 frames)."""
    return FRAME + STEP * (k - 1)


def _noise(rng, n, scale=3000.0):
    return np.clip(rng.normal(size=n) * scale, -32768, 32767).astype(np.int16)


def _speech_like(rng, n):
    """Noise under a decaying tone, so that neighbouring frames and columns differ."""
    t = np.arange(n) / 16000.0
    tone = 4000 * np.sin(2 * np.pi * (180 + 40 * rng.random()) * t) * np.exp(-t)
    return np.clip(rng.normal(size=n) * 1500 + tone, -32768, 32767).astype(np.int16)


def _raw_reference(pcm, feature_type, drop):
    """float64 features of one row, cast to float32, every second frame dropped if asked."""
    pcm = np.asarray(pcm, dtype=np.int16)
    feat = ofeat.mfcc_with_delta(pcm) if feature_type == 'mfcc' else ofeat.log_mel(pcm)
    raw = feat.astype(np.float32)
    return raw[::2] if drop else raw


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def _raw_bar(raw):
    """Before normalisation.  The kernels stay in float64 until the final cast, so the kernel's
    value and the oracle's are two roundings of float64 numbers ~1e-13 apart: at most 1 ulp
    apart.  4 ulp + 1e-6 leaves room (the 1e-6 covers cepstra near 0, whose float64 sums of
    80 terms of ~30 carry ~1e-13 absolute)."""
    return 4 * _ulp(raw) + 1e-6


def _normalized(raw, norm):
    """(reference in float64, std per column [80], bar per element) for 'local' / 'local_scalar'.

    Error propagation: out = (v - mean) / std.  The kernel's v is within 1 ulp(|v|) of the
    oracle's, and its float32 mean within 1/2 ulp(|mean|); both errors reach the output divided
    by std.  The subtraction and the product by the float32 1/std add ~1.5 ulp(|out|).  So the
    bar is 4 ulp(max |v| of the column or matrix) / std + 4 ulp(|out|) + 1e-6."""
    r = raw.astype(np.float64)
    if norm == 'local':
        mean, std = r.mean(axis=0), r.std(axis=0)
        scale = np.abs(r).max(axis=0)
    else:
        mean, std = r.mean(), r.std()
        scale = np.abs(r).max()
        std, scale = np.full(r.shape[1], std), np.full(r.shape[1], scale)
    with np.errstate(divide='ignore', invalid='ignore'):
        ref = (r - mean) / std
        bar = 4 * _ulp(scale) / std + 4 * _ulp(np.nan_to_num(ref)) + 1e-6
    return ref, std, bar


def _check_row(group, got, got_len, pcm, feature_type, norm, drop, expect_len=None):
    """One output row [out_frames, 80] against the reference of its pcm: length, the valid
    frames inside their bars, constant columns all NaN, padding frames exactly 0.
    Returns the number of columns compared at the bar (normalised) or 80."""
    n = len(pcm)
    raw = _raw_reference(pcm, feature_type, drop)
    assert raw.shape[0] == kept(n, drop) == (expect_len or raw.shape[0])
    assert int(got_len) == raw.shape[0], (n, int(got_len), raw.shape[0])
    valid = got[:raw.shape[0]].astype(np.float64)
    assert (got[raw.shape[0]:] == 0).all(), (n, 'padding frames are not 0')
    if norm == 'none':
        err, bar = np.abs(valid - raw), _raw_bar(raw)
        _record(group, err.max(), (err / bar).max())
        assert (err <= bar).all(), (n, err.max(), np.unravel_index(np.argmax(err / bar), err.shape))
        return raw.shape[1]
    ref, std, bar = _normalized(raw, norm)
    constant = std == 0
    assert np.isnan(valid[:, constant]).all(), (n, 'constant column not NaN')
    assert np.isfinite(valid[:, ~constant]).all(), (n, 'non-constant column not finite')
    # columns whose std is too small for the ceiling (bar > 1e-3) are not a parity case
    use = ~constant & (bar.max(axis=0) <= CEILING)
    if use.any():
        err = np.abs(valid[:, use] - ref[:, use])
        _record(group, err.max(), (err / bar[:, use]).max())
        assert (err <= bar[:, use]).all(), (n, err.max())
    return int(use.sum())


def _features(hip, pcm_rows, lengths, feature_type, norm, drop, max_samples=None,
              out_frames=None, poison=False):
    """hip.features on a padded batch; with `poison`, out / out_len start as NaN / garbage and
    the workspace block is (best effort) a freshly freed NaN-filled one.  Returns host arrays."""
    lengths = np.asarray(lengths, dtype=np.int64)
    if max_samples is None:
        max_samples = max(len(p) for p in pcm_rows)
    pcm = np.zeros((len(pcm_rows), max_samples), dtype=np.int16)
    for b, p in enumerate(pcm_rows):
        pcm[b, :min(len(p), max_samples)] = p[:max_samples]
    kept_max = kept(max_samples, drop)
    out = out_len = None
    if out_frames is not None or poison:
        out_frames = kept_max if out_frames is None else out_frames
        out = torch.full((len(pcm_rows), out_frames, 80), float('nan'), device=DEV)
        out_len = torch.full((len(pcm_rows),), -12345, dtype=torch.int32, device=DEV)
    pcm_d = torch.from_numpy(pcm).to(DEV)
    len_d = torch.from_numpy(lengths.astype(np.int32)).to(DEV)
    if poison:
        # best effort: the caching allocator usually hands this block straight back to the
        # wrapper's workspace allocation of the same size
        nbytes = max(int(hip.load().ctcasr_features_workspace_bytes(len(pcm_rows),
                                                                   max_samples)), 256)
        junk = torch.full((nbytes // 4,), float('nan'), device=DEV)
        del junk
    out, out_len = hip.features(pcm_d, len_d, feature_type, norm, drop, out=out, out_len=out_len)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_len.cpu().numpy()


SEAM_LENGTHS = [1, 2, 159, 160, 399, 400, 401, 402, 559, 560, 561, 720, 721, 880, 881, 1040,
                1041]
# the tight length for k frames and one sample more, on both sides of the statistics stride
STRIDE_KS = [2, 3, 11, 12, 13, STATS_STRIDE - 1, STATS_STRIDE, STATS_STRIDE + 1,
             2 * STATS_STRIDE, 2 * STATS_STRIDE + 1]
STRIDE_LENGTHS = sorted({n for k in STRIDE_KS for n in (tight(k), tight(k) + 1)})


def test_frame_counts_match_the_oracle(hip):
    for n in SEAM_LENGTHS + STRIDE_LENGTHS:
        assert hip.features_num_frames(n) == ofeat.num_frames(n) == frames(n), n


@pytest.mark.parametrize('feature_type', ['mel', 'mfcc'])
@pytest.mark.parametrize('norm', ['none', 'local', 'local_scalar'])
@pytest.mark.parametrize('drop', [False, True])
def test_frame_count_seams(hip, feature_type, norm, drop):
    rng = np.random.default_rng(100)
    lengths = SEAM_LENGTHS + STRIDE_LENGTHS
    rows = [_speech_like(rng, n) for n in lengths]
    # all lengths in one ragged batch, the buffer a few samples longer than the longest row
    out, out_len = _features(hip, rows, lengths, feature_type, norm, drop,
                             max_samples=max(lengths) + 7)
    for b, n in enumerate(lengths):
        _check_row('seams', out[b], out_len[b], rows[b], feature_type, norm, drop)
    # each length alone in a buffer of exactly its size: the last frame ends at the buffer end
    for n, row in zip(lengths, rows):
        out1, len1 = _features(hip, [row], [n], feature_type, norm, drop)
        _check_row('seams', out1[0], len1[0], row, feature_type, norm, drop)


@pytest.mark.parametrize('feature_type', ['mel', 'mfcc'])
@pytest.mark.parametrize('norm', ['local', 'local_scalar'])
@pytest.mark.parametrize('drop', [False, True])
def test_normalisation_at_two_and_three_frames(hip, feature_type, norm, drop):
    """The case test_features_match_oracle skips: 'local' / 'local_scalar' at kept = 2 and 3."""
    rng = np.random.default_rng(200)
    if drop:                               # 3-4 frames keep 2, 5-6 frames keep 3
        lengths = [561, 720, 721, 880, 881, 1040, 1041, 1200]
    else:
        lengths = [401, 480, 560, 561, 640, 720]
    rows = [_speech_like(rng, n) for n in lengths] + [_noise(rng, n, 9000) for n in lengths]
    out, out_len = _features(hip, rows, lengths + lengths, feature_type, norm, drop)
    compared = 0
    for b, row in enumerate(rows):
        assert kept(len(row), drop) in (2, 3)
        compared += _check_row('few_frames', out[b], out_len[b], row, feature_type, norm, drop)
    # most columns are well conditioned; at kept = 2 the mfcc deltas are constant (NaN)
    assert compared >= len(rows) * (30 if feature_type == 'mfcc' else 60), compared


# long ones too: a sum of squares of one float32 value is exact in float64 over a few dozen
# rows, so the rounding that made constant columns come out 0 instead of NaN needs length
SILENT_LENGTHS = [1, 399, 400, 401, 561, 1041, tight(STATS_STRIDE) + 1, 16000, 40000, 160000,
                  272000]


@pytest.mark.parametrize('feature_type', ['mel', 'mfcc'])
@pytest.mark.parametrize('drop', [False, True])
def test_constant_columns(hip, feature_type, drop):
    """A column constant over the kept frames has std 0: the reference divides by it and gives
    NaN; so must the kernel, at every length ('local'), and for a constant matrix
    ('local_scalar').  Digital silence makes every frame log(eps); one kept frame makes every
    column constant.  (A DC signal would not do: pre-emphasis makes its first frame and its
    zero-padded last frame differ from the rest.)"""
    rng = np.random.default_rng(300)
    one_frame = [n for n in (1, 160, 400, 401, 560) if kept(n, drop) == 1]
    speech_n = [16000, 3001]
    rows = ([np.zeros(n, dtype=np.int16) for n in SILENT_LENGTHS] +
            [_speech_like(rng, n) for n in one_frame] + [_speech_like(rng, n) for n in speech_n])
    lengths = [len(r) for r in rows]
    silent = range(len(SILENT_LENGTHS))
    single = range(len(SILENT_LENGTHS), len(SILENT_LENGTHS) + len(one_frame))
    for norm in ('none', 'local', 'local_scalar'):
        out, out_len = _features(hip, rows, lengths, feature_type, norm, drop, poison=True)
        for b, row in enumerate(rows):
            _check_row('constant', out[b], out_len[b], row, feature_type, norm, drop)
            valid = out[b, :out_len[b]]
            if norm == 'local' and (b in silent or b in single):
                assert np.isnan(valid).all(), (norm, len(row))
            if norm == 'local_scalar' and b in silent and feature_type == 'mel':
                assert np.isnan(valid).all(), (norm, len(row))
            if norm == 'none' and b in silent:
                if feature_type == 'mel':
                    assert (valid == LOG_EPS).all(), len(row)
                else:
                    assert (valid[:, 0] == LOG_EPS).all(), len(row)
            if b >= len(SILENT_LENGTHS) + len(one_frame):
                assert np.isfinite(valid).all(), (norm, len(row))


@pytest.mark.parametrize('drop', [False, True])
def test_mfcc_deltas_at_one_to_five_frames(hip, drop):
    """Deltas over +-2 frames with the edges clamped: at 1-5 frames the clamp is most or all
    of the result.  They are taken before the drop, as in the reference."""
    rng = np.random.default_rng(400)
    lengths = [300, 400, 401, 560, 561, 720, 721, 880, 881, 1040, tight(10), tight(11)]
    rows = [_speech_like(rng, n) for n in lengths]
    out, out_len = _features(hip, rows, lengths, 'mfcc', 'none', drop, poison=True)
    for b, row in enumerate(rows):
        _check_row('deltas', out[b], out_len[b], row, 'mfcc', 'none', drop)
    if drop:
        # the test tells the two orders apart: deltas of the dropped cepstra are different
        full = ofeat.mfcc_with_delta(rows[-1])
        after = ofeat.delta(full[::2, :40], 2).astype(np.float32)
        assert np.abs(after - out[len(rows) - 1, :out_len[-1], 40:]).max() > 1e-2


def _signals(rng):
    n = 16000
    out = {}
    x = _speech_like(rng, n)
    for name, (lo, hi) in {'silent_start': (0, 3000), 'silent_middle': (6000, 9100),
                           'silent_end': (12500, n)}.items():
        y = x.copy()
        y[lo:hi] = 0
        out[name] = y
    square = np.where((np.arange(n) // 20) % 2 == 0, 32767, -32768).astype(np.int16)
    out['square_full_scale'] = square
    out['square_period_2'] = np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)
    out['clipped_noise'] = np.clip(rng.normal(size=n) * 40000, -32768, 32767).astype(np.int16)
    for off in (0, 1, 2, 3, 127, 128, 129, 200, 255, 256, 257, 383, 398, 399):
        y = np.zeros(4000, dtype=np.int16)
        y[STEP * 10 + off] = 32767 if off % 2 else -32768
        out['impulse_{}'.format(off)] = y
    t = np.arange(n) / 16000.0
    for hz in (1000.0, 500.0, 4000.0, 15.625 * 511):             # bins 64, 32, 256, 511
        out['tone_{:g}'.format(hz)] = np.round(20000 * np.cos(2 * np.pi * hz * t)).astype(np.int16)
    out['dc_offset'] = np.clip(30000 + rng.normal(size=n) * 50, -32768, 32767).astype(np.int16)
    return out


@pytest.mark.parametrize('feature_type', ['mel', 'mfcc'])
@pytest.mark.parametrize('norm', ['none', 'local'])
def test_signals(hip, feature_type, norm):
    sig = _signals(np.random.default_rng(500))
    names = sorted(sig)
    rows = [sig[k] for k in names]
    out, out_len = _features(hip, rows, [len(r) for r in rows], feature_type, norm, False)
    for b, name in enumerate(names):
        _check_row('signals', out[b], out_len[b], rows[b], feature_type, norm, False)
        if norm == 'none' and feature_type == 'mel':
            raw = _raw_reference(rows[b], 'mel', False)
            silent = (raw == LOG_EPS).all(axis=1)
            if name.startswith(('silent', 'impulse')):
                assert silent.any(), name
            assert (out[b, :out_len[b]][silent] == LOG_EPS).all(), name


@pytest.mark.parametrize('batch', [1, 2, 63, 64, 65])
@pytest.mark.parametrize('feature_type', ['mel', 'mfcc'])
def test_ragged_batches_match_single_rows_bitwise(hip, batch, feature_type):
    rng = np.random.default_rng(600 + batch)
    max_samples = 24000
    lengths = rng.integers(1, max_samples + 1, size=batch)
    short = rng.random(batch) < 0.3                      # far shorter than max_samples
    lengths[short] = rng.integers(1, 1200, size=int(short.sum()))
    lengths[0] = max_samples if batch > 1 else 9000      # B = 1: shorter than its buffer
    if batch > 2:
        lengths[1], lengths[2] = 1, 401
    rows = [_speech_like(rng, int(n)) for n in lengths]
    for norm, drop in (('local', False), ('none', True), ('local_scalar', True)):
        out, out_len = _features(hip, rows, lengths, feature_type, norm, drop,
                                 max_samples=max_samples, poison=True)
        for b, row in enumerate(rows):
            _check_row('batches', out[b], out_len[b], row, feature_type, norm, drop)
            one, one_len = _features(hip, [row], [len(row)], feature_type, norm, drop)
            assert one_len[0] == out_len[b]
            k = int(out_len[b])
            # bitwise, NaN included: the row's result does not depend on its neighbours,
            # on B or on max_samples
            assert np.array_equal(out[b, :k].view(np.int32), one[0, :k].view(np.int32)), b


@pytest.mark.parametrize('feature_type', ['mel', 'mfcc'])
@pytest.mark.parametrize('norm', ['none', 'local'])
@pytest.mark.parametrize('drop', [False, True])
def test_output_bands_and_garbage_buffers(hip, feature_type, norm, drop):
    """out_frames beyond kept_max and kept counts around the 16 output bands, with out,
    out_len and (best effort) the workspace starting full of NaN / garbage."""
    rng = np.random.default_rng(700)
    ks = [NORM_SPLIT - 1, NORM_SPLIT, NORM_SPLIT + 1, 2 * NORM_SPLIT, 2 * NORM_SPLIT + 1]
    lengths = [tight(2 * k - 1) if drop else tight(k) for k in ks] + [777]
    rows = [_speech_like(rng, n) for n in lengths]
    kept_max = kept(max(lengths), drop)
    assert kept_max == 2 * NORM_SPLIT + 1
    for extra in (0, 1, 15, 16, 17):
        out, out_len = _features(hip, rows, lengths, feature_type, norm, drop,
                                 out_frames=kept_max + extra, poison=True)
        assert out.shape[1] == kept_max + extra
        for b, row in enumerate(rows):
            _check_row('bands', out[b], out_len[b], row, feature_type, norm, drop)


def test_sampling_rates_other_than_16k_are_refused(hip, monkeypatch):
    """Frame length 400 / step 160 are 25 ms / 10 ms at 16 kHz only; any other rate is refused
    rather than giving wrong features."""
    rng = np.random.default_rng(800)
    pcm = torch.from_numpy(_noise(rng, 4000)[None]).to(DEV)
    n = torch.tensor([4000], dtype=torch.int32, device=DEV)
    for rate in (8000, 22050, 16001):
        with pytest.raises(hip.CtcAsrError, match='features_init_tables'):
            hip.features(pcm, n, 'mel', 'local', False, rate)
    out, out_len = hip.features(pcm, n, 'mel', 'local', False, 16000)
    assert int(out_len[0]) == frames(4000)
    from ctc_asr_amd import input_functions
    from ctc_asr_amd.params import FLAGS
    monkeypatch.setattr(FLAGS, 'sampling_rate', 8000)
    with pytest.raises(hip.CtcAsrError):
        input_functions.features_from_pcm([_noise(rng, 4000)])


BAD_LENGTHS = [0, -5, 'max+1', 2 ** 31 - 1]


@pytest.mark.parametrize('bad', BAD_LENGTHS)
@pytest.mark.parametrize('feature_type', ['mel', 'mfcc'])
@pytest.mark.parametrize('norm', ['none', 'local', 'local_scalar'])
def test_rows_outside_one_to_max_samples_are_refused(hip, bad, feature_type, norm):
    """A row with num_samples < 1 or > max_samples reads none of its PCM: out_len 0, all-zero
    output rows, and its neighbours come out bitwise as in a batch without it."""
    rng = np.random.default_rng(900)
    max_samples = 5000
    bad = max_samples + 1 if bad == 'max+1' else bad
    good = [_speech_like(rng, n) for n in (5000, 1234, 401, 4321)]
    good_len = [len(r) for r in good]
    # the bad row's PCM is full scale, so that a read of it would show
    loud = np.full(max_samples, 32767, dtype=np.int16)
    for drop in (False, True):
        ref, ref_len = _features(hip, good, good_len, feature_type, norm, drop,
                                 max_samples=max_samples)
        for where in (2, len(good)):              # in the middle, and as the last row
            rows = good[:where] + [loud] + good[where:]
            lengths = good_len[:where] + [bad] + good_len[where:]
            out, out_len = _features(hip, rows, lengths, feature_type, norm, drop,
                                     max_samples=max_samples, poison=True)
            assert out_len[where] == 0 and (out[where] == 0).all(), (bad, where)
            others = [b for b in range(len(rows)) if b != where]
            assert out_len[others].tolist() == ref_len.tolist()
            for b_ref, b in enumerate(others):
                k = int(ref_len[b_ref])
                assert np.array_equal(out[b].view(np.int32), ref[b_ref].view(np.int32)), b
                _check_row('refusals', out[b], out_len[b], good[b_ref], feature_type, norm,
                           drop, expect_len=k)
