"""CTC forced alignment of one long sequence (csrc/ctc_align_long.hip, `hip.ctc_align_long`) on
the MI355X.

The kernel's arithmetic is K11's operation for operation, and max and add do not depend on how
the lattice is tiled.  So everything here is compared for EQUAL BITS: with `hip.ctc_align` where
both kernels serve, with `tests.align_long_reference.on_table` (the float64 reference run on the
device's own fp32 table) everywhere, across every ``tile_frames``, and across reuses of one
workspace.  The one tolerance is the table's: 1e-5 against the float64 log-softmax, the bound
tests/test_gpu_align.py holds K11's frame_logp to on the same N(0, 2) logits.

Shapes derive from the tile width TS = hip.ALIGN_LONG_TILE_STATES: label lengths that put the
last state, a blank, and a label state first in a tile column; frame counts from the tight bound
(one path only, s = 2t + 1, every column seam crossed by a skip) to past 2S; tile heights 1, 2, 3,
64, the default and one above T.  The argument checks at the end need no device.
"""

import ctypes

import numpy as np
import pytest
import torch

from oracle import ctc as octc
from tests import align_long_reference as lref

gpu = pytest.mark.gpu
DEV = 'cuda'


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _run(hip, logits, label, blank=None, tile_frames=0, **kw):
    """The wrapper on host arrays -> host (path, score float64, frame_logp, logp, status int)."""
    path, score, frame_logp, logp, status = hip.ctc_align_long(
        _t(logits), _t(np.asarray(label, dtype=np.int32), torch.int32), blank=blank,
        tile_frames=tile_frames, logp=True, **kw)
    return (path.cpu().numpy(), score.cpu().numpy()[0], frame_logp.cpu().numpy(),
            logp.cpu().numpy(), int(status.cpu().numpy()[0]))


def _labels(rng, length, classes, blank, repeat_p):
    ids = [c for c in range(classes) if c != blank]
    out = []
    for _ in range(length):
        if out and rng.random() < repeat_p:
            out.append(out[-1])
        else:
            out.append(int(rng.choice([c for c in ids if not out or c != out[-1]] or ids)))
    return out


def _assert_equals_reference(result, want, what):
    path, score, frame_logp, _, status = result
    assert status == 0, what
    assert lref.same_bits(path, want[1]), what
    assert lref.same_bits(np.float64(score), want[0]), (what, score, want[0])
    assert lref.same_bits(frame_logp, want[2]), what


# ------------------------------------------------------------------------------------------------
# 1. Same as K11 where both serve
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('classes,blank', [(2, 1), (29, 28), (64, 63), (29, 5)])
def test_equals_k11_bit_for_bit_where_both_serve(hip, classes, blank):
    rng = np.random.default_rng(100 + classes + blank)
    for num_labels in (0, 1, 2, 31, 32, 33, 575):
        label = _labels(rng, num_labels, classes, blank, 0.2)
        for num_steps in (1, 2, 3, 63, 64, 65, 300):
            num_steps = max(num_steps, lref.required_time(label))
            logits = (rng.normal(size=(num_steps, classes)) * 2.0).astype(np.float32)
            k_path, k_score, k_flp, k_status = hip.ctc_align(
                _t(logits.reshape(num_steps, 1, classes)),
                _t(label + [0], torch.int32),          # (never empty: K11 wants an address)
                _t([0, num_labels], torch.int32), _t([num_steps], torch.int32),
                max(num_labels, 1), blank=blank)
            k_path, k_flp = k_path.cpu().numpy()[0], k_flp.cpu().numpy()[0]
            k_score, k_status = k_score.cpu().numpy()[0], int(k_status.cpu().numpy()[0])
            assert k_status == 0
            for tile_frames in (1, 2, 7, 64, 0):
                what = (num_labels, num_steps, tile_frames)
                path, score, flp, _, status = _run(hip, logits, label, blank, tile_frames)
                assert status == k_status, what
                assert lref.same_bits(path, k_path), what
                assert lref.same_bits(flp, k_flp), what
                assert lref.same_bits(np.float32(score), k_score), (what, score, k_score)


# ------------------------------------------------------------------------------------------------
# 2. The table
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('classes', [2, 29, 64])
def test_table_is_the_log_softmax_and_the_same_for_every_tile_height(hip, classes):
    rng = np.random.default_rng(200 + classes)
    num_steps, blank = 333, classes - 1
    label = _labels(rng, 40, classes, blank, 0.1)
    num_steps = max(num_steps, lref.required_time(label))
    logits = (rng.normal(size=(num_steps, classes)) * 2.0).astype(np.float32)
    want = octc.log_softmax(logits.astype(np.float64))
    first = None
    for tile_frames in (0, 1, 2, 7, 64, num_steps + 5):
        logp = _run(hip, logits, label, blank, tile_frames)[3]
        assert logp.shape == (num_steps, classes)
        assert np.abs(logp - want).max() <= 1e-5, tile_frames
        first = logp if first is None else first
        assert lref.same_bits(logp, first), tile_frames


# ------------------------------------------------------------------------------------------------
# 3. Seams, against the reference on the device's own table
# ------------------------------------------------------------------------------------------------
def _seam_lengths(hip):
    ts = hip.ALIGN_LONG_TILE_STATES
    return [ts // 2 - 1, ts // 2, ts // 2 + 1, ts - 1, ts, ts + 1, 3 * ts // 2]


@gpu
@pytest.mark.parametrize('which', range(7))
@pytest.mark.parametrize('repeat_p', [0.0, 0.15])
def test_tile_seams_equal_the_reference_on_the_device_table(hip, which, repeat_p):
    num_labels = _seam_lengths(hip)[which]
    rng = np.random.default_rng(300 + which + int(repeat_p * 100))
    classes, blank = 29, 28
    label = _labels(rng, num_labels, classes, blank, repeat_p)
    tight, states = lref.required_time(label), 2 * num_labels + 1
    assert (tight == num_labels) == (repeat_p == 0.0)
    for num_steps in (tight, tight + 1, num_labels + num_labels // 2 + 3, 2 * states + 5):
        num_steps = max(num_steps, tight)
        logits = (rng.normal(size=(num_steps, classes)) * 2.0).astype(np.float32)
        want = None
        for tile_frames in (0, 1, 2, 3, 64, num_steps + 1):
            result = _run(hip, logits, label, blank, tile_frames)
            if want is None:
                want = lref.on_table(result[3], label, blank)
            _assert_equals_reference(result, want, (num_labels, num_steps, tile_frames))


@gpu
def test_tight_bound_without_repeats_crosses_every_column_seam_by_a_skip(hip):
    """T = L and no repeats: the only path is s = 2t + 1.  It enters tile column j at state
    j * TS + 1 from state j * TS - 1: a skip across the seam, at frame j * TS / 2.  With
    tile_frames dividing TS / 2 that is the FIRST frame of a tile row: the value comes from the
    diagonal neighbour (i - 1, j - 1)."""
    ts = hip.ALIGN_LONG_TILE_STATES
    rng = np.random.default_rng(31)
    classes, blank = 29, 28
    num_labels = 3 * ts // 2 + 7
    label = _labels(rng, num_labels, classes, blank, 0.0)
    assert lref.required_time(label) == num_labels
    logits = (rng.normal(size=(num_labels, classes)) * 2.0).astype(np.float32)
    want = None
    for tile_frames in (ts // 2, ts // 4, 64, 1, 2, 3, 0, num_labels):
        result = _run(hip, logits, label, blank, tile_frames)
        if want is None:
            want = lref.on_table(result[3], label, blank)
        _assert_equals_reference(result, want, tile_frames)
        assert result[0].tolist() == [2 * t + 1 for t in range(num_labels)], tile_frames
    for j in (1, 2, 3):                     # the seams it crossed, and how
        t = j * ts // 2
        assert want[1][t - 1] == j * ts - 1 and want[1][t] == j * ts + 1


@gpu
def test_repeated_label_straddling_a_column_seam_forbids_the_skip(hip):
    """Labels TS/2 - 1 and TS/2 are equal: states TS - 1 and TS + 1 sit on both sides of the seam
    between columns 0 and 1, and the skip between them is forbidden.  The logits make the skip
    the tempting move: the blank is hopeless in every frame."""
    ts = hip.ALIGN_LONG_TILE_STATES
    rng = np.random.default_rng(32)
    classes, blank = 29, 28
    num_labels = ts // 2 + 40
    label = _labels(rng, num_labels, classes, blank, 0.0)
    label[ts // 2] = label[ts // 2 - 1]
    label[ts // 2 + 1] = min(c for c in range(28)
                             if c not in (label[ts // 2], label[ts // 2 + 2]))
    assert lref.required_time(label) == num_labels + 1
    for num_steps in (num_labels + 1, num_labels + 2, num_labels + 50):
        logits = (rng.normal(size=(num_steps, classes)) * 2.0).astype(np.float32)
        logits[:, blank] -= 30.0
        want = None
        for tile_frames in (0, 1, 2, 3, 64, num_steps):
            result = _run(hip, logits, label, blank, tile_frames)
            if want is None:
                want = lref.on_table(result[3], label, blank)
            _assert_equals_reference(result, want, (num_steps, tile_frames))
        path = want[1].tolist()
        assert ts in path                    # the blank between the two equal labels is taken
        assert path[path.index(ts) - 1] == ts - 1 and ts + 1 in path


# ------------------------------------------------------------------------------------------------
# 4. Rows without a path; every output written over garbage
# ------------------------------------------------------------------------------------------------
def _raw(hip, logits, label, blank, tile_frames=0, workspace=None):
    """The C ABI on outputs pre-filled with garbage -> host (code, path, score, frame_logp, logp,
    status)."""
    num_steps, classes = logits.shape
    path = torch.full((num_steps,), 123456, dtype=torch.int32, device=DEV)
    flp = torch.full((num_steps,), 7.5, dtype=torch.float32, device=DEV)
    logp = torch.full((num_steps, classes), 7.5, dtype=torch.float32, device=DEV)
    score = torch.full((1,), 7.5, dtype=torch.float64, device=DEV)
    status = torch.full((1,), 99, dtype=torch.int32, device=DEV)
    need = hip.ctc_align_long_workspace_bytes(num_steps, classes, len(label), tile_frames)
    assert need > 0
    if workspace is None:
        workspace = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    x, lab = _t(logits), _t(np.asarray(label, dtype=np.int32), torch.int32)
    code = hip.load().ctcasr_ctc_align_long(
        x.data_ptr(), lab.data_ptr(), num_steps, classes, blank, len(label), tile_frames,
        path.data_ptr(), score.data_ptr(), flp.data_ptr(), logp.data_ptr(), status.data_ptr(),
        workspace.data_ptr(), workspace.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (code, path.cpu().numpy(), score.cpu().numpy()[0], flp.cpu().numpy(),
            logp.cpu().numpy(), int(status.cpu().numpy()[0]))


@gpu
def test_sequences_without_a_path_write_every_output(hip):
    rng = np.random.default_rng(40)
    classes, blank, num_steps = 29, 28, 300
    logits = (rng.normal(size=(num_steps, classes)) * 2.0).astype(np.float32)
    nan_last = logits.copy()
    nan_last[num_steps - 1, 3] = np.nan          # last frame of the last tile row (64: 256..299)
    inf_first = logits.copy()
    inf_first[0, blank] = -np.inf
    long_label = _labels(rng, 301, classes, blank, 0.0)
    cases = [(logits, long_label, 1),                           # T < L
             (logits, [4] * 151, 1),                            # T < L + repeats (301 needed)
             (logits, [1, 2, 29], 2), (logits, [1, blank], 2), (logits, [-1], 2),
             (nan_last, long_label, 1),                         # 1 before 3, as K11
             (nan_last, [1, 2, 29], 2),                         # 2 before 3
             (nan_last, [1, 2, 3], 3), (inf_first, [], 3), (nan_last, long_label[:290], 3)]
    for x, label, want in cases:
        assert lref.expected_status(x, label, blank) == want
        for tile_frames in (64, 0, 1):
            code, path, score, flp, _, status = _raw(hip, x, label, blank, tile_frames)
            what = (label[:3], want, tile_frames)
            assert code == 0 and status == want, what
            assert (path == -1).all() and (flp == 0).all(), what
            assert np.isnan(score) if want == 3 else score == -np.inf, what


@gpu
def test_no_frames_and_no_labels_as_k11(hip):
    rng = np.random.default_rng(41)
    classes, blank = 29, 28
    empty = np.zeros((0, classes), dtype=np.float32)
    code, path, score, _, _, status = _raw(hip, empty, [], blank)
    assert (code, status, score, path.size) == (0, 0, 0.0, 0)        # K11: len 0, L 0 -> score 0
    code, _, score, _, _, status = _raw(hip, empty, [3], blank)
    assert (code, status) == (0, 1) and score == -np.inf             # K11: len 0 < L
    code, _, score, _, _, status = _raw(hip, empty, [blank], blank)
    assert (code, status) == (0, 2) and score == -np.inf
    for num_steps in (1, 5, 70):                                     # L = 0: all blank
        logits = rng.normal(size=(num_steps, classes)).astype(np.float32)
        code, path, score, flp, logp, status = _raw(hip, logits, [], blank, 3)
        assert (code, status) == (0, 0) and path.tolist() == [0] * num_steps
        assert lref.same_bits(flp, logp[:, blank])
        assert score == sum(float(v) for v in logp[:, blank])        # (sequential, as the lattice)
    logits = rng.normal(size=(1, classes)).astype(np.float32)
    code, path, score, flp, logp, status = _raw(hip, logits, [7], blank)
    assert (code, status) == (0, 0) and path.tolist() == [1] and score == np.float64(logp[0, 7])


@gpu
def test_outputs_are_fully_written_over_garbage(hip):
    rng = np.random.default_rng(42)
    classes, blank = 29, 28
    label = _labels(rng, hip.ALIGN_LONG_TILE_STATES // 2 + 9, classes, blank, 0.1)
    num_steps = lref.required_time(label) + 77
    logits = (rng.normal(size=(num_steps, classes)) * 2.0).astype(np.float32)
    for tile_frames in (0, 50):
        code, path, score, flp, logp, status = _raw(hip, logits, label, blank, tile_frames)
        assert code == 0
        want = lref.on_table(logp, label, blank)
        _assert_equals_reference((path, score, flp, logp, status), want, tile_frames)
        assert not (logp == 7.5).any()


# ------------------------------------------------------------------------------------------------
# 5. One workspace, changing data
# ------------------------------------------------------------------------------------------------
@gpu
def test_one_workspace_serves_changing_calls_bit_for_bit(hip):
    rng = np.random.default_rng(50)
    classes, blank = 29, 28
    ts = hip.ALIGN_LONG_TILE_STATES
    long_label = _labels(rng, ts + 100, classes, blank, 0.1)
    short_label = _labels(rng, ts // 2 + 3, classes, blank, 0.1)
    long_steps = lref.required_time(long_label) + 500
    short_steps = (lref.required_time(short_label) + 100) | 1          # odd
    long_logits = (rng.normal(size=(long_steps, classes)) * 2.0).astype(np.float32)
    short_logits = (rng.normal(size=(short_steps, classes)) * 2.0).astype(np.float32)
    for tile_frames in (0, 37):
        fresh_long = _raw(hip, long_logits, long_label, blank, tile_frames)
        fresh_short = _raw(hip, short_logits, short_label, blank, tile_frames)
        assert fresh_long[0] == 0 and fresh_long[5] == 0 and fresh_short[5] == 0
        need = hip.ctc_align_long_workspace_bytes(long_steps, classes, len(long_label),
                                                  tile_frames)
        shared = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
        calls = [(long_logits, long_label, fresh_long), (short_logits, short_label, fresh_short),
                 (long_logits, long_label, fresh_long), (long_logits, long_label, fresh_long)]
        for x, label, fresh in calls:
            again = _raw(hip, x, label, blank, tile_frames, workspace=shared)
            assert again[0] == 0 and again[5] == 0
            for a, b in zip(again[1:5], fresh[1:5]):
                assert lref.same_bits(a, b), tile_frames
        want = lref.on_table(fresh_long[4], long_label, blank)
        _assert_equals_reference(fresh_long[1:], want, tile_frames)


# ------------------------------------------------------------------------------------------------
# 6. Arguments: checked before the device is touched, so these need no GPU
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from ctc_asr_amd import build, hip as module
    build.build(verbose=False)
    return module.load()


def _fake():
    return ctypes.addressof(ctypes.create_string_buffer(4096))


def _call(lib, num_steps=10, classes=29, blank=28, num_labels=3, tile_frames=0, nulls=(),
          workspace_bytes=None):
    buffers = [ctypes.create_string_buffer(4096) for _ in range(8)]
    names = ('logits', 'labels', 'path', 'score', 'frame_logp', 'logp', 'status', 'workspace')
    p = {name: None if name in nulls else ctypes.addressof(buf)
         for name, buf in zip(names, buffers)}
    if workspace_bytes is None:
        workspace_bytes = lib.ctcasr_ctc_align_long_workspace_bytes(num_steps, classes,
                                                                    num_labels, tile_frames)
    return lib.ctcasr_ctc_align_long(p['logits'], p['labels'], num_steps, classes, blank,
                                     num_labels, tile_frames, p['path'], p['score'],
                                     p['frame_logp'], p['logp'], p['status'], p['workspace'],
                                     workspace_bytes, None)


def test_bad_arguments_are_refused_before_the_device_is_touched(lib):
    bad, unsupported, short = -1, -2, -3
    for name in ('logits', 'labels', 'path', 'score', 'status'):
        assert _call(lib, nulls=(name,)) == bad, name
    assert _call(lib, num_steps=-1) == bad
    assert _call(lib, num_labels=-1) == bad
    assert _call(lib, classes=1, blank=0) == bad
    assert _call(lib, blank=29) == bad and _call(lib, blank=-1) == bad
    assert _call(lib, tile_frames=-1) == bad
    assert _call(lib, classes=65, blank=64) == unsupported
    assert _call(lib, num_steps=(1 << 22) + 1, workspace_bytes=1 << 40) == unsupported
    assert _call(lib, num_steps=1 << 21, num_labels=(1 << 20) + 1,
                 workspace_bytes=1 << 40) == unsupported
    assert _call(lib, num_steps=1 << 22, tile_frames=1, workspace_bytes=1 << 40) == unsupported
    need = lib.ctcasr_ctc_align_long_workspace_bytes(10, 29, 3, 0)
    assert need > 0
    assert _call(lib, workspace_bytes=need - 1) == short
    assert _call(lib, nulls=('workspace',)) == short
    assert _call(lib, nulls=('frame_logp', 'logp'), workspace_bytes=need - 1) == short


def test_workspace_bytes_is_host_arithmetic(lib):
    from ctc_asr_amd import hip
    ts, tf = hip.ALIGN_LONG_TILE_STATES, hip.ALIGN_LONG_TILE_FRAMES
    assert (ts, tf) == (1024, 256)
    size = lib.ctcasr_ctc_align_long_workspace_bytes
    # an hour at the ds2 frame rate: 2 bits per cell of the padded lattice dominate
    num_steps, num_labels, classes = 180000, 54000, 29
    cols = -(-(2 * num_labels + 1) // ts)
    rows = -(-num_steps // tf)
    need = size(num_steps, classes, num_labels, 0)
    floor = cols * num_steps * ts // 4 + rows * cols * ts * 8 + cols * num_steps * 8 + \
        num_steps * classes * 4
    assert floor <= need <= floor + 4096
    assert need < 6 << 30
    assert size(num_steps, classes, num_labels, tf) == need
    assert size(10, 65, 3, 0) == 0 and size(10, 29, (1 << 20) + 1, 0) == 0
    assert size(-1, 29, 3, 0) == 0 and size((1 << 22) + 1, 29, 3, 0) == 0
    assert size(0, 29, 0, 0) > 0


def test_a_need_above_max_workspace_bytes_raises_naming_both_numbers(lib):
    from ctc_asr_amd import hip
    logits = torch.zeros(5000, 29)
    labels = torch.zeros(2000, dtype=torch.int32)
    need = hip.ctc_align_long_workspace_bytes(5000, 29, 2000)
    with pytest.raises(ValueError, match='{}.*{}'.format(need, 1 << 20)):
        hip.ctc_align_long(logits, labels, max_workspace_bytes=1 << 20)
    with pytest.raises(hip.CtcAsrError, match='C = 65'):
        hip.ctc_align_long(torch.zeros(10, 65), labels[:3])
    with pytest.raises(hip.CtcAsrError):                 # enough room allowed: no CPU path
        hip.ctc_align_long(logits[:10], labels[:3])
