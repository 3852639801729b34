"""CTC forced alignment with wildcard spans (``ctcasr_ctc_align_partial``, K25, the WILD
instantiations of csrc/ctc_align_long.hip) on the MI355X.

Everything is compared for EQUAL BITS (`same_bits`): with `hip.ctc_align_long` where no wildcard
is among the labels, and with `tests.align_partial_reference.on_table` - the float64 reference on
the device's own fp32 table with a column of row maxima appended - everywhere else, across every
``tile_frames``.  tests/test_align_partial_host.py proves that reference against the enumeration
of all paths.

Shapes: N(0, 2) logits, C = 29 (2 and 64 once), TS = hip.ALIGN_LONG_TILE_STATES.  A thread owns
the labels 2 tid and 2 tid + 1 of its tile column, so a wildcard at an even label index is its
``lab_a`` and at an odd one its ``lab_b``; 31 | 32 lie inside a wavefront, 127 | 128 on both
sides of the seam between wavefronts, TS/2 - 1 | TS/2 | TS/2 + 1 around the seam between tile
columns.  Frame counts run from the tight bound, where every move is forced, upwards.
"""

import numpy as np
import pytest
import torch

from tests import align_long_reference as lref
from tests import align_partial_reference as pref

gpu = pytest.mark.gpu
DEV = 'cuda'
W = pref.WILDCARD


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _run(fn, logits, label, blank=None, tile_frames=0, **kw):
    """A wrapper on host arrays -> host (path, score float64, frame_logp, logp, status int)."""
    path, score, frame_logp, logp, status = fn(
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


def _logits(rng, num_steps, classes):
    return (rng.normal(size=(num_steps, classes)) * 2.0).astype(np.float32)


def _assert_equals_reference(result, want, what):
    path, score, frame_logp, _, status = result
    assert status == 0, what
    assert lref.same_bits(path, want[1]), what
    assert lref.same_bits(np.float64(score), want[0]), (what, score, want[0])
    assert lref.same_bits(frame_logp, want[2]), what


def _check_all_tile_heights(hip, logits, label, blank, heights, what):
    """One reference, on the table of the first call; every tile height must equal it.  Returns
    (the reference, the table)."""
    want = table = None
    for tile_frames in heights:
        result = _run(hip.ctc_align_partial, logits, label, blank, tile_frames)
        if want is None:
            table = result[3]
            want = pref.on_table(table, label, blank)
        assert lref.same_bits(result[3], table), (what, tile_frames)
        _assert_equals_reference(result, want, (what, tile_frames))
    return want, table


# ------------------------------------------------------------------------------------------------
# 1. Without a wildcard: K21, bit for bit
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('which', range(5))
def test_without_a_wildcard_every_output_equals_k21(hip, which):
    ts = hip.ALIGN_LONG_TILE_STATES
    num_labels = [0, 1, 33, ts // 2 + 1, ts + 1][which]
    rng = np.random.default_rng(100 + which)
    classes, blank = 29, 28
    label = _labels(rng, num_labels, classes, blank, 0.15)
    tight, states = max(lref.required_time(label), 1), 2 * num_labels + 1
    for num_steps in (tight, tight + 1, num_labels + num_labels // 2 + 3, 2 * states + 5):
        num_steps = max(num_steps, tight)
        logits = _logits(rng, num_steps, classes)
        for tile_frames in (1, 3, 64, 0):
            what = (num_labels, num_steps, tile_frames)
            want = _run(hip.ctc_align_long, logits, label, blank, tile_frames)
            got = _run(hip.ctc_align_partial, logits, label, blank, tile_frames)
            assert want[4] == 0 and got[4] == 0, what
            assert lref.same_bits(np.float64(got[1]), np.float64(want[1])), what
            for a, b in zip((got[0], got[2], got[3]), (want[0], want[2], want[3])):
                assert lref.same_bits(a, b), what


# ------------------------------------------------------------------------------------------------
# 2. Wildcards at the seams, against the reference on the device's own table
# ------------------------------------------------------------------------------------------------
def _seam_positions(hip, num_labels):
    ts = hip.ALIGN_LONG_TILE_STATES
    return [0, num_labels - 1, 31, 32, 127, 128, ts // 2 - 1, ts // 2, ts // 2 + 1]


@gpu
@pytest.mark.parametrize('which', range(9))
def test_one_wildcard_at_a_lane_wave_or_column_seam(hip, which):
    ts = hip.ALIGN_LONG_TILE_STATES
    num_labels = ts // 2 + 40                 # the last label sits in tile column 1
    k = _seam_positions(hip, num_labels)[which]
    rng = np.random.default_rng(200 + which)
    classes, blank = 29, 28
    label = _labels(rng, num_labels, classes, blank, 0.1)
    label[k] = W
    tight = pref.required_time(label)
    for num_steps in (tight, tight + 1, num_labels + num_labels // 2):
        logits = _logits(rng, num_steps, classes)
        want, table = _check_all_tile_heights(hip, logits, label, blank,
                                              (0, 1, 2, 3, 64, num_steps + 1), (k, num_steps))
        wild = pref.wildcard_frames(want[1], label)
        assert wild.any() and lref.same_bits(want[2][wild], table.max(axis=1)[wild])
        assert set(want[1][wild].tolist()) == {2 * k + 1}


@gpu
def test_both_ends_fifty_wildcards_and_a_transcript_that_is_one_wildcard(hip):
    ts = hip.ALIGN_LONG_TILE_STATES
    rng = np.random.default_rng(21)
    classes, blank = 29, 28
    # the first and the last label
    label = _labels(rng, ts // 2 + 40, classes, blank, 0.1)
    label[0] = label[-1] = W
    tight = pref.required_time(label)
    for num_steps in (tight, tight + 1, len(label) * 3 // 2):
        logits = _logits(rng, num_steps, classes)
        want, _ = _check_all_tile_heights(hip, logits, label, blank,
                                          (0, 1, 2, 3, 64, num_steps + 1), ('ends', num_steps))
        assert want[1][0] == 1 and want[1][-1] in (2 * len(label) - 1, 2 * len(label))
    # 50 wildcards spread over three tile columns, both parities
    label = _labels(rng, 3 * ts // 2, classes, blank, 0.1)
    spots = [7 + 30 * n + (n % 2) for n in range(50)]
    assert spots[-1] < len(label) and {s % 2 for s in spots} == {0, 1}
    for k in spots:
        label[k] = W
    tight = pref.required_time(label)
    for num_steps in (tight, tight + 1, len(label) * 3 // 2):
        logits = _logits(rng, num_steps, classes)
        want, _ = _check_all_tile_heights(hip, logits, label, blank,
                                          (0, 1, 2, 3, 64, num_steps + 1), ('fifty', num_steps))
        wild = pref.wildcard_frames(want[1], label)
        assert {int(s) >> 1 for s in want[1][wild]} == set(spots)
    # L = 1: the transcript is one wildcard
    for num_steps in (1, 2, 65, 300):
        logits = _logits(rng, num_steps, classes)
        want, table = _check_all_tile_heights(hip, logits, [W], blank,
                                              (0, 1, 2, 3, 64, num_steps + 1), ('one', num_steps))
        assert want[1][0] in (0, 1) and 1 in want[1]


@gpu
@pytest.mark.parametrize('classes,blank', [(2, 0), (64, 0), (64, 63)])
def test_two_classes_and_sixty_four_with_the_wildcard_beside_the_last_id(hip, classes, blank):
    """C = 64 is the limit and stays 64 REAL classes; the wildcard stands beside a label with the
    id 63 (the last column of the table) on both sides."""
    ts = hip.ALIGN_LONG_TILE_STATES
    rng = np.random.default_rng(22 + classes + blank)
    top = classes - 1 if blank != classes - 1 else classes - 2
    label = _labels(rng, ts // 2 + 9, classes, blank, 0.1)
    for k in (4, 131, ts // 2):
        label[k - 1], label[k], label[k + 1] = top, W, top
    tight = pref.required_time(label)
    for num_steps in (tight, tight + 1, tight + len(label) // 2):
        logits = _logits(rng, num_steps, classes)
        _check_all_tile_heights(hip, logits, label, blank, (0, 1, 3, 64, num_steps + 1),
                                (classes, num_steps))


# ------------------------------------------------------------------------------------------------
# 3. The tight bound: one path only, every column seam crossed by a skip
# ------------------------------------------------------------------------------------------------
@gpu
def test_tight_bound_crosses_column_seams_by_skips_into_and_out_of_wildcards(hip):
    """T = L, no repeats: the only path is s = 2t + 1.  The wildcards at TS/2 and TS are the FIRST
    label of tile columns 1 and 2: the path skips into them across the seam, from state
    j TS - 1 to j TS + 1, and out of them by the next skip."""
    ts = hip.ALIGN_LONG_TILE_STATES
    rng = np.random.default_rng(31)
    classes, blank = 29, 28
    num_labels = 3 * ts // 2 + 7
    label = _labels(rng, num_labels, classes, blank, 0.0)
    label[ts // 2] = label[ts] = W
    assert pref.required_time(label) == num_labels
    logits = _logits(rng, num_labels, classes)
    want, table = _check_all_tile_heights(hip, logits, label, blank,
                                          (ts // 2, ts // 4, 64, 1, 2, 3, 0, num_labels), 'tight')
    assert want[1].tolist() == [2 * t + 1 for t in range(num_labels)]
    fill = table.max(axis=1)
    for k in (ts // 2, ts):
        assert want[2][k] == fill[k]
    # the same with the wildcards as the LAST label of columns 0 and 1
    label = _labels(rng, num_labels, classes, blank, 0.0)
    label[ts // 2 - 1] = label[ts - 1] = W
    want, _ = _check_all_tile_heights(hip, logits, label, blank, (ts // 2, 64, 1, 3, 0), 'tight-b')
    assert want[1].tolist() == [2 * t + 1 for t in range(num_labels)]


# ------------------------------------------------------------------------------------------------
# 4. Planted logits: the wildcards take the junk, the words land in their spans
# ------------------------------------------------------------------------------------------------
@gpu
def test_planted_junk_goes_to_the_wildcards_and_the_score_is_the_greedy_sum(hip):
    classes, blank = 29, 28
    word_a, word_b = [2, 3, 4], [9, 10]
    junk = ([15, 16, 17, 15], [20, 21], [24, 25, 26])
    frames, owner = [], []                   # the greedy class of each frame, and what planted it
    for name, ids in (('j0', junk[0]), ('a', word_a), ('j1', junk[1]), ('b', word_b),
                      ('j2', junk[2])):
        for sym in ids:
            frames += [sym, sym, blank, blank]
            owner += [name] * 4
    num_steps = len(frames)
    assert 56 <= num_steps <= 80
    logits = np.zeros((num_steps, classes), dtype=np.float32)
    logits[np.arange(num_steps), frames] = 8.0
    label = [W] + word_a + [W] + word_b + [W]
    for tile_frames in (0, 1, 7):
        path, score, flp, table, status = _run(hip.ctc_align_partial, logits, label, blank,
                                               tile_frames)
        assert status == 0
        want = pref.on_table(table, label, blank)
        _assert_equals_reference((path, score, flp, table, status), want, tile_frames)
        fill = table.max(axis=1)
        assert lref.same_bits(np.float64(score), np.cumsum(fill.astype(np.float64))[-1])
        assert lref.same_bits(flp, fill)
        wild = pref.wildcard_frames(path, label)
        for t in range(num_steps):
            s = int(path[t])
            if s & 1 and not wild[t]:        # a label of A or B: inside its planted span
                assert owner[t] == ('a' if (s >> 1) <= len(word_a) else 'b'), t
            if owner[t].startswith('j') and frames[t] != blank:
                assert wild[t], t            # a junk label frame: inside a wildcard
        assert {int(s) for s in path[wild]} == {1, 9, 15}


# ------------------------------------------------------------------------------------------------
# 5. Status, garbage, one workspace
# ------------------------------------------------------------------------------------------------
def _raw(hip, logits, label, blank, tile_frames=0, workspace=None, entry='ctcasr_ctc_align_partial'):
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
    code = getattr(hip.load(), entry)(
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
    logits = _logits(rng, num_steps, classes)
    nan_last = logits.copy()
    nan_last[num_steps - 1, 3] = np.nan
    long_label = _labels(rng, 301, classes, blank, 0.0)
    long_label[0] = long_label[150] = long_label[300] = W
    repeats = [W] + [4] * 150                                   # 151 labels + 149 repeats: 300
    cases = [(logits, [3, W, W, 4], 2), (logits, [W, W], 2),    # two wildcards side by side
             (logits, [W, -2], 2), (logits, [W, 29], 2), (logits, [1, W, blank], 2),
             (logits, long_label, 1),                           # T < L, wildcards count
             (logits, repeats + [4], 1),                        # T < L + repeats (302 needed)
             (nan_last, long_label, 1),                         # 1 before 3
             (nan_last, [W, W], 2), (nan_last, [W, -2], 2),     # 2 before 3
             (nan_last, [W, 1, W], 3), (nan_last, [W], 3), (nan_last, repeats, 3)]
    for x, label, want in cases:
        assert pref.expected_status(x, label, blank) == want
        for tile_frames in (64, 0, 1):
            code, path, score, flp, _, status = _raw(hip, x, label, blank, tile_frames)
            what = (label[:4], want, tile_frames)
            assert code == 0 and status == want, what
            assert (path == -1).all() and (flp == 0).all(), what
            assert np.isnan(score) if want == 3 else score == -np.inf, what
    # exactly enough frames: a wildcard is a label and no repeat
    assert pref.expected_status(logits, repeats, blank) == 0
    code, path, score, flp, logp, status = _raw(hip, logits, repeats, blank, 64)
    assert (code, status) == (0, 0)
    _assert_equals_reference((path, score, flp, logp, status),
                             pref.on_table(logp, repeats, blank), 'repeats')
    # no frames: status 1 for a wildcard, as for any label
    empty = np.zeros((0, classes), dtype=np.float32)
    code, _, score, _, _, status = _raw(hip, empty, [W], blank)
    assert (code, status) == (0, 1) and score == -np.inf
    # K21 keeps refusing the wildcard
    for label in ([W], [1, W, 2]):
        code, path, score, flp, _, status = _raw(hip, logits, label, blank, 0,
                                                 entry='ctcasr_ctc_align_long')
        assert (code, status) == (0, 2) and score == -np.inf
        assert (path == -1).all() and (flp == 0).all()


@gpu
def test_outputs_are_fully_written_and_one_workspace_serves_changing_calls(hip):
    rng = np.random.default_rng(50)
    classes, blank = 29, 28
    ts = hip.ALIGN_LONG_TILE_STATES
    long_label = _labels(rng, ts + 100, classes, blank, 0.1)
    short_label = _labels(rng, ts // 2 + 3, classes, blank, 0.1)
    for k in (0, 200, ts // 2, ts + 99):
        long_label[k] = W
    short_label[ts // 2 + 2] = short_label[77] = W
    long_steps = pref.required_time(long_label) + 500
    short_steps = (pref.required_time(short_label) + 100) | 1          # odd
    long_logits = _logits(rng, long_steps, classes)
    short_logits = _logits(rng, short_steps, classes)
    for tile_frames in (0, 37):
        fresh_long = _raw(hip, long_logits, long_label, blank, tile_frames)
        fresh_short = _raw(hip, short_logits, short_label, blank, tile_frames)
        assert fresh_long[0] == 0 and fresh_long[5] == 0 and fresh_short[5] == 0
        assert not (fresh_long[4] == 7.5).any()
        need = hip.ctc_align_long_workspace_bytes(long_steps, classes, len(long_label),
                                                  tile_frames)
        shared = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
        calls = [(long_logits, long_label, fresh_long), (short_logits, short_label, fresh_short),
                 (long_logits, long_label, fresh_long)]
        for x, label, fresh in calls:
            again = _raw(hip, x, label, blank, tile_frames, workspace=shared)
            assert again[0] == 0 and again[5] == 0
            for a, b in zip(again[1:5], fresh[1:5]):
                assert lref.same_bits(a, b), tile_frames
        if tile_frames == 0:
            _assert_equals_reference(fresh_long[1:], pref.on_table(fresh_long[4], long_label,
                                                                   blank), 'long')
            _assert_equals_reference(fresh_short[1:], pref.on_table(fresh_short[4], short_label,
                                                                    blank), 'short')


# ------------------------------------------------------------------------------------------------
# 6. Replacing labels by a wildcard never lowers the score
# ------------------------------------------------------------------------------------------------
@gpu
def test_a_wildcard_in_place_of_labels_never_lowers_the_score(hip):
    """Map a path of the full row to one of the shortened row that spends the frames of the
    replaced run (blanks between them included) in the wildcard: each frame's emission is >= the
    original, and fp64 addition is monotone, so the maximum is >= too - exactly, no tolerance."""
    ts = hip.ALIGN_LONG_TILE_STATES
    rng = np.random.default_rng(60)
    classes, blank = 29, 28
    label = _labels(rng, ts // 2 + 90, classes, blank, 0.1)
    num_steps = len(label) * 4 // 3
    logits = _logits(rng, num_steps, classes)
    full = _run(hip.ctc_align_partial, logits, label, blank)
    assert full[4] == 0
    for a, b in ((0, 1), (0, 40), (100, 101), (250, 300), (ts // 2 - 5, ts // 2 + 5),
                 (len(label) - 30, len(label)), (1, len(label) - 1), (0, len(label))):
        partial = label[:a] + [W] + label[b:]
        got = _run(hip.ctc_align_partial, logits, partial, blank)
        assert got[4] == 0 and got[1] >= full[1], (a, b, got[1], full[1])
        assert lref.same_bits(got[3], full[3])
