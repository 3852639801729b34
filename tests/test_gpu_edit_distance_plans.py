"""``ctcasr_edit_distance`` at its plan seams and its length ceiling: both sides of every layout
that ``ed_plan`` chooses (four, two or one pair per workgroup; carry columns in LDS or in the
workspace), carry columns handed on through hundreds of strips, plans chosen by a ``max_ref_len``
far above the data, the workspace's bounds, and packed cells with both fields near 2^15.  All
four counts and the status, exact equality, against `edit_reference.error_counts_fast` or pairs
whose counts are known by construction (`edit_reference.known_edits`)."""

import numpy as np
import pytest
import torch

from ctc_asr_amd import metrics
from tests import edit_reference as ref

pytestmark = pytest.mark.gpu

LDS_MAX = 150 * 1024
POISON = -77


def _plan(max_ref_len):
    """(stride, pairs per workgroup, carry columns in LDS, dynamic LDS bytes): `ed_stride` and
    `ed_plan` of csrc/edit_distance.hip, restated."""
    stride = (max_ref_len + 3) // 4 * 4
    waves = 4
    while waves > 1 and waves * stride * 4 > LDS_MAX:
        waves //= 2
    col_in_lds = 2 * waves * stride * 4 <= LDS_MAX
    return stride, waves, col_in_lds, (2 if col_in_lds else 1) * waves * stride * 4


def _t(values):
    return torch.from_numpy(np.asarray(values, dtype=np.int64).astype(np.int32)).cuda()


def _pack(rows):
    lengths = np.array([len(r) for r in rows], dtype=np.int64)
    flat = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows] + [np.zeros(1, np.int64)])
    return flat, np.cumsum(lengths) - lengths, lengths


def _run(hip, hyps, refs, **kwargs):
    """int array [B, 5] of (distance, S, D, I, status) for packed rows.  The outputs start
    poisoned: a pair that no wave took shows, whatever the allocator handed out."""
    hyp, hyp_off, hyp_len = _pack(hyps)
    ref_, ref_off, ref_len = _pack(refs)
    out = torch.full((5, len(hyps)), POISON, dtype=torch.int32, device='cuda')
    hip.edit_distance(_t(hyp), _t(hyp_off), _t(hyp_len), _t(ref_), _t(ref_off), _t(ref_len),
                      out=out, **kwargs)
    return out.t().cpu().numpy()


def _rows(counts):
    return np.array([tuple(c) + (0,) for c in counts], dtype=np.int64)


def _fast(hyps, refs):
    return _rows(ref.error_counts_fast(h, r) for h, r in zip(hyps, refs))


def _same(got, want, hyps, refs):
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, [(int(b), len(hyps[b]), len(refs[b]), got[b].tolist(),
                            want[b].tolist()) for b in bad[:5]]


def _distinct(rng, size):
    """Pairwise distinct ids of both signs."""
    return (rng.permutation(size + 1000)[:size] * 60013 - 2 ** 30).tolist()


def _mutated(rng, row, rate, alphabet, size):
    """``row`` with about ``rate`` each of its symbols substituted, deleted, or followed by an
    insertion, cut or filled up to ``size`` symbols."""
    out = []
    for symbol, kind in zip(row, rng.random(len(row))):
        if kind < rate:
            continue
        out.append(int(rng.integers(0, alphabet)) if kind < 2 * rate else symbol)
        if kind > 1 - rate:
            out.append(int(rng.integers(0, alphabet)))
    out += rng.integers(0, alphabet, size=max(size - len(out), 0)).tolist()
    return out[:size]


def test_the_restated_plan_and_the_workspace_it_implies(hip):
    table = {2048: (4, True), 2049: (4, True), 4800: (4, True), 4801: (4, False),
             9600: (4, False), 9601: (2, False), 19200: (2, False), 19201: (1, False),
             32767: (1, False)}
    for max_ref_len, (waves, col_in_lds) in table.items():
        stride, got_waves, got_in_lds, lds = _plan(max_ref_len)
        assert (got_waves, got_in_lds) == (waves, col_in_lds), max_ref_len
        assert lds <= LDS_MAX and (lds > 64 * 1024) == (max_ref_len >= 2049)
        assert max_ref_len <= stride < max_ref_len + 4 and stride % 4 == 0
    assert _plan(4800)[3] == LDS_MAX and _plan(0)[3] == 0
    # the observable part: the carry columns of the whole batch, or nothing
    query = hip.edit_distance_workspace_bytes
    assert query(5, 100, 4800) == 0
    assert query(5, 100, 4801) == (5 * 4804 * 4 + 255) // 256 * 256
    for batch in (1, 5, 64):
        for max_ref_len in list(table) + [0, 1, 5000, 12345]:
            stride, _, col_in_lds, _ = _plan(max_ref_len)
            want = 0 if col_in_lds else (batch * stride * 4 + 255) // 256 * 256
            assert {query(batch, h, max_ref_len) for h in (0, 64, 32767)} == {want}


# ---- (a) both sides of every plan seam, short hypotheses --------------------------------------
@pytest.mark.parametrize('max_ref_len', [2048, 2049, 4800, 4801, 9600, 9601, 19200, 19201, 32767])
def test_both_sides_of_every_plan_seam(hip, max_ref_len):
    """Five pairs, so the last workgroup is ragged at four, two and one pair per workgroup."""
    rng = np.random.default_rng(max_ref_len)
    pool = _distinct(rng, max_ref_len + 400)
    long_ref, foreign = pool[:max_ref_len], pool[max_ref_len:]
    start = max_ref_len // 2 - 61
    window = long_ref[start:start + 130]
    for k, at in enumerate(rng.choice(130, size=10, replace=False)):
        window[at] = foreign[k]
    other_ref = rng.permutation(long_ref).tolist()
    hyps = [window, foreign[10:75], foreign[100:164], [], foreign[200:400]]
    refs = [long_ref, other_ref, [foreign[140]], long_ref[::-1], []]
    got = _run(hip, hyps, refs, max_ref_len=max_ref_len)
    assert got[0].tolist() == [max_ref_len - 120, 10, max_ref_len - 130, 0, 0]
    assert got[1].tolist() == [max_ref_len, 65, max_ref_len - 65, 0, 0]
    assert got[2].tolist() == [63, 0, 0, 63, 0]
    assert got[3].tolist() == [max_ref_len, 0, max_ref_len, 0, 0]
    assert got[4].tolist() == [200, 0, 0, 200, 0]
    _same(got, _fast(hyps, refs), hyps, refs)


# ---- (b) many strips over one carry column, once per plan -------------------------------------
@pytest.mark.parametrize('hyp_len,ref_len', [(4790, 4800), (4801, 4801), (9601, 9601)])
def test_many_strips_over_one_carry_column_with_frequent_ties(hip, hyp_len, ref_len):
    rng = np.random.default_rng(hyp_len + ref_len)
    refs = [rng.integers(0, 28, size=ref_len).tolist()]
    hyps = [_mutated(rng, refs[0], 0.03, 28, hyp_len)]
    assert len(hyps[0]) == hyp_len and _plan(ref_len)[1:3] == \
        {4800: (4, True), 4801: (4, False), 9601: (2, False)}[ref_len]
    want = _fast(hyps, refs)
    assert 0 < want[0, 1] and 0 < want[0, 2] and 0 < want[0, 3]
    got = _run(hip, hyps, refs)
    _same(got, want, hyps, refs)
    assert (_run(hip, hyps, refs) == got).all()       # the carry column is rewritten in place


def test_many_strips_one_pair_per_workgroup(hip):
    rng = np.random.default_rng(19201)
    hyp, ref_seq, counts = ref.known_edits(rng, 19201, 400, 300, 300)
    assert len(hyp) == 19201 and _plan(19201)[1:3] == (1, False)
    got = _run(hip, [hyp], [ref_seq])
    assert got[0].tolist() == list(counts) + [0]
    assert (_run(hip, [hyp], [ref_seq]) == got).all()


def test_the_length_ceiling_on_both_sides(hip):
    """32767 x 32767, two rows side by side in one launch.  Between two disjoint rows every cell
    of the diagonal is (k, k): the last is 0x7FFF7FFF, and the candidates that `min` compares
    reach 0x80008000 - past the sign bit, with both 16-bit fields at their largest.  One launch
    of the two rows is 2.7 s on the MI355X (profiles/edit_distance.md, "Plans"); it runs twice."""
    rng = np.random.default_rng(32767)
    hyp, ref_seq, counts = ref.known_edits(rng, 32767, 300, 250, 250)
    assert len(hyp) == 32767
    hyps = [hyp, list(range(32767))]
    refs = [ref_seq, list(range(40000, 72767))]
    got = _run(hip, hyps, refs)
    assert got[0].tolist() == list(counts) + [0]
    assert got[1].tolist() == [32767, 32767, 0, 0, 0]
    assert (_run(hip, hyps, refs) == got).all()


def test_512_strips_of_a_short_column_and_the_mirror(hip):
    long_row, short_row = list(range(32767)), list(range(-70, 0))
    hyps, refs = [long_row, short_row], [short_row, long_row]
    want = [[32767, 70, 0, 32697, 0], [32767, 70, 32697, 0, 0]]
    got = _run(hip, hyps, refs)                       # one pair per workgroup, workspace
    assert got.tolist() == want
    assert (_run(hip, hyps, refs) == got).all()
    assert _run(hip, hyps[:1], refs[:1]).tolist() == want[:1]     # max_ref_len = 70: all in LDS
    # the same 512 strips with matches to find: the reference is a subsequence
    picked = long_row[5::470]
    assert len(picked) == 70
    assert _run(hip, [long_row], [picked]).tolist() == [[32697, 0, 0, 32697, 0]]
    assert _run(hip, [picked], [long_row]).tolist() == [[32697, 0, 32697, 0, 0]]


# ---- (c) the plan does not change the answer --------------------------------------------------
def test_a_plan_chosen_far_above_the_data(hip):
    rng = np.random.default_rng(71)
    grid = (0, 1, 63, 64, 65, 129)
    hyps = [rng.integers(0, 2, size=n).tolist() for n in grid for _ in grid]
    refs = [rng.integers(0, 2, size=n).tolist() for _ in grid for n in grid]
    want = _rows(ref.error_counts(h, r) for h, r in zip(hyps, refs))
    _same(_run(hip, hyps, refs), want, hyps, refs)
    for max_ref_len in (4801, 9601, 19201, 32767):
        _same(_run(hip, hyps, refs, max_ref_len=max_ref_len), want, hyps, refs)
        _same(_run(hip, hyps, refs, max_ref_len=max_ref_len, max_hyp_len=32767), want, hyps, refs)
    _same(_run(hip, hyps, refs, max_hyp_len=32767), want, hyps, refs)


@pytest.mark.parametrize('max_ref_len', [9601, 19201])
def test_batches_of_one_two_and_three(hip, max_ref_len):
    rng = np.random.default_rng(max_ref_len + 1)
    refs = [rng.integers(0, 3, size=n).tolist() for n in (max_ref_len, max_ref_len - 1, 700)]
    hyps = [rng.integers(0, 3, size=n).tolist() for n in (70, 129, 130)]
    want = _fast(hyps, refs)
    for batch in (1, 2, 3):
        _same(_run(hip, hyps[:batch], refs[:batch], max_ref_len=max_ref_len), want[:batch],
              hyps, refs)
    # the third pair alone, under the long plan: the workgroup of pair 0 with nothing beside it
    _same(_run(hip, hyps[2:], refs[2:], max_ref_len=max_ref_len), want[2:], hyps[2:], refs[2:])


@pytest.mark.parametrize('max_ref_len', [9601, 19201])
def test_status_2_among_live_rows_of_the_small_workgroups(hip, max_ref_len):
    rng = np.random.default_rng(max_ref_len + 2)
    refs = [rng.integers(0, 3, size=n).tolist()
            for n in (max_ref_len, max_ref_len + 1, 300, 65, max_ref_len, 1, max_ref_len - 3)]
    hyps = [rng.integers(0, 3, size=n).tolist() for n in (100, 100, 129, 90, 66, 64, 130)]
    hyp, hyp_off, hyp_len = _pack(hyps)
    ref_, ref_off, ref_len = _pack(refs)
    hyp_len[3] = -1                  # the beam search's out_len of an exhausted pool
    out = torch.full((5, 7), POISON, dtype=torch.int32, device='cuda')
    hip.edit_distance(_t(hyp), _t(hyp_off), _t(hyp_len), _t(ref_), _t(ref_off), _t(ref_len),
                      max_ref_len=max_ref_len, out=out)
    got = out.t().cpu().numpy()
    want = _fast(hyps, refs)
    want[1] = want[3] = (-1, -1, -1, -1, 2)
    _same(got, want, hyps, refs)
    live = [0, 2, 4, 5, 6]
    alone = _run(hip, [hyps[b] for b in live], [refs[b] for b in live], max_ref_len=max_ref_len)
    assert (alone == got[live]).all()


# ---- (d) the workspace ------------------------------------------------------------------------
def _abi(hip, device_rows, batch, max_hyp_len, max_ref_len, workspace, workspace_bytes):
    """One call of the C entry point on rows already on the device: (code, int array [B, 5])."""
    out = torch.full((5, batch), POISON, dtype=torch.int32, device='cuda')
    code = hip.load().ctcasr_edit_distance(
        *[t.data_ptr() for t in device_rows], batch, max_hyp_len, max_ref_len,
        *[out[k].data_ptr() for k in range(5)],
        None if workspace is None else workspace.data_ptr(), workspace_bytes,
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return code, out.t().cpu().numpy()


def _device_rows(hyps, refs):
    hyp, hyp_off, hyp_len = _pack(hyps)
    ref_, ref_off, ref_len = _pack(refs)
    return [_t(v) for v in (hyp, hyp_off, hyp_len, ref_, ref_off, ref_len)]


@pytest.mark.parametrize('max_ref_len', [4801, 19201])
def test_workspace_of_exactly_the_size_asked_for(hip, max_ref_len):
    rng = np.random.default_rng(max_ref_len + 3)
    refs = [rng.integers(0, 3, size=n).tolist() for n in (max_ref_len, 900, max_ref_len)]
    hyps = [rng.integers(0, 3, size=n).tolist() for n in (130, 200, 129)]
    rows = _device_rows(hyps, refs)
    need = hip.edit_distance_workspace_bytes(3, 200, max_ref_len)
    assert need == (3 * _plan(max_ref_len)[0] * 4 + 255) // 256 * 256
    want = _fast(hyps, refs)

    zeroed = torch.zeros(need, dtype=torch.uint8, device='cuda')
    code, got = _abi(hip, rows, 3, 200, max_ref_len, zeroed, need)
    assert code == 0
    _same(got, want, hyps, refs)

    guard = 4096
    buffer = torch.full((need + guard,), 0xFF, dtype=torch.uint8, device='cuda')
    buffer[need:] = 0xA5
    code, got = _abi(hip, rows, 3, 200, max_ref_len, buffer, need)
    assert code == 0
    _same(got, want, hyps, refs)
    assert (buffer[need:] == 0xA5).all().item()
    assert not (buffer[:need] == 0xFF).all().item()      # the columns did go there

    code, got = _abi(hip, rows, 3, 200, max_ref_len, buffer, need - 1)
    assert code == -3 and (got == POISON).all()
    code, got = _abi(hip, rows, 3, 200, max_ref_len, None, 0)
    assert code == -3 and (got == POISON).all()
    assert (buffer[need:] == 0xA5).all().item()


def test_no_workspace_up_to_4800_and_none_without_a_reference(hip):
    rng = np.random.default_rng(79)
    refs = [rng.integers(0, 3, size=n).tolist() for n in (4800, 10)]
    hyps = [rng.integers(0, 3, size=n).tolist() for n in (129, 70)]
    rows = _device_rows(hyps, refs)
    code, got = _abi(hip, rows, 2, 129, 4800, None, 0)
    assert code == 0
    _same(got, _fast(hyps, refs), hyps, refs)
    code, got = _abi(hip, rows, 2, 129, 4801, None, 0)
    assert code == -3 and (got == POISON).all()

    # max_ref_len = 0: no stride, no LDS, nothing to stage
    hyps = [rng.integers(0, 3, size=n).tolist() for n in (1, 64, 65, 200, 3)]
    empty = [[] for _ in hyps]
    code, got = _abi(hip, _device_rows(hyps, empty), 5, 200, 0, None, 0)
    assert code == 0 and got.tolist() == [[len(h), 0, 0, len(h), 0] for h in hyps]
    code, got = _abi(hip, _device_rows(empty, hyps), 5, 0, 200, None, 0)
    assert code == 0 and got.tolist() == [[len(h), 0, len(h), 0, 0] for h in hyps]
    assert _run(hip, hyps, empty).tolist() == [[len(h), 0, 0, len(h), 0] for h in hyps]
    assert _run(hip, empty, hyps).tolist() == [[len(h), 0, len(h), 0, 0] for h in hyps]


# ---- (e) the path the project uses ------------------------------------------------------------
def test_error_counts_with_the_word_list_of_an_hour_of_speech(hip):
    rng = np.random.default_rng(83)
    hyps = [rng.integers(0, 28, size=int(n)).tolist() for n in rng.integers(0, 180, size=41)]
    refs = [rng.integers(0, 28, size=int(n)).tolist() for n in rng.integers(0, 180, size=41)]
    want = [ref.error_counts(h, r) for h, r in zip(hyps, refs)]
    hyps[17], refs[17], want[17] = ref.known_edits(rng, 10000, 300, 200, 250)
    assert _plan(10000)[1:3] == (2, False)
    got = metrics.error_counts(hyps, refs, 'cuda')
    assert got.dtype == np.int32 and got.shape == (41, 4)
    _same(got, np.array(want), hyps, refs)


def test_error_counts_accepts_rows_of_exactly_32767(hip):
    long_row, short_row = list(range(32767)), list(range(-70, 0))
    got = metrics.error_counts([long_row, short_row, long_row[:100]],
                               [short_row, long_row, long_row[50:150]], 'cuda')
    assert got.tolist() == [[32767, 70, 0, 32697], [32767, 70, 32697, 0], [100, 0, 50, 50]]
