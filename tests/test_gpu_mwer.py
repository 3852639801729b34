"""`ctcasr_ctc_mwer` (csrc/ctc_mwer.hip, `hip.ctc_mwer`): the gradient of the expected error count
over n-best lists, against the float64 reference of tests/mwer_reference.py.

Bars (include/ctcasr.h, K23; set by the issue that asked for the kernel):
  * gradient: |grad - ref| <= 1e-4 * |scale| * max(1, sum_i |c_i|) per utterance, the reference's
    weights recomputed in float64 from the kernel's own fp32 scores.  That is the bar of the loss
    gradient against float64 in tests/test_gpu_ctc_edges.py, scaled by the weight the occupancies
    carry.  Every case prints its largest ratio to that bar (the largest seen on the MI355X:
    0.0015, at L = 575; profiles/mwer.md).
  * posterior and expected_risk: 1e-6 relative (fp64 exp on both sides, one rounding to fp32).
  * score and status: those of `hip.ctc_score` on the same rows, bit for bit - except that a
    non-finite logit is reported as status 3 here, where `ctc_score` returns 0 with the NaN.
The shapes are the smallest at which each path of the kernel can go wrong; every reference is
computed once."""

import numpy as np
import pytest
import torch

from tests import mwer_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CLASSES, BLANK = 29, 28


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _pack(hyps):
    rows = [label for utt in hyps for label in utt]
    offsets = np.zeros(len(rows) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(row) for row in rows])
    flat = np.array([v for row in rows for v in row] or [0], dtype=np.int32)
    return flat, offsets


def _run(hip, logits, seq_len, hyps, risks, n_hyps=None, scale=1.0, blank=None, grad_in=None,
         workspace=None, max_label_len=None):
    """`hip.ctc_mwer` on host data: ``hyps[b]`` the N label lists of utterance b, ``risks[b]``
    their risks.  Returns a dict of host arrays, rows shaped [B, N]."""
    batch, nbest = len(hyps), len(hyps[0])
    flat, offsets = _pack(hyps)
    n_hyps = [nbest] * batch if n_hyps is None else n_hyps
    grad = None if grad_in is None else _t(grad_in)
    out = hip.ctc_mwer(_t(logits), _t(np.asarray(seq_len), torch.int32), _t(flat, torch.int32),
                       _t(offsets, torch.int32), _t(np.asarray(n_hyps), torch.int32),
                       _t(np.asarray(risks, dtype=np.float32).reshape(-1)),
                       max_label_len=max_label_len, blank=blank, scale=scale,
                       accumulate=grad_in is not None, grad=grad, workspace=workspace)
    grad, expected, score, posterior, status = (t.cpu().numpy() for t in out)
    return {'grad': grad, 'expected_risk': expected, 'score': score.reshape(batch, nbest),
            'posterior': posterior.reshape(batch, nbest), 'status': status.reshape(batch, nbest)}


def _against_ctc_score(hip, got, logits, seq_len, hyps, n_hyps, blank, max_label_len):
    """score and status of the used rows are `hip.ctc_score`'s, bit for bit (3 apart)."""
    batch, nbest = len(hyps), len(hyps[0])
    n_hyps = [nbest] * batch if n_hyps is None else n_hyps
    used = [(b, i) for b in range(batch) for i in range(min(max(n_hyps[b], 0), nbest))]
    if not used:
        return
    flat, offsets = _pack([[hyps[b][i] for b, i in used]])
    score, status = hip.ctc_score(_t(logits), _t(np.asarray(seq_len), torch.int32),
                                  _t(flat, torch.int32), _t(offsets, torch.int32),
                                  _t(np.array([b for b, _ in used]), torch.int32),
                                  max_label_len=max_label_len, blank=blank)
    score, status = score.cpu().numpy(), status.cpu().numpy()
    mine = np.array([got['score'][b, i] for b, i in used], dtype=np.float32)
    mine_status = np.array([got['status'][b, i] for b, i in used])
    assert np.array_equal(_bits(mine), _bits(score))
    assert np.array_equal(np.where(mine_status == 3, 0, mine_status), status)
    assert np.isnan(mine[mine_status == 3]).all()


def _verify(hip, logits, seq_len, hyps, risks, n_hyps=None, scale=1.0, blank=None, what='',
            max_label_len=None, reference_risks=None):
    """One call against the reference, every pinned property; returns (got, want)."""
    logits = np.asarray(logits, dtype=np.float32)
    classes = logits.shape[2]
    blank = classes - 1 if blank is None else blank
    got = _run(hip, logits, seq_len, hyps, risks, n_hyps, scale, blank,
               max_label_len=max_label_len)
    want = ref.mwer(logits, seq_len, hyps, risks if reference_risks is None else reference_risks,
                    n_hyps, blank, scale, scores=got['score'], max_label_len=max_label_len)
    assert np.array_equal(got['status'], want['status']), (what, got['status'], want['status'])
    _against_ctc_score(hip, got, logits, seq_len, hyps, n_hyps, blank, max_label_len)
    unused = got['status'] == -1
    assert np.isneginf(got['score'][unused]).all() and not got['posterior'][unused].any()
    worst = 0.0
    for b in range(len(hyps)):
        length = int(seq_len[b])
        live = length if 0 <= length <= logits.shape[0] else 0
        assert not _bits(got['grad'][live:, b]).any(), (what, b)      # +0.0, bit for bit
        if (got['status'][b] == 3).any():
            assert np.isnan(got['grad'][:live, b]).all() and np.isnan(got['expected_risk'][b])
            assert np.isnan(got['posterior'][b][got['status'][b] == 3]).all()
            continue
        bar = 1e-4 * abs(scale) * max(1.0, np.abs(want['c'][b]).sum())
        err = np.abs(got['grad'][:live, b].astype(np.float64) - want['grad'][:live, b])
        worst = max(worst, (err.max() if err.size else 0.0) / bar)
        if (got['status'][b] == 0).sum() < 2:
            assert not _bits(got['grad'][:, b]).any(), (what, b)
        np.testing.assert_allclose(got['posterior'][b], want['posterior'][b], rtol=1e-6,
                                   atol=1e-38, err_msg=what)
        np.testing.assert_allclose(got['expected_risk'][b], want['expected_risk'][b], rtol=1e-6,
                                   atol=1e-38, err_msg=what)
        rows = got['grad'][:live, b].astype(np.float64).sum(axis=1)
        assert (np.abs(rows) <= 2 * bar).all(), (what, b)
    print('mwer ratio to the bar, {}: {:.3g} (sum |c| up to {:.3g})'.format(
        what, worst, np.abs(want['c']).sum(axis=1).max()))
    assert worst <= 1.0, (what, worst)
    return got, want


def _labels(rng, length, classes=CLASSES, blank=BLANK):
    ids = [c for c in range(classes) if c != blank]
    return [ids[int(i)] for i in rng.integers(0, len(ids), size=length)]


def _variants(rng, length):
    """Three hypotheses of about ``length`` labels whose scores are of one order: a random one,
    the same with one label changed, the same without its last label."""
    base = _labels(rng, length)
    other = list(base)
    if length:
        other[length // 2] = (other[length // 2] + 1) % BLANK
    return [base, other, base[:-1]]


# ------------------------------------------------------------------------------------------------
def test_one_frame(hip):
    rng = np.random.default_rng(1)
    logits = rng.normal(size=(1, 2, CLASSES)).astype(np.float32)
    got, want = _verify(hip, logits, [1, 1], [[[], [5]], [[7], [3]]], [[1.0, 0.0], [0.0, 2.0]],
                        what='T = 1')
    assert (got['status'] == 0).all() and np.abs(got['grad']).max() > 1e-3


def test_lengths_7_4_0_and_the_empty_hypothesis(hip):
    """T = 7, B = 3 with seq_len 7, 4, 0; the empty hypothesis among others.  With seq_len 0 only
    the empty hypothesis is feasible: one valid row, an exactly zero gradient."""
    rng = np.random.default_rng(2)
    logits = (rng.normal(size=(7, 3, CLASSES)) * 2).astype(np.float32)
    hyps = [[[0, 1], [1], [], [3, 3]], [[2], [2, 0], [0], []], [[1], [], [2], [3]]]
    risks = [[2.0, 1.0, 3.0, 0.0], [0.0, 1.0, 1.0, 2.0], [1.0, 2.0, 3.0, 4.0]]
    got, _ = _verify(hip, logits, [7, 4, 0], hyps, risks, scale=0.25, what='seq_len 7, 4, 0')
    assert got['status'].tolist() == [[0] * 4, [0] * 4, [1, 0, 1, 1]]
    assert got['expected_risk'][2] == 2.0 and got['posterior'][2].tolist() == [0, 1, 0, 0]
    assert np.abs(got['grad'][:, 0]).max() > 1e-3 and np.abs(got['grad'][:4, 1]).max() > 1e-3
    # accumulate: rows behind seq_len keep grad_in's bits, the others add in fp64
    grad_in = rng.normal(size=logits.shape).astype(np.float32)
    grad_in[6, 1, 0] = -0.0
    added = _run(hip, logits, [7, 4, 0], hyps, risks, scale=0.25, grad_in=grad_in)
    assert np.array_equal(_bits(added['grad'][4:, 1]), _bits(grad_in[4:, 1]))
    assert np.array_equal(_bits(added['grad'][:, 2]), _bits(grad_in[:, 2]))
    # (float)((double)grad_in + sum) against grad_in + (float)sum: the two roundings apart
    exact = grad_in.astype(np.float64) + got['grad'].astype(np.float64)
    slack = np.spacing(np.abs(exact).astype(np.float32)) + np.spacing(np.abs(got['grad']))
    assert (np.abs(added['grad'] - exact) <= slack).all()
    for name in ('score', 'status', 'posterior', 'expected_risk'):
        assert np.array_equal(added[name], got[name]), name
    # accumulate onto zeros is the plain call, bit for bit
    onto_zeros = _run(hip, logits, [7, 4, 0], hyps, risks, scale=0.25,
                      grad_in=np.zeros_like(logits))
    assert np.array_equal(_bits(onto_zeros['grad']), _bits(got['grad']))


def test_repeated_labels_at_and_below_the_feasible_length(hip):
    """aa and aba need exactly 3 frames, aab needs 4: at T = 3 that row is status 1 and takes no
    part - the gradient is that of the list without it, bit for bit."""
    rng = np.random.default_rng(3)
    logits = rng.normal(size=(3, 1, CLASSES)).astype(np.float32)
    hyps = [[[4, 4], [4, 6, 4], [4], [4, 4, 6]]]
    risks = [[0.0, 1.0, 1.0, 2.0]]
    got, _ = _verify(hip, logits, [3], hyps, risks, what='aa, aba at T = 3')
    assert got['status'].tolist() == [[0, 0, 0, 1]] and got['posterior'][0, 3] == 0
    without = _run(hip, logits, [3], hyps, risks, n_hyps=[3])
    assert np.array_equal(_bits(without['grad']), _bits(got['grad']))
    assert np.array_equal(_bits(without['expected_risk']), _bits(got['expected_risk']))
    assert np.abs(got['grad']).max() > 1e-3


@pytest.mark.parametrize('length', [31, 32, 33, 64, 96, 97])
def test_states_per_lane_seams(hip, length):
    """L = 31 .. 97 at T = 2L + 3: S = 2L + 1 on both sides of 64, 128 and 192 states, so the 1,
    2, 3 and 6 states-per-lane kernels and their lane seams are walked."""
    rng = np.random.default_rng(length)
    steps = 2 * length + 3
    logits = rng.normal(size=(steps, 1, CLASSES)).astype(np.float32)
    got, want = _verify(hip, logits, [steps], [_variants(rng, length)], [[0.0, 1.0, 1.0]],
                        what='L = {}'.format(length), max_label_len=length)
    assert (got['status'] == 0).all() and np.abs(want['c']).sum() > 1e-6


def test_the_longest_row(hip):
    """L = 575 at T = 1160: 1151 states, 18 per lane."""
    rng = np.random.default_rng(575)
    logits = rng.normal(size=(1160, 1, CLASSES)).astype(np.float32)
    got, want = _verify(hip, logits, [1160], [_variants(rng, 575)], [[0.0, 1.0, 1.0]],
                        what='L = 575', max_label_len=575)
    assert (got['status'] == 0).all() and np.abs(want['c']).sum() > 1e-6


def test_list_sizes_4_1_0_and_minus_1(hip):
    """N = 4 with n_hyps 4, 1, 0, -1: one valid hypothesis gives an exactly zero gradient, and
    the unused rows' garbage labels and NaN risks change nothing."""
    rng = np.random.default_rng(4)
    logits = (rng.normal(size=(6, 4, CLASSES)) * 2).astype(np.float32)
    good = [[1, 2], [2], [1], []]
    hyps = [good, [[3], [99, -7], [28, 28, 28], [1000] * 5], [[-1], [77], [28], [5000]],
            [[64] * 3, [-9], [123456], [28]]]
    nan = float('nan')
    risks = [[1.0, 0.0, 2.0, 2.0], [3.0, nan, nan, nan], [nan] * 4, [nan] * 4]
    clean = [[1.0, 0.0, 2.0, 2.0], [3.0, 0, 0, 0], [0] * 4, [0] * 4]
    got, _ = _verify(hip, logits, [6, 6, 6, 6], hyps, risks, n_hyps=[4, 1, 0, -1],
                     what='n_hyps 4, 1, 0, -1', reference_risks=clean)
    assert got['status'].tolist() == [[0] * 4, [0, -1, -1, -1], [-1] * 4, [-1] * 4]
    assert got['expected_risk'].tolist() == [got['expected_risk'][0], 3.0, 0.0, 0.0]
    assert not _bits(got['grad'][:, 1:]).any() and np.abs(got['grad'][:, 0]).max() > 1e-3
    tidy = _run(hip, logits, [6, 6, 6, 6], [good, [[3], [], [], []], [[]] * 4, [[]] * 4], clean,
                n_hyps=[4, 1, 0, -1])
    for name in ('grad', 'expected_risk', 'score', 'posterior'):
        assert np.array_equal(_bits(tidy[name]), _bits(got[name])), name


def test_equal_risks_and_a_bad_label(hip):
    rng = np.random.default_rng(5)
    logits = (rng.normal(size=(9, 2, CLASSES)) * 2).astype(np.float32)
    hyps = [[[1, 2, 3], [1, 3], [2]], [[4], [BLANK], [4, CLASSES]]]
    got, _ = _verify(hip, logits, [9, 9], hyps, [[2.0] * 3, [0.0, 1.0, 5.0]],
                     what='equal risks; bad labels')
    assert got['status'].tolist() == [[0, 0, 0], [0, 2, 2]]
    assert np.abs(got['grad'][:, 0]).max() <= 1e-4          # equal risks: within the bar of zero
    assert not _bits(got['grad'][:, 1]).any()               # one valid row
    # a seq_len above T or below 0: status 2 throughout, every row of the gradient +0.0
    odd = _run(hip, logits, [10, -1], hyps, [[1.0, 2.0, 3.0]] * 2)
    assert (odd['status'] == 2).all() and not _bits(odd['grad']).any()
    assert not odd['expected_risk'].any()


def test_non_finite_logits_inside_and_outside_seq_len(hip):
    """+inf / NaN inside seq_len: status 3 and NaN as pinned; outside: no effect.  The other
    utterances keep their bits."""
    rng = np.random.default_rng(6)
    logits = (rng.normal(size=(8, 4, CLASSES)) * 2).astype(np.float32)
    seq_len = [8, 5, 8, 5]
    hyps = [[[1, 2], [2], [1, 1, 1, 1, 1]]] * 4             # the last needs 9 frames: status 1
    risks = [[0.0, 1.0, 2.0]] * 4
    clean = _run(hip, logits, seq_len, hyps, risks)
    dirty_logits = logits.copy()
    dirty_logits[3, 0, 7] = np.inf                          # inside
    dirty_logits[4, 1, 2] = np.nan                          # inside (t = 4 < 5)
    dirty_logits[6, 3, 0] = np.nan                          # outside (t = 6 >= 5)
    dirty_logits[5, 3, 1] = np.inf
    dirty_logits[2, 2, 9] = -np.inf                         # a class of probability zero: legal
    got, _ = _verify(hip, dirty_logits, seq_len, hyps, risks, what='non-finite logits')
    assert got['status'].tolist() == [[3, 3, 1], [3, 3, 1], [0, 0, 1], [0, 0, 1]]
    assert np.isnan(got['grad'][:, 0]).all() and np.isnan(got['grad'][:5, 1]).all()
    assert not _bits(got['grad'][5:, 1]).any()
    for name in ('grad', 'expected_risk', 'score', 'posterior'):
        axis = 1 if name == 'grad' else 0
        assert np.array_equal(_bits(np.take(got[name], 3, axis)),
                              _bits(np.take(clean[name], 3, axis))), name
    assert np.isfinite(got['grad'][:, 2]).all() and np.isfinite(got['expected_risk'][2])
    # accumulate: NaN below seq_len, grad_in above
    grad_in = rng.normal(size=logits.shape).astype(np.float32)
    added = _run(hip, dirty_logits, seq_len, hyps, risks, grad_in=grad_in)
    assert np.isnan(added['grad'][:5, 1]).all()
    assert np.array_equal(_bits(added['grad'][5:, 1]), _bits(grad_in[5:, 1]))


@pytest.mark.parametrize('classes', [2, 64])
def test_class_counts(hip, classes):
    rng = np.random.default_rng(classes)
    logits = (rng.normal(size=(6, 2, classes)) * 2).astype(np.float32)
    if classes == 2:
        hyps = [[[], [0], [0, 0]], [[0, 0, 0], [0], []]]
        got, _ = _verify(hip, logits, [6, 5], hyps, [[0.0, 1.0, 2.0], [0.0, 2.0, 3.0]],
                         what='C = 2')
        blank_first = _verify(hip, logits, [6, 5], [[[], [1], [1, 1]], [[1, 1, 1], [1], []]],
                              [[0.0, 1.0, 2.0], [0.0, 2.0, 3.0]], blank=0,
                              what='C = 2, blank 0')[0]
        assert (blank_first['status'] == 0).all()
    else:
        hyps = [[[62, 0, 31], [62, 31], [0]], [[5, 5], [63], [62]]]
        got, _ = _verify(hip, logits, [6, 6], hyps, [[0.0, 1.0, 2.0], [1.0, 0.0, 3.0]],
                         what='C = 64')
        assert got['status'].tolist() == [[0, 0, 0], [0, 2, 0]]
    assert np.abs(got['grad']).max() > 1e-3


def test_an_utterance_alone_and_inside_a_batch_of_five(hip):
    rng = np.random.default_rng(7)
    logits = (rng.normal(size=(12, 5, CLASSES)) * 2).astype(np.float32)
    seq_len = [12, 9, 12, 10, 7]
    hyps = [[_labels(rng, int(n)) for n in rng.integers(0, 5, size=4)] for _ in range(5)]
    risks = rng.integers(0, 5, size=(5, 4)).astype(np.float32)
    n_hyps = [4, 3, 4, 4, 2]
    whole, _ = _verify(hip, logits, seq_len, hyps, risks, n_hyps=n_hyps, what='batch of 5')
    alone = _run(hip, logits[:, 3:4], seq_len[3:4], hyps[3:4], risks[3:4], n_hyps=n_hyps[3:4])
    assert np.array_equal(_bits(alone['grad'][:, 0]), _bits(whole['grad'][:, 3]))
    for name in ('expected_risk', 'score', 'posterior', 'status'):
        assert np.array_equal(alone[name][0], whole[name][3]), name


def test_one_workspace_twice(hip):
    """Two calls on one workspace with other data in between: what the workspace held does not
    matter, and two runs give equal bits."""
    rng = np.random.default_rng(8)
    logits = (rng.normal(size=(10, 2, CLASSES)) * 2).astype(np.float32)
    hyps = [[[1, 2, 3], [1, 3], [2]], [[4, 4], [4], []]]
    risks = [[0.0, 1.0, 3.0], [1.0, 0.0, 2.0]]
    need = hip.ctc_mwer_workspace_bytes(10, 2, CLASSES, 3, 3)
    workspace = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)
    first = _run(hip, logits, [10, 8], hyps, risks, workspace=workspace, max_label_len=3)
    other = (rng.normal(size=(10, 2, CLASSES)) * 3).astype(np.float32)
    _run(hip, other, [7, 10], [[[5], [6, 7, 8], [9, 9]], [[1], [2], [3]]], risks,
         workspace=workspace, max_label_len=3)
    again = _run(hip, logits, [10, 8], hyps, risks, workspace=workspace, max_label_len=3)
    fresh = _run(hip, logits, [10, 8], hyps, risks, max_label_len=3)
    for name in first:
        assert np.array_equal(first[name].view(np.int32), again[name].view(np.int32)), name
        assert np.array_equal(first[name].view(np.int32), fresh[name].view(np.int32)), name


def test_wrapper_refusals(hip):
    """Refused before any launch: a workspace one byte short, label_offsets / n_hyps / risk of the
    wrong size, a row outside `labels`."""
    logits = torch.zeros((5, 2, CLASSES), device=DEV)
    seq_len = _t([5, 5], torch.int32)
    labels = _t([1, 2, 3, 4, 5, 6], torch.int32)
    offsets = _t([0, 1, 2, 3, 4, 5, 6], torch.int32)
    n_hyps = _t([3, 3], torch.int32)
    risk = _t(np.zeros(6))
    need = hip.ctc_mwer_workspace_bytes(5, 2, CLASSES, 3, 1)
    short = torch.empty(need - 1, dtype=torch.uint8, device=DEV)
    with pytest.raises(hip.CtcAsrError, match='workspace'):
        hip.ctc_mwer(logits, seq_len, labels, offsets, n_hyps, risk, workspace=short)
    with pytest.raises(hip.CtcAsrError, match='label_offsets'):
        hip.ctc_mwer(logits, seq_len, labels, offsets[:-1], n_hyps, risk)
    with pytest.raises(hip.CtcAsrError, match='n_hyps'):
        hip.ctc_mwer(logits, seq_len, labels, offsets, n_hyps[:1], risk)
    with pytest.raises(hip.CtcAsrError, match='risk'):
        hip.ctc_mwer(logits, seq_len, labels, offsets, n_hyps, risk[:5])
    with pytest.raises(hip.CtcAsrError, match='outside'):
        hip.ctc_mwer(logits, seq_len, labels[:5], offsets, n_hyps, risk)
    with pytest.raises(hip.CtcAsrError, match='lengths for a batch'):
        hip.ctc_mwer(logits, seq_len[:1], labels, offsets, n_hyps, risk)
    with pytest.raises(hip.CtcAsrError, match='accumulate'):
        hip.ctc_mwer(logits, seq_len, labels, offsets, n_hyps, risk, accumulate=True)
    # ... and the library itself refuses the short workspace too
    exact = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = hip.ctc_mwer(logits, seq_len, labels, offsets, n_hyps, risk, workspace=exact)
    assert (out[4] == 0).all()
