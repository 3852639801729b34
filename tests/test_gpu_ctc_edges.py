"""The CTC loss, its gradient, greedy decode and the log-softmax export (csrc/ctc.hip) at the
shapes where they go wrong first: utterances of 1-4 frames and 0-1 frames inside longer ones, the
tight bound len = L + repeats (exactly one alignment) and one frame below it, label lengths on
both sides of the sweep kernel's per-thread slot seams (S = 2L + 1 = 384, 768) and at its ceiling
(L = 575), T on both sides of the two boundaries where the log-softmax table leaves LDS, every
class count the grad kernel's 64-lane wave allows and a blank other than C - 1, batches on both
sides of 32 / 64 / 128 with empty rows, peaked / flat / shifted posteriors, caller buffers and
workspaces full of garbage, rows that do not fit max_label_len, greedy decode across its
256-frame chunk seams, and the grid-stride loop of the log-softmax kernels.

The loss is checked against the float64 C oracle (`cref.ctc_loss`, itself pinned against
torch.nn.functional.ctc_loss and path enumeration at these shapes in test_oracle_ctc.py).  The bars
of test_gpu_kernels.py are the ceiling: loss 1e-3, gradient 1e-4 absolute.  Two groups tighten or
restate them (see `_loss_bar`, `test_ctc_short_utterances`)."""

import math

import numpy as np
import pytest
import torch

from oracle import cref
from oracle import ctc as octc
from tests.helpers import pack_labels

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# ctcasr_ctc_loss_fwd_bwd's launcher: s_pad = 2 * max_label_len + 1 lattice slots, at most
# CTC_THREADS * CTC_MAX_PER_THREAD of them; LDS bytes = fixed + T * C * 4, where fixed holds two
# fp64 lattice rows, the int extended labels and four int flags.  Up to 64 KB: no attribute call;
# up to 150 KB: after hipFuncSetAttribute; above: the table is read from HBM.
CTC_THREADS, CTC_MAX_PER_THREAD = 384, 3
MAX_LABEL_LEN = (CTC_THREADS * CTC_MAX_PER_THREAD - 1) // 2        # 575
LDS_PLAIN, LDS_ATTR = 64 * 1024, 150 * 1024

# largest error seen per group, {group: [loss, gradient, loss / its bar, gradient / its bar]}
# (read by whoever runs the module to report it; the asserts do not depend on it)
MEASURED = {}


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _table_bytes(num_steps, classes, max_label_len):
    s_pad = 2 * max_label_len + 1
    return s_pad * (2 * 8 + 4) + 4 * 4 + num_steps * classes * 4


def _table_boundaries(classes, max_label_len):
    """The largest T whose log-softmax table stays in LDS without / with the attribute call."""
    fixed = _table_bytes(0, classes, max_label_len)
    return (LDS_PLAIN - fixed) // (4 * classes), (LDS_ATTR - fixed) // (4 * classes)


def _table_path(num_steps, classes, max_label_len):
    nbytes = _table_bytes(num_steps, classes, max_label_len)
    return 'lds' if nbytes <= LDS_PLAIN else 'lds+attr' if nbytes <= LDS_ATTR else 'hbm'


def _record(group, *errors):
    seen = MEASURED.setdefault(group, [0.0] * len(errors))
    seen[:] = [max(a, float(b)) for a, b in zip(seen, errors)]


def _loss_bar(ref_loss):
    """1e-3 absolute, the bar of test_gpu_kernels.py, up to a loss of 1000; relative 1e-6 above.
    Derived, not measured: a float32 loss of 2e4 alone rounds by up to 1e-3, and every frame's
    table entry (row - lse, rounded to float) carries a relative error ~6e-8 of its own."""
    return np.maximum(1e-3, 1e-6 * np.abs(ref_loss))


def _run(hip, logits, labels, seq_len, max_label_len, blank=None, offsets=None, **kw):
    """The wrapper on host arrays; `offsets` (with `labels` already flat) passes label_offsets
    as given.  Returns host (loss, grad, status)."""
    if offsets is None:
        flat, offsets = pack_labels(labels)
    else:
        flat = np.asarray(labels, dtype=np.int32)
    loss, grad, status = hip.ctc_loss_fwd_bwd(
        _t(logits), _t(flat, torch.int32), _t(offsets, torch.int32),
        _t(np.asarray(seq_len), torch.int32), max_label_len, blank=blank, **kw)
    return loss.cpu().numpy(), grad.cpu().numpy(), status.cpu().numpy()


def _check(hip, group, logits, labels, seq_len, max_label_len=None, blank=None,
           loss_bar=_loss_bar, grad_bar=1e-4):
    """One call against the oracle: status equal; rows with status != 0 give +inf loss and an
    all-zero gradient column; frames t >= seq_len carry exactly no gradient; loss and gradient
    inside their bars."""
    seq_len = np.asarray(seq_len, dtype=np.int32)
    if max_label_len is None:
        max_label_len = max(len(row) for row in labels)
    loss, grad, status = _run(hip, logits, labels, seq_len, max_label_len, blank)
    ref_loss, ref_grad, ref_status = cref.ctc_loss(logits, labels, seq_len, blank)
    assert status.tolist() == ref_status.tolist()
    bad = status != 0
    assert np.isposinf(loss[bad]).all() and (grad[:, bad] == 0).all()
    for b, length in enumerate(seq_len):
        assert (grad[max(int(length), 0):, b] == 0).all(), b
    loss_err = np.abs(loss[~bad] - ref_loss[~bad])
    bar = loss_bar(ref_loss[~bad]) if callable(loss_bar) else loss_bar
    grad_err = np.abs(grad - ref_grad).max()
    _record(group, loss_err.max(initial=0.0), grad_err, (loss_err / bar).max(initial=0.0),
            grad_err / grad_bar)
    assert (loss_err <= bar).all(), (loss_err.max(), loss[~bad], ref_loss[~bad])
    assert grad_err <= grad_bar, grad_err
    return loss, grad, status


def _required(label):
    """Frames the label needs: one per id plus a blank between each adjacent repeat."""
    return len(label) + sum(1 for a, b in zip(label, label[1:]) if a == b)


def _labels_with_repeats(rng, length, classes, blank, repeat_p=0.2):
    ids = [c for c in range(classes) if c != blank]
    out = []
    for _ in range(length):
        out.append(out[-1] if out and rng.random() < repeat_p else int(rng.choice(ids)))
    return out


def _same_as_alone(hip, logits, labels, seq_len, max_label_len, loss, grad, status, rows,
                   blank=None):
    """Each listed row of a batch equals that utterance run alone at B = 1 with the same T and
    max_label_len: loss and status bit for bit, gradient within 1e-6 (its LDS atomics may add in
    another order, the determinism bar of test_gpu_properties.py)."""
    for b in rows:
        one_loss, one_grad, one_status = _run(hip, logits[:, b:b + 1], [labels[b]],
                                              seq_len[b:b + 1], max_label_len, blank)
        assert one_status[0] == status[b], b
        assert one_loss.view(np.int32)[0] == loss.view(np.int32)[b], (b, one_loss[0], loss[b])
        assert np.abs(one_grad[:, 0] - grad[:, b]).max() <= 1e-6, b


# ------------------------------------------------------------------------------------------------
# Short utterances
# ------------------------------------------------------------------------------------------------
SHORT_CLASSES = 7          # blank 6


def _short_rows(num_steps):
    """(label, seq_len) rows for T frames: every degenerate case that fits."""
    rows = [([], num_steps), ([2], num_steps), ([], 0), ([3], 0), ([1, 4], 0)]
    # tight bound with distinct ids (needs T frames) and one frame below it
    rows += [(list(range(num_steps)), num_steps), (list(range(num_steps + 1)), num_steps)]
    # [k] * L needs 2L - 1 frames
    if num_steps % 2:
        rows.append(([5] * ((num_steps + 1) // 2), num_steps))
    else:
        rows.append(([5] * (num_steps // 2) + [0], num_steps))        # L + repeats = T
    rows.append(([5] * ((num_steps + 3) // 2), num_steps))            # needs T + 1 or T + 2
    if num_steps >= 2:
        rows += [([4], 1), ([], 1), ([4, 4], num_steps - 1 if num_steps >= 4 else 2)]
        rows.append(([0, 0], 2))                                      # needs 3
    return rows


@pytest.mark.parametrize('batch', [1, 2, 5])
@pytest.mark.parametrize('num_steps', [1, 2, 3, 4])
def test_ctc_short_utterances(hip, num_steps, batch):
    """T = 1-4 against the oracle, at loss 1e-5 and gradient 1e-6 - ten times and a hundred
    times tighter than the general bars: the lattice is a handful of float exp / log steps on
    double state (~1e-7 each) on top of float table entries (~2e-7 each at these logits).
    Rows cover L = 0 and 1, the tight bound (distinct ids, [k] * L), one frame below it (status
    1, +inf, zero column), len = 0 with L = 0 (loss exactly 0, status 0, zero column) and with
    L > 0 (status 1), and len = 1 inside a longer T."""
    rows = _short_rows(num_steps)
    rng = np.random.default_rng(100 * num_steps + batch)
    for start in range(0, len(rows), batch):
        picked = [rows[(start + i) % len(rows)] for i in range(batch)]
        labels = [r[0] for r in picked]
        seq_len = np.array([r[1] for r in picked], dtype=np.int32)
        logits = (rng.normal(size=(num_steps, batch, SHORT_CLASSES)) * 2).astype(np.float32)
        loss, grad, status = _check(hip, 'short T<=4', logits, labels, seq_len,
                                    max(1, max(len(r) for r in labels)),
                                    loss_bar=1e-5, grad_bar=1e-6)
        for b, (label, length) in enumerate(picked):
            expect = 0 if _required(label) <= length else 1
            assert status[b] == expect, (label, length)
            if length == 0 and not label:
                assert loss[b] == 0.0 and (grad[:, b] == 0).all()
            if _required(label) == length and length > 0:
                # exactly one alignment: the loss is minus its log-probability
                path = []
                for i, sym in enumerate(label):
                    if i and label[i - 1] == sym:
                        path.append(SHORT_CLASSES - 1)
                    path.append(sym)
                logp = octc.log_softmax(logits[:length, b].astype(np.float64))
                one = -sum(logp[t, s] for t, s in enumerate(path))
                assert abs(loss[b] - one) <= 1e-5


# ------------------------------------------------------------------------------------------------
# Label lengths at the slot seams and the ceiling
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('label_len', [191, 192, 383, 384, 575])
def test_ctc_label_length_seams(hip, label_len):
    """S = 2L + 1 = 383 / 385 straddle the first per-thread slot seam (384 threads), 767 / 769
    the second, 1151 is the ceiling.  Rows: T >= 2L + 1, the tight bound (one alignment) and one
    frame below it.  At T = 2L + 7, C = 29 the table sits in LDS without the attribute call at
    L = 191 / 192, with it at 383 / 384, and in HBM at L = 575."""
    classes = 29
    rng = np.random.default_rng(label_len)
    num_steps = 2 * label_len + 7
    labels = [_labels_with_repeats(rng, label_len, classes, classes - 1) for _ in range(3)]
    labels[0] = list(rng.permutation(np.arange(label_len) % (classes - 1)))
    tight = _required(labels[1])
    labels[2] = labels[1]
    seq_len = np.array([num_steps, tight, tight - 1], dtype=np.int32)
    assert tight <= num_steps and _required(labels[0]) <= num_steps
    logits = (rng.normal(size=(num_steps, 3, classes)) * 2).astype(np.float32)
    _, _, status = _check(hip, 'label-length seams', logits, labels, seq_len, label_len)
    assert status.tolist() == [0, 0, 1]


def test_ctc_max_label_len_ceiling(hip):
    """max_label_len = 576 (S = 1153 > 1152 slots) is refused; 575 for short rows gives the loss
    and status of the true maximum bit for bit, the gradient within 1e-6."""
    classes = 29
    rng = np.random.default_rng(5)
    for num_steps in (1, 9, 60):
        labels = [_labels_with_repeats(rng, int(rng.integers(0, min(num_steps, 20) + 1)), classes,
                                       classes - 1) for _ in range(4)]
        labels[0] = []
        seq_len = np.array([num_steps, num_steps, max(1, num_steps // 2), 0], dtype=np.int32)
        logits = (rng.normal(size=(num_steps, 4, classes)) * 2).astype(np.float32)
        true_max = max(len(r) for r in labels)
        assert _table_path(num_steps, classes, MAX_LABEL_LEN) == 'lds'
        loss, grad, status = _run(hip, logits, labels, seq_len, true_max)
        loss2, grad2, status2 = _run(hip, logits, labels, seq_len, MAX_LABEL_LEN)
        assert np.array_equal(status, status2)
        assert np.array_equal(loss.view(np.int32), loss2.view(np.int32))
        assert np.abs(grad - grad2).max() <= 1e-6
        with pytest.raises(hip.CtcAsrError, match='unsupported'):
            _run(hip, logits, labels, seq_len, MAX_LABEL_LEN + 1)


# ------------------------------------------------------------------------------------------------
# Where the log-softmax table lives
# ------------------------------------------------------------------------------------------------
def _placement_cases():
    cases = []
    for classes, max_label_len in ((29, 10), (64, 100), (2, 0)):
        plain, attr = _table_boundaries(classes, max_label_len)
        for num_steps, path in ((plain, 'lds'), (plain + 1, 'lds+attr'), (attr, 'lds+attr'),
                                (attr + 1, 'hbm')):
            cases.append((classes, max_label_len, num_steps, path))
    return cases


@pytest.mark.parametrize('classes,max_label_len,num_steps,path', _placement_cases())
def test_ctc_table_placement_boundaries(hip, classes, max_label_len, num_steps, path):
    """T on both sides of the two boundaries, computed from the launcher's formula: B = 3 with
    ragged lengths and label lengths (max_label_len, about half, none)."""
    assert _table_path(num_steps, classes, max_label_len) == path
    rng = np.random.default_rng(num_steps)
    blank = classes - 1
    labels = [_labels_with_repeats(rng, max_label_len, classes, blank),
              _labels_with_repeats(rng, max_label_len // 2, classes, blank), []]
    seq_len = np.array([num_steps, num_steps - 1 - num_steps // 3, num_steps // 2 + 1],
                       dtype=np.int32)
    logits = (rng.normal(size=(num_steps, 3, classes)) * 2).astype(np.float32)
    _, _, status = _check(hip, 'table placement', logits, labels, seq_len, max_label_len)
    assert (status == 0).all()


# ------------------------------------------------------------------------------------------------
# Classes and blank
# ------------------------------------------------------------------------------------------------
def _class_cases():
    return [(c, blank) for c in (2, 3, 33, 63, 64) for blank in sorted({c - 1, 0, c // 2})]


@pytest.mark.parametrize('classes,blank', _class_cases())
def test_ctc_classes_and_blank(hip, classes, blank):
    """C = 2 (the smallest legal case) to 64 (every lane of the grad kernel's wave), with the
    blank at C - 1, 0 and C // 2; every non-blank id appears; a label equal to the blank gives
    status 2."""
    rng = np.random.default_rng(classes * 100 + blank)
    ids = [c for c in range(classes) if c != blank]
    labels = [list(rng.permutation(ids)), _labels_with_repeats(rng, 12, classes, blank, 0.4), [],
              [ids[0], blank, ids[-1]]]
    num_steps = 2 * max(_required(r) for r in labels) + 9
    seq_len = np.array([num_steps, num_steps - 3, num_steps // 2, num_steps], dtype=np.int32)
    logits = (rng.normal(size=(num_steps, 4, classes)) * 2).astype(np.float32)
    _, _, status = _check(hip, 'classes and blank', logits, labels, seq_len, blank=blank)
    assert status.tolist() == [0, 0, 0, 2]


@pytest.mark.parametrize('classes', [1, 65])
def test_ctc_class_count_refused(hip, classes):
    logits = np.zeros((4, 1, classes), dtype=np.float32)
    with pytest.raises(hip.CtcAsrError):
        _run(hip, logits, [[]], [4], 1)


# ------------------------------------------------------------------------------------------------
# Batch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('batch', [31, 32, 33, 64, 65, 130])
def test_ctc_batch_sizes(hip, batch):
    """Ragged seq_len and L, with empty rows, len = 0 rows and infeasible rows; against the
    oracle, and each row against the same utterance run alone."""
    classes, num_steps = 29, 48
    rng = np.random.default_rng(batch)
    labels = [_labels_with_repeats(rng, int(rng.integers(0, 16)), classes, classes - 1)
              for _ in range(batch)]
    seq_len = rng.integers(0, num_steps + 1, size=batch).astype(np.int32)
    labels[0], labels[batch // 2], labels[-1] = [], [], [3, 4]
    seq_len[0], seq_len[1], seq_len[-1] = num_steps, 0, 1                   # last: status 1
    max_label_len = max(len(r) for r in labels)
    logits = (rng.normal(size=(num_steps, batch, classes)) * 2).astype(np.float32)
    loss, grad, status = _check(hip, 'batch', logits, labels, seq_len, max_label_len)
    assert status[-1] == 1 and (status == 0).sum() > batch // 3
    _same_as_alone(hip, logits, labels, seq_len, max_label_len, loss, grad, status, range(batch))


# ------------------------------------------------------------------------------------------------
# Posterior shape
# ------------------------------------------------------------------------------------------------
def _alignments(label, length):
    """The number of CTC paths of `length` frames that collapse to `label` (exact integers)."""
    ext = octc.extended_labels(label, -1)
    size = len(ext)
    count = [0] * size
    count[0] = 1
    if size > 1:
        count[1] = 1
    for _ in range(1, length):
        nxt = list(count)
        for u in range(1, size):
            nxt[u] += count[u - 1]
            if u >= 2 and ext[u] != -1 and ext[u] != ext[u - 2]:
                nxt[u] += count[u - 2]
        count = nxt
    return count[-1] + (count[-2] if size > 1 else 0)


@pytest.mark.parametrize('kind', ['peaked', 'flat', 'shifted'])
@pytest.mark.parametrize('shape', [(60, 3, 29, 20), (300, 4, 64, 100), (1699, 1, 64, 575)])
def test_ctc_posterior_shapes(hip, shape, kind):
    """peaked: logits x 30 (near one-hot) against random labels, so the loss is large and every
    path runs through tiny probabilities; flat: all-zero logits, where p(label) is the number
    of alignments over C^len; shifted: logits plus a per-frame offset of +-50 against the
    unshifted ones.  (1699, 64, 575): the longest utterance at the widest class count and the
    label ceiling, with the table in HBM.  The loss bar is relative above a loss of 1000
    (`_loss_bar`)."""
    num_steps, batch, classes, label_len = shape
    rng = np.random.default_rng(num_steps + label_len)
    blank = classes - 1
    labels = [_labels_with_repeats(rng, label_len - 3 * b, classes, blank) for b in range(batch)]
    seq_len = np.array([num_steps - 7 * b for b in range(batch)], dtype=np.int32)
    base = rng.normal(size=(num_steps, batch, classes)).astype(np.float32)
    # (shifted: on a 2^-17 grid, so that x +- 50 is exact in float32 and the two inputs differ
    # by the offset alone)
    unshifted = (np.round(base * 2 * 2 ** 17) / 2 ** 17).astype(np.float32)
    if kind == 'peaked':
        logits = base * 30
    elif kind == 'flat':
        logits = np.zeros_like(base)
    else:
        logits = unshifted + rng.choice([-50.0, 50.0], size=(num_steps, batch, 1))
    logits = logits.astype(np.float32)
    loss, grad, status = _check(hip, 'posterior ' + kind, logits, labels, seq_len, label_len)
    assert (status == 0).all()
    if kind == 'flat':
        for b in range(batch):
            exact = seq_len[b] * math.log(classes) - math.log(_alignments(labels[b], seq_len[b]))
            assert abs(loss[b] - exact) <= _loss_bar(exact), (loss[b], exact)
    if kind == 'shifted':
        assert np.array_equal(np.abs(logits - unshifted), np.full_like(logits, 50))
        loss0, grad0, _ = _run(hip, unshifted, labels, seq_len, label_len)
        assert (np.abs(loss - loss0) <= 2 * _loss_bar(loss0)).all()
        assert np.abs(grad - grad0).max() <= 1e-5


# ------------------------------------------------------------------------------------------------
# Caller buffers and workspaces
# ------------------------------------------------------------------------------------------------
def _mixed_batch(rng, num_steps, classes, max_label_len):
    """Rows with status 0, 1 (infeasible), 2 (bad label), 0 (len = 0, L = 0), 1 (len = 0,
    L > 0), 0 (odd len), 0 (empty label)."""
    blank = classes - 1
    labels = [_labels_with_repeats(rng, max_label_len, classes, blank),
              [7] * max_label_len, [1, blank, 2], [], [4, 5],
              _labels_with_repeats(rng, max_label_len // 2, classes, blank), []]
    seq_len = np.array([num_steps, max_label_len, num_steps, 0, 0,
                        num_steps - 2 if num_steps % 2 else num_steps - 1, num_steps // 2],
                       dtype=np.int32)
    logits = (rng.normal(size=(num_steps, len(labels), classes)) * 2).astype(np.float32)
    return logits, labels, seq_len


def _dirty_call(hip, logits, labels, seq_len, max_label_len, workspace):
    num_steps, batch, _ = logits.shape
    loss = torch.full((batch,), float('nan'), device=DEV)
    grad = torch.full(logits.shape, float('nan'), device=DEV)
    status = torch.full((batch,), -7, dtype=torch.int32, device=DEV)
    return _run(hip, logits, labels, seq_len, max_label_len, loss=loss, grad=grad, status=status,
                workspace=workspace)


def _fresh_call(hip, logits, labels, seq_len, max_label_len):
    num_steps, batch, classes = logits.shape
    nbytes = hip.ctc_loss_workspace_bytes(num_steps, batch, classes, max_label_len)
    return _run(hip, logits, labels, seq_len, max_label_len,
                workspace=torch.zeros(nbytes, dtype=torch.uint8, device=DEV))


def _assert_same(got, want):
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32))
    assert np.abs(got[1] - want[1]).max() <= 1e-6


@pytest.mark.parametrize('num_steps,classes', [(40, 29), (700, 64)])
def test_ctc_writes_every_output(hip, num_steps, classes):
    """loss / grad pre-filled with NaN, status with -7, a workspace of 0xFF bytes sized for a
    larger call: every entry is written, rows t >= len and whole columns of failed rows are
    exactly 0, and the result is that of a fresh zeroed workspace.  (700, 64) reads the table
    from HBM, so the table region of the dirty workspace is NaN until the sweeps write it."""
    max_label_len = 12
    assert _table_path(num_steps, classes, max_label_len) == ('lds' if num_steps < 100 else 'hbm')
    rng = np.random.default_rng(num_steps)
    logits, labels, seq_len = _mixed_batch(rng, num_steps, classes, max_label_len)
    batch = logits.shape[1]
    big = hip.ctc_loss_workspace_bytes(num_steps + 33, batch + 3, classes, 2 * max_label_len)
    workspace = torch.full((big,), 0xFF, dtype=torch.uint8, device=DEV)
    got = _dirty_call(hip, logits, labels, seq_len, max_label_len, workspace)
    loss, grad, status = got
    assert status.tolist() == [0, 1, 2, 0, 1, 0, 0]
    assert not np.isnan(loss).any() and not np.isnan(grad).any()
    assert loss[3] == 0.0 and np.isposinf(loss[[1, 2, 4]]).all()
    for b in range(batch):
        live = seq_len[b] if status[b] == 0 else 0
        assert (grad[live:, b] == 0).all(), b
    ref_loss, ref_grad, ref_status = cref.ctc_loss(logits, labels, seq_len)
    assert np.array_equal(status, ref_status)
    assert np.abs(loss[status == 0] - ref_loss[status == 0]).max() <= 1e-3
    assert np.abs(grad - ref_grad).max() <= 1e-4
    _assert_same(got, _fresh_call(hip, logits, labels, seq_len, max_label_len))


def test_ctc_one_workspace_large_small_large(hip):
    """One dirty workspace through (T, B, max_label_len) = large, small (odd T), large, each
    with new data: each call equals a fresh one."""
    classes = 29
    rng = np.random.default_rng(77)
    shapes = [(120, 30), (37, 7), (120, 30)]           # (T, max_label_len); B = 7
    big = max(hip.ctc_loss_workspace_bytes(t, 7, classes, m) for t, m in shapes)
    workspace = torch.full((big,), 0xFF, dtype=torch.uint8, device=DEV)
    for num_steps, max_label_len in shapes:
        logits, labels, seq_len = _mixed_batch(rng, num_steps, classes, max_label_len)
        _assert_same(_dirty_call(hip, logits, labels, seq_len, max_label_len, workspace),
                     _fresh_call(hip, logits, labels, seq_len, max_label_len))


# ------------------------------------------------------------------------------------------------
# Rows that do not fit max_label_len
# ------------------------------------------------------------------------------------------------
def test_ctc_row_longer_than_max_label_len(hip):
    """A row with L = max_label_len + 1 whose extra id is 0 (blank C - 1, enough frames) in
    position 0: status 2, +inf, zero column - without the guard its extended labels ran past
    the lattice rows into the flags, which the id 0 cleared, and the loss came out finite and
    wrong.  The other rows equal their standalone results."""
    classes, num_steps, max_label_len = 29, 60, 10
    rng = np.random.default_rng(21)
    assert _table_path(num_steps, classes, max_label_len) == 'lds'
    labels = [list(rng.integers(1, classes - 1, size=max_label_len)) + [0],
              _labels_with_repeats(rng, max_label_len, classes, classes - 1),
              _labels_with_repeats(rng, 4, classes, classes - 1)]
    seq_len = np.array([num_steps, num_steps - 5, 30], dtype=np.int32)
    logits = (rng.normal(size=(num_steps, 3, classes)) * 2).astype(np.float32)
    loss, grad, status = _run(hip, logits, labels, seq_len, max_label_len)
    assert status.tolist() == [2, 0, 0]
    assert np.isposinf(loss[0]) and (grad[:, 0] == 0).all()
    _same_as_alone(hip, logits, labels, seq_len, max_label_len, loss, grad, status, (1, 2))


def test_ctc_decreasing_label_offsets(hip):
    """label_offsets that decrease (L = -3 for row 1): status 2; rows 0 and 2 (whose labels
    overlap) equal their standalone results."""
    classes, num_steps = 29, 40
    rng = np.random.default_rng(22)
    flat = rng.integers(0, classes - 1, size=8).astype(np.int32)
    offsets = np.array([0, 5, 2, 8], dtype=np.int32)
    labels = [flat[0:5].tolist(), None, flat[2:8].tolist()]
    seq_len = np.array([num_steps, num_steps, num_steps - 9], dtype=np.int32)
    logits = (rng.normal(size=(num_steps, 3, classes)) * 2).astype(np.float32)
    loss, grad, status = _run(hip, logits, flat, seq_len, 6, offsets=offsets)
    assert status.tolist() == [0, 2, 0]
    assert np.isposinf(loss[1]) and (grad[:, 1] == 0).all()
    _same_as_alone(hip, logits, labels, seq_len, 6, loss, grad, status, (0, 2))


# ------------------------------------------------------------------------------------------------
# Greedy decode
# ------------------------------------------------------------------------------------------------
def _logits_of_paths(rng, paths, classes):
    """[T, B, C] logits whose per-frame argmax is paths[b][t], with margin >= 1."""
    num_steps = len(paths[0])
    logits = rng.uniform(-3, 0, size=(num_steps, len(paths), classes)).astype(np.float32)
    for b, path in enumerate(paths):
        logits[np.arange(num_steps), b, path] = rng.uniform(1, 4, size=num_steps)
    return logits


@pytest.mark.parametrize('num_steps', [255, 256, 257, 511, 512, 513, 1000])
def test_greedy_decode_chunk_seams(hip, num_steps):
    """The kernel decodes in 256-frame chunks and carries the last argmax across each seam:
    row 0 holds a symbol run across frames 255 / 256 and 511 / 512 (one symbol each), row 1 a
    blank exactly on frames 255 and 511 between equal symbols (two symbols each), row 2 a run
    that ends at len - 1 with other symbols beyond len, row 3 a lone symbol on each seam frame."""
    classes, blank = 29, 28
    rng = np.random.default_rng(num_steps)
    paths = np.where(rng.random((4, num_steps)) < 0.5, blank,
                     rng.integers(0, classes - 1, size=(4, num_steps)))
    seq_len = np.array([num_steps, num_steps, num_steps - 3, num_steps], dtype=np.int32)
    for seam in (256, 512):
        if seam > num_steps:
            continue
        hi = min(seam + 4, num_steps)
        paths[0, seam - 4:hi] = 5
        paths[1, seam - 3:hi] = 9
        paths[1, seam - 1] = blank
        paths[3, seam - 2:hi] = blank
        paths[3, seam - 1] = 11
        if seam < num_steps:
            paths[3, seam] = 12
    end = seq_len[2]
    paths[2, end - 5:end] = 7
    paths[2, end - 6] = blank
    paths[2, end:] = 3
    logits = _logits_of_paths(rng, paths, classes)
    out, out_len = hip.ctc_greedy_decode(_t(logits), _t(seq_len, torch.int32))
    out, out_len = out.cpu().numpy(), out_len.cpu().numpy()
    ref = octc.greedy_decode(logits, seq_len)
    for b in range(4):
        assert ref[b] == list(octc.collapse_path(paths[b, :seq_len[b]].tolist(), blank))
        assert out[b, :out_len[b]].tolist() == ref[b], b
        assert (out[b, out_len[b]:] == 0).all()
    assert ref[2][-1] == 7


@pytest.mark.parametrize('classes,blank', [(1, 0), (2, 0), (2, 1), (29, 0), (64, 0), (64, 63),
                                           (100, 0), (100, 99)])
def test_greedy_decode_ties_and_lengths(hip, classes, blank):
    """Exact ties go to the lowest id (`argmax`: first maximum) - between symbols, between a
    symbol and the blank, across all C; seq_len 0, > T (decodes T frames) and < 0 (nothing);
    C beyond 64 (greedy decode has no class limit); out and out_len pre-filled with -7, each row
    zero-padded past out_len."""
    num_steps, batch = 300, 6
    rng = np.random.default_rng(classes * 7 + blank)
    logits = rng.normal(size=(num_steps, batch, classes)).astype(np.float32)
    logits = np.round(logits * 2) / 2              # many exact ties at every C
    logits[::5] = 0.0                              # whole frames of ties: id 0 wins
    if classes >= 4:
        logits[1::7, :, :] = -1.0
        logits[1::7, :, classes - 1] = 1.0         # the blank or the top id ...
        logits[1::7, :, 2] = 1.0                   # ... ties with id 2: id 2 wins
    seq_len = np.array([num_steps, 0, num_steps + 40, -5, 257, 1], dtype=np.int32)
    out = torch.full((batch, num_steps), -7, dtype=torch.int32, device=DEV)
    out_len = torch.full((batch,), -7, dtype=torch.int32, device=DEV)
    hip.ctc_greedy_decode(_t(logits), _t(seq_len, torch.int32), blank=blank, out=out,
                          out_len=out_len)
    out, out_len = out.cpu().numpy(), out_len.cpu().numpy()
    ref = octc.greedy_decode(logits, np.clip(seq_len, 0, num_steps), blank)
    assert out_len[1] == 0 and out_len[3] == 0
    for b in range(batch):
        assert out_len[b] == len(ref[b]), b
        assert out[b, :out_len[b]].tolist() == ref[b], b
        assert (out[b, out_len[b]:] == 0).all(), b


# ------------------------------------------------------------------------------------------------
# Log-softmax export
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', [1, 3, 16383, 16384, 16385, 70001])
@pytest.mark.parametrize('classes', [1, 2, 31, 32, 33, 63, 64])
def test_log_softmax_edges(hip, classes, rows):
    """One wave per row, at most 4096 workgroups of four: rows past 16 384 only the grid-stride
    loop reaches.  Rows with |x| up to 1e4 and a -inf entry are mixed in.  Forward bar: 2 ulp of
    the row's largest |x| plus 1e-6 (x - mx and log(sum) are each rounded once, lse and x - lse
    once more).  Backward bar: 4 ulp of sum |dy| plus 1e-6 (the 64-lane tree sum rounds six
    times, at most 3 ulp of the partial sums, and the product and difference once)."""
    rng = np.random.default_rng(classes * 100000 + rows)
    x = (rng.normal(size=(rows, classes)) * 3).astype(np.float32)
    big = np.unique(np.array([0, rows // 2, rows - 1]))
    x[big] = rng.uniform(-1e4, 1e4, size=(len(big), classes)).astype(np.float32)
    if classes > 1 and rows > 1:
        x[1, classes // 2] = -np.inf
        x[rows - 1, 0] = -np.inf
    y = hip.log_softmax_fwd(_t(x)).cpu().numpy()
    ref = torch.log_softmax(torch.from_numpy(x).double(), -1).numpy()
    neg = np.isneginf(x)
    assert np.array_equal(np.isneginf(y), neg)
    scale = np.abs(np.where(neg, 0, x)).max(-1, keepdims=True)
    bar = 2 * np.spacing(scale.astype(np.float32)).astype(np.float64) + 1e-6
    err = np.abs(np.where(neg, 0, y) - np.where(neg, 0, ref))
    fwd = float((err / bar).max())
    assert fwd <= 1, (err.max(), np.unravel_index(np.argmax(err / bar), err.shape))
    y32 = ref.astype(np.float32)
    dy = rng.normal(size=(rows, classes)).astype(np.float32)
    dx = hip.log_softmax_bwd(_t(y32), _t(dy)).cpu().numpy()
    ref_dx = dy - np.exp(y32.astype(np.float64)) * dy.astype(np.float64).sum(-1, keepdims=True)
    bar = 4 * np.spacing(np.abs(dy).sum(-1, keepdims=True)).astype(np.float64) + 1e-6
    bwd = float((np.abs(dx - ref_dx) / bar).max())
    _record('log-softmax error / bar (fwd, bwd)', fwd, bwd)
    assert bwd <= 1, bwd


def test_log_softmax_class_limit(hip):
    x = _t(np.zeros((4, 65), dtype=np.float32))
    with pytest.raises(hip.CtcAsrError, match='unsupported'):
        hip.log_softmax_fwd(x)
    with pytest.raises(hip.CtcAsrError, match='unsupported'):
        hip.log_softmax_bwd(x, x)
